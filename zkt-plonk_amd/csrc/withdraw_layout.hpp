// Host-only planner of the withdraw circuit: WithdrawCircuit::synthesize (circuits/src/withdraw.rs:57-150) as rows, from
// (Poseidon parameters, INPUTS, HEIGHT) alone.  Variable numbering and row order are the reference composer's allocation
// order, statement by statement; the witness kernels of withdraw.hip find every variable through the closed form in
// Shape, which the walk below is checked against.
//
// What it makes:
//   * one gadget TEMPLATE per arity (1, 2, 3): the P rows of one PoseidonRef::hash relative to its first variable.  A
//     wire reference is k (the k-th variable of this hash), REF_INPUT | k (its k-th input) or REF_ZERO.  The selectors
//     depend on the round constants, the MDS entries and the domain tag only (add_constant / mul_constant fold into the
//     selectors of the gate that consumes them, composer.rs:84-114);
//   * the list of hash calls (first row, first variable, input variables);
//   * the glue rows (per note 7 H + 4, 130 + INPUTS global ones), whose selectors take nine values only and are kept as
//     codes;
//   * the public-input positions, ascending: root, nullifiers, withdraw_amount, new_identifier, new_leaf
//     (bin/src/main.rs:266-271).
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <vector>

#include "fp.hpp"
#include "fx.hpp"

namespace zkt {
namespace withdraw {

constexpr uint32_t REF_ZERO = 0xFFFFFFFFu;    // ZKT_VARIABLE_ZERO
constexpr uint32_t REF_INPUT = 0x80000000u;   // template only: | k = the call's k-th input
constexpr int MAX_WIDTH = 8, MAX_INPUTS = 32, MAX_HEIGHT = 64;

// the values a glue row's selector takes: 0, 1, -1 and the multipliers of bits_le_constrain (mod.rs:175-213: 2, squared
// on a u64 at every level; 64 bits take six levels)
enum : uint8_t { G_0 = 0, G_1, G_M1, G_2, G_4, G_16, G_256, G_65536, G_2P32, G_COUNT };

struct GlueRow {
    uint32_t row;
    uint32_t w[3];      // w_l, w_r, w_o
    uint8_t q[6];       // codes of q_m, q_l, q_r, q_o, q_c, q_lookup
    uint8_t pad[2];
};

struct HashCall {
    uint32_t row, base, arity;
    uint32_t in[3];
};

struct Shape {
    int width = 0, half_full = 0, partial = 0, inputs = 0, height = 0;
    uint32_t P = 0;           // variables = rows of one hash
    uint32_t hash_off = 0;    // the hash value's variable, relative to the call's first
    uint32_t per_level = 0;   // 6 + P
    uint32_t note_vars = 0, note_rows = 0;
    uint32_t note0 = 0;       // first variable of note 0 (its secret)
    uint32_t glob0 = 0;       // first variable after the notes (bit 0 of amount_out)
    uint32_t row_glob0 = 0;   // first row after the notes
    uint64_t n_vars = 0, n_gates = 0;
    uint32_t n_hashes = 0, n_pi = 0;

    // ---- closed form of the variable numbering (k = note, all relative to one request's map) ----
    uint32_t amount_var(int k) const { return (uint32_t)k; }
    uint32_t ident_var(int k) const { return (uint32_t)(inputs + k); }
    uint32_t root_var() const { return (uint32_t)(2 * inputs); }
    uint32_t secret_var(int k) const { return note0 + (uint32_t)k * note_vars; }
    uint32_t commit_base(int k) const { return secret_var(k) + 1; }
    uint32_t inv_var(int k) const { return secret_var(k) + 1 + P; }
    uint32_t null_base(int k) const { return secret_var(k) + 2 + P; }
    uint32_t leaf_base(int k) const { return secret_var(k) + 2 + 2 * P; }
    uint32_t bit0(int k) const { return secret_var(k) + 2 + 3 * P; }
    uint32_t sib0(int k) const { return bit0(k) + (uint32_t)height; }
    uint32_t path_base(int k) const { return sib0(k) + (uint32_t)height; }
    uint32_t path_root(int k) const { return path_base(k) + (uint32_t)(height - 1) * per_level + 6 + hash_off; }
    uint32_t lookup_var(int k) const { return path_base(k) + (uint32_t)height * per_level; }
    uint32_t out_bit0() const { return glob0; }
    uint32_t recomb0() const { return glob0 + 64; }
    uint32_t out_var() const { return glob0 + 126; }
    uint32_t sum0() const { return glob0 + 127; }
    uint32_t new_secret_var() const { return glob0 + 126 + (uint32_t)inputs; }
    uint32_t new_ident_var() const { return new_secret_var() + 1; }
    uint32_t new_commit_base() const { return new_ident_var() + 1; }
    uint32_t new_leaf_base() const { return new_commit_base() + P; }
    // public inputs
    uint32_t null_row(int k) const { return 1 + (uint32_t)k * note_rows + 2 * P + 1; }
    uint32_t balance_row() const { return row_glob0 + 126 + (uint32_t)inputs; }
};

// false: a shape the circuit does not have (width 3 cannot hash a leaf: three inputs make it FullBuffer)
inline bool shape_make(int width, int half_full, int partial, int inputs, int height, Shape& s) {
    if (width < 4 || width > MAX_WIDTH || inputs < 1 || inputs > MAX_INPUTS || height < 1 || height > MAX_HEIGHT) return false;
    if (half_full < 1 || partial < 1 || half_full > 1024 || partial > 4096) return false;
    const uint64_t W = (uint64_t)width, I = (uint64_t)inputs, H = (uint64_t)height;
    const uint64_t P = 2 * (uint64_t)half_full * (3 * W + W * W) + (uint64_t)partial * (3 + W * W);
    const uint64_t note_vars = 3 * P + 3 + 2 * H + H * (6 + P);
    const uint64_t note_rows = (3 + H) * P + 7 * H + 4;
    const uint64_t n_vars = 2 * I + 1 + I * note_vars + 127 + (I - 1) + 2 + 2 * P;
    const uint64_t n_gates = I * note_rows + 2 * P + 130 + I;
    if (n_vars >= 0x7FFFFFFFull || n_gates >= 0x7FFFFFFFull) return false;
    s.width = width; s.half_full = half_full; s.partial = partial; s.inputs = inputs; s.height = height;
    s.P = (uint32_t)P;
    s.hash_off = (uint32_t)(P - 1 - (W - 2) * W);
    s.per_level = (uint32_t)(6 + P);
    s.note_vars = (uint32_t)note_vars;
    s.note_rows = (uint32_t)note_rows;
    s.note0 = (uint32_t)(2 * I + 1);
    s.glob0 = (uint32_t)(2 * I + 1 + I * note_vars);
    s.row_glob0 = (uint32_t)(1 + I * note_rows);
    s.n_vars = n_vars;
    s.n_gates = n_gates;
    s.n_hashes = (uint32_t)(I * (3 + H) + 2);
    s.n_pi = (uint32_t)(I + 4);
    return true;
}

struct Plan {
    Shape s;
    std::vector<HashCall> calls;
    std::vector<GlueRow> glue;
    std::vector<size_t> pi_pos;
};

// the walk: withdraw.rs:57-150 statement by statement, allocating variables and rows as the composer does.  Returns false
// if the closed form of Shape disagrees with it anywhere (a bug, never an input).
inline bool plan_make(const Shape& s, Plan& pl) {
    pl.s = s;
    pl.calls.clear();
    pl.glue.clear();
    pl.pi_pos.clear();
    const int I = s.inputs, H = s.height;
    uint32_t var = 0, row = 0;
    bool ok = true;
    auto glue = [&](uint32_t l, uint32_t r, uint32_t o, uint8_t qm, uint8_t ql, uint8_t qr, uint8_t qo, uint8_t qc, uint8_t lk) {
        GlueRow g{};
        g.row = row++;
        g.w[0] = l; g.w[1] = r; g.w[2] = o;
        g.q[0] = qm; g.q[1] = ql; g.q[2] = qr; g.q[3] = qo; g.q[4] = qc; g.q[5] = lk;
        pl.glue.push_back(g);
    };
    auto pub = [&](uint32_t v) {                      // set_variable_public, mod.rs:216-240
        pl.pi_pos.push_back(row);
        glue(REF_ZERO, REF_ZERO, v, G_0, G_0, G_0, G_M1, G_0, G_0);
    };
    auto hash = [&](int arity, uint32_t a, uint32_t b, uint32_t c) {
        HashCall h{};
        h.row = row; h.base = var; h.arity = (uint32_t)arity;
        h.in[0] = a; h.in[1] = b; h.in[2] = c;
        pl.calls.push_back(h);
        row += s.P;
        var += s.P;
        return h.base + s.hash_off;
    };
    var = (uint32_t)(2 * I);                           // amounts, identifiers
    const uint32_t root = var++;
    ok &= root == s.root_var();
    pub(root);
    for (int k = 0; k < I; ++k) {
        ok &= row == 1 + (uint32_t)k * s.note_rows;
        const uint32_t secret = var++;
        ok &= secret == s.secret_var(k) && var == s.commit_base(k);
        const uint32_t commitment = hash(1, secret, REF_ZERO, REF_ZERO);
        const uint32_t inv = var++;                    // div_gate(1, secret): secret z - 1 = 0, wires (secret, z, Zero)
        ok &= inv == s.inv_var(k) && var == s.null_base(k);
        glue(secret, inv, REF_ZERO, G_1, G_0, G_0, G_M1, G_M1, G_0);
        const uint32_t nullifier = hash(1, inv, REF_ZERO, REF_ZERO);
        ok &= row == s.null_row(k);
        pub(nullifier);
        ok &= var == s.leaf_base(k);
        uint32_t cur = hash(3, s.ident_var(k), s.amount_var(k), commitment);
        ok &= var == s.bit0(k);
        const uint32_t b0 = var;
        for (int l = 0; l < H; ++l) {                  // PoECircuit::synthesize, binary.rs:42-78
            const uint32_t b = var++;
            glue(b, b, b, G_1, G_0, G_0, G_M1, G_0, G_0);          // boolean_gate
        }
        const uint32_t s0 = var;
        var += (uint32_t)H;
        ok &= s0 == s.sib0(k) && var == s.path_base(k);
        for (int l = 0; l < H; ++l) {                  // merkle_proof, binary.rs:8-30
            const uint32_t b = b0 + (uint32_t)l, sv = s0 + (uint32_t)l;
            uint32_t pair[2];
            for (int side = 0; side < 2; ++side) {     // conditional_select(bit, a, o), mod.rs:318-373
                const uint32_t a = side == 0 ? sv : cur, o = side == 0 ? cur : sv;
                const uint32_t x = var++, y = var++, z = var++;
                glue(b, a, x, G_1, G_0, G_0, G_M1, G_0, G_0);
                glue(b, o, y, G_M1, G_0, G_1, G_M1, G_0, G_0);
                glue(x, y, z, G_0, G_1, G_1, G_M1, G_0, G_0);
                pair[side] = z;
            }
            cur = hash(2, pair[0], pair[1], REF_ZERO);
        }
        ok &= cur == s.path_root(k);
        glue(cur, root, REF_ZERO, G_0, G_1, G_M1, G_0, G_0, G_0);  // equal_constrain(root, pub_root)
        const uint32_t lk = var++;
        ok &= lk == s.lookup_var(k);
        glue(s.ident_var(k), REF_ZERO, lk, G_0, G_1, G_0, G_M1, G_0, G_1);   // lookup_constrain(identifier)
    }
    ok &= var == s.glob0 && row == s.row_glob0;
    std::vector<uint32_t> vs;
    for (int k = 0; k < 64; ++k) {
        const uint32_t b = var++;
        glue(b, b, b, G_1, G_0, G_0, G_M1, G_0, G_0);
        vs.push_back(b);
    }
    ok &= var == s.recomb0();
    uint8_t mult = G_2;
    while (vs.size() > 1) {                            // bits_le_constrain
        std::vector<uint32_t> nxt;
        for (size_t k = 0; k < vs.size(); k += 2) {
            const uint32_t nv = var++;
            glue(vs[k], vs[k + 1], nv, G_0, G_1, mult, G_M1, G_0, G_0);
            nxt.push_back(nv);
        }
        vs.swap(nxt);
        ++mult;
    }
    ok &= mult == G_COUNT && vs[0] == s.out_var() && var == s.sum0();
    uint32_t right = REF_ZERO;
    for (int k = 1; k < I; ++k) {
        const uint32_t nv = var++;
        glue(right, s.amount_var(k), nv, G_0, G_1, G_1, G_M1, G_0, G_0);
        right = nv;
    }
    ok &= row == s.balance_row();
    pl.pi_pos.push_back(row);
    glue(s.amount_var(0), right, vs[0], G_0, G_M1, G_M1, G_1, G_0, G_0);     // withdraw.rs: the balance gate, public withdraw_amount
    const uint32_t ns = var++, ni = var++;
    ok &= ns == s.new_secret_var() && ni == s.new_ident_var() && var == s.new_commit_base();
    const uint32_t nc = hash(1, ns, REF_ZERO, REF_ZERO);
    ok &= var == s.new_leaf_base();
    const uint32_t nl = hash(3, ni, vs[0], nc);
    pub(ni);
    pub(nl);
    ok &= var == s.n_vars && row == s.n_gates && pl.calls.size() == s.n_hashes && pl.pi_pos.size() == s.n_pi;
    ok &= pl.glue.size() + (size_t)s.n_hashes * s.P == s.n_gates;
    return ok;
}

// One hash's rows relative to its first variable.  sel: q_m, q_l, q_r, q_o, q_c (q_lookup is 0 on every hash row).
template <class P>
struct Template {
    std::vector<Fe<P>> sel[5];
    std::vector<uint32_t> w[3];
};

// rc: (2 half_full + partial) x width, mds: width x width row major (m[i][j]), tag: one scalar; Montgomery form
template <class P>
inline void template_make(const Shape& s, const Fe<P>* rc, const Fe<P>* mds, const Fe<P>& tag, int arity, Template<P>& t) {
    const int W = s.width;
    const Fe<P> zero = fe_zero<P>(), one = fe_one<P>(), m1 = fe_neg<P>(fe_one<P>());
    for (auto& v : t.sel) v.clear();
    for (auto& v : t.w) v.clear();
    auto push = [&](uint32_t l, uint32_t r, uint32_t o, const Fe<P>& qm, const Fe<P>& ql, const Fe<P>& qr, const Fe<P>& qc) {
        t.w[0].push_back(l); t.w[1].push_back(r); t.w[2].push_back(o);
        t.sel[0].push_back(qm); t.sel[1].push_back(ql); t.sel[2].push_back(qr); t.sel[3].push_back(m1); t.sel[4].push_back(qc);
    };
    uint32_t v[MAX_WIDTH];     // the state as LTVariables with coefficient 1: (variable, offset)
    Fe<P> o[MAX_WIDTH];
    for (int i = 0; i < W; ++i) {
        v[i] = (i >= 1 && i <= arity) ? (REF_INPUT | (uint32_t)(i - 1)) : REF_ZERO;
        o[i] = i == 0 ? tag : zero;
    }
    uint32_t tv = 0;
    size_t k = 0;
    for (int r = 0; r < 2 * s.half_full + s.partial; ++r) {
        const bool full = r < s.half_full || r >= s.half_full + s.partial;
        for (int i = 0; i < W; ++i) o[i] = fe_add<P>(o[i], rc[k + i]);          // add_constant: offsets only
        k += (size_t)W;
        for (int i = 0; i < (full ? W : 1); ++i) {
            // (v + o)^2 = v v + o v + o v + o^2 ; x^4 = x^2 x^2 ; x^5 = x^4 (v + o) = x^4 v + o x^4
            push(v[i], v[i], tv, one, o[i], o[i], fe_mul<P>(o[i], o[i]));
            push(tv, tv, tv + 1, one, zero, zero, zero);
            push(tv + 1, v[i], tv + 2, one, o[i], zero, zero);
            v[i] = tv + 2;
            o[i] = zero;
            tv += 3;
        }
        uint32_t nv[MAX_WIDTH];
        for (int j = 0; j < W; ++j) {
            uint32_t acc = REF_ZERO;
            for (int i = 0; i < W; ++i) {
                const Fe<P>& m = mds[(size_t)i * W + j];
                push(acc, v[i], tv, zero, one, m, fe_mul<P>(o[i], m));           // acc + m (v + o) = new
                acc = tv++;
            }
            nv[j] = acc;
        }
        for (int j = 0; j < W; ++j) {
            v[j] = nv[j];
            o[j] = zero;
        }
    }
}

template <class P>
inline void glue_consts(Fe<P>* out /* G_COUNT */) {
    out[G_0] = fe_zero<P>();
    out[G_1] = fe_one<P>();
    out[G_M1] = fe_neg<P>(fe_one<P>());
    Fe<P> x = fe_add<P>(out[G_1], out[G_1]);
    for (int k = G_2; k < G_COUNT; ++k) {
        out[k] = x;
        x = fe_mul<P>(x, x);
    }
}

inline uint32_t relocate(uint32_t ref, const HashCall& h) {
    if (ref == REF_ZERO) return ref;
    return (ref & REF_INPUT) ? h.in[ref & ~REF_INPUT] : h.base + ref;
}

// The rows written out on the host: what the two layout kernels of withdraw.hip write on the device.  sel[6] / w[3]:
// n_gates entries each, any of them may be null.
template <class P>
inline void expand_host(const Plan& pl, const Template<P>* tmpl /* by arity, 1..3 at [1..3] */, Fe<P>* const* sel, uint32_t* const* w) {
    Fe<P> gc[G_COUNT];
    glue_consts<P>(gc);
    for (const HashCall& h : pl.calls) {
        const Template<P>& t = tmpl[h.arity];
        for (uint32_t r = 0; r < pl.s.P; ++r) {
            const size_t row = (size_t)h.row + r;
            for (int q = 0; q < 5; ++q)
                if (sel[q]) sel[q][row] = t.sel[q][r];
            if (sel[5]) sel[5][row] = gc[G_0];
            for (int x = 0; x < 3; ++x)
                if (w[x]) w[x][row] = relocate(t.w[x][r], h);
        }
    }
    for (const GlueRow& g : pl.glue) {
        for (int q = 0; q < 6; ++q)
            if (sel[q]) sel[q][g.row] = gc[g.q[q]];
        for (int x = 0; x < 3; ++x)
            if (w[x]) w[x][g.row] = g.w[x];
    }
}

}  // namespace withdraw
}  // namespace zkt
