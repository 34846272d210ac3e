// Witness completion from the circuit's free variables: the host planner (witness_plan.hip holds the kernels;
// include/zkt_plonk.h, zkt_witness_plan_create, states the rule as part of the interface).
// Measured on an MI355X (docs/EXPERIMENTS.md, "witness completion from the free variables"): the BN254 2^20 withdrawal
// (1 019 498 gates, depth 33 853) completes in 78.9 ms at batch 1 and 85.2 ms at batch 64, 2.3 us a level; its plan is made
// in 143 ms and holds 33 MB.
//
// Row i asserts  q_m a b + q_l a + q_r b + q_o c + q_c + PI_i = 0  with a = x[w_l[i]], b = x[w_r[i]], c = x[w_o[i]].  The rows
// are walked in ascending order; a variable is UNSEEN at row i when it stands on no wire of a row before i.  Variable::Zero
// and rows >= n_rows define nothing.
//   public-input row   defines nothing; PI_i = -(q_m a b + q_l a + q_r b + q_o c + q_c) is an output
//   rule Z             only under WP_RULES_IS_ZERO (ZKT_WITNESS_RULE_IS_ZERO), tried before rule O: neither row i nor row i + 1
//                      public, i + 1 < n_rows; row i = (x, y, z) with q_m != 0, q_o != 0, q_l = q_r = 0 (q_c arbitrary), y and z
//                      real, unseen, distinct from each other and from x, x real or Zero; row i + 1 = (x, z, Zero) with
//                      q_m != 0 and q_l = q_r = q_o = q_c = 0 (it asserts x z = 0).  Row i then defines both:
//                          x = 0:   y = 0, z = -q_c / q_o          x != 0:   z = 0, y = -q_c / (q_m x)
//                      (should_be_zero_with_output, mod.rs:243-289: y = x^-1 or 0, z = (x == 0)); never unsolvable; row i + 1
//                      defines nothing; level(y) = level(z) = 1 + level(x).  A clause that fails: rules O and R as ever.
//   rule O             otherwise, q_o[i] != 0 and v = w_o[i] real, unseen, different from w_l[i] and w_r[i]:
//                          v = -(q_m a b + q_l a + q_r b + q_c) / q_o
//                      (add, sub, mul, square, linear_transform, the selects' three rows, bits_le, the lookup copy)
//   rule R             otherwise, v = w_r[i] real, unseen, different from w_l[i] and w_o[i], and w_l[i], w_o[i] each Zero or
//                      seen:   v = -(q_l a + q_o c + q_c) / (q_m a + q_r)      (div_gate, arithmetic.rs:104-130)
//                      a zero denominator is a property of the witness: v = 0 and the row is reported
//   free               every other variable first seen on some wire; a boolean row (x, x, x) defines nothing by the "different
//                      from" clauses; a variable on no wire is never touched.  There is no left-wire rule.
// level(v) of a defined variable = 1 + the largest level of the other two wires of its row; free variables and Zero: 0.
// Rows of one level read only variables of lower levels, so a level is evaluated in any order.
//
// Schedule: the defining rows sorted by level (counting sort, stable in the row), level_start[l] .. level_start[l + 1]
// the rows of level l (level_start[0] = level_start[1] = 0).  Per scheduled row a 32-byte record: the two variables it
// reads, the one it writes (rule Z: the two), its row, flags, and the index of its coefficient tuple.  Tuples (five scalars, 160 B) are kept
// once per distinct value: a Poseidon circuit repeats a few hundred of them a million times.
//   rule O tuple   t_k = -q_k / q_o for k = m, l, r, c (slot 3 unused):  v = t_m a b + t_l a + t_r b + t_c, no inversion
//   rule R tuple   (q_m, -q_l, q_r, -q_o, -q_c):                          v = (t_l a + t_o c + t_c) / (t_m a + t_r)
//   rule Z tuple   t_m = -q_c / q_m, t_o = -q_c / q_o (one record per pair, out = y, out2 = z; slot l is WP_ZERO when x is
//                  Variable::Zero and WP_ONE otherwise):                   x = 0: y = 0, z = t_o;  else z = 0, y = t_m / x
// Flags carry two bits per slot (WP_GEN / WP_ZERO / WP_ONE / WP_MINUS_ONE), so that the kernel skips the product: a mul gate
// is one product, an add gate none.  A slot whose variable is Variable::Zero is flagged WP_ZERO, so the kernel never loads
// through such an index.
// Device bytes of a plan (zkt_witness_plan_info device_bytes):  32 B x scheduled rows + 160 B x distinct tuples
// + 4 B x (depth + 2) + 192 B x n_pi (the public rows: three indices and five raw selectors, padded) + the status block of
// 16 B x ZKT_WITNESS_BATCH_MAX, each rounded up to 256 B.
#pragma once
#include "fp.hpp"
#include "fx.hpp"
#include "hostinv.hpp"

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

namespace zkt {

constexpr uint32_t WP_VAR_ZERO = 0xFFFFFFFFu;   // ZKT_VARIABLE_ZERO
constexpr uint32_t WP_NO_ROW = 0xFFFFFFFFu;
constexpr int WP_MAX_LAUNCHES = 64;
enum { WP_UNUSED = 0, WP_FREE = 1, WP_OUT = 2, WP_RIGHT = 3, WP_ZINV = 4, WP_ZFLAG = 5 };   // kind (4, 5: rule Z's y and z)
enum { WP_GEN = 0, WP_ZERO = 1, WP_ONE = 2, WP_MINUS_ONE = 3 };         // a slot's two flag bits
enum { WP_M = 0, WP_L = 1, WP_R = 2, WP_O = 3, WP_C = 4 };              // slots
constexpr uint32_t WP_RULE_R = 1u << 31;
constexpr uint32_t WP_RULE_Z = 1u << 30;
constexpr uint32_t WP_RULES_IS_ZERO = 1;   // ZKT_WITNESS_RULE_IS_ZERO

struct alignas(32) WpRow {
    uint32_t in0;     // w_l
    uint32_t in1;     // rule O: w_r; rule R: w_o
    uint32_t out;     // rule Z: y
    uint32_t row;
    uint32_t flags;
    uint32_t coef;    // tuple index
    uint32_t out2;    // rule Z: z
    uint32_t pad;
};
static_assert(sizeof(WpRow) == 32, "one scheduled row = 32 bytes");

template <class R>
struct WpTuple {
    Fe<R> t[5];
};
template <class R>
struct WpPublic {   // a public-input row: raw selectors, wires (WP_VAR_ZERO for a padded row)
    uint32_t w[3];
    uint32_t pad;
    Fe<R> q[5];
    uint32_t pad2[4];
};

template <class R>
struct WitnessPlan {
    std::vector<uint8_t> kind;           // per variable
    std::vector<uint32_t> def_row;       // per variable: its defining row, WP_NO_ROW when none
    std::vector<uint32_t> level;         // per variable
    std::vector<WpRow> rows;             // the schedule
    std::vector<uint32_t> level_start;   // depth + 2 entries
    std::vector<WpTuple<R>> tuples;
    uint64_t n_free = 0, n_out = 0, n_right = 0, n_unused = 0, n_pairs = 0;   // n_pairs: rule-Z records (two variables each)
    uint32_t depth = 0, max_level_rows = 0;
};

ZKT_HD uint32_t wp_flag(uint32_t flags, int slot) { return (flags >> (2 * slot)) & 3u; }

// sel[0..4] = q_m q_l q_r q_o q_c, at least n_rows evaluations each (Montgomery form); w[0..2] = w_l w_r w_o, n_rows indices each
// (an index >= n_vars is read as Variable::Zero: the C-ABI refuses such wiring before it gets here); pi_pos ascending;
// rules: WP_RULES_IS_ZERO or 0
template <class R>
void witness_plan_make(const Fe<R>* const* sel, const uint32_t* const* w, size_t n_rows, size_t n_vars, const size_t* pi_pos,
                       size_t n_pi, WitnessPlan<R>& W, uint32_t rules = 0) {
    using F = Fe<R>;
    W = WitnessPlan<R>{};
    W.kind.assign(n_vars, WP_UNUSED);
    W.def_row.assign(n_vars, WP_NO_ROW);
    W.level.assign(n_vars, 0);
    std::vector<bool> seen(n_vars, false);
    auto real = [&](uint32_t v) { return (size_t)v < n_vars; };
    auto lvl = [&](uint32_t v) { return real(v) ? W.level[v] : 0u; };
    std::vector<uint32_t> def_rows;   // in row order
    size_t next_pi = 0;
    for (size_t i = 0; i < n_rows; ++i) {
        const uint32_t a = w[0][i], b = w[1][i], o = w[2][i];
        while (next_pi < n_pi && pi_pos[next_pi] < i) ++next_pi;
        const bool is_pi = next_pi < n_pi && pi_pos[next_pi] == i;
        if (!is_pi) {
            uint32_t v = WP_VAR_ZERO, other = 0;
            int kind = 0;
            bool pair = false;
            if ((rules & WP_RULES_IS_ZERO) && i + 1 < n_rows && !(next_pi < n_pi && pi_pos[next_pi] == i + 1)) {
                const size_t j = i + 1;
                auto zero = [&](int k, size_t r) { return fe_is_zero<R>(sel[k][r]); };
                pair = !zero(WP_M, i) && !zero(WP_O, i) && zero(WP_L, i) && zero(WP_R, i) && real(b) && real(o) && !seen[b] && !seen[o] &&
                       b != o && b != a && o != a && (real(a) ? w[0][j] == a : !real(w[0][j])) && w[1][j] == o && !real(w[2][j]) &&
                       !zero(WP_M, j) && zero(WP_L, j) && zero(WP_R, j) && zero(WP_O, j) && zero(WP_C, j);
            }
            if (pair) {
                W.kind[b] = WP_ZINV;
                W.kind[o] = WP_ZFLAG;
                W.def_row[b] = W.def_row[o] = (uint32_t)i;
                W.level[b] = W.level[o] = 1 + lvl(a);
                if (W.level[o] > W.depth) W.depth = W.level[o];
                def_rows.push_back((uint32_t)i);
                ++W.n_pairs;
            } else if (!fe_is_zero<R>(sel[WP_O][i]) && real(o) && !seen[o] && o != a && o != b) {
                v = o; other = b; kind = WP_OUT;
            } else if (real(b) && !seen[b] && b != a && b != o && (!real(a) || seen[a]) && (!real(o) || seen[o])) {
                v = b; other = o; kind = WP_RIGHT;
            }
            if (kind) {
                W.kind[v] = (uint8_t)kind;
                W.def_row[v] = (uint32_t)i;
                const uint32_t la = lvl(a), lo = lvl(other);
                W.level[v] = 1 + (la > lo ? la : lo);
                if (W.level[v] > W.depth) W.depth = W.level[v];
                def_rows.push_back((uint32_t)i);
            }
        }
        const uint32_t three[3] = {a, b, o};
        for (uint32_t v : three)
            if (real(v)) {
                if (W.kind[v] == WP_UNUSED) W.kind[v] = WP_FREE;
                seen[v] = true;
            }
    }
    for (size_t v = 0; v < n_vars; ++v) {
        const uint8_t k = W.kind[v];
        if (k == WP_ZINV || k == WP_ZFLAG) continue;   // counted by the pair
        ++(k == WP_FREE ? W.n_free : k == WP_OUT ? W.n_out : k == WP_RIGHT ? W.n_right : W.n_unused);
    }

    // counting sort by level, stable in the row
    W.level_start.assign((size_t)W.depth + 2, 0);
    auto row_var = [&](uint32_t i) {   // the variable row i defines
        const uint32_t o = w[2][i];
        return real(o) && W.def_row[o] == i ? o : w[1][i];
    };
    for (uint32_t i : def_rows) ++W.level_start[(size_t)W.level[row_var(i)] + 1];
    for (size_t l = 0; l + 1 < W.level_start.size(); ++l) {
        const uint32_t cnt = W.level_start[l + 1];
        if (cnt > W.max_level_rows) W.max_level_rows = cnt;
        W.level_start[l + 1] += W.level_start[l];
    }
    std::vector<uint32_t> at(W.level_start.begin(), W.level_start.end() - 1);
    W.rows.resize(def_rows.size());

    const F one = fe_one<R>(), minus_one = fe_neg<R>(fe_one<R>());
    auto flag_of = [&](const F& x) -> uint32_t {
        return fe_is_zero<R>(x) ? WP_ZERO : fe_eq<R>(x, one) ? WP_ONE : fe_eq<R>(x, minus_one) ? WP_MINUS_ONE : WP_GEN;
    };
    std::unordered_map<std::string, uint32_t> ids;
    std::unordered_map<std::string, F> neg_inv;   // -1 / q by value (q_o; rule Z: q_m too): a circuit has a handful
    auto neg_inv_of = [&](const F& q) -> F {
        if (fe_eq<R>(q, minus_one)) return one;
        if (fe_eq<R>(q, one)) return minus_one;
        const std::string key((const char*)q.v, sizeof(q.v));
        auto it = neg_inv.find(key);
        if (it == neg_inv.end()) it = neg_inv.emplace(key, fe_neg<R>(fe_inv_host<R>(q))).first;
        return it->second;
    };
    for (uint32_t i : def_rows) {
        const uint32_t v = row_var(i);
        const bool right = W.kind[v] == WP_RIGHT, pair = W.kind[v] == WP_ZFLAG;
        WpTuple<R> T;
        for (F& x : T.t) x = fe_zero<R>();
        WpRow r{};
        r.in0 = real(w[0][i]) ? w[0][i] : WP_VAR_ZERO;
        r.out = v;
        r.row = i;
        if (pair) {
            r.in1 = WP_VAR_ZERO;
            r.out = w[1][i];
            r.out2 = v;
            T.t[WP_M] = fe_mul<R>(neg_inv_of(sel[WP_M][i]), sel[WP_C][i]);
            T.t[WP_O] = fe_mul<R>(neg_inv_of(sel[WP_O][i]), sel[WP_C][i]);
            r.flags = WP_RULE_Z | flag_of(T.t[WP_M]) << (2 * WP_M) | (uint32_t)(r.in0 == WP_VAR_ZERO ? WP_ZERO : WP_ONE) << (2 * WP_L) |
                      (uint32_t)WP_ZERO << (2 * WP_R) | flag_of(T.t[WP_O]) << (2 * WP_O) | (uint32_t)WP_ZERO << (2 * WP_C);
        } else if (!right) {
            const uint32_t b = w[1][i];
            r.in1 = real(b) ? b : WP_VAR_ZERO;
            const F s = neg_inv_of(sel[WP_O][i]);
            const int slots[4] = {WP_M, WP_L, WP_R, WP_C};
            for (int k : slots) T.t[k] = fe_eq<R>(s, one) ? sel[k][i] : fe_mul<R>(s, sel[k][i]);
            const bool za = r.in0 == WP_VAR_ZERO, zb = r.in1 == WP_VAR_ZERO;
            r.flags = (za || zb ? WP_ZERO : flag_of(T.t[WP_M])) << (2 * WP_M) | (za ? WP_ZERO : flag_of(T.t[WP_L])) << (2 * WP_L) |
                      (zb ? WP_ZERO : flag_of(T.t[WP_R])) << (2 * WP_R) | (uint32_t)WP_ZERO << (2 * WP_O) |
                      flag_of(T.t[WP_C]) << (2 * WP_C);
        } else {
            const uint32_t o = w[2][i];
            r.in1 = real(o) ? o : WP_VAR_ZERO;
            T.t[WP_M] = sel[WP_M][i];
            T.t[WP_L] = fe_neg<R>(sel[WP_L][i]);
            T.t[WP_R] = sel[WP_R][i];
            T.t[WP_O] = fe_neg<R>(sel[WP_O][i]);
            T.t[WP_C] = fe_neg<R>(sel[WP_C][i]);
            const bool za = r.in0 == WP_VAR_ZERO, zo = r.in1 == WP_VAR_ZERO;
            r.flags = WP_RULE_R | (za ? WP_ZERO : flag_of(T.t[WP_M])) << (2 * WP_M) | (za ? WP_ZERO : flag_of(T.t[WP_L])) << (2 * WP_L) |
                      flag_of(T.t[WP_R]) << (2 * WP_R) | (zo ? WP_ZERO : flag_of(T.t[WP_O])) << (2 * WP_O) |
                      flag_of(T.t[WP_C]) << (2 * WP_C);
        }
        // a slot that the flags make unread is stored as zero, so that equal behaviour is one tuple
        for (int k = 0; k < 5; ++k)
            if (wp_flag(r.flags, k) != WP_GEN) T.t[k] = fe_zero<R>();
        const std::string key((const char*)T.t, sizeof(T.t));
        auto it = ids.find(key);
        if (it == ids.end()) {
            it = ids.emplace(key, (uint32_t)W.tuples.size()).first;
            W.tuples.push_back(T);
        }
        r.coef = it->second;
        W.rows[at[W.level[v]]++] = r;
    }
}

// The launches that fill the map under the threshold wide_min_rows (>= 1): a level with at least that many rows is a launch
// of its own (wide, a thread per (witness, row)), a run of narrower levels between two such is one launch of one workgroup
// per witness (narrow).  More than WP_MAX_LAUNCHES: one narrow launch altogether.  The closing public-input launch is not
// among them.
struct WpLaunch {
    uint32_t level0, level1;   // levels [level0, level1)
    bool wide;
};
inline std::vector<WpLaunch> witness_plan_split(const std::vector<uint32_t>& level_start, uint32_t depth, uint32_t wide_min_rows) {
    std::vector<WpLaunch> out;
    for (uint32_t l = 1; l <= depth; ++l) {
        const bool wide = level_start[l + 1] - level_start[l] >= wide_min_rows;
        if (!wide && !out.empty() && !out.back().wide) out.back().level1 = l + 1;
        else out.push_back(WpLaunch{l, l + 1, wide});
    }
    if (out.size() > (size_t)WP_MAX_LAUNCHES) out.assign(1, WpLaunch{1, depth + 1, false});
    return out;
}

}  // namespace zkt
