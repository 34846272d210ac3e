// The withdraw circuit as a library component (include/zkt_plonk.h, "The withdraw circuit"): its rows made on the device
// from (Poseidon parameters, INPUTS, HEIGHT), its setup, and the whole variable map and public inputs of a batch of
// withdrawals made on the device from the notes themselves.  The planner is host code (withdraw_layout.hpp); the hash
// traces, the Merkle paths and the note tree are the existing entry points of poseidon.hip, called as any caller would.
#include "circuit.hpp"
#include "ctx.hpp"
#include "hostinv.hpp"
#include "merkle_tree.hpp"
#include "withdraw_layout.hpp"

#include <algorithm>
#include <array>
#include <cstring>
#include <map>
#include <memory>
#include <vector>

namespace zkt {

namespace wd = withdraw;

// ---- layout kernels -----------------------------------------------------------------------------------------------------
template <class P>
struct WdHashRowsArgs {
    const wd::HashCall* calls;
    const Fe<P>* tsel[4];        // by arity: 5 x per_hash selectors (q_m, q_l, q_r, q_o, q_c)
    const uint32_t* tw[4];       // by arity: 3 x per_hash wire references
    Fe<P>* sel[6];               // outputs, n_gates each; all six or none
    uint32_t* w[3];              // outputs, n_gates each; all three or none
    uint32_t per_hash;
    uint64_t total;              // n_hashes x per_hash
};

// One thread per (hash call, template row): consecutive threads write consecutive rows of every vector.
template <class P>
__global__ __launch_bounds__(256) void k_withdraw_hash_rows(WdHashRowsArgs<P> a) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.total) return;
    const uint32_t h = (uint32_t)(t / a.per_hash), r = (uint32_t)(t - (uint64_t)h * a.per_hash);
    const wd::HashCall c = a.calls[h];
    const size_t row = (size_t)c.row + r;
    if (a.sel[0]) {
        const Fe<P>* ts = a.tsel[c.arity];
#pragma unroll
        for (int q = 0; q < 5; ++q) fe_store<P>(a.sel[q] + row, fe_load<P>(ts + (size_t)q * a.per_hash + r));
        fe_store<P>(a.sel[5] + row, fe_zero<P>());
    }
    if (a.w[0]) {
        const uint32_t* tw = a.tw[c.arity];
#pragma unroll
        for (int x = 0; x < 3; ++x) {
            const uint32_t ref = tw[(size_t)x * a.per_hash + r];
            uint32_t v = ref;
            if (ref != wd::REF_ZERO) v = (ref & wd::REF_INPUT) ? c.in[(ref & 3u) % 3u] : c.base + ref;
            a.w[x][row] = v;
        }
    }
}

template <class P>
struct WdGlueRowsArgs {
    const wd::GlueRow* glue;
    Fe<P> consts[wd::G_COUNT];
    Fe<P>* sel[6];
    uint32_t* w[3];
    uint32_t total;
};

template <class P>
__global__ __launch_bounds__(256) void k_withdraw_glue_rows(WdGlueRowsArgs<P> a) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.total) return;
    const wd::GlueRow g = a.glue[t];
    if (a.sel[0]) {
#pragma unroll
        for (int q = 0; q < 6; ++q) fe_store<P>(a.sel[q] + g.row, a.consts[g.q[q] < wd::G_COUNT ? g.q[q] : 0]);
    }
    if (a.w[0]) {
#pragma unroll
        for (int x = 0; x < 3; ++x) a.w[x][g.row] = g.w[x];
    }
}

// q_table as zkt_circuit_setup documents it: 0 for the first table_size rows, 1 after
template <class P>
__global__ __launch_bounds__(256) void k_withdraw_table_mask(Fe<P>* out, uint64_t table_size, uint64_t n) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    fe_store<P>(out + t, t < table_size ? fe_zero<P>() : fe_one<P>());
}

// ---- witness kernels ----------------------------------------------------------------------------------------------------
// The closed form of the variable numbering, as the kernels need it (withdraw_layout.hpp Shape)
struct WdShapeDev {
    uint32_t inputs, height, P, hash_off, per_level, note_vars, note0, glob0, n_pi;
};

// The staged requests of one call (device copy of the handle's pinned buffer): per request 2 I + 3 scalars (secrets,
// identifiers, root, new_secret, new_identifier), 2 I + 4 words (amounts, leaf indices, amount_out, withdraw_amount,
// siblings given, unused), I x H siblings.
template <class P>
struct WdStage {
    const Fe<P>* fe;
    const uint64_t* u;
    const Fe<P>* sib;
};

template <class P>
struct WdBaseArgs {
    WdShapeDev s;
    WdStage<P> st;
    Fe<P>* vars;
    uint64_t stride;
    uint32_t per_request;    // threads one request takes
};

template <class P>
ZKT_D Fe<P> wd_bit(uint64_t b) {
    return b ? fe_one<P>() : fe_zero<P>();
}

// Every variable that is neither a hash trace nor a select: grid.y = request, one thread per variable or small group.
template <class P>
__global__ __launch_bounds__(128) void k_withdraw_base(WdBaseArgs<P> a) {
    uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= a.per_request) return;
    const uint32_t b = blockIdx.y, I = a.s.inputs, H = a.s.height;
    const Fe<P>* fe = a.st.fe + (size_t)b * (2 * I + 3);
    const uint64_t* u = a.st.u + (size_t)b * (2 * I + 4);
    Fe<P>* v = a.vars + (size_t)b * a.stride;
    if (j < I) {                                         // note j: amount, identifier, secret, 1 / secret, the lookup copy
        const uint32_t sv = a.s.note0 + j * a.s.note_vars;
        const Fe<P> secret = fe_load<P>(fe + j), ident = fe_load<P>(fe + I + j);
        fe_store<P>(v + j, fe_from_u64<P>(u[j]));
        fe_store<P>(v + I + j, ident);
        fe_store<P>(v + sv, secret);
        fe_store<P>(v + sv + 1 + a.s.P, fe_inv<P>(secret));              // div_gate(1, secret)
        fe_store<P>(v + sv + 2 + 3 * a.s.P + 2 * H + H * a.s.per_level, ident);
        return;
    }
    j -= I;
    if (j == 0) {
        fe_store<P>(v + 2 * I, fe_load<P>(fe + 2 * I));                  // root
        fe_store<P>(v + a.s.glob0 + 126 + I, fe_load<P>(fe + 2 * I + 1));   // new_secret
        fe_store<P>(v + a.s.glob0 + 127 + I, fe_load<P>(fe + 2 * I + 2));   // new_identifier
        return;
    }
    j -= 1;
    const uint64_t amount_out = u[2 * I];
    if (j < 64) {                                        // view_bits::<Lsb0>() of amount_out
        fe_store<P>(v + a.s.glob0 + j, wd_bit<P>((amount_out >> j) & 1));
        return;
    }
    j -= 64;
    if (j < 63) {                                        // bits_le_constrain: level l holds 32 >> l sums of 2 << l bits each
        uint32_t l = 0, first = 0;
        while (j >= first + (32u >> l)) {
            first += 32u >> l;
            ++l;
        }
        const uint32_t width = 2u << l, idx = j - first;
        const uint64_t x = amount_out >> (idx * width);                   // idx * width <= 62
        fe_store<P>(v + a.s.glob0 + 64 + j, fe_from_u64<P>(width == 64 ? x : x & (((uint64_t)1 << width) - 1)));
        return;
    }
    j -= 63;
    if (j < I - 1) {                                     // the running sums amounts[1] + .. + amounts[j + 1] (no overflow: checked)
        uint64_t sum = 0;
        for (uint32_t k = 1; k <= j + 1; ++k) sum += u[k];
        fe_store<P>(v + a.s.glob0 + 127 + j, fe_from_u64<P>(sum));
        return;
    }
    j -= I - 1;
    {                                                    // position bit and sibling (note k, level l)
        const uint32_t k = j / H, l = j - k * H;
        const uint32_t b0 = a.s.note0 + k * a.s.note_vars + 2 + 3 * a.s.P;
        fe_store<P>(v + b0 + l, wd_bit<P>((u[I + k] >> l) & 1));
        if (u[2 * I + 2]) fe_store<P>(v + b0 + H + l, fe_load<P>(a.st.sib + ((size_t)b * I + k) * H + l));
    }
}

struct WdExpandArgs {
    const uint32_t* rel;
    uint32_t* out;
    uint32_t off[9];         // the eight vectors' first entries in rel, and its length
    uint64_t stride;
    uint32_t batch;
};

// The index vectors of the gadget and path launches for every batch slot: slot b's entries are request 0's plus b x stride.
// Vector v of the output starts at off[v] x batch and holds batch x (off[v + 1] - off[v]) entries, slot-major.
__global__ __launch_bounds__(256) void k_withdraw_expand(WdExpandArgs a) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (j >= a.off[8] || b >= a.batch) return;
    int v = 0;
    while (v < 7 && j >= a.off[v + 1]) ++v;
    const uint32_t len = a.off[v + 1] - a.off[v];
    a.out[(size_t)a.off[v] * a.batch + (size_t)b * len + (j - a.off[v])] = a.rel[j] + (uint32_t)(b * a.stride);
}

template <class P>
struct WdCloseArgs {
    WdShapeDev s;
    const uint64_t* u;
    const Fe<P>* vars;
    uint64_t stride;
    Fe<P>* pi;               // batch x n_pi
    uint32_t* status;        // batch
};

// The public inputs in position order (root, nullifiers, withdraw_amount, new_identifier, new_leaf), and per request the
// notes whose path does not end in the root.  grid.y = request.
template <class P>
__global__ __launch_bounds__(64) void k_withdraw_close(WdCloseArgs<P> a) {
    const uint32_t j = threadIdx.x, b = blockIdx.y, I = a.s.inputs;
    if (j > a.s.n_pi) return;
    const Fe<P>* v = a.vars + (size_t)b * a.stride;
    if (j == a.s.n_pi) {
        const Fe<P> root = fe_load<P>(v + 2 * I);
        uint32_t bad = 0;
        for (uint32_t k = 0; k < I; ++k) {
            const uint32_t pb = a.s.note0 + k * a.s.note_vars + 2 + 3 * a.s.P + 2 * a.s.height;
            const uint32_t rv = pb + (a.s.height - 1) * a.s.per_level + 6 + a.s.hash_off;
            if (!fe_eq<P>(fe_load<P>(v + rv), root)) bad |= 1u << k;
        }
        a.status[b] = bad;
        return;
    }
    Fe<P> x;
    if (j == 0) x = fe_load<P>(v + 2 * I);
    else if (j <= I) x = fe_load<P>(v + a.s.note0 + (j - 1) * a.s.note_vars + 2 + a.s.P + a.s.hash_off);
    else if (j == I + 1) x = fe_from_u64<P>(a.u[(size_t)b * (2 * I + 4) + 2 * I + 1]);
    else if (j == I + 2) x = fe_load<P>(v + a.s.glob0 + 127 + I);
    else x = fe_load<P>(v + a.s.glob0 + 128 + I + a.s.P + a.s.hash_off);
    fe_store<P>(a.pi + (size_t)b * a.s.n_pi + j, x);
}

// identifier, amount (a word), commitment -> the three inputs of the leaf hash, one thread per deposit
template <class P>
__global__ __launch_bounds__(256) void k_note_leaf_inputs(const Fe<P>* ident, const uint64_t* amount, const Fe<P>* commitment, Fe<P>* out,
                                                           uint64_t m) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= m) return;
    fe_store<P>(out + 3 * t, fe_load<P>(ident + t));
    fe_store<P>(out + 3 * t + 1, fe_from_u64<P>(amount[t]));
    fe_store<P>(out + 3 * t + 2, fe_load<P>(commitment + t));
}

// The new leaves of the requests a chunk of zkt_withdraw_prove takes into the tree: slot b of the chunk's maps is taken when
// bit b of `mask` is set (256 slots: ZKT_WITNESS_BATCH_MAX), and lands behind the taken slots below it.
struct WdSlotMask {
    uint64_t w[4];
};
template <class P>
__global__ __launch_bounds__(256) void k_withdraw_new_leaves(const Fe<P>* vars, uint64_t stride, uint32_t leaf_var, WdSlotMask mask, uint32_t slots,
                                                              Fe<P>* out) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= slots || !((mask.w[b >> 6] >> (b & 63)) & 1)) return;
    uint32_t at = 0;
    for (uint32_t k = 0; k < (b >> 6); ++k) at += __popcll(mask.w[k]);
    at += __popcll(mask.w[b >> 6] & (((uint64_t)1 << (b & 63)) - 1));
    fe_store<P>(out + at, fe_load<P>(vars + (size_t)b * stride + leaf_var));
}

}  // namespace zkt

// the opaque handle of include/zkt_plonk.h
struct zkt_withdraw {
    explicit zkt_withdraw(int dev) : set(dev) {}
    int curve = 0;
    zkt::withdraw::Plan plan;
    zkt_poseidon* pos = nullptr;         // owned
    zkt::DevSet set;                     // everything below
    size_t device_bytes = 0;
    uint32_t* d_w[3] = {};               // the wiring, n_gates each
    void* d_tsel[4] = {};                // templates by arity
    uint32_t* d_tw[4] = {};
    zkt::withdraw::HashCall* d_calls = nullptr;
    zkt::withdraw::GlueRow* d_glue = nullptr;
    // the index vectors of one request: arity-1 trace bases and inputs, arity-3 trace bases and inputs, path leaves, bases,
    // bits, siblings -- and their expansion to the batch slots of the last call's (stride, batch)
    uint32_t rel_off[9] = {};
    uint32_t* d_rel = nullptr;
    uint32_t* d_exp = nullptr;
    uint64_t exp_stride = 0;
    size_t exp_batch = 0;
    // staging of the requests: pinned, and its device copy
    char* h_stage = nullptr;
    char* d_stage = nullptr;
    hipEvent_t staged = nullptr;         // the last upload out of h_stage
    bool stage_busy = false;
    void* d_pi = nullptr;                // batch x n_pi
    uint32_t* d_status = nullptr;        // batch
    void* d_new_leaves = nullptr;        // zkt_withdraw_prove: the leaves of one call's append, ZKT_WITHDRAW_PROVE_MAX scalars
};

namespace zkt {

static size_t wd_stage_fe(const wd::Shape& s) { return 2 * (size_t)s.inputs + 3; }
static size_t wd_stage_u(const wd::Shape& s) { return 2 * (size_t)s.inputs + 4; }
static size_t wd_stage_sib(const wd::Shape& s) { return (size_t)s.inputs * (size_t)s.height; }

static WdShapeDev wd_shape_dev(const wd::Shape& s) {
    WdShapeDev d;
    d.inputs = (uint32_t)s.inputs; d.height = (uint32_t)s.height; d.P = s.P; d.hash_off = s.hash_off; d.per_level = s.per_level;
    d.note_vars = s.note_vars; d.note0 = s.note0; d.glob0 = s.glob0; d.n_pi = s.n_pi;
    return d;
}

static int wd_log_n_min(const wd::Shape& s) {
    int l = 0;
    while (((uint64_t)1 << l) < s.n_gates) ++l;
    return l;
}

static void wd_info(const wd::Shape& s, size_t device_bytes, zkt_withdraw_info* o) {
    o->inputs = s.inputs; o->height = s.height; o->width = s.width; o->log_n_min = wd_log_n_min(s);
    o->n_gates = (size_t)s.n_gates; o->n_vars = (size_t)s.n_vars; o->n_hashes = s.n_hashes; o->vars_per_hash = s.P; o->n_pi = s.n_pi;
    o->device_bytes = device_bytes;
}

static int wd_check_params(zkt_ctx* c, const zkt_poseidon_params* p, int inputs, int height, wd::Shape& s) {
    if (!p || !p->round_constants || !p->mds || !p->domain_tag) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (!wd::shape_make(p->width, p->half_full_rounds, p->partial_rounds, inputs, height, s))
        return set_err(c, ZKT_ERR_INVALID_ARGUMENT,
                       "withdraw: 4 <= width <= 8 (width 3 cannot hash a leaf), 1 <= inputs <= 32, 1 <= height <= 64, rounds >= 1");
    return ZKT_OK;
}

template <class P>
static void wd_templates(const wd::Shape& s, const zkt_poseidon_params* p, wd::Template<P>* t /* [4] */) {
    const size_t n_rc = (size_t)(2 * s.half_full + s.partial) * s.width, n_mds = (size_t)s.width * s.width;
    std::vector<Fe<P>> rc(n_rc), mds(n_mds);
    Fe<P> tag;
    memcpy((void*)rc.data(), p->round_constants, n_rc * 32);
    memcpy((void*)mds.data(), p->mds, n_mds * 32);
    memcpy((void*)&tag, p->domain_tag, 32);
    for (int a = 1; a <= 3; ++a) wd::template_make<P>(s, rc.data(), mds.data(), tag, a, t[a]);
}

template <class P>
static int wd_layout_host_t(const wd::Shape& s, const zkt_poseidon_params* p, const wd::Plan& pl, uint64_t* const* sel6, uint32_t* const* w3) {
    wd::Template<P> t[4];
    wd_templates<P>(s, p, t);
    Fe<P>* sel[6] = {};
    uint32_t* w[3] = {};
    for (int q = 0; q < 6; ++q) sel[q] = sel6 ? (Fe<P>*)sel6[q] : nullptr;
    for (int x = 0; x < 3; ++x) w[x] = w3 ? w3[x] : nullptr;
    wd::expand_host<P>(pl, t, sel, w);
    return ZKT_OK;
}

// the two layout launches: selectors (six device vectors, or null) and wires (three, or null)
template <class P>
static int wd_rows_enqueue_t(zkt_ctx* c, const zkt_withdraw* w, void* const* d_sel, uint32_t* const* d_wires) {
    const wd::Shape& s = w->plan.s;
    WdHashRowsArgs<P> h{};
    h.calls = w->d_calls;
    for (int a = 1; a <= 3; ++a) {
        h.tsel[a] = (const Fe<P>*)w->d_tsel[a];
        h.tw[a] = w->d_tw[a];
    }
    h.tsel[0] = h.tsel[1];
    h.tw[0] = h.tw[1];
    WdGlueRowsArgs<P> g{};
    g.glue = w->d_glue;
    wd::glue_consts<P>(g.consts);
    for (int q = 0; q < 6; ++q) h.sel[q] = g.sel[q] = d_sel ? (Fe<P>*)d_sel[q] : nullptr;
    for (int x = 0; x < 3; ++x) h.w[x] = g.w[x] = d_wires ? d_wires[x] : nullptr;
    h.per_hash = s.P;
    h.total = (uint64_t)s.n_hashes * s.P;
    g.total = (uint32_t)w->plan.glue.size();
    hipLaunchKernelGGL((k_withdraw_hash_rows<P>), dim3((unsigned)((h.total + 255) / 256)), dim3(256), 0, c->stream, h);
    ZKT_HIP(c, hipGetLastError());
    hipLaunchKernelGGL((k_withdraw_glue_rows<P>), dim3((g.total + 255) / 256), dim3(256), 0, c->stream, g);
    ZKT_HIP(c, hipGetLastError());
    return ZKT_OK;
}

static int wd_rows_enqueue(zkt_ctx* c, const zkt_withdraw* w, void* const* d_sel, uint32_t* const* d_wires) {
    ProfScope ps(c, "withdraw_layout");
    return c->curve == ZKT_CURVE_BN254 ? wd_rows_enqueue_t<Bn254Fr>(c, w, d_sel, d_wires) : wd_rows_enqueue_t<Bls381Fr>(c, w, d_sel, d_wires);
}

template <class P>
static int wd_create_t(zkt_ctx* c, const zkt_poseidon_params* p, zkt_withdraw* w) {
    const wd::Shape& s = w->plan.s;
    wd::Template<P> t[4];
    wd_templates<P>(s, p, t);
    int rc;
    auto alloc = [&](void** d, size_t bytes) -> int {
        w->device_bytes += bytes;
        return w->set.alloc(c, d, bytes);
    };
    auto up = [&](void* d, const void* h, size_t bytes) -> int {
        ZKT_HIP(c, hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, c->stream));
        return ZKT_OK;
    };
    std::vector<Fe<P>> tsel[4];
    std::vector<uint32_t> tw[4];
    for (int a = 1; a <= 3; ++a) {
        for (int q = 0; q < 5; ++q) tsel[a].insert(tsel[a].end(), t[a].sel[q].begin(), t[a].sel[q].end());
        for (int x = 0; x < 3; ++x) tw[a].insert(tw[a].end(), t[a].w[x].begin(), t[a].w[x].end());
        if (tsel[a].size() != 5 * (size_t)s.P || tw[a].size() != 3 * (size_t)s.P) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "withdraw: template size");
        if ((rc = alloc(&w->d_tsel[a], tsel[a].size() * 32))) return rc;
        if ((rc = alloc((void**)&w->d_tw[a], tw[a].size() * 4))) return rc;
        if ((rc = up(w->d_tsel[a], tsel[a].data(), tsel[a].size() * 32))) return rc;
        if ((rc = up(w->d_tw[a], tw[a].data(), tw[a].size() * 4))) return rc;
    }
    if ((rc = alloc((void**)&w->d_calls, w->plan.calls.size() * sizeof(wd::HashCall)))) return rc;
    if ((rc = alloc((void**)&w->d_glue, w->plan.glue.size() * sizeof(wd::GlueRow)))) return rc;
    if ((rc = up(w->d_calls, w->plan.calls.data(), w->plan.calls.size() * sizeof(wd::HashCall)))) return rc;
    if ((rc = up(w->d_glue, w->plan.glue.data(), w->plan.glue.size() * sizeof(wd::GlueRow)))) return rc;
    for (int x = 0; x < 3; ++x)
        if ((rc = alloc((void**)&w->d_w[x], (size_t)s.n_gates * 4))) return rc;

    // one request's index vectors, in the order the launches of zkt_withdraw_witness take them
    const int I = s.inputs, H = s.height;
    std::vector<uint32_t> rel, v[8];
    for (int k = 0; k < I; ++k) {
        v[0].push_back(s.commit_base(k)); v[1].push_back(s.secret_var(k));
        v[0].push_back(s.null_base(k));   v[1].push_back(s.inv_var(k));
        v[2].push_back(s.leaf_base(k));
        v[3].push_back(s.ident_var(k)); v[3].push_back(s.amount_var(k)); v[3].push_back(s.commit_base(k) + s.hash_off);
        v[4].push_back(s.leaf_base(k) + s.hash_off);
        v[5].push_back(s.path_base(k));
        for (int l = 0; l < H; ++l) {
            v[6].push_back(s.bit0(k) + (uint32_t)l);
            v[7].push_back(s.sib0(k) + (uint32_t)l);
        }
    }
    v[0].push_back(s.new_commit_base()); v[1].push_back(s.new_secret_var());
    v[2].push_back(s.new_leaf_base());
    v[3].push_back(s.new_ident_var()); v[3].push_back(s.out_var()); v[3].push_back(s.new_commit_base() + s.hash_off);
    for (int k = 0; k < 8; ++k) {
        w->rel_off[k] = (uint32_t)rel.size();
        rel.insert(rel.end(), v[k].begin(), v[k].end());
    }
    w->rel_off[8] = (uint32_t)rel.size();
    const size_t B = ZKT_WITNESS_BATCH_MAX;
    if ((rc = alloc((void**)&w->d_rel, rel.size() * 4))) return rc;
    if ((rc = alloc((void**)&w->d_exp, rel.size() * 4 * B))) return rc;
    if ((rc = up(w->d_rel, rel.data(), rel.size() * 4))) return rc;
    const size_t stage = B * (wd_stage_fe(s) * 32 + wd_stage_u(s) * 8 + wd_stage_sib(s) * 32);
    if ((rc = alloc((void**)&w->d_stage, stage))) return rc;
    if ((rc = w->set.pinned(c, (void**)&w->h_stage, stage))) return rc;
    if ((rc = w->set.event(c, &w->staged))) return rc;
    if ((rc = alloc(&w->d_pi, B * s.n_pi * 32))) return rc;
    if ((rc = alloc((void**)&w->d_status, B * 4))) return rc;
    if ((rc = alloc(&w->d_new_leaves, (size_t)ZKT_WITHDRAW_PROVE_MAX * 32))) return rc;
    {
        ProfScope ps(c, "withdraw_layout");
        if ((rc = wd_rows_enqueue_t<P>(c, w, nullptr, w->d_w))) return rc;
    }
    ZKT_HIP(c, hipStreamSynchronize(c->stream));   // the staging vectors die with this call
    return ZKT_OK;
}

static int wd_check(zkt_ctx* c, const zkt_withdraw* w) {
    if (!c || !w) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (w->curve != c->curve) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "withdraw: the handle belongs to another curve");
    if (w->set.device != c->device) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "withdraw: the handle lives on another device");
    return ZKT_OK;
}

// Everything zkt_withdraw_witness can refuse on the host, for `batch` requests, before anything is enqueued.  amount_out:
// batch words, the sums less the withdrawn amounts (may be null).
template <class P>
static int wd_validate_t(zkt_ctx* c, const zkt_withdraw* w, const zkt_withdraw_request* reqs, size_t batch, zkt_merkle_tree* tree,
                         uint64_t* amount_out, bool& any_sib, bool& any_tree, bool& tree_root) {
    const wd::Shape& s = w->plan.s;
    const size_t I = (size_t)s.inputs, H = (size_t)s.height;
    any_sib = any_tree = tree_root = false;
    for (size_t b = 0; b < batch; ++b) {
        const zkt_withdraw_request& r = reqs[b];
        if (!r.secrets || !r.identifiers || !r.amounts || !r.leaf_indices || !r.new_secret || !r.new_identifier)
            return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "withdraw: a request holds a null pointer");
        uint64_t sum = 0;
        for (size_t k = 0; k < I; ++k) {
            if (__builtin_add_overflow(sum, r.amounts[k], &sum))
                return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "withdraw: the sum of the amounts overflows u64");
            if (H < 64 && (r.leaf_indices[k] >> H)) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "withdraw: a leaf index is not below 2^height");
        }
        if (r.withdraw_amount > sum) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "withdraw: invalid withdraw amount (withdraw.rs:59)");
        if (amount_out) amount_out[b] = sum - r.withdraw_amount;
        for (size_t k = 0; k < I; ++k) {
            Fe<P> x;
            memcpy((void*)&x, r.secrets + 4 * k, 32);
            if (fe_is_zero<P>(x)) return set_err(c, ZKT_ERR_ZERO_DENOMINATOR, "withdraw: a secret is 0 (1 / secret, main.rs:257)");
        }
        (r.siblings ? any_sib : any_tree) = true;
        if (!r.root) tree_root = true;
    }
    if (any_tree || tree_root) {
        int th = 0;
        if (!tree) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "withdraw: siblings or root left to a tree, and no tree given");
        if (zkt_merkle_tree_info(tree, &th, nullptr, nullptr) || th != s.height)
            return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "withdraw: the tree has another height");
    }
    return ZKT_OK;
}

template <class P>
static int wd_witness_t(zkt_ctx* c, zkt_withdraw* w, const zkt_withdraw_request* reqs, size_t batch, zkt_merkle_tree* tree, void* d_variables,
                        size_t stride, uint64_t* out_pi, zkt_withdraw_status* out_status) {
    const wd::Shape& s = w->plan.s;
    const size_t I = (size_t)s.inputs, H = (size_t)s.height;
    const size_t FA = wd_stage_fe(s), UA = wd_stage_u(s), SA = wd_stage_sib(s);
    // ---- everything that can be refused, before anything is enqueued ----
    bool any_sib = false, any_tree = false, tree_root = false;
    std::vector<uint64_t> amount_out(batch);
    if (int rc = wd_validate_t<P>(c, w, reqs, batch, tree, amount_out.data(), any_sib, any_tree, tree_root)) return rc;
    Fe<P> troot = fe_zero<P>();
    if (tree_root)
        if (int rc = zkt_merkle_tree_root(c, tree, (uint64_t*)&troot)) return rc;

    // ---- staging: the previous call's upload must have left the pinned buffer ----
    if (w->stage_busy) {
        ZKT_HIP(c, hipEventSynchronize(w->staged));
        w->stage_busy = false;
    }
    char* hs = w->h_stage;
    const size_t off_u = batch * FA * 32, off_s = off_u + batch * UA * 8;
    for (size_t b = 0; b < batch; ++b) {
        const zkt_withdraw_request& r = reqs[b];
        char* fe = hs + b * FA * 32;
        memcpy(fe, r.secrets, I * 32);
        memcpy(fe + I * 32, r.identifiers, I * 32);
        memcpy(fe + 2 * I * 32, r.root ? (const void*)r.root : (const void*)&troot, 32);
        memcpy(fe + (2 * I + 1) * 32, r.new_secret, 32);
        memcpy(fe + (2 * I + 2) * 32, r.new_identifier, 32);
        uint64_t* u = (uint64_t*)(hs + off_u) + b * UA;
        memcpy(u, r.amounts, I * 8);
        memcpy(u + I, r.leaf_indices, I * 8);
        u[2 * I] = amount_out[b];
        u[2 * I + 1] = r.withdraw_amount;
        u[2 * I + 2] = r.siblings ? 1 : 0;
        u[2 * I + 3] = 0;
        if (r.siblings) memcpy(hs + off_s + b * SA * 32, r.siblings, SA * 32);
    }
    const size_t up_bytes = any_sib ? off_s + batch * SA * 32 : off_s;
    ProfScope ps(c, "withdraw_witness");
    ZKT_HIP(c, hipMemcpyAsync(w->d_stage, hs, up_bytes, hipMemcpyHostToDevice, c->stream));
    ZKT_HIP(c, hipEventRecord(w->staged, c->stream));
    w->stage_busy = true;

    const WdShapeDev sd = wd_shape_dev(s);
    WdStage<P> st{(const Fe<P>*)w->d_stage, (const uint64_t*)(w->d_stage + off_u), (const Fe<P>*)(w->d_stage + off_s)};
    // the index vectors of every slot, unless the last call left them for this (stride, batch)
    if (w->exp_stride != stride || w->exp_batch != batch) {
        WdExpandArgs e{};
        e.rel = w->d_rel;
        e.out = w->d_exp;
        for (int k = 0; k < 9; ++k) e.off[k] = w->rel_off[k];
        e.stride = stride;
        e.batch = (uint32_t)batch;
        hipLaunchKernelGGL(k_withdraw_expand, dim3((e.off[8] + 255) / 256, (unsigned)batch), dim3(256), 0, c->stream, e);
        ZKT_HIP(c, hipGetLastError());
        w->exp_stride = stride;
        w->exp_batch = batch;
    }
    // 1. the variables that are neither hash traces nor selects
    {
        WdBaseArgs<P> a{};
        a.s = sd;
        a.st = st;
        a.vars = (Fe<P>*)d_variables;
        a.stride = stride;
        a.per_request = (uint32_t)(I + 1 + 127 + (I - 1) + I * H);
        hipLaunchKernelGGL((k_withdraw_base<P>), dim3((a.per_request + 127) / 128, (unsigned)batch), dim3(128), 0, c->stream, a);
        ZKT_HIP(c, hipGetLastError());
    }
    const size_t map_vars = (batch - 1) * stride + (size_t)s.n_vars;
    if (any_tree) {
        std::vector<uint64_t> idx;
        std::vector<uint32_t> sib0;
        for (size_t b = 0; b < batch; ++b)
            if (!reqs[b].siblings)
                for (size_t k = 0; k < I; ++k) {
                    idx.push_back(reqs[b].leaf_indices[k]);
                    sib0.push_back((uint32_t)(b * stride) + s.sib0((int)k));
                }
        for (size_t at = 0; at < idx.size(); at += ZKT_MERKLE_TREE_PATHS_MAX) {
            const size_t k = std::min<size_t>(ZKT_MERKLE_TREE_PATHS_MAX, idx.size() - at);
            if (int rc = zkt_merkle_tree_paths_to_variables_dev(c, tree, idx.data() + at, k, d_variables, map_vars, nullptr, sib0.data() + at))
                return rc;
        }
    }
    const uint32_t* ex = w->d_exp;
    auto vec = [&](int k) { return ex + (size_t)w->rel_off[k] * batch; };
    // 2. arity 1: commitments, nullifiers, the new commitment;  3. arity 3: the leaves and the new leaf
    for (int pass = 0; pass < 2; ++pass) {
        zkt_poseidon_gadget_args g{};
        g.batch = batch * (pass == 0 ? 2 * I + 1 : I + 1);
        g.arity = pass == 0 ? 1 : 3;
        g.d_input_vars = vec(pass == 0 ? 1 : 3);
        g.d_variables = d_variables;
        g.n_vars = map_vars;
        g.d_trace_base = vec(pass == 0 ? 0 : 2);
        if (int rc = zkt_poseidon_gadget_witness_dev(c, w->pos, &g)) return rc;
    }
    // 4. the paths: the selects and the hash trace of every level
    {
        zkt_merkle_path_args m{};
        m.batch = batch * I;
        m.height = s.height;
        m.d_variables = d_variables;
        m.n_vars = map_vars;
        m.d_leaf_var = vec(4);
        m.d_path_base = vec(5);
        m.d_bit_vars = vec(6);
        m.d_sibling_vars = vec(7);
        if (int rc = zkt_poseidon_merkle_path_witness_dev(c, w->pos, &m)) return rc;
    }
    // 5. the public inputs and the paths that miss the root
    {
        WdCloseArgs<P> a{};
        a.s = sd;
        a.u = st.u;
        a.vars = (const Fe<P>*)d_variables;
        a.stride = stride;
        a.pi = (Fe<P>*)w->d_pi;
        a.status = w->d_status;
        hipLaunchKernelGGL((k_withdraw_close<P>), dim3(1, (unsigned)batch), dim3(64), 0, c->stream, a);
        ZKT_HIP(c, hipGetLastError());
    }
    if (out_pi || out_status) {
        static_assert(sizeof(zkt_withdraw_status) == 4, "one word per request");
        if (out_pi) ZKT_HIP(c, hipMemcpyAsync(out_pi, w->d_pi, batch * s.n_pi * 32, hipMemcpyDeviceToHost, c->stream));
        if (out_status) ZKT_HIP(c, hipMemcpyAsync(out_status, w->d_status, batch * 4, hipMemcpyDeviceToHost, c->stream));
        ZKT_HIP(c, hipStreamSynchronize(c->stream));
    }
    return ZKT_OK;
}

template <class P>
static int note_leaves_t(zkt_ctx* c, const zkt_poseidon* pos, const void* d_secrets, const void* d_identifiers, const void* d_amounts, size_t m,
                         void* d_out, void* d_tmp) {
    // H(secret) into the output, the three inputs beside it, H(identifier, amount, commitment) over the output
    if (int rc = zkt_poseidon_hash_batch_dev(c, pos, d_secrets, m, 1, d_out, nullptr)) return rc;
    hipLaunchKernelGGL((k_note_leaf_inputs<P>), dim3((unsigned)((m + 255) / 256)), dim3(256), 0, c->stream, (const Fe<P>*)d_identifiers,
                       (const uint64_t*)d_amounts, (const Fe<P>*)d_out, (Fe<P>*)d_tmp, (uint64_t)m);
    ZKT_HIP(c, hipGetLastError());
    return zkt_poseidon_hash_batch_dev(c, pos, d_tmp, m, 3, d_out, nullptr);
}

// ---- ProveWithdraw in one call ---------------------------------------------------------------------------------------------
// the codes with which zkt_prove refuses ONE proof (its witness or its challenges), as opposed to a failure of the call
static bool wd_is_proof_refusal(int rc) {
    return rc == ZKT_ERR_NOT_IN_TABLE || rc == ZKT_ERR_EQUAL_CHALLENGES || rc == ZKT_ERR_ZERO_DENOMINATOR || rc == ZKT_ERR_QUOTIENT_TOO_SHORT;
}

// the loaded circuit's commitments as the transcripts are seeded from them: canonical little-endian bytes and flags
template <class C>
static void wd_seed_bytes(const CircuitState* S, uint8_t* xy_le, uint8_t* inf) {
    using Q = typename C::Fq;
    for (int k = 0; k < 10; ++k) {
        Fe<Q> x, y;
        memcpy(x.v, S->vk_commits + (size_t)k * Q::N, Q::N * 4);
        memcpy(y.v, S->vk_commits + (size_t)k * Q::N + Q::N / 2, Q::N * 4);
        fq_to_le<Q>(x, xy_le + (size_t)k * 2 * Q::N * 4);
        fq_to_le<Q>(y, xy_le + ((size_t)k * 2 + 1) * Q::N * 4);
        inf[k] = S->vk_inf[k] ? 1 : 0;
    }
}

// VerifierKey::pi_roots: w^pos for the circuit's public-input rows
template <class R>
static void wd_pi_roots(int log_n, const std::vector<size_t>& pi_pos, uint64_t* out) {
    const Fe<R> w = root_of_unity<R>(log_n);
    for (size_t i = 0; i < pi_pos.size(); ++i) {
        const Fe<R> r = fe_pow_u64<R>(w, (uint64_t)pi_pos[i]);
        memcpy(out + 4 * i, r.v, 32);
    }
}

}  // namespace zkt

using namespace zkt;

extern "C" {

int zkt_debug_withdraw_layout_host(int curve_id, const zkt_poseidon_params* params, int inputs, int height, zkt_withdraw_info* info,
                                   uint64_t* const* out_selectors6, uint32_t* const* out_wires3, size_t* out_pi_pos,
                                   uint32_t* out_hash_calls) {
    if (curve_id != ZKT_CURVE_BN254 && curve_id != ZKT_CURVE_BLS12_381) return ZKT_ERR_INVALID_ARGUMENT;
    wd::Shape s;
    if (int rc = wd_check_params(nullptr, params, inputs, height, s)) return rc;
    wd::Plan pl;
    if (!wd::plan_make(s, pl)) return ZKT_ERR_INVALID_ARGUMENT;
    if (info) wd_info(s, 0, info);
    if (out_pi_pos)
        for (size_t k = 0; k < pl.pi_pos.size(); ++k) out_pi_pos[k] = pl.pi_pos[k];
    if (out_hash_calls)
        for (size_t k = 0; k < pl.calls.size(); ++k) {
            const wd::HashCall& h = pl.calls[k];
            uint32_t* o = out_hash_calls + 5 * k;
            o[0] = h.base; o[1] = h.arity; o[2] = h.in[0]; o[3] = h.in[1]; o[4] = h.in[2];
        }
    if (!out_selectors6 && !out_wires3) return ZKT_OK;
    return curve_id == ZKT_CURVE_BN254 ? wd_layout_host_t<Bn254Fr>(s, params, pl, out_selectors6, out_wires3)
                                       : wd_layout_host_t<Bls381Fr>(s, params, pl, out_selectors6, out_wires3);
}

int zkt_withdraw_create(zkt_ctx* c, const zkt_poseidon_params* params, int inputs, int height, zkt_withdraw** out) {
    if (!c || !out) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    wd::Shape s;
    if (int rc = wd_check_params(c, params, inputs, height, s)) return rc;
    (void)hipSetDevice(c->device);
    zkt_withdraw* w = new zkt_withdraw(c->device);
    w->curve = c->curve;
    int rc = ZKT_OK;
    if (!wd::plan_make(s, w->plan)) rc = set_err(c, ZKT_ERR_INVALID_ARGUMENT, "withdraw: the planner's closed form disagrees with its walk");
    if (!rc) rc = zkt_poseidon_load(c, params, &w->pos);
    if (!rc) rc = c->curve == ZKT_CURVE_BN254 ? wd_create_t<Bn254Fr>(c, params, w) : wd_create_t<Bls381Fr>(c, params, w);
    if (rc) {
        zkt_withdraw_free(c, w);
        return rc;
    }
    *out = w;
    return ZKT_OK;
}

void zkt_withdraw_free(zkt_ctx* c, zkt_withdraw* w) {
    if (!w) return;
    if (c) {
        (void)hipSetDevice(c->device);
        (void)hipStreamSynchronize(c->stream);
    }
    if (w->pos) zkt_poseidon_free(c, w->pos);
    delete w;
}

const zkt_poseidon* zkt_withdraw_poseidon(const zkt_withdraw* w) { return w ? w->pos : nullptr; }

int zkt_withdraw_get_info(const zkt_withdraw* w, zkt_withdraw_info* out) {
    if (!w || !out) return ZKT_ERR_INVALID_ARGUMENT;
    wd_info(w->plan.s, w->device_bytes, out);
    return ZKT_OK;
}

int zkt_withdraw_pi_pos(const zkt_withdraw* w, size_t* out) {
    if (!w || !out) return ZKT_ERR_INVALID_ARGUMENT;
    for (size_t k = 0; k < w->plan.pi_pos.size(); ++k) out[k] = w->plan.pi_pos[k];
    return ZKT_OK;
}

int zkt_withdraw_rows(zkt_ctx* c, const zkt_withdraw* w, uint64_t* const* out_selectors6, uint32_t* const* out_wires3) {
    if (int rc = wd_check(c, w)) return rc;
    if (!out_selectors6 && !out_wires3) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    for (int q = 0; q < 6; ++q)
        if (out_selectors6 && !out_selectors6[q]) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    for (int x = 0; x < 3; ++x)
        if (out_wires3 && !out_wires3[x]) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    (void)hipSetDevice(c->device);
    const size_t g = (size_t)w->plan.s.n_gates;
    DevSet tmp(c->device);
    void* d_sel[6] = {};
    uint32_t* d_wr[3] = {};
    auto run = [&]() -> int {
        int rc;
        for (int q = 0; q < 6 && out_selectors6; ++q)
            if ((rc = tmp.alloc(c, &d_sel[q], g * 32))) return rc;
        for (int x = 0; x < 3 && out_wires3; ++x)
            if ((rc = tmp.alloc(c, (void**)&d_wr[x], g * 4))) return rc;
        if ((rc = wd_rows_enqueue(c, w, out_selectors6 ? d_sel : nullptr, out_wires3 ? d_wr : nullptr))) return rc;
        for (int q = 0; q < 6 && out_selectors6; ++q)
            ZKT_HIP(c, hipMemcpyAsync(out_selectors6[q], d_sel[q], g * 32, hipMemcpyDeviceToHost, c->stream));
        for (int x = 0; x < 3 && out_wires3; ++x) ZKT_HIP(c, hipMemcpyAsync(out_wires3[x], d_wr[x], g * 4, hipMemcpyDeviceToHost, c->stream));
        return ZKT_OK;
    };
    const int rc = run();
    const hipError_t e = hipStreamSynchronize(c->stream);   // before `tmp` goes, whatever happened
    if (rc) return rc;
    ZKT_HIP(c, e);
    return ZKT_OK;
}

int zkt_withdraw_setup(zkt_ctx* c, const zkt_withdraw* w, int log_n, size_t table_size, uint64_t* out_commitments, int* out_is_infinity) {
    if (int rc = wd_check(c, w)) return rc;
    if (!out_commitments) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (log_n < wd_log_n_min(w->plan.s) || log_n > 25) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "withdraw: log_n below log_n_min (or above 25)");
    const size_t n = (size_t)1 << log_n, g = (size_t)w->plan.s.n_gates;
    if (table_size >= n) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "withdraw: table_size must be below n");
    (void)hipSetDevice(c->device);
    DevSet tmp(c->device);
    void* d_sel[6] = {};
    void* d_table = nullptr;
    auto run = [&]() -> int {
        int rc;
        // the selectors end at n_gates: setup pads every vector with zeros to n (setup.rs:28-35 pad_to)
        for (int q = 0; q < 6; ++q)
            if ((rc = tmp.alloc(c, &d_sel[q], g * 32))) return rc;
        if ((rc = tmp.alloc(c, &d_table, n * 32))) return rc;
        if ((rc = wd_rows_enqueue(c, w, d_sel, nullptr))) return rc;
        if (c->curve == ZKT_CURVE_BN254)
            hipLaunchKernelGGL((k_withdraw_table_mask<Bn254Fr>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, (Fe<Bn254Fr>*)d_table,
                               (uint64_t)table_size, (uint64_t)n);
        else
            hipLaunchKernelGGL((k_withdraw_table_mask<Bls381Fr>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, (Fe<Bls381Fr>*)d_table,
                               (uint64_t)table_size, (uint64_t)n);
        ZKT_HIP(c, hipGetLastError());
        const uint64_t* ev[10] = {(const uint64_t*)d_sel[0], (const uint64_t*)d_sel[1], (const uint64_t*)d_sel[2], (const uint64_t*)d_sel[3],
                                  (const uint64_t*)d_sel[4], nullptr, nullptr, nullptr, (const uint64_t*)d_sel[5], (const uint64_t*)d_table};
        const size_t lens[10] = {g, g, g, g, g, 0, 0, 0, g, n};
        return zkt_circuit_setup_wiring(c, log_n, ev, lens, 1, w->d_w[0], w->d_w[1], w->d_w[2], g, (size_t)w->plan.s.n_vars, 1, out_commitments,
                                        out_is_infinity);
    };
    const int rc = run();
    (void)hipStreamSynchronize(c->stream);   // before `tmp` goes
    if (!rc) {   // what zkt_withdraw_prove seeds its transcripts from, and the table size q_table was masked for: kept with the circuit
        CircuitState* S = c->circuit.get();
        const size_t words = c->curve == ZKT_CURVE_BN254 ? 8 : 12;
        memcpy(S->vk_commits, out_commitments, 10 * words * 8);
        for (int k = 0; k < 10; ++k)   // the identity comes back as (0, 0) with its flag; the flags are optional for the caller
            S->vk_inf[k] = out_is_infinity ? out_is_infinity[k]
                                           : std::all_of(out_commitments + k * words, out_commitments + (k + 1) * words, [](uint64_t x) { return x == 0; });
        S->vk_srs_generation = c->srs_generation;
        S->vk_table_size = table_size;
        S->vk_cached = true;
    }
    return rc;
}

int zkt_withdraw_witness(zkt_ctx* c, zkt_withdraw* w, const zkt_withdraw_request* reqs, size_t batch, zkt_merkle_tree* tree, void* d_variables,
                         size_t stride, uint64_t* out_pi, zkt_withdraw_status* out_status) {
    if (int rc = wd_check(c, w)) return rc;
    if (!reqs || !d_variables) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (batch < 1 || batch > ZKT_WITNESS_BATCH_MAX) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "withdraw: 1 <= batch <= ZKT_WITNESS_BATCH_MAX");
    if (stride < w->plan.s.n_vars) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "withdraw: stride below n_vars");
    if (stride > 0xFFFFFFFEull / batch) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "withdraw: batch x stride must fit 32-bit variable indices");
    (void)hipSetDevice(c->device);
    return c->curve == ZKT_CURVE_BN254 ? wd_witness_t<Bn254Fr>(c, w, reqs, batch, tree, d_variables, stride, out_pi, out_status)
                                       : wd_witness_t<Bls381Fr>(c, w, reqs, batch, tree, d_variables, stride, out_pi, out_status);
}

int zkt_withdraw_prove_inputs(const zkt_withdraw* w, const void* d_variables, size_t stride, size_t b, const size_t* pi_pos,
                              const uint64_t* pi_vals, zkt_prove_inputs* out) {
    if (!w || !d_variables || !out || stride < w->plan.s.n_vars) return ZKT_ERR_INVALID_ARGUMENT;
    out->a_evals = out->b_evals = out->c_evals = nullptr;
    out->n_rows = (size_t)w->plan.s.n_gates;
    out->pi_pos = pi_pos;
    out->pi_vals = pi_vals;
    out->n_pi = w->plan.s.n_pi;
    out->wires_on_device = 1;
    out->variables = (const uint64_t*)d_variables + 4 * b * stride;
    out->n_vars = (size_t)w->plan.s.n_vars;
    out->w_l = w->d_w[0];
    out->w_r = w->d_w[1];
    out->w_o = w->d_w[2];
    return ZKT_OK;
}

int zkt_withdraw_prove(zkt_ctx* c, zkt_withdraw* w, const zkt_withdraw_request* reqs, size_t batch, zkt_merkle_tree* tree,
                       const zkt_withdraw_prove_args* a, uint8_t* proofs, size_t proof_stride, uint64_t* out_pi, zkt_withdraw_result* results) {
    if (int rc = wd_check(c, w)) return rc;
    if (!reqs || !a || !proofs || !results || !a->d_variables || !a->blinders || (a->set_len && !a->identifiers_set))
        return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (a->verify && (!a->g_xy_mont || !a->h_g2_mont || !a->beta_h_g2_mont))
        return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "withdraw prove: verify needs g, h and beta h");
    const wd::Shape& s = w->plan.s;
    const size_t n_pi = s.n_pi, proof_len = c->curve == ZKT_CURVE_BN254 ? 802 : 1010;
    if (batch < 1 || batch > ZKT_WITHDRAW_PROVE_MAX) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "withdraw prove: 1 <= batch <= ZKT_WITHDRAW_PROVE_MAX");
    if (a->slots < 1 || a->slots > ZKT_WITNESS_BATCH_MAX) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "withdraw prove: 1 <= slots <= ZKT_WITNESS_BATCH_MAX");
    if (a->stride < s.n_vars) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "withdraw: stride below n_vars");
    if (a->stride > 0xFFFFFFFEull / a->slots) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "withdraw: slots x stride must fit 32-bit variable indices");
    if (proof_stride < proof_len) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "withdraw prove: proof_stride below the proof's length");
    if (a->transcript_kind != ZKT_TRANSCRIPT_MERLIN && a->transcript_kind != ZKT_TRANSCRIPT_ETHEREUM)
        return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "withdraw prove: unknown transcript kind");
    if (tree && tree->curve != c->curve) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "withdraw prove: the tree belongs to another curve");
    if (int rc = circuit_entry(c, ENTRY_SRS | ENTRY_DEVICE)) return rc;
    (void)zkt_prove_set_next(c, nullptr);   // the chain below is the only one
    const std::shared_ptr<CircuitState> circuit = c->circuit;
    const uint64_t n = circuit->n;
    CircuitState* S = circuit.get();

    // the identifiers set as a LookupTable: the first of equal values stays
    std::vector<uint64_t> table;
    {
        std::map<std::array<uint64_t, 4>, bool> seen;
        for (size_t i = 0; i < a->set_len; ++i) {
            std::array<uint64_t, 4> v;
            memcpy(v.data(), a->identifiers_set + 4 * i, 32);
            if (seen.emplace(v, true).second) table.insert(table.end(), v.begin(), v.end());
        }
    }
    const size_t table_len = table.size() / 4, table_max = S->vk_table_size ? S->vk_table_size : (size_t)n - 1;
    if (table_len > table_max) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "withdraw prove: table size exceeds max size (lookup/table.rs:57)");
    {
        bool any_sib, any_tree, tree_root;
        const int rc = c->curve == ZKT_CURVE_BN254 ? wd_validate_t<Bn254Fr>(c, w, reqs, batch, tree, nullptr, any_sib, any_tree, tree_root)
                                                   : wd_validate_t<Bls381Fr>(c, w, reqs, batch, tree, nullptr, any_sib, any_tree, tree_root);
        if (rc) return rc;
    }
    if (a->append) {
        int th = 0;
        uint64_t count = 0, capacity = 0;
        if (!tree || zkt_merkle_tree_info(tree, &th, &count, &capacity) || th != s.height)
            return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "withdraw prove: append needs a tree of the circuit's height");
        if (batch > capacity - count) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "withdraw prove: the tree has no room for `batch` more leaves");
    }
    // the commitments of a circuit that zkt_withdraw_setup did not make, or under another SRS than it had: once
    if (!S->vk_cached || S->vk_srs_generation != c->srs_generation) {
        S->vk_cached = false;
        if (int rc = zkt_circuit_commitments(c, S->vk_commits, S->vk_inf)) return rc;
        S->vk_srs_generation = c->srs_generation;
        S->vk_cached = true;
    }
    const size_t fq_bytes = c->curve == ZKT_CURVE_BN254 ? 32 : 48;
    uint8_t seed_xy[10 * 2 * 48], seed_inf[10];
    if (c->curve == ZKT_CURVE_BN254) wd_seed_bytes<Bn254Curve>(S, seed_xy, seed_inf);
    else wd_seed_bytes<Bls381Curve>(S, seed_xy, seed_inf);
    auto transcript = [&]() {
        zkt_transcript* t = zkt_transcript_new(a->transcript_kind, a->label);
        if (t) zkt_transcript_seed(t, n, seed_xy, seed_inf, fq_bytes);
        return t;
    };
    std::vector<uint64_t> pi_roots(a->verify ? 4 * n_pi : 0), pi_own(out_pi ? 0 : batch * n_pi * 4);
    if (a->verify) {
        if (c->curve == ZKT_CURVE_BN254) wd_pi_roots<Bn254Fr>(circuit->log_n, w->plan.pi_pos, pi_roots.data());
        else wd_pi_roots<Bls381Fr>(circuit->log_n, w->plan.pi_pos, pi_roots.data());
    }
    uint64_t* pi = out_pi ? out_pi : pi_own.data();
    for (size_t b = 0; b < batch; ++b) results[b] = zkt_withdraw_result{ZKT_OK, 0, 0, UINT64_MAX};
    const uint32_t leaf_var = s.new_leaf_base() + s.hash_off;

    std::vector<size_t> taken;   // the requests whose leaves wait in d_new_leaves, in order
    auto run = [&]() -> int {
        std::vector<zkt_prove_inputs> ins(a->slots);
        std::vector<uint32_t> status(a->slots);
        for (size_t base = 0; base < batch; base += a->slots) {
            const size_t cnt = std::min(a->slots, batch - base);
            if (int rc = zkt_withdraw_witness(c, w, reqs + base, cnt, tree, a->d_variables, a->stride, pi + base * n_pi * 4,
                                              (zkt_withdraw_status*)status.data()))
                return rc;
            std::vector<size_t> good;
            for (size_t b = 0; b < cnt; ++b) {
                zkt_withdraw_result& r = results[base + b];
                memset(proofs + (base + b) * proof_stride, 0, proof_len);
                r.bad_paths = status[b];
                if (status[b]) {
                    r.code = ZKT_ERR_INVALID_ARGUMENT;
                    continue;
                }
                zkt_withdraw_prove_inputs(w, a->d_variables, a->stride, b, w->plan.pi_pos.data(), pi + (base + b) * n_pi * 4, &ins[b]);
                ins[b].table = table.data();
                ins[b].table_len = table_len;
                ins[b].blinders = a->blinders + (base + b) * 19 * 4;
                good.push_back(b);
            }
            WdSlotMask mask{};
            size_t n_taken = 0;
            for (size_t k = 0; k < good.size(); ++k) {
                const size_t b = good[k];
                zkt_withdraw_result& r = results[base + b];
                uint8_t* proof = proofs + (base + b) * proof_stride;
                if (int rc = zkt_prove_set_next(c, k + 1 < good.size() ? &ins[good[k + 1]] : nullptr)) return rc;
                zkt_transcript* t = transcript();
                if (!t) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "withdraw prove: the transcript could not be made");
                size_t len = 0;
                const int rc = zkt_prove(c, &ins[b], t, proof, proof_len, &len);
                zkt_transcript_free(t);
                if (rc) {
                    if (!wd_is_proof_refusal(rc)) return rc;
                    memset(proof, 0, proof_len);
                    r.code = rc;
                    continue;
                }
                if (a->verify) {
                    zkt_verify_inputs v{};
                    v.n = n;
                    v.vk_commitments = S->vk_commits;
                    v.vk_is_infinity = S->vk_inf;
                    v.pi_roots = pi_roots.data();
                    v.pub_inputs = ins[b].pi_vals;
                    v.n_pi = n_pi;
                    v.proof = proof;
                    v.proof_len = len;
                    v.g = a->g_xy_mont;
                    int accepted = 0;
                    zkt_transcript* tv = transcript();
                    if (!tv) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "withdraw prove: the transcript could not be made");
                    const int vrc = zkt_verify(c->curve, &v, tv, a->h_g2_mont, a->beta_h_g2_mont, &accepted);
                    zkt_transcript_free(tv);
                    r.verified = !vrc && accepted ? 1 : 0;
                    if (!r.verified) continue;
                }
                if (a->append) {
                    mask.w[b >> 6] |= (uint64_t)1 << (b & 63);
                    taken.push_back(base + b);
                    ++n_taken;
                }
            }
            if (n_taken) {   // this chunk's leaves leave the maps before the next chunk's witness overwrites them
                void* out = (char*)w->d_new_leaves + (taken.size() - n_taken) * 32;
                if (c->curve == ZKT_CURVE_BN254)
                    hipLaunchKernelGGL((k_withdraw_new_leaves<Bn254Fr>), dim3(1), dim3(256), 0, c->stream, (const Fe<Bn254Fr>*)a->d_variables,
                                       (uint64_t)a->stride, leaf_var, mask, (uint32_t)cnt, (Fe<Bn254Fr>*)out);
                else
                    hipLaunchKernelGGL((k_withdraw_new_leaves<Bls381Fr>), dim3(1), dim3(256), 0, c->stream, (const Fe<Bls381Fr>*)a->d_variables,
                                       (uint64_t)a->stride, leaf_var, mask, (uint32_t)cnt, (Fe<Bls381Fr>*)out);
                ZKT_HIP(c, hipGetLastError());
            }
        }
        if (!taken.empty()) {
            uint64_t first = 0;
            if (int rc = zkt_merkle_tree_append_dev(c, tree, w->d_new_leaves, taken.size(), &first)) return rc;
            for (size_t k = 0; k < taken.size(); ++k) results[taken[k]].new_leaf_index = first + k;
        }
        return ZKT_OK;
    };
    const int rc = run();
    (void)zkt_prove_set_next(c, nullptr);
    const hipError_t e = hipStreamSynchronize(c->stream);
    if (rc) return rc;
    ZKT_HIP(c, e);
    return ZKT_OK;
}

int zkt_note_leaves(zkt_ctx* c, const zkt_poseidon* pos, const void* d_secrets, const void* d_identifiers, const void* d_amounts_u64, size_t m,
                    void* d_out_leaves) {
    if (!c || !pos) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (m == 0) return ZKT_OK;
    if (!d_secrets || !d_identifiers || !d_amounts_u64 || !d_out_leaves) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (m > ZKT_MERKLE_TREE_MAX) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "note leaves: at most ZKT_MERKLE_TREE_MAX deposits a call");
    (void)hipSetDevice(c->device);
    DevSet tmp(c->device);
    void* d_tmp = nullptr;
    int rc = tmp.alloc(c, &d_tmp, m * 3 * 32);
    if (!rc)
        rc = c->curve == ZKT_CURVE_BN254 ? note_leaves_t<Bn254Fr>(c, pos, d_secrets, d_identifiers, d_amounts_u64, m, d_out_leaves, d_tmp)
                                         : note_leaves_t<Bls381Fr>(c, pos, d_secrets, d_identifiers, d_amounts_u64, m, d_out_leaves, d_tmp);
    const hipError_t e = hipStreamSynchronize(c->stream);   // before `tmp` goes
    if (rc) return rc;
    ZKT_HIP(c, e);
    return ZKT_OK;
}

}  // extern "C"
