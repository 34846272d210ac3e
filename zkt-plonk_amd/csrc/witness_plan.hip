// zkt_witness_plan_* / zkt_witness_complete*: the variable map completed on the device from the circuit's free variables
// (include/zkt_plonk.h states the rule; witness_plan.hpp is the host planner and describes the schedule).
//
//   k_wp_narrow    one workgroup of 256 threads per witness walks a run of levels.  Within a level each thread takes rows at
//                  the workgroup's stride: it loads the row's record, its operands from the variable map with plain loads,
//                  computes, and writes the result with a plain vector store; __syncthreads() separates the levels.  A value
//                  written inside the launch is read only by the workgroup that wrote it (its own witness's map): workgroups
//                  exchange nothing inside a launch -- no grid barrier, no flags, no spinning, no atomics on values.
//   k_wp_wide      one level, a thread per (witness, row): a level reads only lower levels, which earlier launches finished.
//   k_wp_public    the closing launch, a thread per (witness, public row): PI = -(q_m a b + q_l a + q_r b + q_o c + q_c).
//
// Arithmetic: canonical Montgomery words from end to end (fe_add / fe_sub / fe_neg of fp.hpp, fe_mul through fx.hpp), as the
// prover requires its witness.  Rule R inverts with fe_inv, the Fermat ladder the kernels use; a circuit has a handful of
// such rows, and the threads of their level wait for them.  Rule Z (a pair's record) decides x = 0 on the canonical words,
// inverts with the same ladder when x != 0, and stores its two values with plain vector stores; it writes no status.
// Status block: per witness two 64-bit words, the number of rule-R rows with a zero denominator (atomicAdd) and
// 2^32 - their smallest row (atomicMax, 0 = none, so that clearing is a memset): a sum and a maximum, independent of the
// order of the atomics; vector atomics only.  Such rows are rare, so every thread that meets one reports it itself.
#include "witness_plan.hpp"
#include "poly.hpp"

#include <algorithm>
#include <cstring>
#include <vector>

namespace zkt {

constexpr int WP_THREADS = 256;
// A level with at least this many rows is a launch of its own.  Swept over 64 .. 4096 and "never" on an MI355X on the BN254
// withdraw circuits at 2^14 and 2^20 (docs/EXPERIMENTS.md, "witness completion from the free variables"): the depth decides
// the time, not the split -- batch 1 is the same within its spread everywhere, batch 8 is 2 % faster at 256 and 1024 (five
// launches on the 2^20 circuit: its widest levels on their own) than with everything in the narrow kernel.
constexpr uint32_t WP_WIDE_MIN_ROWS = 1024;

template <class P>
struct WpArgs {
    const WpRow* rows;
    const WpTuple<P>* tuples;
    const uint32_t* level_start;
    Fe<P>* vars;
    uint64_t stride;                 // scalars between two witnesses
    unsigned long long* status;      // two words per witness
    uint32_t level0, level1;
};

template <class P>
__device__ __attribute__((noinline)) Fe<P> wp_inv(const Fe<P>& a) {
    return fe_inv<P>(a);
}

// acc += t x, by the slot's flag
template <class P>
ZKT_D void wp_term(Fe<P>& acc, uint32_t flag, const Fe<P>* t, const Fe<P>& x) {
    if (flag == WP_ONE) acc = fe_add<P>(acc, x);
    else if (flag == WP_MINUS_ONE) acc = fe_sub<P>(acc, x);
    else if (flag == WP_GEN) acc = fe_add<P>(acc, fe_mul<P>(fe_load<P>(t), x));
}
// acc += t
template <class P>
ZKT_D void wp_const(Fe<P>& acc, uint32_t flag, const Fe<P>* t) {
    if (flag == WP_ONE) acc = fe_add<P>(acc, fe_one<P>());
    else if (flag == WP_MINUS_ONE) acc = fe_sub<P>(acc, fe_one<P>());
    else if (flag == WP_GEN) acc = fe_add<P>(acc, fe_load<P>(t));
}

// rule Z's record: x = 0: y = 0, z = t_o; else z = 0, y = t_m / x.  Not inlined, as wp_inv: a circuit has few such records,
// and the registers of k_wp_narrow stay those of rules O and R.  The record's words travel by value: a reference would pin the
// caller's copy of every record, rule O's too, to scratch
template <class P>
__device__ __attribute__((noinline)) void wp_pair(uint32_t in0, uint32_t out, uint32_t out2, uint32_t flags, const Fe<P>* t, Fe<P>* x) {
    const uint32_t fm = wp_flag(flags, WP_M), fo = wp_flag(flags, WP_O);
    Fe<P> a = fe_zero<P>(), y = fe_zero<P>(), z = fe_zero<P>();
    if (wp_flag(flags, WP_L) != WP_ZERO) a = fe_load<P>(x + in0);
    if (fe_is_zero<P>(a)) {     // canonical words: zero is all-zero words
        wp_const<P>(z, fo, t + WP_O);
    } else if (fm != WP_ZERO) {
        wp_term<P>(y, fm, t + WP_M, wp_inv<P>(a));
    }
    fe_store<P>(x + out, y);
    fe_store<P>(x + out2, z);
}

// one scheduled row of witness `wit` (x = its map): every index was checked against n_vars when the plan was made
template <class P>
ZKT_D void wp_row(const WpArgs<P>& q, uint32_t k, Fe<P>* x, uint32_t wit) {
    const WpRow r = q.rows[k];
    const Fe<P>* const t = q.tuples[r.coef].t;
    const uint32_t fm = wp_flag(r.flags, WP_M), fl = wp_flag(r.flags, WP_L), fr = wp_flag(r.flags, WP_R), fo = wp_flag(r.flags, WP_O),
                   fc = wp_flag(r.flags, WP_C);
    Fe<P> v = fe_zero<P>();
    if (!(r.flags & (WP_RULE_R | WP_RULE_Z))) {   // v = t_m a b + t_l a + t_r b + t_c (one test in front of rule O, as ever)
        Fe<P> a = fe_zero<P>(), b = fe_zero<P>();
        if (fm != WP_ZERO || fl != WP_ZERO) a = fe_load<P>(x + r.in0);
        if (fm != WP_ZERO || fr != WP_ZERO) b = fe_load<P>(x + r.in1);
        wp_const<P>(v, fc, t + WP_C);
        if (fm != WP_ZERO) wp_term<P>(v, fm, t + WP_M, fe_mul<P>(a, b));
        wp_term<P>(v, fl, t + WP_L, a);
        wp_term<P>(v, fr, t + WP_R, b);
    } else if (r.flags & WP_RULE_Z) {
        wp_pair<P>(r.in0, r.out, r.out2, r.flags, t, x);
        return;
    } else {                        // v = (t_l a + t_o c + t_c) / (t_m a + t_r)
        Fe<P> a = fe_zero<P>(), c = fe_zero<P>(), den = fe_zero<P>();
        if (fm != WP_ZERO || fl != WP_ZERO) a = fe_load<P>(x + r.in0);
        if (fo != WP_ZERO) c = fe_load<P>(x + r.in1);
        wp_const<P>(den, fr, t + WP_R);
        wp_term<P>(den, fm, t + WP_M, a);
        if (fe_is_zero<P>(den)) {   // the witness has no such value: 0 is written and the row reported
            atomicAdd(q.status + 2 * wit, 1ull);
            atomicMax(q.status + 2 * wit + 1, (1ull << 32) - r.row);
        } else {
            wp_const<P>(v, fc, t + WP_C);
            wp_term<P>(v, fl, t + WP_L, a);
            wp_term<P>(v, fo, t + WP_O, c);
            v = fe_mul<P>(v, wp_inv<P>(den));
        }
    }
    fe_store<P>(x + r.out, v);
}

template <class P>
__global__ __launch_bounds__(WP_THREADS) void k_wp_narrow(WpArgs<P> q) {
    Fe<P>* const x = q.vars + (uint64_t)blockIdx.x * q.stride;
#pragma unroll 1
    for (uint32_t l = q.level0; l < q.level1; ++l) {
        const uint32_t end = q.level_start[l + 1];
#pragma unroll 1
        for (uint32_t k = q.level_start[l] + threadIdx.x; k < end; k += WP_THREADS) wp_row<P>(q, k, x, blockIdx.x);
        __syncthreads();   // the level's stores are visible to this workgroup before the next level's loads
    }
}

template <class P>
__global__ __launch_bounds__(WP_THREADS) void k_wp_wide(WpArgs<P> q) {
    const uint32_t first = q.level_start[q.level0], end = q.level_start[q.level0 + 1];
    const uint32_t k = first + blockIdx.x * WP_THREADS + threadIdx.x;   // rows < 2^25: no wrap
    if (k < end) wp_row<P>(q, k, q.vars + (uint64_t)blockIdx.y * q.stride, blockIdx.y);
}

template <class P>
__global__ __launch_bounds__(64) void k_wp_public(const WpPublic<P>* pub, uint32_t n_pi, const Fe<P>* vars, uint64_t stride, Fe<P>* out) {
    const uint32_t j = blockIdx.x * 64 + threadIdx.x;
    if (j >= n_pi) return;
    const Fe<P>* const x = vars + (uint64_t)blockIdx.y * stride;
    const WpPublic<P>* const r = pub + j;
    const uint32_t ia = r->w[0], ib = r->w[1], ic = r->w[2];
    const Fe<P> a = ia == WP_VAR_ZERO ? fe_zero<P>() : fe_load<P>(x + ia);
    const Fe<P> b = ib == WP_VAR_ZERO ? fe_zero<P>() : fe_load<P>(x + ib);
    const Fe<P> c = ic == WP_VAR_ZERO ? fe_zero<P>() : fe_load<P>(x + ic);
    Fe<P> t = fe_add<P>(fe_mul<P>(fe_load<P>(r->q + WP_M), b), fe_load<P>(r->q + WP_L));   // (q_m b + q_l) a + ...
    t = fe_mul<P>(t, a);
    t = fe_add<P>(t, fe_mul<P>(fe_load<P>(r->q + WP_R), b));
    t = fe_add<P>(t, fe_mul<P>(fe_load<P>(r->q + WP_O), c));
    t = fe_add<P>(t, fe_load<P>(r->q + WP_C));
    fe_store<P>(out + (uint64_t)blockIdx.y * n_pi + j, fe_neg<P>(t));
}

}  // namespace zkt

struct zkt_witness_plan {
    int curve = 0;
    size_t n_vars = 0, n_pi = 0;
    std::vector<uint8_t> kind;
    std::vector<uint32_t> level_start;
    uint32_t depth = 0, max_level_rows = 0;
    uint64_t n_free = 0, n_out = 0, n_right = 0, n_unused = 0, n_pairs = 0, device_bytes = 0;
    std::vector<zkt::WpLaunch> launches;
    zkt::DevSet mem;                       // everything the plan holds on the device: freed with the plan
    void *d_rows = nullptr, *d_tuples = nullptr, *d_level_start = nullptr, *d_public = nullptr, *d_status = nullptr;
    explicit zkt_witness_plan(int dev) : mem(dev) {}
};

namespace zkt {

static size_t wp_round(size_t bytes) { return (std::max<size_t>(bytes, 1) + 255) / 256 * 256; }

template <class P>
static int plan_create_t(zkt_ctx* c, const WitnessPlanKeys& K, const uint32_t* const* w, size_t n_rows, size_t n_vars,
                         const size_t* pi_pos, size_t n_pi, uint32_t rules, zkt_witness_plan* pl) {
    using F = Fe<P>;
    static_assert(sizeof(F) == 32 && sizeof(WpTuple<P>) == 160 && sizeof(WpPublic<P>) == 192, "layouts of witness_plan.hpp");
    const size_t n = (size_t)1 << K.log_n;
    // the selector evaluations, made as the witness check makes them, and brought to the host
    DevSet tmp(c->device);
    void* d_sel[5];
    for (void*& d : d_sel)
        if (int rc = tmp.alloc(c, &d, n * 32)) return rc;
    if (int rc = selector_evals_enqueue(c, K.log_n, K.pk, d_sel)) {
        (void)hipStreamSynchronize(c->stream);
        return rc;
    }
    std::vector<F> sel[5];
    for (int k = 0; k < 5; ++k) {
        sel[k].resize(n);
        ZKT_HIP(c, hipMemcpyAsync(sel[k].data(), d_sel[k], n * 32, hipMemcpyDeviceToHost, c->stream));
    }
    ZKT_HIP(c, hipStreamSynchronize(c->stream));
    const F* selp[5];
    for (int k = 0; k < 5; ++k) selp[k] = sel[k].data();

    WitnessPlan<P> W;
    witness_plan_make<P>(selp, w, n_rows, n_vars, pi_pos, n_pi, W, rules);
    std::vector<WpPublic<P>> pub(n_pi);
    for (size_t j = 0; j < n_pi; ++j) {
        const size_t i = pi_pos[j];
        memset((void*)&pub[j], 0, sizeof(pub[j]));
        for (int k = 0; k < 3; ++k) pub[j].w[k] = i < n_rows ? w[k][i] : WP_VAR_ZERO;
        for (int k = 0; k < 5; ++k) pub[j].q[k] = sel[k][i];
    }

    pl->curve = c->curve;
    pl->n_vars = n_vars;
    pl->n_pi = n_pi;
    pl->kind = W.kind;
    pl->level_start = W.level_start;
    pl->depth = W.depth;
    pl->max_level_rows = W.max_level_rows;
    pl->n_free = W.n_free; pl->n_out = W.n_out; pl->n_right = W.n_right; pl->n_unused = W.n_unused;
    pl->n_pairs = W.n_pairs;
    pl->launches = witness_plan_split(pl->level_start, pl->depth, WP_WIDE_MIN_ROWS);

    struct Part {
        void** d;
        const void* h;
        size_t bytes;
    } parts[] = {{&pl->d_rows, W.rows.data(), W.rows.size() * sizeof(WpRow)},
                 {&pl->d_tuples, W.tuples.data(), W.tuples.size() * sizeof(WpTuple<P>)},
                 {&pl->d_level_start, W.level_start.data(), W.level_start.size() * 4},
                 {&pl->d_public, pub.data(), pub.size() * sizeof(WpPublic<P>)},
                 {&pl->d_status, nullptr, (size_t)ZKT_WITNESS_BATCH_MAX * 16}};
    for (const Part& p : parts) {
        const size_t bytes = wp_round(p.bytes);
        if (int rc = pl->mem.alloc(c, p.d, bytes)) return rc;
        pl->device_bytes += bytes;
        if (p.h && p.bytes) ZKT_HIP(c, hipMemcpyAsync(*p.d, p.h, p.bytes, hipMemcpyHostToDevice, c->stream));
        if (!p.h) ZKT_HIP(c, hipMemsetAsync(*p.d, 0, bytes, c->stream));
    }
    ZKT_HIP(c, hipStreamSynchronize(c->stream));   // the uploads read this frame's vectors
    return ZKT_OK;
}

int witness_plan_create(zkt_ctx* c, const WitnessPlanKeys& K, const uint32_t* w_l, const uint32_t* w_r, const uint32_t* w_o,
                        size_t n_rows, size_t n_vars, int wiring_on_device, const size_t* pi_pos, size_t n_pi, uint32_t rules,
                        zkt_witness_plan** out) {
    const size_t n = (size_t)1 << K.log_n;
    if (rules & ~(uint32_t)ZKT_WITNESS_RULE_IS_ZERO) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "unknown rule bits");
    if (n_rows > n) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "more rows than the circuit bound");
    if (n_rows && (!w_l || !w_r || !w_o)) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null wire index vector");
    if (n_pi && !pi_pos) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null public-input positions");
    if (n_vars > 0xFFFFFFFEull) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "too many variables");
    for (size_t j = 0; j < n_pi; ++j) {
        if (pi_pos[j] >= n) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "public input position out of range");
        if (j && pi_pos[j] <= pi_pos[j - 1])
            return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "public input positions must be ascending and distinct");
    }
    (void)hipSetDevice(c->device);
    std::vector<uint32_t> host[3];
    const uint32_t* w[3] = {w_l, w_r, w_o};
    if (wiring_on_device && n_rows) {
        for (int k = 0; k < 3; ++k) {
            host[k].resize(n_rows);
            ZKT_HIP(c, hipMemcpyAsync(host[k].data(), w[k], n_rows * 4, hipMemcpyDeviceToHost, c->stream));
        }
        ZKT_HIP(c, hipStreamSynchronize(c->stream));
        for (int k = 0; k < 3; ++k) w[k] = host[k].data();
    }
    for (int k = 0; k < 3; ++k)
        for (size_t i = 0; i < n_rows; ++i)
            if (w[k][i] != ZKT_VARIABLE_ZERO && w[k][i] >= n_vars)
                return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "wire index outside the variable map: every entry must be < n_vars or ZKT_VARIABLE_ZERO");
    zkt_witness_plan* pl = new zkt_witness_plan(c->device);
    const int rc = c->curve == ZKT_CURVE_BN254 ? plan_create_t<Bn254Fr>(c, K, w, n_rows, n_vars, pi_pos, n_pi, rules, pl)
                                                : plan_create_t<Bls381Fr>(c, K, w, n_rows, n_vars, pi_pos, n_pi, rules, pl);
    if (rc) {
        (void)hipStreamSynchronize(c->stream);
        delete pl;
        return rc;
    }
    *out = pl;
    return ZKT_OK;
}

template <class P>
static int complete_enqueue_t(zkt_ctx* c, const zkt_witness_plan* pl, void* d_variables, size_t stride, size_t batch, void* d_out_pi) {
    ProfScope prof(c, "witness_complete");
    WpArgs<P> q{};
    q.rows = (const WpRow*)pl->d_rows;
    q.tuples = (const WpTuple<P>*)pl->d_tuples;
    q.level_start = (const uint32_t*)pl->d_level_start;
    q.vars = (Fe<P>*)d_variables;
    q.stride = stride;
    q.status = (unsigned long long*)pl->d_status;
    for (const WpLaunch& L : pl->launches) {
        q.level0 = L.level0;
        q.level1 = L.level1;
        if (L.wide) {
            const uint32_t rows = pl->level_start[L.level0 + 1] - pl->level_start[L.level0];
            hipLaunchKernelGGL(k_wp_wide<P>, dim3((rows + WP_THREADS - 1) / WP_THREADS, (unsigned)batch), dim3(WP_THREADS), 0, c->stream, q);
        } else {
            hipLaunchKernelGGL(k_wp_narrow<P>, dim3((unsigned)batch), dim3(WP_THREADS), 0, c->stream, q);
        }
    }
    if (d_out_pi && pl->n_pi)
        hipLaunchKernelGGL(k_wp_public<P>, dim3((unsigned)((pl->n_pi + 63) / 64), (unsigned)batch), dim3(64), 0, c->stream,
                           (const WpPublic<P>*)pl->d_public, (uint32_t)pl->n_pi, (const Fe<P>*)d_variables, (uint64_t)stride,
                           (Fe<P>*)d_out_pi);
    ZKT_HIP(c, hipGetLastError());
    return ZKT_OK;
}

static int complete_check(zkt_ctx* c, const zkt_witness_plan* pl, const void* vars, size_t stride, size_t batch) {
    if (!c) return ZKT_ERR_INVALID_ARGUMENT;
    if (!pl) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null plan");
    if (pl->curve != c->curve || pl->mem.device != c->device)
        return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "the plan belongs to another curve or device");
    if (batch < 1 || batch > ZKT_WITNESS_BATCH_MAX) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "1 <= batch <= ZKT_WITNESS_BATCH_MAX");
    if (stride < pl->n_vars) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "stride below n_vars");
    if (!vars && pl->n_vars) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null variable map");
    return ZKT_OK;
}

// zkt_debug_witness_plan_host: the host planner alone, on caller-supplied selectors and wiring (no device, no context)
template <class R>
static int debug_plan_host_t(const uint64_t* const* selectors, const uint32_t* const* w, size_t n_rows, size_t n_vars, const size_t* pi_pos,
                             size_t n_pi, uint32_t rules, uint8_t* out_kind, uint32_t* out_def_row, uint32_t* out_level) {
    const Fe<R>* sel[5];
    for (int k = 0; k < 5; ++k) sel[k] = reinterpret_cast<const Fe<R>*>(selectors[k]);
    WitnessPlan<R> W;
    witness_plan_make<R>(sel, w, n_rows, n_vars, pi_pos, n_pi, W, rules);
    if (n_vars) {
        memcpy(out_kind, W.kind.data(), n_vars);
        memcpy(out_def_row, W.def_row.data(), n_vars * 4);
        memcpy(out_level, W.level.data(), n_vars * 4);
    }
    return ZKT_OK;
}

}  // namespace zkt

using namespace zkt;

extern "C" {

void zkt_witness_plan_free(zkt_ctx* c, zkt_witness_plan* pl) {
    if (!pl) return;
    if (c) (void)hipStreamSynchronize(c->stream);
    delete pl;
}

int zkt_witness_plan_info(const zkt_witness_plan* pl, zkt_witness_plan_report* info) {
    if (!pl || !info) return ZKT_ERR_INVALID_ARGUMENT;
    memset(info, 0, sizeof(*info));
    info->n_free = pl->n_free;
    info->n_out = pl->n_out;
    info->n_right = pl->n_right;
    info->n_unused = pl->n_unused;
    info->depth = pl->depth;
    info->max_level_rows = pl->max_level_rows;
    info->launches = (uint32_t)pl->launches.size();
    info->reserved = (uint32_t)pl->n_pairs;
    info->device_bytes = pl->device_bytes;
    return ZKT_OK;
}

int zkt_witness_plan_kinds(const zkt_witness_plan* pl, uint8_t* out_kind) {
    if (!pl || (!out_kind && pl->n_vars)) return ZKT_ERR_INVALID_ARGUMENT;
    if (pl->n_vars) memcpy(out_kind, pl->kind.data(), pl->n_vars);
    return ZKT_OK;
}

int zkt_debug_witness_plan_split(zkt_witness_plan* pl, uint32_t wide_min_rows) {
    if (!pl) return ZKT_ERR_INVALID_ARGUMENT;
    pl->launches = witness_plan_split(pl->level_start, pl->depth, wide_min_rows ? wide_min_rows : WP_WIDE_MIN_ROWS);
    return ZKT_OK;
}

int zkt_witness_complete_enqueue(zkt_ctx* c, const zkt_witness_plan* pl, void* d_variables, size_t stride, size_t batch, void* d_out_pi) {
    if (int rc = complete_check(c, pl, d_variables, stride, batch)) return rc;
    (void)hipSetDevice(c->device);
    return c->curve == ZKT_CURVE_BN254 ? complete_enqueue_t<Bn254Fr>(c, pl, d_variables, stride, batch, d_out_pi)
                                       : complete_enqueue_t<Bls381Fr>(c, pl, d_variables, stride, batch, d_out_pi);
}

int zkt_witness_complete_status(zkt_ctx* c, const zkt_witness_plan* pl, size_t batch, zkt_witness_status* out) {
    if (!c) return ZKT_ERR_INVALID_ARGUMENT;
    if (!pl || !out) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (pl->mem.device != c->device) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "the plan belongs to another device");
    if (batch < 1 || batch > ZKT_WITNESS_BATCH_MAX) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "1 <= batch <= ZKT_WITNESS_BATCH_MAX");
    (void)hipSetDevice(c->device);
    unsigned long long h[2 * ZKT_WITNESS_BATCH_MAX];
    ZKT_HIP(c, hipMemcpyAsync(h, pl->d_status, batch * 16, hipMemcpyDeviceToHost, c->stream));
    ZKT_HIP(c, hipMemsetAsync(pl->d_status, 0, (size_t)ZKT_WITNESS_BATCH_MAX * 16, c->stream));
    ZKT_HIP(c, hipStreamSynchronize(c->stream));
    for (size_t k = 0; k < batch; ++k) {
        out[k].n_unsolvable = h[2 * k];
        out[k].first_unsolvable = h[2 * k + 1] ? (1ull << 32) - h[2 * k + 1] : ZKT_CHECK_NONE;
    }
    return ZKT_OK;
}

int zkt_witness_complete(zkt_ctx* c, const zkt_witness_plan* pl, uint64_t* variables, size_t stride, size_t batch, uint64_t* out_pi,
                         zkt_witness_status* out_status) {
    if (int rc = complete_check(c, pl, variables, stride, batch)) return rc;
    (void)hipSetDevice(c->device);
    DevSet tmp(c->device);
    void *d_vars = nullptr, *d_pi = nullptr;
    const size_t bytes = batch * stride * 32, pi_bytes = batch * pl->n_pi * 32;
    int rc = tmp.alloc(c, &d_vars, bytes);
    if (!rc && out_pi && pi_bytes) rc = tmp.alloc(c, &d_pi, pi_bytes);
    auto run = [&]() -> int {
        if (bytes) ZKT_HIP(c, hipMemcpyAsync(d_vars, variables, bytes, hipMemcpyHostToDevice, c->stream));
        if (int r = zkt_witness_complete_enqueue(c, pl, d_vars, stride, batch, d_pi)) return r;
        if (bytes) ZKT_HIP(c, hipMemcpyAsync(variables, d_vars, bytes, hipMemcpyDeviceToHost, c->stream));
        if (d_pi) ZKT_HIP(c, hipMemcpyAsync(out_pi, d_pi, pi_bytes, hipMemcpyDeviceToHost, c->stream));
        if (out_status) return zkt_witness_complete_status(c, pl, batch, out_status);
        ZKT_HIP(c, hipStreamSynchronize(c->stream));
        return ZKT_OK;
    };
    if (!rc) rc = run();
    if (rc) (void)hipStreamSynchronize(c->stream);   // before `tmp` goes
    return rc;
}

int zkt_debug_witness_plan_host_ex(int curve, const uint64_t* const* selectors, const uint32_t* const* wires, size_t n_rows, size_t n_vars,
                                   const size_t* pi_pos, size_t n_pi, uint32_t rules, uint8_t* out_kind, uint32_t* out_def_row,
                                   uint32_t* out_level) {
    if (rules & ~(uint32_t)ZKT_WITNESS_RULE_IS_ZERO) return ZKT_ERR_INVALID_ARGUMENT;
    if (!selectors || !wires || (n_vars && (!out_kind || !out_def_row || !out_level)) || (n_pi && !pi_pos)) return ZKT_ERR_INVALID_ARGUMENT;
    if (n_vars > 0xFFFFFFFEull) return ZKT_ERR_INVALID_ARGUMENT;
    for (int k = 0; k < 5; ++k)
        if (n_rows && !selectors[k]) return ZKT_ERR_INVALID_ARGUMENT;
    for (int k = 0; k < 3; ++k)
        if (n_rows && !wires[k]) return ZKT_ERR_INVALID_ARGUMENT;
    for (size_t j = 1; j < n_pi; ++j)
        if (pi_pos[j] <= pi_pos[j - 1]) return ZKT_ERR_INVALID_ARGUMENT;
    if (curve == ZKT_CURVE_BN254) return debug_plan_host_t<Bn254Fr>(selectors, wires, n_rows, n_vars, pi_pos, n_pi, rules, out_kind, out_def_row, out_level);
    if (curve == ZKT_CURVE_BLS12_381)
        return debug_plan_host_t<Bls381Fr>(selectors, wires, n_rows, n_vars, pi_pos, n_pi, rules, out_kind, out_def_row, out_level);
    return ZKT_ERR_INVALID_ARGUMENT;
}

int zkt_debug_witness_plan_host(int curve, const uint64_t* const* selectors, const uint32_t* const* wires, size_t n_rows, size_t n_vars,
                                const size_t* pi_pos, size_t n_pi, uint8_t* out_kind, uint32_t* out_def_row, uint32_t* out_level) {
    return zkt_debug_witness_plan_host_ex(curve, selectors, wires, n_rows, n_vars, pi_pos, n_pi, 0, out_kind, out_def_row, out_level);
}

}  // extern "C"
