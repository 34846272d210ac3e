// zkt_circuit_check_witness: check_gate of the reference's circuit debugger (constraint_system/helper.rs:13-75) over every
// row of the loaded circuit, on the device, reduced to "which row, which rule, how many".
//
//   selector evaluations  q_m q_l q_r q_o q_c on the n domain = fft(n) of the key's coefficients, four and one in a batched
//                         transform each; made per call into the call's scratch, never cached in the circuit state
//   k_check_gates         one row per thread in a grid-stride loop.  Variables form: the gather variables[w_x[i]] is fused
//                         in, the three wire vectors are never materialised.  Arithmetic rule: the gate equation's value
//                         is not 0.  Lookup rule, only where q_lookup is not 0: q_lookup c is not 0 and a binary search
//                         does not find it in the call's own sorted copy of the table (sorted on the host, by the order
//                         of key_cmp in poly.hip: the Montgomery words as one big integer)
//   k_check_residual      one thread: the gate equation's value again at the first failing row
//   k_check_sigma         ZKT_CHECK_WIRING: the sigma evaluations made from the given wiring (sigma_enqueue, sigma.hip)
//                         against the key's, 32 bytes a wire, keyed by the wire number p = 3 row + column
//
// Public inputs: the kernel binary-searches its row in the sorted positions (a handful of 32-bit words every thread of a
// wave reads alike, so they stay in cache) rather than reading a scattered n-vector: that vector would cost a memset and
// a read of n x 32 B for the few rows that have a value, and n_pi separate small uploads instead of two.
//
// Arithmetic: every value is a canonical Montgomery residue (< p) from end to end -- the transforms store canonical words,
// fe_mul and fe_add return canonical words, the witness is canonical as the prover requires -- so there is no lazy sum and
// zero is decided by fe_is_zero on a fully reduced value: a sum that is 0 only modulo p has already been folded to 0.
//
// Reduction: per thread a count and a minimum per rule; per wave by shuffles; per workgroup through four LDS slots; then
// one 64-bit atomicMin and one atomicAdd per rule per workgroup into the status block.  These are minima and sums: no
// result depends on the order of the atomics or on which workgroup runs first.  The status block is written with ordinary
// vector stores and vector atomics only.
//
// The batch (zkt_circuit_check_witness_batch): `batch` variable maps under one wiring, as a completion leaves them.
//   selector evaluations    once per call, as above
//   k_check_gates_batch     grid (rows, tiles of CKB_TILE witnesses).  A thread loads, once per row, the five selectors,
//                           q_lookup, the three wire indices (checked against n_vars there) and the row's public-input slot,
//                           then walks its tile: per witness three gathers, the gate equation, and the binary search in
//                           that witness's own sorted table (all tables are sorted on the host and uploaded end to end,
//                           with an (offset, length) pair per witness).  Then the reduction above, per witness of the tile,
//                           into that witness's own CK_WORDS block: one atomicAdd and one atomicMin per rule per witness
//                           per workgroup, sums and minima, vector atomics only
//   k_check_residual_batch  a thread per witness
//   k_check_sigma           the shared wiring once, into witness 0's block; the host copies it into every report
// CKB_TILE = 8.  In registers: a count and a minimum per rule per witness, 4 x CKB_TILE = 32 VGPRs, beside the 40 + 4 that
// the row's five selectors, three indices and slot occupy across the tile (q_lookup is kept as one bit and read again by the
// few rows that look up) and what one gate evaluation and the compiler's overlapping of the tile's gathers need: 166 by the
// compiler's count, the last size at which three waves a SIMD fit (512 / 3 = 170); 16 would add 32 more and cost the third.
// In bytes: a row's shared part is 6 x 32 + 3 x 4 = 204 B, read once per tile instead of once per witness, while the three
// gathered values, 96 B a witness, cannot be shared.  A tile of T reads 204 / T + 96 B a witness and row: 300 at T = 1,
// 121.5 at T = 8, 108.8 at T = 16, 96 at best.  T = 8 is within 27 % of the floor; doubling it again gains 10 % of the
// traffic for a fifth more registers.
#include "poly.hpp"

#include <algorithm>
#include <cstring>
#include <numeric>
#include <vector>

namespace zkt {

constexpr int CK_THREADS = 256;
constexpr int CK_ROWS_PER_THREAD = 4;     // what the grid is sized for; above CK_MAX_BLOCKS workgroups the loop turns more often
constexpr unsigned CK_MAX_BLOCKS = 2048;
constexpr uint32_t CK_NONE32 = 0xFFFFFFFFu;
constexpr int CKB_TILE = 8;               // witnesses a thread of k_check_gates_batch walks per row (head comment)
// status block, 64-bit words
enum { CK_N_ARITH = 0, CK_FIRST_ARITH, CK_N_LOOKUP, CK_FIRST_LOOKUP, CK_N_WIRING, CK_FIRST_WIRING, CK_BAD_INDEX, CK_PAD, CK_RESIDUAL,
       CK_WORDS = CK_RESIDUAL + 4 };

struct CheckArgs {
    const void *q_m, *q_l, *q_r, *q_o, *q_c, *q_lookup;   // n evaluations each
    const void *a, *b, *c;                                // evaluation form: n_rows values each
    const void* variables;                                // variables form
    const uint32_t *w_l, *w_r, *w_o;
    uint32_t n, n_rows, n_vars;
    const uint32_t* pi_pos;                               // ascending
    const void* pi_vals;
    uint32_t n_pi;
    const void* table;                                    // sorted, distinct
    uint32_t table_len;
    unsigned long long* status;
};

// the order of key_cmp (poly.hip): the Montgomery words compared from the top
template <class P>
ZKT_HD int ck_cmp(const Fe<P>& a, const Fe<P>& b) {
#pragma unroll
    for (int i = P::N - 1; i >= 0; --i) {
        if (a.v[i] < b.v[i]) return -1;
        if (a.v[i] > b.v[i]) return 1;
    }
    return 0;
}

template <class P, bool VARS>
ZKT_D Fe<P> ck_wire(const CheckArgs& q, const void* evals, const uint32_t* idx, uint32_t i) {
    if (i >= q.n_rows) return fe_zero<P>();
    if (!VARS) return fe_load<P>((const Fe<P>*)evals + i);
    const uint32_t k = idx[i];
    if (k == ZKT_VARIABLE_ZERO) return fe_zero<P>();
    if (k < q.n_vars) return fe_load<P>((const Fe<P>*)q.variables + k);
    atomicOr(q.status + CK_BAD_INDEX, 1ull);   // reported as ZKT_ERR_INVALID_ARGUMENT; the row is read as Variable::Zero
    return fe_zero<P>();
}

// q_m a b + q_l a + q_r b + q_o c + q_c + pi at row i, as (q_m b + q_l) a + ...; canonical
template <class P>
ZKT_D Fe<P> ck_gate(const CheckArgs& q, uint32_t i, const Fe<P>& a, const Fe<P>& b, const Fe<P>& c) {
    const Fe<P>* const sel[5] = {(const Fe<P>*)q.q_m, (const Fe<P>*)q.q_l, (const Fe<P>*)q.q_r, (const Fe<P>*)q.q_o, (const Fe<P>*)q.q_c};
    Fe<P> t = fe_add<P>(fe_mul<P>(fe_load<P>(sel[0] + i), b), fe_load<P>(sel[1] + i));
    t = fe_mul<P>(t, a);
    t = fe_add<P>(t, fe_mul<P>(fe_load<P>(sel[2] + i), b));
    t = fe_add<P>(t, fe_mul<P>(fe_load<P>(sel[3] + i), c));
    t = fe_add<P>(t, fe_load<P>(sel[4] + i));
    uint32_t lo = 0, hi = q.n_pi;                   // the first position >= i
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (q.pi_pos[mid] < i) lo = mid + 1;
        else hi = mid;
    }
    if (lo < q.n_pi && q.pi_pos[lo] == i) t = fe_add<P>(t, fe_load<P>((const Fe<P>*)q.pi_vals + lo));
    return t;
}

// count and minimum of the workgroup into the status block: one atomicAdd and one atomicMin when anything failed
ZKT_D void ck_block_reduce(uint32_t cnt, uint32_t mn, unsigned long long* n_slot, unsigned long long* first_slot, uint32_t* sh_cnt,
                           uint32_t* sh_min) {
    constexpr int WAVES = CK_THREADS / 64;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        cnt += __shfl_xor(cnt, off);
        const uint32_t o = __shfl_xor(mn, off);
        mn = o < mn ? o : mn;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        sh_cnt[wave] = cnt;
        sh_min[wave] = mn;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t total = 0, first = CK_NONE32;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            total += sh_cnt[w];
            first = sh_min[w] < first ? sh_min[w] : first;
        }
        if (total) {
            atomicAdd(n_slot, (unsigned long long)total);
            atomicMin(first_slot, (unsigned long long)first);
        }
    }
    __syncthreads();
}

template <class P, bool VARS>
__global__ __launch_bounds__(CK_THREADS) void k_check_gates(CheckArgs q) {
    __shared__ uint32_t sh_cnt[CK_THREADS / 64], sh_min[CK_THREADS / 64];
    uint32_t n_arith = 0, first_arith = CK_NONE32, n_lookup = 0, first_lookup = CK_NONE32;
    const uint32_t stride = gridDim.x * CK_THREADS;
#pragma unroll 1
    for (uint32_t i = blockIdx.x * CK_THREADS + threadIdx.x; i < q.n; i += stride) {   // n <= 2^25: no wrap
        const Fe<P> a = ck_wire<P, VARS>(q, q.a, q.w_l, i);
        const Fe<P> b = ck_wire<P, VARS>(q, q.b, q.w_r, i);
        const Fe<P> c = ck_wire<P, VARS>(q, q.c, q.w_o, i);
        if (!fe_is_zero<P>(ck_gate<P>(q, i, a, b, c))) {
            ++n_arith;
            first_arith = i < first_arith ? i : first_arith;   // rows rise along the loop; kept explicit
        }
        const Fe<P> ql = fe_load<P>((const Fe<P>*)q.q_lookup + i);
        if (!fe_is_zero<P>(ql)) {
            const Fe<P> f = fe_mul<P>(ql, c);
            if (!fe_is_zero<P>(f)) {
                const Fe<P>* const tab = (const Fe<P>*)q.table;
                uint32_t lo = 0, hi = q.table_len;
                while (lo < hi) {
                    const uint32_t mid = lo + (hi - lo) / 2;
                    if (ck_cmp<P>(fe_load<P>(tab + mid), f) < 0) lo = mid + 1;
                    else hi = mid;
                }
                if (lo >= q.table_len || ck_cmp<P>(fe_load<P>(tab + lo), f) != 0) {
                    ++n_lookup;
                    first_lookup = i < first_lookup ? i : first_lookup;
                }
            }
        }
    }
    ck_block_reduce(n_arith, first_arith, q.status + CK_N_ARITH, q.status + CK_FIRST_ARITH, sh_cnt, sh_min);
    ck_block_reduce(n_lookup, first_lookup, q.status + CK_N_LOOKUP, q.status + CK_FIRST_LOOKUP, sh_cnt, sh_min);
}

// after k_check_gates on the same stream: the equation's value at the first failing row, two 32-bit words per status word
template <class P, bool VARS>
__global__ void k_check_residual(CheckArgs q) {
    if (blockIdx.x || threadIdx.x) return;
    const unsigned long long first = q.status[CK_FIRST_ARITH];
    if (first >= q.n) return;                       // none: the residual words stay 0
    const uint32_t i = (uint32_t)first;
    const Fe<P> t = ck_gate<P>(q, i, ck_wire<P, VARS>(q, q.a, q.w_l, i), ck_wire<P, VARS>(q, q.b, q.w_r, i),
                               ck_wire<P, VARS>(q, q.c, q.w_o, i));
#pragma unroll
    for (int k = 0; k < 4; ++k) q.status[CK_RESIDUAL + k] = (unsigned long long)t.v[2 * k] | ((unsigned long long)t.v[2 * k + 1] << 32);
}

// wires (col, g) whose sigma evaluation made from the given wiring differs from the key's; key p = 3 g + col
template <class P>
__global__ __launch_bounds__(CK_THREADS) void k_check_sigma(const Fe<P>* m0, const Fe<P>* m1, const Fe<P>* m2, const Fe<P>* k0,
                                                            const Fe<P>* k1, const Fe<P>* k2, uint32_t n, unsigned long long* status) {
    __shared__ uint32_t sh_cnt[CK_THREADS / 64], sh_min[CK_THREADS / 64];
    const Fe<P>* const made[3] = {m0, m1, m2};
    const Fe<P>* const key[3] = {k0, k1, k2};
    uint32_t cnt = 0, first = CK_NONE32;
    const uint32_t stride = gridDim.x * CK_THREADS;
#pragma unroll 1
    for (uint32_t g = blockIdx.x * CK_THREADS + threadIdx.x; g < n; g += stride) {
#pragma unroll
        for (uint32_t col = 0; col < 3; ++col) {
            if (!fe_eq<P>(fe_load<P>(made[col] + g), fe_load<P>(key[col] + g))) {
                ++cnt;
                const uint32_t p = 3 * g + col;     // n <= 2^25: below 2^27
                first = p < first ? p : first;
            }
        }
    }
    ck_block_reduce(cnt, first, status + CK_N_WIRING, status + CK_FIRST_WIRING, sh_cnt, sh_min);
}

static unsigned ck_blocks(size_t n) {
    const size_t per = (size_t)CK_THREADS * CK_ROWS_PER_THREAD;
    return (unsigned)std::min<size_t>(std::max<size_t>((n + per - 1) / per, 1), CK_MAX_BLOCKS);
}

int selector_evals_enqueue(zkt_ctx* c, int log_n, const void* const* pk, void* const* outs) {
    const size_t n = (size_t)1 << log_n;
    size_t lens[5];
    for (size_t& l : lens) l = n;   // the key's buffers hold n coefficients, zero above their length
    static_assert(NTT_MAX_BATCH >= 4, "four selectors in one batch");
    if (int rc = ntt_run_batch(c, log_n, 0, 0, 4, pk, lens, outs)) return rc;
    return ntt_run_batch(c, log_n, 0, 0, 1, pk + 4, lens + 4, outs + 4);
}

template <class P>
static int witness_check_t(zkt_ctx* c, const WitnessCheckKeys& K, const zkt_prove_inputs& in, int flags, zkt_witness_report* out) {
    using F = Fe<P>;
    static_assert(sizeof(F) == 32, "scalar field element = 8 words");
    const int log_n = K.log_n;
    const size_t n = (size_t)1 << log_n;
    const bool vars = in.a_evals == nullptr;
    const bool wiring = (flags & ZKT_CHECK_WIRING) != 0;
    const bool on_device = in.wires_on_device != 0;
    const size_t rows = in.n_rows, n_pi = in.n_pi, tl = in.table_len;

    // ---- host side: the table sorted by the kernel's order (as the prover sorts its keys), the public inputs by row ----
    std::vector<F> sorted(tl);
    if (tl) {
        const F* t = reinterpret_cast<const F*>(in.table);
        std::vector<uint32_t> order(tl);
        std::iota(order.begin(), order.end(), 0u);
        std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return ck_cmp<P>(t[x], t[y]) < 0; });
        for (size_t i = 0; i < tl; ++i) sorted[i] = t[order[i]];
        for (size_t i = 1; i < tl; ++i)
            if (ck_cmp<P>(sorted[i - 1], sorted[i]) == 0)
                return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "lookup table holds a repeated value");
    }
    std::vector<uint32_t> pos(n_pi);
    std::vector<F> pvals(n_pi);
    if (n_pi) {
        std::vector<uint32_t> order(n_pi);
        std::iota(order.begin(), order.end(), 0u);
        std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return in.pi_pos[x] < in.pi_pos[y]; });
        for (size_t i = 0; i < n_pi; ++i) {
            pos[i] = (uint32_t)in.pi_pos[order[i]];
            pvals[i] = reinterpret_cast<const F*>(in.pi_vals)[order[i]];
        }
    }

    // ---- the call's scratch, one block carved on 256-byte boundaries ----
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t here = at;
        at += (bytes + 255) / 256 * 256;
        return here;
    };
    const size_t o_status = take(CK_WORDS * 8);
    size_t o_sel[5];
    for (size_t& o : o_sel) o = take(n * 32);
    const size_t o_pos = take(n_pi * 4), o_pvals = take(n_pi * 32), o_table = take(tl * 32);
    size_t o_wit[3] = {}, o_vars = 0, o_idx[3] = {};
    if (!on_device) {
        if (vars) {
            o_vars = take(in.n_vars * 32);
            for (size_t& o : o_idx) o = take(rows * 4);
        } else {
            for (size_t& o : o_wit) o = take(rows * 32);
        }
    }
    size_t o_made[3] = {}, o_sigma = 0;
    if (wiring) {
        for (size_t& o : o_made) o = take(n * 32);
        o_sigma = take(sigma_scratch_bytes(log_n, rows));
    }
    int rc = grow(c, c->check_scratch, at);
    if (rc) return rc;
    char* const base = (char*)c->check_scratch.p;
    unsigned long long* const d_status = (unsigned long long*)(base + o_status);

    unsigned long long h_status[CK_WORDS] = {};
    struct Drain {   // an early return must not leave copies from this frame's host staging in flight
        zkt_ctx* c;
        bool done = false;
        ~Drain() {
            if (!done) (void)hipStreamSynchronize(c->stream);
        }
    } drain{c};
    h_status[CK_FIRST_ARITH] = h_status[CK_FIRST_LOOKUP] = h_status[CK_FIRST_WIRING] = ~0ull;
    ZKT_HIP(c, hipMemcpyAsync(d_status, h_status, sizeof(h_status), hipMemcpyHostToDevice, c->stream));
    if (n_pi) {
        ZKT_HIP(c, hipMemcpyAsync(base + o_pos, pos.data(), n_pi * 4, hipMemcpyHostToDevice, c->stream));
        ZKT_HIP(c, hipMemcpyAsync(base + o_pvals, pvals.data(), n_pi * 32, hipMemcpyHostToDevice, c->stream));
    }
    if (tl) ZKT_HIP(c, hipMemcpyAsync(base + o_table, sorted.data(), tl * 32, hipMemcpyHostToDevice, c->stream));

    CheckArgs q{};
    q.a = in.a_evals; q.b = in.b_evals; q.c = in.c_evals;
    q.variables = in.variables;
    q.w_l = in.w_l; q.w_r = in.w_r; q.w_o = in.w_o;
    if (!on_device) {   // a host witness travels inside the call
        if (vars) {
            if (in.n_vars) ZKT_HIP(c, hipMemcpyAsync(base + o_vars, in.variables, in.n_vars * 32, hipMemcpyHostToDevice, c->stream));
            q.variables = base + o_vars;
            const uint32_t* src[3] = {in.w_l, in.w_r, in.w_o};
            const uint32_t** dst[3] = {&q.w_l, &q.w_r, &q.w_o};
            for (int k = 0; k < 3; ++k) {
                if (rows) ZKT_HIP(c, hipMemcpyAsync(base + o_idx[k], src[k], rows * 4, hipMemcpyHostToDevice, c->stream));
                *dst[k] = (const uint32_t*)(base + o_idx[k]);
            }
        } else {
            const uint64_t* src[3] = {in.a_evals, in.b_evals, in.c_evals};
            const void** dst[3] = {&q.a, &q.b, &q.c};
            for (int k = 0; k < 3; ++k) {
                if (rows) ZKT_HIP(c, hipMemcpyAsync(base + o_wit[k], src[k], rows * 32, hipMemcpyHostToDevice, c->stream));
                *dst[k] = base + o_wit[k];
            }
        }
    }
    q.q_m = base + o_sel[0]; q.q_l = base + o_sel[1]; q.q_r = base + o_sel[2]; q.q_o = base + o_sel[3]; q.q_c = base + o_sel[4];
    q.q_lookup = K.q_lookup_ev;
    q.n = (uint32_t)n; q.n_rows = (uint32_t)rows; q.n_vars = (uint32_t)in.n_vars;
    q.pi_pos = (const uint32_t*)(base + o_pos); q.pi_vals = base + o_pvals; q.n_pi = (uint32_t)n_pi;
    q.table = base + o_table; q.table_len = (uint32_t)tl;
    q.status = d_status;

    {
        ProfScope prof(c, "check_witness");
        void* outs[5];
        for (int k = 0; k < 5; ++k) outs[k] = base + o_sel[k];
        if ((rc = selector_evals_enqueue(c, log_n, K.pk, outs))) return rc;

        if (vars) {
            hipLaunchKernelGGL((k_check_gates<P, true>), dim3(ck_blocks(n)), dim3(CK_THREADS), 0, c->stream, q);
            hipLaunchKernelGGL((k_check_residual<P, true>), dim3(1), dim3(64), 0, c->stream, q);
        } else {
            hipLaunchKernelGGL((k_check_gates<P, false>), dim3(ck_blocks(n)), dim3(CK_THREADS), 0, c->stream, q);
            hipLaunchKernelGGL((k_check_residual<P, false>), dim3(1), dim3(64), 0, c->stream, q);
        }
        ZKT_HIP(c, hipGetLastError());
        if (wiring) {
            void* made[3] = {base + o_made[0], base + o_made[1], base + o_made[2]};
            // an index outside the map raises the same word the gate kernel raises (its low half)
            if ((rc = sigma_enqueue(c, log_n, q.w_l, q.w_r, q.w_o, rows, in.n_vars, made, base + o_sigma,
                                    (uint32_t*)(d_status + CK_BAD_INDEX))))
                return rc;
            hipLaunchKernelGGL(k_check_sigma<P>, dim3(ck_blocks(n)), dim3(CK_THREADS), 0, c->stream, (const F*)made[0], (const F*)made[1],
                               (const F*)made[2], (const F*)K.sigma_ev[0], (const F*)K.sigma_ev[1], (const F*)K.sigma_ev[2], (uint32_t)n,
                               d_status);
            ZKT_HIP(c, hipGetLastError());
        }
    }
    ZKT_HIP(c, hipMemcpyAsync(h_status, d_status, sizeof(h_status), hipMemcpyDeviceToHost, c->stream));
    ZKT_HIP(c, hipStreamSynchronize(c->stream));
    drain.done = true;
    if (h_status[CK_BAD_INDEX])
        return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "wire index outside the variable map: every entry must be < n_vars or ZKT_VARIABLE_ZERO");

    zkt_witness_report r;
    memset(&r, 0, sizeof(r));   // padding too: equal results are equal bytes
    r.checked = 3 | (wiring ? 4 : 0);
    r.n_arithmetic = h_status[CK_N_ARITH];
    r.first_arithmetic = h_status[CK_FIRST_ARITH];
    for (int k = 0; k < 4; ++k) r.residual[k] = h_status[CK_RESIDUAL + k];
    r.n_lookup = h_status[CK_N_LOOKUP];
    r.first_lookup = h_status[CK_FIRST_LOOKUP];
    r.n_wiring = h_status[CK_N_WIRING];
    r.first_wiring_row = ZKT_CHECK_NONE;
    r.first_wiring_column = -1;
    if (h_status[CK_FIRST_WIRING] != ~0ull) {
        r.first_wiring_row = h_status[CK_FIRST_WIRING] / 3;
        r.first_wiring_column = (int)(h_status[CK_FIRST_WIRING] % 3);
    }
    r.satisfied = !r.n_arithmetic && !r.n_lookup && !r.n_wiring;
    memcpy(out, &r, sizeof(r));
    return ZKT_OK;
}

int witness_check(zkt_ctx* c, const WitnessCheckKeys& keys, const zkt_prove_inputs& in, int flags, zkt_witness_report* out) {
    return c->curve == ZKT_CURVE_BN254 ? witness_check_t<Bn254Fr>(c, keys, in, flags, out)
                                       : witness_check_t<Bls381Fr>(c, keys, in, flags, out);
}

// ---- zkt_circuit_check_witness_batch: the same rules over `batch` variable maps under one wiring ----------------------
// (the head comment, "The batch", describes the kernels and the choice of CKB_TILE)
struct CheckBatchArgs {
    const void *q_m, *q_l, *q_r, *q_o, *q_c, *q_lookup;   // n evaluations each
    const void* variables;                                // witness w = variables + w * stride
    unsigned long long stride;
    uint32_t batch;
    const uint32_t *w_l, *w_r, *w_o;
    uint32_t n, n_rows, n_vars;
    const uint32_t* pi_pos;                               // ascending
    const uint32_t* pi_slot;                              // the caller's index of each sorted position
    const void* pi_vals;                                  // batch x n_pi, the caller's order
    uint32_t n_pi;
    const void* tables;                                   // every witness's sorted table, concatenated
    const unsigned long long* tab;                        // per witness: offset into `tables`, length
    unsigned long long* status;                           // CK_WORDS per witness
};

// what a row holds for every witness alike
template <class P>
struct CkbRow {
    Fe<P> q[5];
    bool looks;         // q_lookup != 0; the value itself is read again where a witness needs it: such rows are few
    uint32_t w[3];      // CK_NONE32: the wire is zero (Variable::Zero, a padded row, an index outside the map)
    uint32_t slot;      // its public input's index within a witness's n_pi values, CK_NONE32 when it has none
};

template <class P>
ZKT_D void ckb_row_load(const CheckBatchArgs& q, uint32_t i, CkbRow<P>& r) {
    const Fe<P>* const sel[5] = {(const Fe<P>*)q.q_m, (const Fe<P>*)q.q_l, (const Fe<P>*)q.q_r, (const Fe<P>*)q.q_o, (const Fe<P>*)q.q_c};
#pragma unroll
    for (int k = 0; k < 5; ++k) r.q[k] = fe_load<P>(sel[k] + i);
    r.looks = !fe_is_zero<P>(fe_load<P>((const Fe<P>*)q.q_lookup + i));
    const uint32_t* const idx[3] = {q.w_l, q.w_r, q.w_o};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        uint32_t v = CK_NONE32;
        if (i < q.n_rows) {
            v = idx[k][i];
            if (v != ZKT_VARIABLE_ZERO && v >= q.n_vars) {   // reported as ZKT_ERR_INVALID_ARGUMENT; read as Variable::Zero
                atomicOr(q.status + CK_BAD_INDEX, 1ull);
                v = CK_NONE32;
            }
        }
        r.w[k] = v;
    }
    uint32_t lo = 0, hi = q.n_pi;                   // the first position >= i
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (q.pi_pos[mid] < i) lo = mid + 1;
        else hi = mid;
    }
    r.slot = lo < q.n_pi && q.pi_pos[lo] == i ? q.pi_slot[lo] : CK_NONE32;
}

// the gate equation of row r on witness w and the wire value the lookup reads; canonical
template <class P>
ZKT_D Fe<P> ckb_gate(const CheckBatchArgs& q, const CkbRow<P>& r, uint32_t w, Fe<P>& c) {
    const Fe<P>* const x = (const Fe<P>*)q.variables + (unsigned long long)w * q.stride;
    const Fe<P> a = r.w[0] == CK_NONE32 ? fe_zero<P>() : fe_load<P>(x + r.w[0]);
    const Fe<P> b = r.w[1] == CK_NONE32 ? fe_zero<P>() : fe_load<P>(x + r.w[1]);
    c = r.w[2] == CK_NONE32 ? fe_zero<P>() : fe_load<P>(x + r.w[2]);
    Fe<P> t = fe_add<P>(fe_mul<P>(r.q[0], b), r.q[1]);
    t = fe_mul<P>(t, a);
    t = fe_add<P>(t, fe_mul<P>(r.q[2], b));
    t = fe_add<P>(t, fe_mul<P>(r.q[3], c));
    t = fe_add<P>(t, r.q[4]);
    if (r.slot != CK_NONE32) t = fe_add<P>(t, fe_load<P>((const Fe<P>*)q.pi_vals + (unsigned long long)w * q.n_pi + r.slot));
    return t;
}

template <class P>
__global__ __launch_bounds__(CK_THREADS) void k_check_gates_batch(CheckBatchArgs q) {
    __shared__ uint32_t sh_cnt[CK_THREADS / 64], sh_min[CK_THREADS / 64];
    uint32_t n_arith[CKB_TILE], first_arith[CKB_TILE], n_lookup[CKB_TILE], first_lookup[CKB_TILE];
#pragma unroll
    for (int t = 0; t < CKB_TILE; ++t) {
        n_arith[t] = n_lookup[t] = 0;
        first_arith[t] = first_lookup[t] = CK_NONE32;
    }
    const uint32_t w0 = blockIdx.y * CKB_TILE;      // this workgroup's witnesses: w0 .. w0 + CKB_TILE, below batch
    const uint32_t stride = gridDim.x * CK_THREADS;
#pragma unroll 1
    for (uint32_t i = blockIdx.x * CK_THREADS + threadIdx.x; i < q.n; i += stride) {   // n <= 2^25: no wrap
        CkbRow<P> r;
        ckb_row_load<P>(q, i, r);
#pragma unroll
        for (int t = 0; t < CKB_TILE; ++t) {
            const uint32_t w = w0 + t;
            if (w >= q.batch) continue;
            Fe<P> c;
            if (!fe_is_zero<P>(ckb_gate<P>(q, r, w, c))) {
                ++n_arith[t];
                first_arith[t] = i < first_arith[t] ? i : first_arith[t];
            }
            if (!r.looks) continue;
            const Fe<P> f = fe_mul<P>(fe_load<P>((const Fe<P>*)q.q_lookup + i), c);
            if (fe_is_zero<P>(f)) continue;
            const Fe<P>* const tab = (const Fe<P>*)q.tables + q.tab[2 * w];
            const uint32_t len = (uint32_t)q.tab[2 * w + 1];
            uint32_t lo = 0, hi = len;
            while (lo < hi) {
                const uint32_t mid = lo + (hi - lo) / 2;
                if (ck_cmp<P>(fe_load<P>(tab + mid), f) < 0) lo = mid + 1;
                else hi = mid;
            }
            if (lo >= len || ck_cmp<P>(fe_load<P>(tab + lo), f) != 0) {
                ++n_lookup[t];
                first_lookup[t] = i < first_lookup[t] ? i : first_lookup[t];
            }
        }
    }
#pragma unroll
    for (int t = 0; t < CKB_TILE; ++t) {
        if (w0 + t >= q.batch) break;               // uniform over the workgroup
        unsigned long long* const st = q.status + (size_t)(w0 + t) * CK_WORDS;
        ck_block_reduce(n_arith[t], first_arith[t], st + CK_N_ARITH, st + CK_FIRST_ARITH, sh_cnt, sh_min);
        ck_block_reduce(n_lookup[t], first_lookup[t], st + CK_N_LOOKUP, st + CK_FIRST_LOOKUP, sh_cnt, sh_min);
    }
}

// after k_check_gates_batch on the same stream, a thread per witness: the equation's value at its first failing row
template <class P>
__global__ __launch_bounds__(64) void k_check_residual_batch(CheckBatchArgs q) {
    const uint32_t w = blockIdx.x * 64 + threadIdx.x;
    if (w >= q.batch) return;
    unsigned long long* const st = q.status + (size_t)w * CK_WORDS;
    const unsigned long long first = st[CK_FIRST_ARITH];
    if (first >= q.n) return;                       // none: the residual words stay 0
    CkbRow<P> r;
    ckb_row_load<P>(q, (uint32_t)first, r);
    Fe<P> c;
    const Fe<P> t = ckb_gate<P>(q, r, w, c);
#pragma unroll
    for (int k = 0; k < 4; ++k) st[CK_RESIDUAL + k] = (unsigned long long)t.v[2 * k] | ((unsigned long long)t.v[2 * k + 1] << 32);
}

template <class P>
static int witness_check_batch_t(zkt_ctx* c, const WitnessCheckKeys& K, const zkt_witness_batch& in, int flags, zkt_witness_report* out) {
    using F = Fe<P>;
    const int log_n = K.log_n;
    const size_t n = (size_t)1 << log_n;
    const bool wiring = (flags & ZKT_CHECK_WIRING) != 0;
    const bool on_device = in.wiring_on_device != 0;
    const size_t rows = in.n_rows, n_pi = in.n_pi, batch = in.batch;

    // ---- host side: every table sorted by the kernel's order and laid end to end, the public-input positions by row ----
    std::vector<F> sorted;
    std::vector<unsigned long long> tab(2 * batch, 0);
    for (size_t k = 0; k < in.n_tables; ++k) {
        const size_t tl = in.table_lens[k], at0 = sorted.size();
        const F* t = reinterpret_cast<const F*>(in.tables[k]);
        std::vector<uint32_t> order(tl);
        std::iota(order.begin(), order.end(), 0u);
        std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return ck_cmp<P>(t[x], t[y]) < 0; });
        for (size_t i = 0; i < tl; ++i) sorted.push_back(t[order[i]]);
        for (size_t i = 1; i < tl; ++i)
            if (ck_cmp<P>(sorted[at0 + i - 1], sorted[at0 + i]) == 0)
                return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "lookup table holds a repeated value");
        for (size_t w = in.n_tables == 1 ? 0 : k; w < (in.n_tables == 1 ? batch : k + 1); ++w) {
            tab[2 * w] = at0;
            tab[2 * w + 1] = tl;
        }
    }
    std::vector<uint32_t> pos(n_pi), slot(n_pi);
    if (n_pi) {
        std::iota(slot.begin(), slot.end(), 0u);
        std::stable_sort(slot.begin(), slot.end(), [&](uint32_t x, uint32_t y) { return in.pi_pos[x] < in.pi_pos[y]; });
        for (size_t i = 0; i < n_pi; ++i) pos[i] = (uint32_t)in.pi_pos[slot[i]];
    }

    // ---- the call's scratch, one block carved on 256-byte boundaries ----
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t here = at;
        at += (bytes + 255) / 256 * 256;
        return here;
    };
    const size_t status_bytes = batch * CK_WORDS * 8;
    const size_t o_status = take(status_bytes);
    size_t o_sel[5];
    for (size_t& o : o_sel) o = take(n * 32);
    const size_t o_pos = take(n_pi * 4), o_slot = take(n_pi * 4), o_table = take(sorted.size() * 32), o_tab = take(tab.size() * 8);
    size_t o_idx[3] = {};
    if (!on_device)
        for (size_t& o : o_idx) o = take(rows * 4);
    size_t o_made[3] = {}, o_sigma = 0;
    if (wiring) {
        for (size_t& o : o_made) o = take(n * 32);
        o_sigma = take(sigma_scratch_bytes(log_n, rows));
    }
    int rc = grow(c, c->check_scratch, at);
    if (rc) return rc;
    char* const base = (char*)c->check_scratch.p;
    unsigned long long* const d_status = (unsigned long long*)(base + o_status);

    std::vector<unsigned long long> h_status(batch * CK_WORDS, 0);
    struct Drain {   // an early return must not leave copies from this frame's host staging in flight
        zkt_ctx* c;
        bool done = false;
        ~Drain() {
            if (!done) (void)hipStreamSynchronize(c->stream);
        }
    } drain{c};
    for (size_t w = 0; w < batch; ++w) {
        unsigned long long* const st = h_status.data() + w * CK_WORDS;
        st[CK_FIRST_ARITH] = st[CK_FIRST_LOOKUP] = st[CK_FIRST_WIRING] = ~0ull;
    }
    ZKT_HIP(c, hipMemcpyAsync(d_status, h_status.data(), status_bytes, hipMemcpyHostToDevice, c->stream));
    if (n_pi) {
        ZKT_HIP(c, hipMemcpyAsync(base + o_pos, pos.data(), n_pi * 4, hipMemcpyHostToDevice, c->stream));
        ZKT_HIP(c, hipMemcpyAsync(base + o_slot, slot.data(), n_pi * 4, hipMemcpyHostToDevice, c->stream));
    }
    if (!sorted.empty()) ZKT_HIP(c, hipMemcpyAsync(base + o_table, sorted.data(), sorted.size() * 32, hipMemcpyHostToDevice, c->stream));
    ZKT_HIP(c, hipMemcpyAsync(base + o_tab, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, c->stream));

    CheckBatchArgs q{};
    q.variables = in.d_variables;
    q.stride = in.stride;
    q.batch = (uint32_t)batch;
    q.w_l = in.w_l; q.w_r = in.w_r; q.w_o = in.w_o;
    if (!on_device) {   // a host wiring travels inside the call
        const uint32_t* src[3] = {in.w_l, in.w_r, in.w_o};
        const uint32_t** dst[3] = {&q.w_l, &q.w_r, &q.w_o};
        for (int k = 0; k < 3; ++k) {
            if (rows) ZKT_HIP(c, hipMemcpyAsync(base + o_idx[k], src[k], rows * 4, hipMemcpyHostToDevice, c->stream));
            *dst[k] = (const uint32_t*)(base + o_idx[k]);
        }
    }
    q.q_m = base + o_sel[0]; q.q_l = base + o_sel[1]; q.q_r = base + o_sel[2]; q.q_o = base + o_sel[3]; q.q_c = base + o_sel[4];
    q.q_lookup = K.q_lookup_ev;
    q.n = (uint32_t)n; q.n_rows = (uint32_t)rows; q.n_vars = (uint32_t)in.n_vars;
    q.pi_pos = (const uint32_t*)(base + o_pos); q.pi_slot = (const uint32_t*)(base + o_slot); q.pi_vals = in.d_pi_vals;
    q.n_pi = (uint32_t)n_pi;
    q.tables = base + o_table;
    q.tab = (const unsigned long long*)(base + o_tab);
    q.status = d_status;

    {
        ProfScope prof(c, "check_witness_batch");
        void* outs[5];
        for (int k = 0; k < 5; ++k) outs[k] = base + o_sel[k];
        if ((rc = selector_evals_enqueue(c, log_n, K.pk, outs))) return rc;
        const unsigned tiles = (unsigned)((batch + CKB_TILE - 1) / CKB_TILE);
        hipLaunchKernelGGL(k_check_gates_batch<P>, dim3(ck_blocks(n), tiles), dim3(CK_THREADS), 0, c->stream, q);
        hipLaunchKernelGGL(k_check_residual_batch<P>, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, c->stream, q);
        ZKT_HIP(c, hipGetLastError());
        if (wiring) {   // the shared wiring, once, into witness 0's block
            void* made[3] = {base + o_made[0], base + o_made[1], base + o_made[2]};
            if ((rc = sigma_enqueue(c, log_n, q.w_l, q.w_r, q.w_o, rows, in.n_vars, made, base + o_sigma,
                                    (uint32_t*)(d_status + CK_BAD_INDEX))))
                return rc;
            hipLaunchKernelGGL(k_check_sigma<P>, dim3(ck_blocks(n)), dim3(CK_THREADS), 0, c->stream, (const F*)made[0], (const F*)made[1],
                               (const F*)made[2], (const F*)K.sigma_ev[0], (const F*)K.sigma_ev[1], (const F*)K.sigma_ev[2], (uint32_t)n,
                               d_status);
            ZKT_HIP(c, hipGetLastError());
        }
    }
    ZKT_HIP(c, hipMemcpyAsync(h_status.data(), d_status, status_bytes, hipMemcpyDeviceToHost, c->stream));
    ZKT_HIP(c, hipStreamSynchronize(c->stream));
    drain.done = true;
    if (h_status[CK_BAD_INDEX])
        return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "wire index outside the variable map: every entry must be < n_vars or ZKT_VARIABLE_ZERO");

    for (size_t w = 0; w < batch; ++w) {
        const unsigned long long* const st = h_status.data() + w * CK_WORDS;
        zkt_witness_report r;
        memset(&r, 0, sizeof(r));   // padding too: equal results are equal bytes
        r.checked = 3 | (wiring ? 4 : 0);
        r.n_arithmetic = st[CK_N_ARITH];
        r.first_arithmetic = st[CK_FIRST_ARITH];
        for (int k = 0; k < 4; ++k) r.residual[k] = st[CK_RESIDUAL + k];
        r.n_lookup = st[CK_N_LOOKUP];
        r.first_lookup = st[CK_FIRST_LOOKUP];
        r.n_wiring = h_status[CK_N_WIRING];          // the wiring is the batch's: witness 0's block holds it
        r.first_wiring_row = ZKT_CHECK_NONE;
        r.first_wiring_column = -1;
        if (h_status[CK_FIRST_WIRING] != ~0ull) {
            r.first_wiring_row = h_status[CK_FIRST_WIRING] / 3;
            r.first_wiring_column = (int)(h_status[CK_FIRST_WIRING] % 3);
        }
        r.satisfied = !r.n_arithmetic && !r.n_lookup && !r.n_wiring;
        memcpy(out + w, &r, sizeof(r));
    }
    return ZKT_OK;
}

int witness_check_batch(zkt_ctx* c, const WitnessCheckKeys& keys, const zkt_witness_batch& in, int flags, zkt_witness_report* out) {
    return c->curve == ZKT_CURVE_BN254 ? witness_check_batch_t<Bn254Fr>(c, keys, in, flags, out)
                                       : witness_check_batch_t<Bls381Fr>(c, keys, in, flags, out);
}

}  // namespace zkt
