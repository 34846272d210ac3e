// Lagrange-basis committer key: commitments of polynomials that the prover holds as EVALUATIONS.
//
// The reference commits to every polynomial through its coefficients (plonk-core/src/proof_system/prove.rs:133-135,
// 178-180,249-251: poly_from_evals -> add_blinders_to_poly -> PC::commit = one dense MSM over n + k scalars each).  Four of
// those polynomials are piecewise constant as evaluation vectors: the lookup table t (its values, then zeros:
// lookup/table.rs:52-61), the sorted halves h1 / h2 (runs of equal table values: lookup/multiset.rs:103-146) and the
// lookup grand product z2 (its ratio is 1 wherever f, t, h1, h2 stand still: lookup/mod.rs:94-154).  With
//     [L_i(tau)] G   the key in the Lagrange basis of the circuit's domain (the inverse DFT of the powers [tau^j] G),
//     S_k = sum_{i < k} [L_i(tau)] G   its prefix sums,
// Abel summation turns  commit(p) = sum_i e_i [L_i(tau)] G  into  sum_{k=1..n} (e_{k-1} - e_k) S_k  (e_n := 0): an MSM
// whose scalars are the DIFFERENCES of neighbouring evaluations -- zero inside every run, so its cost follows the number
// of runs (a few thousand), not n.  The same group element, hence the same bytes; a dense evaluation vector simply costs
// what the coefficient form costs.  Blinders b_j X^(n+j) - b_j X^j (prove.rs:472-483) ride along as k extra bases
// V_j = [tau^(n+j)] G - [tau^j] G.
//
// This file builds that second base table once per (key, domain size): the inverse DFT over G1 (radix-2 DIF, one scalar
// multiplication per butterfly: (n/2) log n of them, ~0.5 s at n = 2^20 on BN254), the prefix sums, the blinder points,
// then the window multiples exactly as for the powers (msm_table_finish).  1/n is NOT applied to the points: the scalars
// carry it (poly.hip k_lagrange_scalars).  The table holds R^-1-scaled bases like the first one (msm.hip header), which
// is free here: the transform is linear and starts from table[0].
#include "ctx.hpp"
#include "ec.hpp"
#include "hostec.hpp"
#include "msm.hpp"
#include "poly.hpp"
#include "wire_elim.hpp"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <vector>

namespace zkt {

// A[j] = table[0][j] as an XYZZ point with arkworks-form coordinates (the table keeps canonical R' words)
template <class C>
__global__ void k_lag_init(const Affine<typename C::Fq>* table, Xyzz<typename C::Fq>* A, size_t n) {
    using Q = typename C::Fq;
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    Affine<Q> p = aff_load<Q>(table + j);
    if (!aff_is_inf<Q>(p)) {
        p.x = fx_to_ark<Q>(fx_unpack<Q>(p.x));
        p.y = fx_to_ark<Q>(fx_unpack<Q>(p.y));
    }
    xyzz_store<Q>(A + j, xyzz_from_affine<Q>(p));
}

// tw[j] = w^j as a canonical integer (w = omega^-1 in Montgomery form)
template <class R>
__global__ void k_lag_twiddles(Fe<R>* tw, size_t half, Fe<R> w) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= half) return;
    fe_store<R>(tw + j, fe_from_mont<R>(fe_pow_u64<R>(w, (uint64_t)j)));
}

template <class Q>
ZKT_HD Xyzz<Q> xyzz_neg(const Xyzz<Q>& p) {
    Xyzz<Q> r = p;
    r.y = fe_neg<Q>(p.y);
    return r;
}

// [k] P by the non-adjacent form read off 3k and k (digit i = bit i+1 of 3k minus bit i+1 of k): one doubling per bit, an
// addition every third bit on average, no table.  k canonical, below 2^(32 N - 2).
template <class Q, class R>
ZKT_D Xyzz<Q> xyzz_scalar_mul(const Xyzz<Q>& P, const Fe<R>& k) {
    constexpr int N = R::N;
    uint32_t h[N + 1];
    uint32_t carry = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const uint64_t t = (uint64_t)k.v[i] * 3u + carry;
        h[i] = (uint32_t)t;
        carry = (uint32_t)(t >> 32);
    }
    h[N] = carry;
    const Xyzz<Q> Pn = xyzz_neg<Q>(P);
    Xyzz<Q> acc = xyzz_identity<Q>();
#pragma unroll 1
    for (int li = N; li >= 0; --li) {   // (a word of h and of k per 32 doublings: the indexed reads cost nothing here)
        const uint32_t hw = h[li], kw = li < N ? k.v[li] : 0u;
        if (li == N && hw == 0u) continue;
#pragma unroll 1
        for (int b = (li == N ? 1 : 31); b >= (li == 0 ? 1 : 0); --b) {
            acc = xyzz_double<Q>(acc);
            const uint32_t hb = (hw >> b) & 1u, kb = (kw >> b) & 1u;
            if (hb != kb) acc = xyzz_add<Q>(acc, hb ? P : Pn);
        }
    }
    return acc;
}

// one level of the in-place decimation-in-frequency transform: (u, v) -> (u + v, [w^(j stride)] (u - v))
template <class C>
__global__ __launch_bounds__(128) void k_lag_level(Xyzz<typename C::Fq>* A, size_t n, size_t h, const Fe<typename C::Fr>* tw,
                                                   size_t stride) {
    using Q = typename C::Fq;
    using R = typename C::Fr;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n / 2) return;
    const size_t blk = t / h, j = t % h;
    const size_t i0 = blk * 2 * h + j, i1 = i0 + h;
    const Xyzz<Q> u = xyzz_load<Q>(A + i0), v = xyzz_load<Q>(A + i1);
    xyzz_store<Q>(A + i0, xyzz_add<Q>(u, v));
    Xyzz<Q> d = xyzz_add<Q>(u, xyzz_neg<Q>(v));
    if (j != 0 && !xyzz_is_identity<Q>(d)) d = xyzz_scalar_mul<Q, R>(d, fe_load<R>(tw + j * stride));
    xyzz_store<Q>(A + i1, d);
}

ZKT_D size_t lag_bitrev(size_t i, int bits) {
    return bits ? (size_t)(__brev((uint32_t)i) >> (32 - bits)) : 0;
}

// the transform leaves frequency i at A[bitrev(i)]; seg[s] = sum of the frequencies [s len, (s + 1) len)
template <class C>
__global__ __launch_bounds__(64) void k_lag_seg_sum(const Xyzz<typename C::Fq>* A, int log_n, size_t len, size_t nseg,
                                                    Xyzz<typename C::Fq>* seg) {
    using Q = typename C::Fq;
    const size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nseg) return;
    Xyzz<Q> acc = xyzz_identity<Q>();
#pragma unroll 1
    for (size_t i = s * len; i < (s + 1) * len; ++i) acc = xyzz_add<Q>(acc, xyzz_load<Q>(A + lag_bitrev(i, log_n)));
    xyzz_store<Q>(seg + s, acc);
}

// out[i] = S_(i+1) = pre[s] + the frequencies of segment s up to and including i, affine
template <class C>
__global__ __launch_bounds__(64) void k_lag_prefix(const Xyzz<typename C::Fq>* A, int log_n, size_t len, size_t nseg,
                                                   const Xyzz<typename C::Fq>* pre, Affine<typename C::Fq>* out) {
    using Q = typename C::Fq;
    const size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nseg) return;
    Xyzz<Q> acc = xyzz_load<Q>(pre + s);
#pragma unroll 1
    for (size_t i = s * len; i < (s + 1) * len; ++i) {
        acc = xyzz_add<Q>(acc, xyzz_load<Q>(A + lag_bitrev(i, log_n)));
        aff_store<Q>(out + i, xyzz_to_affine<Q>(acc));
    }
}

// out[n + t] = table[0][n + t] - table[0][t]: the base a blinder at X^(n+t) (minus itself at X^t) multiplies
template <class C>
__global__ void k_lag_blinder_points(const Affine<typename C::Fq>* table, size_t n, size_t extra, Affine<typename C::Fq>* out) {
    using Q = typename C::Fq;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= extra) return;
    Affine<Q> hi = aff_load<Q>(table + n + t), lo = aff_load<Q>(table + t);
    if (!aff_is_inf<Q>(hi)) {
        hi.x = fx_to_ark<Q>(fx_unpack<Q>(hi.x));
        hi.y = fx_to_ark<Q>(fx_unpack<Q>(hi.y));
    }
    Xyzz<Q> acc = xyzz_from_affine<Q>(hi);
    if (!aff_is_inf<Q>(lo)) {
        lo.x = fx_to_ark<Q>(fx_unpack<Q>(lo.x));
        lo.y = fe_neg<Q>(fx_to_ark<Q>(fx_unpack<Q>(lo.y)));
        acc = xyzz_add_mixed<Q>(acc, lo);
    }
    aff_store<Q>(out + n + t, xyzz_to_affine<Q>(acc));
}

constexpr size_t LAG_MAX_SEGMENTS = 4096;   // segment totals the host scans
constexpr size_t LAG_MAX_EXTRA = 8;         // blinder bases kept (the prover uses at most three per polynomial)

template <class C>
static int lagrange_build_t(zkt_ctx* c, int log_n) {
    using Q = typename C::Fq;
    using R = typename C::Fr;
    MsmState& st = *c->msm;
    const size_t n = (size_t)1 << log_n;
    const size_t extra = std::min(st.count - n, LAG_MAX_EXTRA);
    const size_t count2 = n + extra;
    int rc;
    void *A = nullptr, *tw = nullptr, *seg = nullptr, *table2 = nullptr;
    auto mem = std::make_shared<DevShared>(c->device);   // the table goes with it unless the build succeeds
    if ((rc = mem->alloc(c, &table2, (size_t)st.plan.W * count2 * sizeof(Affine<Q>)))) return rc;
    DevSet tmp(c->device);
    if ((rc = tmp.alloc(c, &A, n * sizeof(Xyzz<Q>)))) return rc;
    hipLaunchKernelGGL(k_lag_init<C>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream,
                       (const Affine<Q>*)st.table, (Xyzz<Q>*)A, n);
    if (log_n >= 1) {
        const size_t half = n / 2;
        if ((rc = tmp.alloc(c, &tw, half * sizeof(Fe<R>)))) return rc;
        const Fe<R> winv = fe_inv_host<R>(root_of_unity<R>(log_n));
        hipLaunchKernelGGL(k_lag_twiddles<R>, dim3((unsigned)((half + 255) / 256)), dim3(256), 0, c->stream, (Fe<R>*)tw, half, winv);
        for (size_t h = half; h >= 1; h >>= 1)
            hipLaunchKernelGGL(k_lag_level<C>, dim3((unsigned)((half + 127) / 128)), dim3(128), 0, c->stream, (Xyzz<Q>*)A, n, h,
                               (const Fe<R>*)tw, half / h);
    }
    if (hipGetLastError() != hipSuccess) return set_err(c, ZKT_ERR_HIP, "Lagrange key: launch failed");
    // prefix sums: segment totals on the device, their scan on the host (a few thousand additions), the rest on the device
    const size_t nseg = std::min(n, LAG_MAX_SEGMENTS), len = n / nseg;
    if ((rc = tmp.alloc(c, &seg, 2 * nseg * sizeof(Xyzz<Q>)))) return rc;
    Xyzz<Q>* d_tot = (Xyzz<Q>*)seg;
    Xyzz<Q>* d_pre = d_tot + nseg;
    hipLaunchKernelGGL(k_lag_seg_sum<C>, dim3((unsigned)((nseg + 63) / 64)), dim3(64), 0, c->stream, (const Xyzz<Q>*)A, log_n, len,
                       nseg, d_tot);
    std::vector<Xyzz<Q>> tot(nseg), pre(nseg);
    if (hipMemcpyAsync(tot.data(), d_tot, nseg * sizeof(Xyzz<Q>), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess)
        return set_err(c, ZKT_ERR_HIP, "Lagrange key: the transform failed");
    Xyzz<Q> run = xyzz_identity<Q>();
    for (size_t s = 0; s < nseg; ++s) {
        pre[s] = run;
        run = xyzz_add<Q>(run, tot[s]);
    }
    if (hipMemcpyAsync(d_pre, pre.data(), nseg * sizeof(Xyzz<Q>), hipMemcpyHostToDevice, c->stream) != hipSuccess)
        return set_err(c, ZKT_ERR_HIP, "Lagrange key: upload failed");
    hipLaunchKernelGGL(k_lag_prefix<C>, dim3((unsigned)((nseg + 63) / 64)), dim3(64), 0, c->stream, (const Xyzz<Q>*)A, log_n, len,
                       nseg, (const Xyzz<Q>*)d_pre, (Affine<Q>*)table2);
    if (extra)
        hipLaunchKernelGGL(k_lag_blinder_points<C>, dim3(1), dim3(64), 0, c->stream, (const Affine<Q>*)st.table, n, extra,
                           (Affine<Q>*)table2);
    if (hipGetLastError() != hipSuccess) return set_err(c, ZKT_ERR_HIP, "Lagrange key: launch failed");
    if ((rc = msm_table_finish(c, table2, count2))) return rc;   // synchronises: `pre` may go
    wire_bases_drop(c);   // sums of the table being replaced
    st.lag_mem = mem;
    st.table2 = table2;
    st.count2 = count2;
    st.lag_log_n = log_n;
    return ZKT_OK;
}

// Makes the table for the domain of size 2^log_n available if the key allows it (not sharded, at least n + 1 powers).
// Returns ZKT_OK either way; lagrange_ready tells whether evaluations can be committed directly.
int lagrange_ensure(zkt_ctx* c, int log_n) {
    if (!c->msm) return ZKT_OK;
    MsmState& st = *c->msm;
    if (st.table2 && st.lag_log_n == log_n) return ZKT_OK;
    if (st.lag_failed && st.lag_log_n == log_n) return ZKT_OK;
    const size_t n = (size_t)1 << log_n;
    const bool whole_key = !c->sharded() && st.slice_off == 0 && st.total == st.count;
    if (!whole_key || st.count <= n || log_n > 30 || (uint64_t)st.plan.W * (n + LAG_MAX_EXTRA) >= ((uint64_t)1 << 31)) {
        wire_bases_drop(c);
        static_cast<LagrangeTable&>(st) = LagrangeTable{};
        st.lag_log_n = log_n;
        st.lag_failed = true;
        return ZKT_OK;
    }
    st.lag_failed = false;
    ++c->msm_epoch;
    if (c->curve == ZKT_CURVE_BN254) return lagrange_build_t<Bn254Curve>(c, log_n);
    return lagrange_build_t<Bls381Curve>(c, log_n);
}

bool lagrange_ready(const zkt_ctx* c, int log_n) {
    return c->msm && c->msm->table2 && c->msm->lag_log_n == log_n;
}
size_t lagrange_bases(const zkt_ctx* c) { return c->msm ? c->msm->count2 : 0; }

// ---- wire base tables ------------------------------------------------------------------------------------------
// A wire's evaluation vector is a gather of the variable map (prove.rs:49-55: a[i] = variables[w_l[i]]), so
//     commit(a) = sum_v variables[v] T_v + blinder terms,   T_v = sum_{i : w_l[i] = v} [L_i(tau)] G :
// one scalar per DISTINCT variable of the wire instead of one per row (the withdraw circuit at n = 2^20 has 276 491 on
// the right wire and 843 607 on the left against 1 019 498 rows).  The points T_v depend on the key and the wiring only.
// [L_i(tau)] G is read off the prefix table as S_(i+1) - S_i (window 0 of table2, which keeps 1/n out of the points: the
// scalars carry it), the blinder points V_0, V_1 are table2's own, and msm_table_finish makes the window multiples and
// the R' form exactly as for the other two tables.
//
// Build (once per wiring, inside the first proof that brings it): per wire a count of every variable's rows (device),
// the scan of the counts (host: the distinct variables, ascending, and the start of each one's rows), the rows grouped by
// variable (device), one thread per distinct variable summing its few points in XYZZ and normalising them, the window
// multiples.  A wire is left to the coefficient route when its distinct variables are WIRE_BASES_MAX_FRAC of the rows or
// more (nothing to gain: the output wire), when a T_v is the identity, or when the table cannot be allocated.  An identity
// T_v means a degenerate tau: one in the circuit's domain, under which all [L_i(tau)] G but one are the identity and so
// are nearly all T_v.  The MSM itself would take such a table (k_msm_accumulate skips a base at infinity, as it does for
// a key that holds one); the wire is left alone because the table has nothing to offer then, and because the fold over
// the free variables below (wire_fold_range) reads every T_v as a plain affine point.
//
// Staleness: the tables are keyed on the three vectors' addresses, n_rows, n_vars, the key and the domain -- and a
// caller may overwrite the vectors in place.  So the build stores a 128-bit digest of their contents (two sums of
// position-keyed 64-bit mixes: a change of any entry changes both; it guards against reuse, not against an adversary,
// who could as well hand over a wrong witness), every proof on this route launches the same digest over the vectors it
// was given, and the host compares the two when it collects round 1, before anything is absorbed into the transcript
// (prover.hip).  A wire whose blinded polynomial was trimmed below n coefficients (a constant or empty vector: the
// blinders then sit elsewhere, k_lagrange_scalars) is caught by the same comparison and committed through its coefficients.
constexpr double WIRE_BASES_MAX_FRAC = 0.9;

__global__ void k_wire_count(const uint32_t* idx, size_t rows, uint32_t n_vars, uint32_t* cnt) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    const uint32_t v = idx[i];
    if (v < n_vars) atomicAdd(cnt + v, 1u);   // Variable::Zero (0xFFFFFFFF) and indices outside the map (reported by k_gather_pad)
}
// rows grouped by variable: start[v] = first slot of variable v, cur[v] counts up from zero (the order inside a group is
// whatever the atomics make it: the sum does not depend on it)
__global__ void k_wire_fill(const uint32_t* idx, size_t rows, uint32_t n_vars, const uint32_t* start, uint32_t* cur, uint32_t* grouped) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    const uint32_t v = idx[i];
    if (v < n_vars) grouped[start[v] + atomicAdd(cur + v, 1u)] = (uint32_t)i;
}

// window 0 of a finished table (canonical R' words) -> arkworks-form affine point
template <class Q>
ZKT_D Affine<Q> wire_load_base(const Affine<Q>* p) {
    Affine<Q> a = aff_load<Q>(p);
    if (!aff_is_inf<Q>(a)) {
        a.x = fx_to_ark<Q>(fx_unpack<Q>(a.x));
        a.y = fx_to_ark<Q>(fx_unpack<Q>(a.y));
    }
    return a;
}

// out[j] = sum over the rows i of distinct variable j of S_(i+1) - S_i (pre[i] = S_(i+1)), affine; *bad is set when a sum is the identity
template <class C>
__global__ __launch_bounds__(64) void k_wire_sum(const Affine<typename C::Fq>* pre, const uint32_t* grouped, const uint32_t* ofs,
                                                  size_t cnt, Affine<typename C::Fq>* out, uint32_t* bad) {
    using Q = typename C::Fq;
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= cnt) return;
    Xyzz<Q> acc = xyzz_identity<Q>();
#pragma unroll 1
    for (uint32_t r = ofs[j]; r < ofs[j + 1]; ++r) {
        const uint32_t i = grouped[r];
        const Affine<Q> hi = wire_load_base<Q>(pre + i);
        if (!aff_is_inf<Q>(hi)) acc = xyzz_add_mixed<Q>(acc, hi);
        if (i) {
            Affine<Q> lo = wire_load_base<Q>(pre + i - 1);
            if (!aff_is_inf<Q>(lo)) {
                lo.y = fe_neg<Q>(lo.y);
                acc = xyzz_add_mixed<Q>(acc, lo);
            }
        }
    }
    if (xyzz_is_identity<Q>(acc)) atomicOr(bad, 1u);
    aff_store<Q>(out + j, xyzz_to_affine<Q>(acc));
}
// out[cnt + t] = V_t, the blinder points the prefix table keeps behind its n sums
template <class C>
__global__ void k_wire_blinder_points(const Affine<typename C::Fq>* pre, size_t n, size_t cnt, Affine<typename C::Fq>* out) {
    using Q = typename C::Fq;
    if (threadIdx.x < 2) aff_store<Q>(out + cnt + threadIdx.x, wire_load_base<Q>(pre + n + threadIdx.x));
}

ZKT_HD uint64_t wire_mix(uint64_t x) {   // splitmix64's finaliser
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27; x *= 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}
// out[0], out[1] += two sums over (position, value) of all three vectors
__global__ __launch_bounds__(256) void k_wire_digest(const uint32_t* w0, const uint32_t* w1, const uint32_t* w2, size_t rows,
                                                     unsigned long long* out) {
    __shared__ unsigned long long sh[2][256];
    unsigned long long a = 0, b = 0;
    const size_t total = 3 * rows;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const size_t k = e / rows, i = e - k * rows;
        const uint32_t v = (k == 0 ? w0 : k == 1 ? w1 : w2)[i];
        const uint64_t x = ((uint64_t)e << 32) | v;
        a += wire_mix(x + 0x9e3779b97f4a7c15ull);
        b += wire_mix(~x * 0xd6e8feb86659fd93ull);
    }
    sh[0][threadIdx.x] = a;
    sh[1][threadIdx.x] = b;
    __syncthreads();
    for (unsigned s = 128; s; s >>= 1) {
        if (threadIdx.x < s) {
            sh[0][threadIdx.x] += sh[0][threadIdx.x + s];
            sh[1][threadIdx.x] += sh[1][threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        atomicAdd(out, sh[0][0]);
        atomicAdd(out + 1, sh[1][0]);
    }
}

// s[j] = variables[u[j]] / n for the cnt variables of the table, then 1 / n for the constant point of a table over free
// variables (extra = 1, else 0), then the wire's two blinders (as lagrange_scalars places them)
template <class P>
__global__ void k_wire_scalars(const Fe<P>* vars, const uint32_t* u, size_t cnt, size_t extra, const Fe<P>* bl, Fe<P> ninv, Fe<P>* out) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= cnt + extra + 2) return;
    fe_store<P>(out + j, j < cnt ? fe_mul<P>(fe_load<P>(vars + u[j]), ninv) : j < cnt + extra ? ninv : fe_load<P>(bl + (j - cnt - extra)));
}

void wire_bases_drop(zkt_ctx* c) {
    if (!c->msm) return;
    WireBases& wb = c->msm->wb;
    if (wb.built) (void)hipStreamSynchronize(c->stream);
    wb = WireBases{};
}

static int wire_digest_enqueue(zkt_ctx* c, const uint32_t* const* d_idx, size_t n_rows) {
    MsmState& st = *c->msm;
    if (!st.wb_dig)
        if (int rc = st.work.alloc(c, (void**)&st.wb_dig, 16)) return rc;
    if (!st.wb_pin)
        if (int rc = st.work.pinned(c, (void**)&st.wb_pin, 64)) return rc;
    ZKT_HIP(c, hipMemsetAsync(st.wb_dig, 0, 16, c->stream));
    if (n_rows) {
        const size_t blocks = std::min<size_t>((3 * n_rows + 2047) / 2048, 4096);
        hipLaunchKernelGGL(k_wire_digest, dim3((unsigned)blocks), dim3(256), 0, c->stream, d_idx[0], d_idx[1], d_idx[2], n_rows,
                           (unsigned long long*)st.wb_dig);
        ZKT_HIP(c, hipGetLastError());
    }
    ZKT_HIP(c, hipMemcpyAsync(st.wb_pin, st.wb_dig, 16, hipMemcpyDeviceToHost, c->stream));
    return ZKT_OK;
}

// a wire's rows grouped by variable: the counts come from the device, their scan is the host's
struct WireGroups {
    DevSet mem;   // owns the d_* arrays
    explicit WireGroups(int device) : mem(device) {}
    void *d_cnt = nullptr, *d_start = nullptr, *d_grouped = nullptr, *d_ofs = nullptr, *d_bad = nullptr;
    std::vector<uint32_t> start;   // per variable: the first slot of its rows
    std::vector<uint32_t> u, ofs;  // the distinct variables, ascending, and the first slot of each (d + 1 entries)
    size_t d = 0;
    uint32_t at = 0;               // rows that carry a variable
};
// false: an allocation or a copy failed.  Synchronises the stream.
static bool wire_groups_count(zkt_ctx* c, const uint32_t* d_idx, size_t n_rows, size_t n_vars, WireGroups& g) {
    if (g.mem.alloc(c, &g.d_cnt, (n_vars + 1) * 4)) return false;
    if (hipMemsetAsync(g.d_cnt, 0, (n_vars + 1) * 4, c->stream) != hipSuccess) return false;
    const unsigned rb = (unsigned)((n_rows + 255) / 256);
    if (n_rows) hipLaunchKernelGGL(k_wire_count, dim3(rb), dim3(256), 0, c->stream, d_idx, n_rows, (uint32_t)n_vars, (uint32_t*)g.d_cnt);
    g.start.assign(n_vars + 1, 0);
    if (hipMemcpyAsync(g.start.data(), g.d_cnt, n_vars * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess)
        return false;
    uint32_t at = 0;
    for (size_t v = 0; v < n_vars; ++v) {
        const uint32_t m = g.start[v];
        g.start[v] = at;
        if (m) {
            g.u.push_back((uint32_t)v);
            g.ofs.push_back(at);
            at += m;
        }
    }
    g.ofs.push_back(at);
    g.at = at;
    g.d = g.u.size();
    return true;
}
// out[j] = T of g.u[j], j < g.d, as an affine point in arkworks form.  false: a failure, or a T_v that is the identity (a
// degenerate tau).  Synchronises the stream.
template <class C>
static bool wire_points(zkt_ctx* c, const uint32_t* d_idx, size_t n_rows, size_t n_vars, WireGroups& g, Affine<typename C::Fq>* out) {
    using Q = typename C::Fq;
    MsmState& st = *c->msm;
    const size_t d = g.d;
    if (g.mem.alloc(c, &g.d_start, (n_vars + 1) * 4) || g.mem.alloc(c, &g.d_grouped, ((size_t)g.at + 1) * 4) ||
        g.mem.alloc(c, &g.d_ofs, (d + 1) * 4) || g.mem.alloc(c, &g.d_bad, 4))
        return false;
    if (hipMemcpyAsync(g.d_start, g.start.data(), n_vars * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipMemcpyAsync(g.d_ofs, g.ofs.data(), (d + 1) * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipMemsetAsync(g.d_cnt, 0, (n_vars + 1) * 4, c->stream) != hipSuccess || hipMemsetAsync(g.d_bad, 0, 4, c->stream) != hipSuccess)
        return false;
    const unsigned rb = (unsigned)((n_rows + 255) / 256);
    if (n_rows)
        hipLaunchKernelGGL(k_wire_fill, dim3(rb), dim3(256), 0, c->stream, d_idx, n_rows, (uint32_t)n_vars, (const uint32_t*)g.d_start,
                           (uint32_t*)g.d_cnt, (uint32_t*)g.d_grouped);
    if (d)
        hipLaunchKernelGGL(k_wire_sum<C>, dim3((unsigned)((d + 63) / 64)), dim3(64), 0, c->stream, (const Affine<Q>*)st.table2,
                           (const uint32_t*)g.d_grouped, (const uint32_t*)g.d_ofs, d, out, (uint32_t*)g.d_bad);
    uint32_t bad = 0;
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&bad, g.d_bad, 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess)   // (the staging vectors may go after this)
        return false;
    return bad == 0;
}

template <class C>
static int wire_bases_build_wire(zkt_ctx* c, int log_n, int k, const uint32_t* d_idx, size_t n_rows, size_t n_vars, double frac) {
    using Q = typename C::Fq;
    MsmState& st = *c->msm;
    WireBases& wb = st.wb;
    const size_t n = (size_t)1 << log_n;
    WireGroups g(c->device);
    void *table = nullptr, *d_u = nullptr;
    auto done = [&](bool keep) {   // a wire that cannot have its table is committed through its coefficients: never an error
        if (!keep) { wb.mem->release(table); wb.mem->release(d_u); }
        (void)hipGetLastError();
        return ZKT_OK;
    };
    if (!wire_groups_count(c, d_idx, n_rows, n_vars, g)) return done(false);
    const size_t d = g.d;
    if ((double)d >= frac * (double)n_rows || (uint64_t)st.plan.W * (d + 2) >= ((uint64_t)1 << 31)) return done(false);
    if (wb.mem->alloc(c, &table, (size_t)st.plan.W * (d + 2) * sizeof(Affine<Q>)) || wb.mem->alloc(c, &d_u, (d + 1) * 4)) return done(false);
    if (hipMemcpyAsync(d_u, g.u.data(), d * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess) return done(false);
    if (!wire_points<C>(c, d_idx, n_rows, n_vars, g, (Affine<Q>*)table)) return done(false);
    hipLaunchKernelGGL(k_wire_blinder_points<C>, dim3(1), dim3(64), 0, c->stream, (const Affine<Q>*)st.table2, n, d, (Affine<Q>*)table);
    if (hipGetLastError() != hipSuccess || msm_table_finish(c, table, d + 2)) return done(false);
    wb.table[k] = table;
    wb.u[k] = (uint32_t*)d_u;
    wb.cnt[k] = d;
    wb.use[k] = true;
    return done(true);
}

// ---- wire tables over the circuit's free variables -------------------------------------------------------------
// Most variables of a circuit are not free: a row with q_m = 0 and q_o = +-1 whose output appears there for the first time
// DEFINES it as an affine function of earlier variables (wire_elim.hpp: the host pass, once per wiring, public-input
// positions, circuit and key).  With x_v = kappa_v + sum_f M[v][f] x_f over the free variables f,
//     commit(wire k) = sum_v x_v T^k_v + blinder terms = sum_f x_f A^k_f + C^k + blinder terms,
//     A^k_f = sum_v M[v][f] T^k_v  (f itself with coefficient 1),   C^k = sum_v kappa_v T^k_v :
// one scalar per free variable that reaches the wire, and one for the constant point.  The same group element WHENEVER THE
// WITNESS SATISFIES THE DEFINING ROWS; for any other witness the proof is refused as before, because the quotient is
// still made from the true wire polynomials (status bit 2).
// Build, per wire: T^k_v of every distinct variable (the kernels above; no threshold); the terms of every free variable
// -- and those of the constant point, which is one more group -- cut into pieces of WIRE_FOLD_PIECE, one thread per piece
// multiplying each T^k_v by its full-size coefficient (double-and-add, as k_lag_level) and summing (a variable that
// nearly every row reaches would otherwise be one thread's work); one thread per group adding its pieces; the blinder
// points; msm_table_finish.  The table holds the A^k_f
// of the free variables that reach the wire, then C^k unless it is the identity, then the two blinder points.  A wire
// keeps its present route (its per-variable table, or its coefficients) when a point that has to be a base is the
// identity, when an allocation fails, or when its base count would be WIRE_BASES_MAX_FRAC or more of what it uses now.
constexpr uint32_t WIRE_NONE = 0xFFFFFFFFu;
constexpr uint32_t WIRE_FOLD_PIECE = 32;

// sum over the entries [lo, hi) of coefficient x T of the entry's variable; variables that are not on this wire are skipped
template <class C>
ZKT_D Xyzz<typename C::Fq> wire_fold_range(const Affine<typename C::Fq>* T, const uint32_t* pos, const uint32_t* ent_v,
                                           const Fe<typename C::Fr>* ent_c, uint32_t lo, uint32_t hi) {
    using Q = typename C::Fq;
    using R = typename C::Fr;
    const Fe<R> one = fe_one<R>();
    Xyzz<Q> acc = xyzz_identity<Q>();
#pragma unroll 1
    for (uint32_t e = lo; e < hi; ++e) {
        const uint32_t j = pos[ent_v[e]];
        if (j == WIRE_NONE) continue;
        const Affine<Q> p = aff_load<Q>(T + j);   // never the identity: k_wire_sum reports one and the wire is left alone
        const Fe<R> cm = fe_load<R>(ent_c + e);
        if (fe_eq<R>(cm, one)) acc = xyzz_add_mixed<Q>(acc, p);
        else acc = xyzz_add<Q>(acc, xyzz_scalar_mul<Q, R>(xyzz_from_affine<Q>(p), fe_from_mont<R>(cm)));
    }
    return acc;
}
// part[t] = the sum over piece t = the entries [piece[t].x, piece[t].y)
template <class C>
__global__ __launch_bounds__(64) void k_wire_fold(const Affine<typename C::Fq>* T, const uint32_t* pos, const uint32_t* ent_v,
                                                   const Fe<typename C::Fr>* ent_c, const uint2* piece, size_t np,
                                                   Xyzz<typename C::Fq>* part) {
    using Q = typename C::Fq;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= np) return;
    const uint2 pc = piece[t];
    xyzz_store<Q>(part + t, wire_fold_range<C>(T, pos, ent_v, ent_c, pc.x, pc.y));
}
// out[j] = the sum of the pieces [pstart[j], pstart[j + 1]) of group j, affine.  The first cnt groups are free variables:
// flags[0] is set when one of their points is the identity.  A group behind them is the constant point: flags[1] is set
// when it is NOT the identity.
template <class C>
__global__ __launch_bounds__(64) void k_wire_fold_sum(const Xyzz<typename C::Fq>* part, const uint32_t* pstart, size_t cnt, size_t groups,
                                                       Affine<typename C::Fq>* out, uint32_t* flags) {
    using Q = typename C::Fq;
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= groups) return;
    Xyzz<Q> acc = xyzz_identity<Q>();
#pragma unroll 1
    for (uint32_t t = pstart[j]; t < pstart[j + 1]; ++t) acc = xyzz_add<Q>(acc, xyzz_load<Q>(part + t));
    const bool none = xyzz_is_identity<Q>(acc);
    if (j < cnt ? none : !none) atomicOr(flags + (j < cnt ? 0 : 1), 1u);
    aff_store<Q>(out + j, xyzz_to_affine<Q>(acc));
}

// what the host pass leaves for the three wires: the forms grouped by free variable (group g = free variable free_vars[g]:
// itself with coefficient 1, then every defined variable that holds it), then one group of the constants (kappa_v per
// defined variable that has one); ofs has free_vars.size() + 2 entries
struct WireElimShared {
    std::vector<uint32_t> free_vars, ofs, ent_v;
    size_t n_defined = 0, n_const = 0;
    DevSet mem;   // owns the two arrays below
    void *d_ent_v = nullptr, *d_ent_c = nullptr;
    explicit WireElimShared(int device) : mem(device) {}
};

// The host pass: selector evaluations and index vectors to the host, the elimination, the transposed forms to the device.
// false: it could not be done (memory); the wires then keep their present routes.
template <class C>
static bool wire_elim_host(zkt_ctx* c, int log_n, const uint32_t* const* d_idx, size_t n_rows, size_t n_vars, const WireElimKeys& ew,
                           WireElimShared& D) {
    using R = typename C::Fr;
    using F = Fe<R>;
    const size_t n = (size_t)1 << log_n;
    DevSet tmp(c->device);
    void* d_sel[5] = {};
    std::vector<F> sel_h[5];
    std::vector<uint32_t> w_h[3];
    bool ok = true;
    for (int k = 0; k < 5 && ok; ++k) ok = tmp.alloc(c, &d_sel[k], n * sizeof(F)) == ZKT_OK;
    if (ok) ok = selector_evals_enqueue(c, log_n, ew.pk, d_sel) == ZKT_OK;
    for (int k = 0; k < 5 && ok; ++k) {
        sel_h[k].resize(n_rows);
        ok = hipMemcpyAsync(sel_h[k].data(), d_sel[k], n_rows * sizeof(F), hipMemcpyDeviceToHost, c->stream) == hipSuccess;
    }
    for (int k = 0; k < 3 && ok; ++k) {
        w_h[k].resize(n_rows);
        ok = hipMemcpyAsync(w_h[k].data(), d_idx[k], n_rows * 4, hipMemcpyDeviceToHost, c->stream) == hipSuccess;
    }
    if (hipStreamSynchronize(c->stream) != hipSuccess) ok = false;
    tmp.clear();   // the selectors are on the host: the elimination below needs the memory more
    if (!ok) {
        (void)hipGetLastError();
        return false;
    }
    WireElim<R> E;
    {
        const F* sp[5] = {sel_h[0].data(), sel_h[1].data(), sel_h[2].data(), sel_h[3].data(), sel_h[4].data()};
        const uint32_t* wp[3] = {w_h[0].data(), w_h[1].data(), w_h[2].data()};
        wire_eliminate<R>(sp, wp, n_rows, n_vars, ew.pi_pos, ew.n_pi, WIRE_ELIM_K, E);
    }
    const size_t nf = E.free_vars.size(), nd = E.def_vars.size();
    if (!nf || !nd) return false;   // nothing is defined: the per-variable tables are the best there is
    size_t nk = 0;
    for (const F& k : E.kappa) nk += !fe_is_zero<R>(k);
    const uint64_t total = (uint64_t)nf + E.term_f.size() + nk;
    if (total >= 0xFFFFFFFFull) return false;
    std::vector<uint32_t> fid(n_vars, 0), cur(nf + 1, 0);
    for (size_t g = 0; g < nf; ++g) fid[E.free_vars[g]] = (uint32_t)g;
    D.ofs.assign(nf + 2, 0);
    for (size_t g = 0; g < nf; ++g) D.ofs[g + 1] = 1;
    for (uint32_t f : E.term_f) ++D.ofs[fid[f] + 1];
    D.ofs[nf + 1] = (uint32_t)nk;
    for (size_t g = 0; g <= nf; ++g) D.ofs[g + 1] += D.ofs[g];
    D.ent_v.resize(total);
    std::vector<F> ent_c(total);
    const F one = fe_one<R>();
    for (size_t g = 0; g < nf; ++g) {
        cur[g] = D.ofs[g];
        D.ent_v[cur[g]] = E.free_vars[g];
        ent_c[cur[g]++] = one;
    }
    cur[nf] = D.ofs[nf];
    for (size_t d = 0; d < nd; ++d) {
        for (uint64_t t = E.def_start[d]; t < E.def_start[d + 1]; ++t) {
            const uint32_t g = fid[E.term_f[t]];
            D.ent_v[cur[g]] = E.def_vars[d];
            ent_c[cur[g]++] = E.term_c[t];
        }
        if (!fe_is_zero<R>(E.kappa[d])) {
            D.ent_v[cur[nf]] = E.def_vars[d];
            ent_c[cur[nf]++] = E.kappa[d];
        }
    }
    D.free_vars.swap(E.free_vars);
    D.n_defined = nd;
    D.n_const = nk;
    ok = !D.mem.alloc(c, &D.d_ent_v, total * 4) && !D.mem.alloc(c, &D.d_ent_c, total * sizeof(F));
    ok = ok && hipMemcpyAsync(D.d_ent_v, D.ent_v.data(), total * 4, hipMemcpyHostToDevice, c->stream) == hipSuccess &&
         hipMemcpyAsync(D.d_ent_c, ent_c.data(), total * sizeof(F), hipMemcpyHostToDevice, c->stream) == hipSuccess;
    if (hipStreamSynchronize(c->stream) != hipSuccess) ok = false;   // the staging vectors go with this frame
    if (!ok) (void)hipGetLastError();
    return ok;
}

// true: wire k got its table over free variables; false: it keeps its present route (nothing of it is left behind)
template <class C>
static bool wire_elim_build_wire(zkt_ctx* c, int log_n, int k, const uint32_t* d_idx, size_t n_rows, size_t n_vars, double frac,
                                 const WireElimShared& D, size_t* nonzeros) {
    using Q = typename C::Fq;
    using R = typename C::Fr;
    MsmState& st = *c->msm;
    WireBases& wb = st.wb;
    const size_t n = (size_t)1 << log_n;
    WireGroups g(c->device);
    DevSet tmp(c->device);
    void *d_T = nullptr, *d_pos = nullptr, *d_piece = nullptr, *d_pstart = nullptr, *d_part = nullptr, *d_flag = nullptr, *table = nullptr,
         *d_u = nullptr;
    auto done = [&](bool keep) {
        if (!keep) { wb.mem->release(table); wb.mem->release(d_u); }
        (void)hipGetLastError();
        return keep;
    };
    *nonzeros = 0;
    if (!wire_groups_count(c, d_idx, n_rows, n_vars, g)) return done(false);
    const size_t d = g.d;
    if (!d) return done(false);
    const size_t present = (double)d < frac * (double)n_rows ? d : n_rows;   // bases of its present route
    std::vector<uint32_t> pos(n_vars, WIRE_NONE), u, pstart(1, 0);
    std::vector<uint2> piece;
    for (size_t j = 0; j < d; ++j) pos[g.u[j]] = (uint32_t)j;
    const size_t nf = D.free_vars.size();
    auto cut = [&](size_t grp) {   // the pieces of a group
        for (uint32_t lo = D.ofs[grp]; lo < D.ofs[grp + 1]; lo += WIRE_FOLD_PIECE)
            piece.push_back(make_uint2(lo, std::min(lo + WIRE_FOLD_PIECE, D.ofs[grp + 1])));
        pstart.push_back((uint32_t)piece.size());
    };
    for (size_t f = 0; f < nf; ++f) {
        size_t here = 0;
        for (uint32_t e = D.ofs[f]; e < D.ofs[f + 1]; ++e) here += pos[D.ent_v[e]] != WIRE_NONE;
        if (here) {
            u.push_back(D.free_vars[f]);
            cut(f);
            *nonzeros += here;
        }
    }
    const size_t cnt = u.size();
    // the constant point counts as a base here whether or not it turns out to be the identity
    if (!cnt || (double)(cnt + 1) >= frac * (double)present || (uint64_t)st.plan.W * (cnt + 3) >= ((uint64_t)1 << 31)) return done(false);
    if (D.n_const) cut(nf);
    const size_t groups = pstart.size() - 1, np = piece.size();
    if (tmp.alloc(c, &d_T, d * sizeof(Affine<Q>)) || tmp.alloc(c, &d_pos, n_vars * 4) || tmp.alloc(c, &d_piece, np * sizeof(uint2)) ||
        tmp.alloc(c, &d_pstart, (groups + 1) * 4) || wb.mem->alloc(c, &d_u, (cnt + 1) * 4) || tmp.alloc(c, &d_part, np * sizeof(Xyzz<Q>)) ||
        tmp.alloc(c, &d_flag, 8) || wb.mem->alloc(c, &table, (size_t)st.plan.W * (cnt + 3) * sizeof(Affine<Q>)))
        return done(false);
    if (hipMemcpyAsync(d_pos, pos.data(), n_vars * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipMemcpyAsync(d_piece, piece.data(), np * sizeof(uint2), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipMemcpyAsync(d_pstart, pstart.data(), (groups + 1) * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipMemcpyAsync(d_u, u.data(), cnt * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipMemsetAsync(d_flag, 0, 8, c->stream) != hipSuccess)
        return done(false);
    if (!wire_points<C>(c, d_idx, n_rows, n_vars, g, (Affine<Q>*)d_T)) return done(false);   // synchronises: the staging vectors may go
    hipLaunchKernelGGL(k_wire_fold<C>, dim3((unsigned)((np + 63) / 64)), dim3(64), 0, c->stream, (const Affine<Q>*)d_T,
                       (const uint32_t*)d_pos, (const uint32_t*)D.d_ent_v, (const Fe<R>*)D.d_ent_c, (const uint2*)d_piece, np,
                       (Xyzz<Q>*)d_part);
    hipLaunchKernelGGL(k_wire_fold_sum<C>, dim3((unsigned)((groups + 63) / 64)), dim3(64), 0, c->stream, (const Xyzz<Q>*)d_part,
                       (const uint32_t*)d_pstart, cnt, groups, (Affine<Q>*)table, (uint32_t*)d_flag);
    uint32_t flags[2] = {0, 0};
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(flags, d_flag, 8, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess)
        return done(false);
    if (flags[0]) return done(false);   // an A_f that is the identity
    const size_t has_c = flags[1] ? 1 : 0;
    hipLaunchKernelGGL(k_wire_blinder_points<C>, dim3(1), dim3(64), 0, c->stream, (const Affine<Q>*)st.table2, n, cnt + has_c,
                       (Affine<Q>*)table);
    if (hipGetLastError() != hipSuccess || msm_table_finish(c, table, cnt + has_c + 2)) return done(false);
    wb.table[k] = table;
    wb.u[k] = (uint32_t*)d_u;
    wb.cnt[k] = cnt;
    wb.use[k] = true;
    wb.elim[k] = true;
    wb.has_c[k] = has_c != 0;
    return done(true);
}

template <class C>
static int wire_bases_build_all(zkt_ctx* c, int log_n, const uint32_t* const* d_idx, size_t n_rows, size_t n_vars, double frac,
                                const WireElimKeys* ew, bool trace) {
    using clk = std::chrono::steady_clock;
    auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    WireElimShared D(c->device);
    bool elim = false;
    const auto t0 = clk::now();
    if (ew) elim = wire_elim_host<C>(c, log_n, d_idx, n_rows, n_vars, *ew, D);
    const auto t1 = clk::now();
    size_t nz[3] = {};
    int rc = ZKT_OK;
    for (int k = 0; k < 3 && !rc; ++k)
        if (!elim || !wire_elim_build_wire<C>(c, log_n, k, d_idx[k], n_rows, n_vars, frac, D, &nz[k]))
            rc = wire_bases_build_wire<C>(c, log_n, k, d_idx[k], n_rows, n_vars, frac);
    if (trace && ew) {
        const WireBases& wb = c->msm->wb;
        fprintf(stderr, "[zkt host] wire elimination%s: %zu free, %zu defined (%zu with a constant); non-zeros per wire %zu / %zu / %zu; "
                "routes %d / %d / %d (2 = free variables); host pass %.1f ms, device build %.1f ms\n", elim ? "" : " (not possible)",
                D.free_vars.size(), D.n_defined, D.n_const, nz[0], nz[1], nz[2], wb.use[0] + wb.elim[0], wb.use[1] + wb.elim[1],
                wb.use[2] + wb.elim[2], ms(t0, t1), ms(t1, clk::now()));
    }
    return rc;
}

int wire_bases_prepare(zkt_ctx* c, int log_n, const uint32_t* const* d_idx, size_t n_rows, size_t n_vars, const WireElimKeys* ew) {
    if (!c->msm) return ZKT_OK;
    MsmState& st = *c->msm;
    WireBases& wb = st.wb;
    const size_t n = (size_t)1 << log_n;
    const bool possible = lagrange_ready(c, log_n) && !c->sharded() && !c->lagrange_off && st.count2 >= n + 2 && n_rows <= n &&
                          n_vars <= 0xFFFFFFFEull && !(exp_env("ZKT_WIRE_BASES") && atoi(exp_env("ZKT_WIRE_BASES")) == 0);
    if (ew && exp_env("ZKT_WIRE_ELIM") && atoi(exp_env("ZKT_WIRE_ELIM")) == 0) ew = nullptr;   // experiment: same-build A/B
    // tables over free variables also depend on where the proof's public inputs stand
    std::vector<size_t> pi;
    if (ew) {
        pi.assign(ew->pi_pos, ew->pi_pos + ew->n_pi);
        std::sort(pi.begin(), pi.end());
    }
    const bool same = wb.built && !wb.stale && wb.w[0] == d_idx[0] && wb.w[1] == d_idx[1] && wb.w[2] == d_idx[2] &&
                      wb.n_rows == n_rows && wb.n_vars == n_vars && wb.log_n == log_n && wb.srs_generation == c->srs_generation &&
                      wb.elim_wanted == (ew != nullptr) && wb.pi_pos == pi;
    if (possible && same) return ZKT_OK;
    // tables that contexts forked from this one read stay where they are: this context then commits densely until they are gone
    if (wb.built && dev_shared_has_readers(wb.mem)) {
        if (!same || !possible) wb.stale = true;
        return ZKT_OK;
    }
    wire_bases_drop(c);
    if (!possible) return ZKT_OK;
    wb.mem = std::make_shared<DevShared>(c->device);
    double frac = WIRE_BASES_MAX_FRAC;
    if (const char* e = exp_env("ZKT_WIRE_BASES_FRAC")) frac = atof(e);   // experiment: the threshold's A/B
    hipEvent_t e0 = nullptr, e1 = nullptr;
    const bool trace = exp_env("ZKT_HOST_TRACE") != nullptr;
    if (trace) {
        (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
        (void)hipEventRecord(e0, c->stream);
    }
    if (int rc = c->curve == ZKT_CURVE_BN254 ? wire_bases_build_all<Bn254Curve>(c, log_n, d_idx, n_rows, n_vars, frac, ew, trace)
                                             : wire_bases_build_all<Bls381Curve>(c, log_n, d_idx, n_rows, n_vars, frac, ew, trace))
        return rc;
    if (int rc = wire_digest_enqueue(c, d_idx, n_rows)) return rc;
    ZKT_HIP(c, hipStreamSynchronize(c->stream));
    if (trace) {
        float ms = 0;
        (void)hipEventRecord(e1, c->stream); (void)hipEventSynchronize(e1); (void)hipEventElapsedTime(&ms, e0, e1);
        fprintf(stderr, "[zkt host] wire base tables: %zu / %zu / %zu bases of %zu rows (0 = dense), %.1f ms\n",
                wb.use[0] ? wb.cnt[0] : 0, wb.use[1] ? wb.cnt[1] : 0, wb.use[2] ? wb.cnt[2] : 0, n_rows, ms);
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    }
    wb.digest[0] = st.wb_pin[0];
    wb.digest[1] = st.wb_pin[1];
    for (int k = 0; k < 3; ++k) wb.w[k] = d_idx[k];
    wb.n_rows = n_rows; wb.n_vars = n_vars; wb.log_n = log_n; wb.srs_generation = c->srs_generation;
    wb.elim_wanted = ew != nullptr;
    wb.pi_pos.swap(pi);
    wb.built = true;
    ++c->msm_epoch;
    return ZKT_OK;
}

bool wire_bases_use(const zkt_ctx* c, int k) {
    return c->msm && c->msm->wb.built && !c->msm->wb.stale && c->msm->wb.use[k];
}
int wire_bases_route(const zkt_ctx* c, int k) { return !wire_bases_use(c, k) ? 0 : c->msm->wb.elim[k] ? 2 : 1; }
int wire_bases_digest(zkt_ctx* c, const uint32_t* const* d_idx, size_t n_rows) { return wire_digest_enqueue(c, d_idx, n_rows); }
int wire_bases_lens(zkt_ctx* c, const uint32_t* d_lens) {
    ZKT_HIP(c, hipMemcpyAsync(c->msm->wb_pin + 2, d_lens, 12, hipMemcpyDeviceToHost, c->stream));
    return ZKT_OK;
}

template <class C>
static int wire_scalars_t(zkt_ctx* c, int k, const void* d_vars, const void* d_bl, size_t n, const void** out, size_t* len) {
    using R = typename C::Fr;
    MsmState& st = *c->msm;
    const size_t cnt = st.wb.cnt[k], extra = st.wb.has_c[k] ? 1 : 0;
    if (int rc = grow(c, st.wb_scalars[k], (cnt + extra + 2) * sizeof(Fe<R>), &st.work)) return rc;
    Fe<R> nn = fe_zero<R>();
    nn.v[0] = (uint32_t)(n & 0xffffffffu);
    nn.v[1] = (uint32_t)((uint64_t)n >> 32);
    const Fe<R> ninv = fe_inv_host<R>(fe_to_mont<R>(nn));
    hipLaunchKernelGGL(k_wire_scalars<R>, dim3((unsigned)((cnt + extra + 2 + 255) / 256)), dim3(256), 0, c->stream, (const Fe<R>*)d_vars,
                       (const uint32_t*)st.wb.u[k], cnt, extra, (const Fe<R>*)d_bl, ninv, (Fe<R>*)st.wb_scalars[k].p);
    ZKT_HIP(c, hipGetLastError());
    *out = st.wb_scalars[k].p;
    *len = cnt + extra + 2;
    return ZKT_OK;
}
int wire_bases_scalars(zkt_ctx* c, int k, const void* d_vars, const void* d_blinders, size_t n, const void** out, size_t* len) {
    if (c->curve == ZKT_CURVE_BN254) return wire_scalars_t<Bn254Curve>(c, k, d_vars, d_blinders, n, out, len);
    return wire_scalars_t<Bls381Curve>(c, k, d_vars, d_blinders, n, out, len);
}

// after the stream has passed the digest and the length copy of the proof being collected
bool wire_bases_check(zkt_ctx* c, int k, size_t n) {
    MsmState& st = *c->msm;
    if (st.wb_pin[0] != st.wb.digest[0] || st.wb_pin[1] != st.wb.digest[1]) {
        st.wb.stale = true;
        return false;
    }
    return ((const uint32_t*)(st.wb_pin + 2))[k] == (uint32_t)n;
}

// zkt_debug_wire_elimination: the host pass alone, on caller-supplied selectors and wiring (no device, no context)
template <class R>
static int debug_wire_elimination_t(const uint64_t* const* selectors, const uint32_t* const* w, size_t n_rows, size_t n_vars,
                                    const size_t* pi_pos, size_t n_pi, int K, uint8_t* out_kind, uint32_t* out_free, size_t* out_n_free,
                                    uint32_t* out_term_v, uint32_t* out_term_f, uint64_t* out_term_coef, size_t* out_n_terms,
                                    uint64_t* out_kappa) {
    using F = Fe<R>;
    static_assert(sizeof(F) == 32, "scalar field element = 4 x 64-bit words");
    const F* sel[5];
    for (int k = 0; k < 5; ++k) sel[k] = reinterpret_cast<const F*>(selectors[k]);
    WireElim<R> E;
    wire_eliminate<R>(sel, w, n_rows, n_vars, pi_pos, n_pi, K, E);
    if (n_vars) memcpy(out_kind, E.kind.data(), n_vars);
    if (!E.free_vars.empty()) memcpy(out_free, E.free_vars.data(), E.free_vars.size() * 4);
    *out_n_free = E.free_vars.size();
    memset(out_kappa, 0, n_vars * 32);
    size_t t = 0;
    for (size_t d = 0; d < E.def_vars.size(); ++d) {
        memcpy(out_kappa + 4 * (size_t)E.def_vars[d], E.kappa[d].v, 32);
        for (uint64_t e = E.def_start[d]; e < E.def_start[d + 1]; ++e, ++t) {
            out_term_v[t] = E.def_vars[d];
            out_term_f[t] = E.term_f[e];
            memcpy(out_term_coef + 4 * t, E.term_c[e].v, 32);
        }
    }
    *out_n_terms = t;
    return ZKT_OK;
}

}  // namespace zkt

using namespace zkt;

int zkt_debug_wire_elimination(int curve, const uint64_t* const* selectors, const uint32_t* w_l, const uint32_t* w_r, const uint32_t* w_o,
                               size_t n_rows, size_t n_vars, const size_t* pi_pos, size_t n_pi, int K, uint8_t* out_kind,
                               uint32_t* out_free, size_t* out_n_free, uint32_t* out_term_v, uint32_t* out_term_f,
                               uint64_t* out_term_coef, size_t* out_n_terms, uint64_t* out_kappa) {
    if (!selectors || !out_kind || !out_free || !out_n_free || !out_term_v || !out_term_f || !out_term_coef || !out_n_terms || !out_kappa ||
        (n_pi && !pi_pos) || (n_rows && (!w_l || !w_r || !w_o)))
        return ZKT_ERR_INVALID_ARGUMENT;
    for (int k = 0; k < 5; ++k)
        if (n_rows && !selectors[k]) return ZKT_ERR_INVALID_ARGUMENT;
    if (K < 1 || K > WIRE_ELIM_K_MAX || n_vars > 0xFFFFFFFEull) return ZKT_ERR_INVALID_ARGUMENT;
    const uint32_t* w[3] = {w_l, w_r, w_o};
    if (curve == ZKT_CURVE_BN254)
        return debug_wire_elimination_t<Bn254Fr>(selectors, w, n_rows, n_vars, pi_pos, n_pi, K, out_kind, out_free, out_n_free, out_term_v,
                                                 out_term_f, out_term_coef, out_n_terms, out_kappa);
    if (curve == ZKT_CURVE_BLS12_381)
        return debug_wire_elimination_t<Bls381Fr>(selectors, w, n_rows, n_vars, pi_pos, n_pi, K, out_kind, out_free, out_n_free, out_term_v,
                                                  out_term_f, out_term_coef, out_n_terms, out_kappa);
    return ZKT_ERR_INVALID_ARGUMENT;
}
