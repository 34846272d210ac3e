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

#include <algorithm>
#include <cstdio>
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
    if ((rc = dev_alloc(c, &table2, (size_t)st.plan.W * count2 * sizeof(Affine<Q>)))) return rc;
    auto release = [&](int code) {
        dev_free(c, A);
        dev_free(c, tw);
        dev_free(c, seg);
        if (code) dev_free(c, table2);
        return code;
    };
    if ((rc = dev_alloc(c, &A, n * sizeof(Xyzz<Q>)))) return release(rc);
    hipLaunchKernelGGL(k_lag_init<C>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream,
                       (const Affine<Q>*)st.table, (Xyzz<Q>*)A, n);
    if (log_n >= 1) {
        const size_t half = n / 2;
        if ((rc = dev_alloc(c, &tw, half * sizeof(Fe<R>)))) return release(rc);
        const Fe<R> winv = fe_inv_host<R>(root_of_unity<R>(log_n));
        hipLaunchKernelGGL(k_lag_twiddles<R>, dim3((unsigned)((half + 255) / 256)), dim3(256), 0, c->stream, (Fe<R>*)tw, half, winv);
        for (size_t h = half; h >= 1; h >>= 1)
            hipLaunchKernelGGL(k_lag_level<C>, dim3((unsigned)((half + 127) / 128)), dim3(128), 0, c->stream, (Xyzz<Q>*)A, n, h,
                               (const Fe<R>*)tw, half / h);
    }
    if (hipGetLastError() != hipSuccess) return release(set_err(c, ZKT_ERR_HIP, "Lagrange key: launch failed"));
    // prefix sums: segment totals on the device, their scan on the host (a few thousand additions), the rest on the device
    const size_t nseg = std::min(n, LAG_MAX_SEGMENTS), len = n / nseg;
    if ((rc = dev_alloc(c, &seg, 2 * nseg * sizeof(Xyzz<Q>)))) return release(rc);
    Xyzz<Q>* d_tot = (Xyzz<Q>*)seg;
    Xyzz<Q>* d_pre = d_tot + nseg;
    hipLaunchKernelGGL(k_lag_seg_sum<C>, dim3((unsigned)((nseg + 63) / 64)), dim3(64), 0, c->stream, (const Xyzz<Q>*)A, log_n, len,
                       nseg, d_tot);
    std::vector<Xyzz<Q>> tot(nseg), pre(nseg);
    if (hipMemcpyAsync(tot.data(), d_tot, nseg * sizeof(Xyzz<Q>), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess)
        return release(set_err(c, ZKT_ERR_HIP, "Lagrange key: the transform failed"));
    Xyzz<Q> run = xyzz_identity<Q>();
    for (size_t s = 0; s < nseg; ++s) {
        pre[s] = run;
        run = xyzz_add<Q>(run, tot[s]);
    }
    if (hipMemcpyAsync(d_pre, pre.data(), nseg * sizeof(Xyzz<Q>), hipMemcpyHostToDevice, c->stream) != hipSuccess)
        return release(set_err(c, ZKT_ERR_HIP, "Lagrange key: upload failed"));
    hipLaunchKernelGGL(k_lag_prefix<C>, dim3((unsigned)((nseg + 63) / 64)), dim3(64), 0, c->stream, (const Xyzz<Q>*)A, log_n, len,
                       nseg, (const Xyzz<Q>*)d_pre, (Affine<Q>*)table2);
    if (extra)
        hipLaunchKernelGGL(k_lag_blinder_points<C>, dim3(1), dim3(64), 0, c->stream, (const Affine<Q>*)st.table, n, extra,
                           (Affine<Q>*)table2);
    if (hipGetLastError() != hipSuccess) return release(set_err(c, ZKT_ERR_HIP, "Lagrange key: launch failed"));
    if ((rc = msm_table_finish(c, table2, count2))) return release(rc);   // synchronises: `pre` may go
    wire_bases_drop(c);   // sums of the table being replaced
    if (!st.table2_borrowed) dev_free(c, st.table2);
    st.table2_borrowed = false;
    st.table2 = table2;
    st.count2 = count2;
    st.lag_log_n = log_n;
    return release(ZKT_OK);
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
        if (!st.table2_borrowed) dev_free(c, st.table2);
        st.table2_borrowed = false;
        st.table2 = nullptr;
        st.count2 = 0;
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
// more (nothing to gain: the output wire), when a T_v is the identity (a degenerate tau: the MSM's tables hold no such
// base), or when the table cannot be allocated.
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

// s[j] = variables[u[j]] / n for the distinct variables, then the wire's two blinders (as lagrange_scalars places them)
template <class P>
__global__ void k_wire_scalars(const Fe<P>* vars, const uint32_t* u, size_t cnt, const Fe<P>* bl, Fe<P> ninv, Fe<P>* out) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= cnt + 2) return;
    fe_store<P>(out + j, j < cnt ? fe_mul<P>(fe_load<P>(vars + u[j]), ninv) : fe_load<P>(bl + (j - cnt)));
}

void wire_bases_drop(zkt_ctx* c) {
    if (!c->msm) return;
    WireBases& wb = c->msm->wb;
    if (!wb.borrowed && wb.built) {
        (void)hipStreamSynchronize(c->stream);
        for (int k = 0; k < 3; ++k) {
            dev_free(c, wb.table[k]);
            dev_free(c, wb.u[k]);
        }
    }
    wb = WireBases{};
}

static int wire_digest_enqueue(zkt_ctx* c, const uint32_t* const* d_idx, size_t n_rows) {
    MsmState& st = *c->msm;
    if (!st.wb_dig)
        if (int rc = dev_alloc(c, (void**)&st.wb_dig, 16)) return rc;
    if (!st.wb_pin) ZKT_HIP(c, hipHostMalloc((void**)&st.wb_pin, 64));
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

template <class C>
static int wire_bases_build_wire(zkt_ctx* c, int log_n, int k, const uint32_t* d_idx, size_t n_rows, size_t n_vars, double frac) {
    using Q = typename C::Fq;
    MsmState& st = *c->msm;
    WireBases& wb = st.wb;
    const size_t n = (size_t)1 << log_n;
    void *d_cnt = nullptr, *d_start = nullptr, *d_grouped = nullptr, *d_ofs = nullptr, *d_bad = nullptr, *table = nullptr, *d_u = nullptr;
    auto done = [&](bool keep) {   // a wire that cannot have its table is committed through its coefficients: never an error
        dev_free(c, d_cnt); dev_free(c, d_start); dev_free(c, d_grouped); dev_free(c, d_ofs); dev_free(c, d_bad);
        if (!keep) { dev_free(c, table); dev_free(c, d_u); }
        (void)hipGetLastError();
        return ZKT_OK;
    };
    if (dev_alloc(c, &d_cnt, (n_vars + 1) * 4)) return done(false);
    ZKT_HIP(c, hipMemsetAsync(d_cnt, 0, (n_vars + 1) * 4, c->stream));
    const unsigned rb = (unsigned)((n_rows + 255) / 256);
    if (n_rows) hipLaunchKernelGGL(k_wire_count, dim3(rb), dim3(256), 0, c->stream, d_idx, n_rows, (uint32_t)n_vars, (uint32_t*)d_cnt);
    std::vector<uint32_t> cnt(n_vars + 1);
    if (hipMemcpyAsync(cnt.data(), d_cnt, n_vars * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess)
        return done(false);
    std::vector<uint32_t> u, ofs;
    uint32_t at = 0;
    for (size_t v = 0; v < n_vars; ++v) {
        const uint32_t m = cnt[v];
        cnt[v] = at;             // becomes start[v]
        if (m) {
            u.push_back((uint32_t)v);
            ofs.push_back(at);
            at += m;
        }
    }
    ofs.push_back(at);
    const size_t d = u.size();
    if ((double)d >= frac * (double)n_rows || (uint64_t)st.plan.W * (d + 2) >= ((uint64_t)1 << 31)) return done(false);
    if (dev_alloc(c, &table, (size_t)st.plan.W * (d + 2) * sizeof(Affine<Q>)) || dev_alloc(c, &d_u, (d + 1) * 4) ||
        dev_alloc(c, &d_start, (n_vars + 1) * 4) || dev_alloc(c, &d_grouped, ((size_t)at + 1) * 4) || dev_alloc(c, &d_ofs, (d + 1) * 4) ||
        dev_alloc(c, &d_bad, 4))
        return done(false);
    ZKT_HIP(c, hipMemcpyAsync(d_start, cnt.data(), n_vars * 4, hipMemcpyHostToDevice, c->stream));
    ZKT_HIP(c, hipMemcpyAsync(d_u, u.data(), d * 4, hipMemcpyHostToDevice, c->stream));
    ZKT_HIP(c, hipMemcpyAsync(d_ofs, ofs.data(), (d + 1) * 4, hipMemcpyHostToDevice, c->stream));
    ZKT_HIP(c, hipMemsetAsync(d_cnt, 0, (n_vars + 1) * 4, c->stream));
    ZKT_HIP(c, hipMemsetAsync(d_bad, 0, 4, c->stream));
    if (n_rows)
        hipLaunchKernelGGL(k_wire_fill, dim3(rb), dim3(256), 0, c->stream, d_idx, n_rows, (uint32_t)n_vars, (const uint32_t*)d_start,
                           (uint32_t*)d_cnt, (uint32_t*)d_grouped);
    if (d)
        hipLaunchKernelGGL(k_wire_sum<C>, dim3((unsigned)((d + 63) / 64)), dim3(64), 0, c->stream, (const Affine<Q>*)st.table2,
                           (const uint32_t*)d_grouped, (const uint32_t*)d_ofs, d, (Affine<Q>*)table, (uint32_t*)d_bad);
    hipLaunchKernelGGL(k_wire_blinder_points<C>, dim3(1), dim3(64), 0, c->stream, (const Affine<Q>*)st.table2, n, d, (Affine<Q>*)table);
    uint32_t bad = 0;
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess)   // (the staging vectors may go after this)
        return done(false);
    if (bad || msm_table_finish(c, table, d + 2)) return done(false);
    wb.table[k] = table;
    wb.u[k] = (uint32_t*)d_u;
    wb.cnt[k] = d;
    wb.use[k] = true;
    return done(true);
}

int wire_bases_prepare(zkt_ctx* c, int log_n, const uint32_t* const* d_idx, size_t n_rows, size_t n_vars) {
    if (!c->msm) return ZKT_OK;
    MsmState& st = *c->msm;
    WireBases& wb = st.wb;
    const size_t n = (size_t)1 << log_n;
    const bool possible = lagrange_ready(c, log_n) && !c->sharded() && !c->lagrange_off && st.count2 >= n + 2 && n_rows <= n &&
                          n_vars <= 0xFFFFFFFEull && !(exp_env("ZKT_WIRE_BASES") && atoi(exp_env("ZKT_WIRE_BASES")) == 0);
    const bool same = wb.built && !wb.stale && wb.w[0] == d_idx[0] && wb.w[1] == d_idx[1] && wb.w[2] == d_idx[2] &&
                      wb.n_rows == n_rows && wb.n_vars == n_vars && wb.log_n == log_n && wb.srs_generation == c->srs_generation;
    if (possible && same) return ZKT_OK;
    // tables that forks of this context read stay where they are: this context then commits densely until they are gone
    if (wb.built && !wb.borrowed && c->forks.load() > 0) {
        if (!same || !possible) wb.stale = true;
        return ZKT_OK;
    }
    wire_bases_drop(c);
    if (!possible) return ZKT_OK;
    double frac = WIRE_BASES_MAX_FRAC;
    if (const char* e = exp_env("ZKT_WIRE_BASES_FRAC")) frac = atof(e);   // experiment: the threshold's A/B
    hipEvent_t e0 = nullptr, e1 = nullptr;
    const bool trace = exp_env("ZKT_HOST_TRACE") != nullptr;
    if (trace) {
        (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
        (void)hipEventRecord(e0, c->stream);
    }
    for (int k = 0; k < 3; ++k) {
        const int rc = c->curve == ZKT_CURVE_BN254 ? wire_bases_build_wire<Bn254Curve>(c, log_n, k, d_idx[k], n_rows, n_vars, frac)
                                                    : wire_bases_build_wire<Bls381Curve>(c, log_n, k, d_idx[k], n_rows, n_vars, frac);
        if (rc) return rc;
    }
    if (int rc = wire_digest_enqueue(c, d_idx, n_rows)) return rc;
    ZKT_HIP(c, hipStreamSynchronize(c->stream));
    if (trace) {
        float ms = 0;
        (void)hipEventRecord(e1, c->stream); (void)hipEventSynchronize(e1); (void)hipEventElapsedTime(&ms, e0, e1);
        fprintf(stderr, "[zkt host] wire base tables: %zu / %zu / %zu distinct of %zu rows (0 = dense), %.1f ms\n",
                wb.use[0] ? wb.cnt[0] : 0, wb.use[1] ? wb.cnt[1] : 0, wb.use[2] ? wb.cnt[2] : 0, n_rows, ms);
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    }
    wb.digest[0] = st.wb_pin[0];
    wb.digest[1] = st.wb_pin[1];
    for (int k = 0; k < 3; ++k) wb.w[k] = d_idx[k];
    wb.n_rows = n_rows; wb.n_vars = n_vars; wb.log_n = log_n; wb.srs_generation = c->srs_generation;
    wb.built = true;
    ++c->msm_epoch;
    return ZKT_OK;
}

bool wire_bases_use(const zkt_ctx* c, int k) {
    return c->msm && c->msm->wb.built && !c->msm->wb.stale && c->msm->wb.use[k];
}
int wire_bases_digest(zkt_ctx* c, const uint32_t* const* d_idx, size_t n_rows) { return wire_digest_enqueue(c, d_idx, n_rows); }
int wire_bases_lens(zkt_ctx* c, const uint32_t* d_lens) {
    ZKT_HIP(c, hipMemcpyAsync(c->msm->wb_pin + 2, d_lens, 12, hipMemcpyDeviceToHost, c->stream));
    return ZKT_OK;
}

template <class C>
static int wire_scalars_t(zkt_ctx* c, int k, const void* d_vars, const void* d_bl, size_t n, const void** out, size_t* len) {
    using R = typename C::Fr;
    MsmState& st = *c->msm;
    const size_t cnt = st.wb.cnt[k];
    if (int rc = grow(c, st.wb_scalars[k], (cnt + 2) * sizeof(Fe<R>))) return rc;
    Fe<R> nn = fe_zero<R>();
    nn.v[0] = (uint32_t)(n & 0xffffffffu);
    nn.v[1] = (uint32_t)((uint64_t)n >> 32);
    const Fe<R> ninv = fe_inv_host<R>(fe_to_mont<R>(nn));
    hipLaunchKernelGGL(k_wire_scalars<R>, dim3((unsigned)((cnt + 2 + 255) / 256)), dim3(256), 0, c->stream, (const Fe<R>*)d_vars,
                       (const uint32_t*)st.wb.u[k], cnt, (const Fe<R>*)d_bl, ninv, (Fe<R>*)st.wb_scalars[k].p);
    ZKT_HIP(c, hipGetLastError());
    *out = st.wb_scalars[k].p;
    *len = cnt + 2;
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

}  // namespace zkt
