// zkt_g1_check / zkt_srs_check: a committer key validated on the device before it is loaded.
//
// Per point (k_g1_check, one thread per point as k_g1_decompress; the rules are g1c_point's in g1decomp.hpp): the raw limbs
// below the modulus, not the identity, on the curve, in the prime-order subgroup (BLS12-381).  The points are untrusted:
// a thread reads its own point and writes its own status byte, nothing is indexed by data, every refusal is a status.
// k_g1_status_reduce then counts the statuses of a chunk and finds its first bad point: sums and a minimum within the
// wave, then across the workgroup's waves in LDS, then one atomic per total and workgroup.
//
// Structure (srs_check): is there a tau with P_i = tau^i P_0 for all i and beta_h = tau h?  With D_i = P_(i+1) - tau P_i
// the key is good iff every D_i = 0, and for a challenge rho sum_i rho^i D_i = 0 is ONE pairing equation,
// e(A, beta_h) = e(B, h), A = sum_(i < count-1) rho^i P_i, B = sum_(i < count-1) rho^i P_(i+1).  A key with some D_i != 0
// passes for at most count - 1 values of rho (the roots of a polynomial of that degree over the group's exponents), i.e.
// with probability below count / r for a rho the key's author could not foresee.  One MSM serves both sides: with
// S = sum_(i < count) rho^i P_i,  rho B = S - P_0  and  A = S - rho^(count-1) P_(count-1), so the check is
//     e(rho S - rho^count P_(count-1), beta_h) e(P_0 - S, h) == 1.
// The device sums S chunk by chunk (k_gen_powers from rho^start, then the msm_bases path); the host adds the chunk sums,
// does the two short scalar multiplications and the pairing product (srs_check_finish).
//
// Resources (gfx950, docs/EXPERIMENTS.md "checking a committer key"): no scratch on either curve.
#include "g1decomp.hpp"
#include "msm.hpp"
#include "poly.hpp"

#include <algorithm>
#include <cstring>
#include <vector>

namespace zkt {

constexpr int G1C_THREADS = 64;          // one wave per workgroup, as k_g1_decompress
constexpr int G1C_RED_THREADS = 256;
constexpr unsigned G1C_RED_BLOCKS = 256;
constexpr uint32_t G1C_NO_KEY = 0xFFFFFFFFu;
constexpr int G1C_STATUSES = 6;          // ZKT_G1_VALID .. ZKT_G1_NOT_IN_SUBGROUP

// what k_g1_status_reduce adds up for one chunk: how many points got each status, and the least (index << 3 | status) over
// the points that are not valid (an index within the chunk, below 2^22: the key fits 32 bits)
struct G1cTotals {
    unsigned long long by_status[G1C_STATUSES];
    uint32_t key;
    uint32_t pad;
};

template <class C>
__global__ __launch_bounds__(G1C_THREADS) void k_g1_check(const uint4* __restrict__ in, uint32_t n, uint8_t* __restrict__ status,
                                                          Fx<typename C::Fq> beta) {
    using Q = typename C::Fq;
    constexpr int N = Q::N;
    const uint32_t i = blockIdx.x * G1C_THREADS + threadIdx.x;
    if (i >= n) return;
    Fe<Q> xw, yw;
#pragma unroll
    for (int k = 0; k < N / 4; ++k) {
        const uint4 v = in[(size_t)i * (N / 2) + k], w = in[(size_t)i * (N / 2) + N / 4 + k];
        xw.v[4 * k] = v.x; xw.v[4 * k + 1] = v.y; xw.v[4 * k + 2] = v.z; xw.v[4 * k + 3] = v.w;
        yw.v[4 * k] = w.x; yw.v[4 * k + 1] = w.y; yw.v[4 * k + 2] = w.z; yw.v[4 * k + 3] = w.w;
    }
    status[i] = (uint8_t)g1c_point<C>(xw, yw, beta);
}

// status: n bytes, readable as whole 32-bit words (the buffer is padded to a multiple of four bytes).  tot: cleared to zero
// counts and key G1C_NO_KEY by the caller.
__global__ __launch_bounds__(G1C_RED_THREADS) void k_g1_status_reduce(const uint32_t* __restrict__ status, uint32_t n, G1cTotals* tot) {
    __shared__ uint32_t sh[G1C_RED_THREADS / 64][G1C_STATUSES + 1];
    uint32_t cnt[G1C_STATUSES], key = G1C_NO_KEY;
#pragma unroll
    for (int k = 0; k < G1C_STATUSES; ++k) cnt[k] = 0;
    const uint32_t words = (n + 3) / 4;
    for (uint32_t w = blockIdx.x * G1C_RED_THREADS + threadIdx.x; w < words; w += gridDim.x * G1C_RED_THREADS) {
        const uint32_t v = status[w];
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t i = 4 * w + j, st = (v >> (8 * j)) & 0xFFu;
            if (i < n) {
#pragma unroll
                for (uint32_t k = 0; k < (uint32_t)G1C_STATUSES; ++k) cnt[k] += st == k ? 1u : 0u;
                if (st != ZKT_G1_VALID) key = min(key, (i << 3) | (st & 7u));
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int k = 0; k < G1C_STATUSES; ++k) cnt[k] += __shfl_down(cnt[k], off, 64);
        key = min(key, (uint32_t)__shfl_down(key, off, 64));
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < G1C_STATUSES; ++k) sh[wave][k] = cnt[k];
        sh[wave][G1C_STATUSES] = key;
    }
    __syncthreads();
    if (threadIdx.x <= G1C_STATUSES) {       // thread k owns total k: one atomic each, none for a zero count
        uint32_t v = sh[0][threadIdx.x];
        for (int w = 1; w < G1C_RED_THREADS / 64; ++w)
            v = threadIdx.x < G1C_STATUSES ? v + sh[w][threadIdx.x] : min(v, sh[w][threadIdx.x]);
        if (threadIdx.x < G1C_STATUSES) {
            if (v) atomicAdd(&tot->by_status[threadIdx.x], (unsigned long long)v);
        } else if (v != G1C_NO_KEY) {
            atomicMin(&tot->key, v);
        }
    }
}

static size_t g1c_up(size_t b) { return (b + 255) / 256 * 256; }

// Enqueues the statuses of m points at d_pts (device, 16-byte aligned) into the state's status buffer and their totals in
// front of it; 1 <= m <= ZKT_MSM_BASES_MAX.  No synchronisation.
template <class C>
static int g1c_enqueue_t(zkt_ctx* c, MsmBasesState* st, const void* d_pts, size_t m) {
    using Q = typename C::Fq;
    static const Fx<Q> beta = C::ID == 1 ? g1d_beta<Q>() : fx_zero<Q>();
    char* const base = (char*)st->check_status.p;
    G1cTotals* const tot = (G1cTotals*)base;
    uint8_t* const status = (uint8_t*)(base + g1c_up(sizeof(G1cTotals)));
    ZKT_HIP(c, hipMemsetAsync(tot, 0, sizeof(G1cTotals), c->stream));
    ZKT_HIP(c, hipMemsetAsync(&tot->key, 0xFF, sizeof(uint32_t), c->stream));
    hipLaunchKernelGGL(k_g1_check<C>, dim3((unsigned)((m + G1C_THREADS - 1) / G1C_THREADS)), dim3(G1C_THREADS), 0, c->stream,
                       (const uint4*)d_pts, (uint32_t)m, status, beta);
    const size_t words = (m + 3) / 4;
    const unsigned blocks = (unsigned)std::min<size_t>((words + G1C_RED_THREADS - 1) / G1C_RED_THREADS, G1C_RED_BLOCKS);
    hipLaunchKernelGGL(k_g1_status_reduce, dim3(blocks), dim3(G1C_RED_THREADS), 0, c->stream, (const uint32_t*)status, (uint32_t)m, tot);
    ZKT_HIP(c, hipGetLastError());
    return ZKT_OK;
}

// One chunk: m points from `pts` (host: uploaded into the state's own buffer; device: read where they are, behind the work
// already on the stream) -> *d_pts the chunk on the device, *tot its totals, out_status (host, may be null) its m status
// bytes.  Synchronises the stream, on failure too once the upload has been enqueued (it reads the caller's memory).
static int g1c_chunk(zkt_ctx* c, MsmBasesState* st, const void* pts, bool on_device, size_t m, const void** d_pts, G1cTotals* tot,
                     uint8_t* out_status) {
    const size_t pt_bytes = c->curve == ZKT_CURVE_BN254 ? 64 : 96;
    int rc = grow(c, st->check_status, g1c_up(sizeof(G1cTotals)) + g1c_up(m), &st->mem);
    if (rc) return rc;
    *d_pts = pts;
    if (!on_device) {
        if ((rc = grow(c, st->check_points, m * pt_bytes, &st->mem))) return rc;
        ZKT_HIP(c, hipMemcpyAsync(st->check_points.p, pts, m * pt_bytes, hipMemcpyHostToDevice, c->stream));
        *d_pts = st->check_points.p;
    }
    {
        ProfScope prof(c, "srs_check_points");
        rc = c->curve == ZKT_CURVE_BN254 ? g1c_enqueue_t<Bn254Curve>(c, st, *d_pts, m) : g1c_enqueue_t<Bls381Curve>(c, st, *d_pts, m);
    }
    hipError_t e = hipSuccess;
    if (!rc) {
        const char* const base = (const char*)st->check_status.p;
        e = hipMemcpyAsync(tot, base, sizeof(G1cTotals), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess && out_status)
            e = hipMemcpyAsync(out_status, base + g1c_up(sizeof(G1cTotals)), m, hipMemcpyDeviceToHost, c->stream);
    }
    const hipError_t es = hipStreamSynchronize(c->stream);
    if (rc) return rc;
    if (e != hipSuccess) return hip_fail(c, e, "g1_check: download");
    if (es != hipSuccess) return hip_fail(c, es, "g1_check: hipStreamSynchronize");
    return ZKT_OK;
}

static size_t g1c_chunk_points(const zkt_ctx* c) { return c->srs_check_chunk ? c->srs_check_chunk : (size_t)ZKT_MSM_BASES_MAX; }

template <class C>
static void g1_check_host_t(const uint64_t* pts, size_t n, uint8_t* out_status) {
    using Q = typename C::Fq;
    static const Fx<Q> beta = C::ID == 1 ? g1d_beta<Q>() : fx_zero<Q>();
    for (size_t i = 0; i < n; ++i) {
        Fe<Q> xw, yw;
        memcpy(xw.v, pts + i * Q::N, Q::N * 4);
        memcpy(yw.v, pts + i * Q::N + Q::N / 2, Q::N * 4);
        out_status[i] = (uint8_t)g1c_point<C>(xw, yw, beta);
    }
}

// seed32 as a little-endian integer mod r -> canonical words; false when that is zero
template <class R>
static bool rho_from_seed(const uint8_t* seed32, Fe<R>* rho) {
    static_assert(R::N == 8 && R::BITS >= 254, "2^256 < 6 r");
    Fe<R> v;
    memcpy(v.v, seed32, 32);
    for (int k = 0; k < 6; ++k) v = fe_reduce_once<R>(v);   // subtracts r while the value is not below it
    *rho = v;
    return !fe_is_zero<R>(v);
}

// The host's end of the structure test (see the head of the file): S, P0, Plast affine Montgomery limbs, rho canonical and
// non-zero mod r.  *ok = 1 / 0; an error when the pairing refuses a point (not on the curve, outside G1).
template <class C>
static int srs_check_finish_t(const uint64_t* S, int S_inf, const uint64_t* P0, const uint64_t* Plast, uint64_t count,
                              const uint64_t* rho4, const uint64_t* h, const uint64_t* beta_h, int* ok) {
    using Q = typename C::Fq;
    using R = typename C::Fr;
    constexpr int L64 = Q::N / 2;
    if (count == 1) {          // nothing to relate
        *ok = 1;
        return ZKT_OK;
    }
    Fe<R> rho;
    if (!rho_from_seed<R>((const uint8_t*)rho4, &rho)) return ZKT_ERR_INVALID_ARGUMENT;   // reduced once more; zero is no challenge
    const Fe<R> rho_m = fe_to_mont<R>(rho);
    const Fe<R> rho_n = fe_neg<R>(fe_pow_u64<R>(rho_m, count));                // -rho^count, Montgomery form
    uint64_t pts[2 * 2 * 6] = {0}, sc[2 * 4], g1[2 * 2 * 6] = {0}, g2[2 * 4 * 6];
    if (!S_inf) memcpy(pts, S, 2 * L64 * 8);
    memcpy(pts + 2 * L64, Plast, 2 * L64 * 8);
    memcpy(sc, rho_m.v, 32);
    memcpy(sc + 4, rho_n.v, 32);
    int inf = 0, rc;
    if ((rc = zkt_g1_msm_host(C::ID, pts, sc, 2, 1, g1, &inf))) return rc;     // rho S - rho^count Plast = rho A
    // P0 - S = -(rho B)
    uint64_t pm[2 * 2 * 6] = {0};
    memcpy(pm, P0, 2 * L64 * 8);
    if (!S_inf) {
        Fe<Q> y;
        memcpy(y.v, S + L64, L64 * 8);
        y = fe_neg<Q>(y);
        memcpy(pm + 2 * L64, S, L64 * 8);
        memcpy(pm + 3 * L64, y.v, L64 * 8);
    }
    if ((rc = zkt_g1_sum_host(C::ID, pm, 2, g1 + 2 * L64, &inf))) return rc;
    memcpy(g2, beta_h, 4 * L64 * 8);
    memcpy(g2 + 4 * L64, h, 4 * L64 * 8);
    int one = 0;
    if ((rc = zkt_pairing_product_is_one(C::ID, g1, g2, 2, &one))) return rc;
    *ok = one ? 1 : 0;
    return ZKT_OK;
}

static int srs_check_finish(int curve, const uint64_t* S, int S_inf, const uint64_t* P0, const uint64_t* Plast, uint64_t count,
                            const uint64_t* rho4, const uint64_t* h, const uint64_t* beta_h, int* ok) {
    if (curve == ZKT_CURVE_BN254) return srs_check_finish_t<Bn254Curve>(S, S_inf, P0, Plast, count, rho4, h, beta_h, ok);
    return srs_check_finish_t<Bls381Curve>(S, S_inf, P0, Plast, count, rho4, h, beta_h, ok);
}

template <class C>
static int srs_check_t(zkt_ctx* c, const void* pts, size_t count, bool on_device, const uint64_t* h, const uint64_t* beta_h,
                       const uint8_t* seed32, uint8_t* out_status, zkt_srs_report* rep) {
    using Q = typename C::Fq;
    using R = typename C::Fr;
    constexpr size_t PT = 2 * Q::N * 4;       // bytes of a point
    constexpr int L64 = Q::N / 2;
    Fe<R> rho;
    if (!rho_from_seed<R>(seed32, &rho)) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "srs_check: the seed reduces to rho = 0");
    const Fe<R> rho_m = fe_to_mont<R>(rho);
    MsmBasesState* st = nullptr;
    int rc = msm_bases_scratch(c, &st);
    if (rc) return rc;
    memset(rep, 0, sizeof(*rep));
    rep->count = count;
    rep->first_bad = count;
    uint64_t ends[2][2 * L64];                // P_0 and P_(count-1)
    std::vector<uint64_t> sums;               // the chunks' sums, affine
    const size_t chunk = g1c_chunk_points(c);
    for (size_t start = 0; start < count; start += chunk) {
        const size_t m = std::min(chunk, count - start);
        const void* d_pts = nullptr;
        G1cTotals tot;
        if ((rc = g1c_chunk(c, st, (const char*)pts + start * PT, on_device, m, &d_pts, &tot, out_status ? out_status + start : nullptr)))
            return rc;
        for (int k = 0; k < G1C_STATUSES; ++k) rep->by_status[k] += tot.by_status[k];
        if (tot.key != G1C_NO_KEY && rep->n_bad == 0) {
            rep->first_bad = start + (tot.key >> 3);
            rep->first_bad_status = (int)(tot.key & 7u);
        }
        rep->n_bad += m - tot.by_status[ZKT_G1_VALID];
        if (rep->n_bad) continue;             // the later chunks still get their statuses and counts, and no MSM
        if ((rc = grow(c, st->scalars, m * 32, &st->mem))) return rc;
        // the key's two ends for the host's finish; msm_bases waits for the stream, and so does every way out before it
        hipError_t e = hipSuccess;
        if (start == 0) e = hipMemcpyAsync(ends[0], d_pts, PT, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess && start + m == count)
            e = hipMemcpyAsync(ends[1], (const char*)d_pts + (m - 1) * PT, PT, hipMemcpyDeviceToHost, c->stream);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(c->stream);
            return hip_fail(c, e, "srs_check: download");
        }
        ProfScope prof(c, "srs_check_msm");
        const Fe<R> first = fe_pow_u64<R>(rho_m, (uint64_t)start);
        if ((rc = gen_powers(c, st->scalars.p, m, rho_m.v, first.v))) {
            (void)hipStreamSynchronize(c->stream);
            return rc;
        }
        sums.resize(sums.size() + 2 * L64);
        rc = msm_bases(c, d_pts, true, st->scalars.p, true, m, 1, sums.data() + sums.size() - 2 * L64, nullptr);
        if (rc) {
            (void)hipStreamSynchronize(c->stream);
            return rc;
        }
    }
    rep->points_ok = rep->n_bad == 0;
    if (!rep->points_ok) return ZKT_OK;
    if ((rc = zkt_g1_sum_host(c->curve, sums.data(), sums.size() / (2 * L64), rep->sum_xy_mont, &rep->sum_is_infinity))) return rc;
    rep->structure_checked = 1;
    uint64_t rho4[4];
    memcpy(rho4, rho.v, 32);
    if ((rc = srs_check_finish(c->curve, rep->sum_xy_mont, rep->sum_is_infinity, ends[0], ends[1], count, rho4, h, beta_h,
                               &rep->structure_ok)))
        return set_err(c, rc, "srs_check: the pairing refused its arguments (h, beta_h not on the twist?)");
    rep->ok = rep->points_ok && rep->structure_ok;
    return ZKT_OK;
}

}  // namespace zkt

using namespace zkt;

extern "C" {

int zkt_debug_g1_check_host(int curve_id, const uint64_t* points, size_t n, uint8_t* out_status) {
    if (n && (!points || !out_status)) return ZKT_ERR_INVALID_ARGUMENT;
    if (curve_id == ZKT_CURVE_BN254) g1_check_host_t<Bn254Curve>(points, n, out_status);
    else if (curve_id == ZKT_CURVE_BLS12_381) g1_check_host_t<Bls381Curve>(points, n, out_status);
    else return ZKT_ERR_INVALID_ARGUMENT;
    return ZKT_OK;
}

int zkt_g1_check(zkt_ctx* c, const void* points_xy_mont, size_t n, int points_on_device, uint8_t* out_status) {
    if (!c) return ZKT_ERR_INVALID_ARGUMENT;
    if (n == 0) return ZKT_OK;
    if (!points_xy_mont || !out_status) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (points_on_device && ((uintptr_t)points_xy_mont & 15u))
        return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "g1_check: device points must be 16-byte aligned");
    (void)hipSetDevice(c->device);
    MsmBasesState* st = nullptr;
    int rc = msm_bases_scratch(c, &st);
    if (rc) return rc;
    const size_t pt_bytes = c->curve == ZKT_CURVE_BN254 ? 64 : 96, chunk = ZKT_MSM_BASES_MAX;
    for (size_t start = 0; start < n; start += chunk) {
        const size_t m = std::min(chunk, n - start);
        const void* d_pts = nullptr;
        G1cTotals tot;
        if ((rc = g1c_chunk(c, st, (const char*)points_xy_mont + start * pt_bytes, points_on_device != 0, m, &d_pts, &tot,
                            out_status + start)))
            return rc;
    }
    return ZKT_OK;
}

int zkt_srs_check(zkt_ctx* c, const void* g1_xy_mont, size_t count, int points_on_device, const uint64_t* h_g2_mont,
                  const uint64_t* beta_h_g2_mont, const uint8_t seed32[32], uint8_t* out_status, zkt_srs_report* report) {
    if (!c) return ZKT_ERR_INVALID_ARGUMENT;
    if (!g1_xy_mont || !h_g2_mont || !beta_h_g2_mont || !seed32 || !report) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (count == 0) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "srs_check: a key has at least one power");
    if (count > ZKT_SRS_CHECK_MAX) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "srs_check: more points than ZKT_SRS_CHECK_MAX (2^24 + 1)");
    if (points_on_device && ((uintptr_t)g1_xy_mont & 15u))
        return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "srs_check: device points must be 16-byte aligned");
    (void)hipSetDevice(c->device);
    if (c->curve == ZKT_CURVE_BN254)
        return srs_check_t<Bn254Curve>(c, g1_xy_mont, count, points_on_device != 0, h_g2_mont, beta_h_g2_mont, seed32, out_status, report);
    return srs_check_t<Bls381Curve>(c, g1_xy_mont, count, points_on_device != 0, h_g2_mont, beta_h_g2_mont, seed32, out_status, report);
}

int zkt_debug_srs_check_chunk(zkt_ctx* c, size_t max_points) {
    if (!c) return ZKT_ERR_INVALID_ARGUMENT;
    if (max_points > ZKT_MSM_BASES_MAX) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "srs_check: a chunk holds at most ZKT_MSM_BASES_MAX points");
    c->srs_check_chunk = max_points;
    return ZKT_OK;
}

int zkt_debug_srs_check_finish_host(int curve_id, const uint64_t* S, int S_inf, const uint64_t* P0, const uint64_t* Plast,
                                    uint64_t count, const uint64_t* rho_canonical4, const uint64_t* h, const uint64_t* beta_h,
                                    int* structure_ok) {
    if ((!S && !S_inf) || !P0 || !Plast || !rho_canonical4 || !h || !beta_h || !structure_ok || count == 0) return ZKT_ERR_INVALID_ARGUMENT;
    if (curve_id != ZKT_CURVE_BN254 && curve_id != ZKT_CURVE_BLS12_381) return ZKT_ERR_INVALID_ARGUMENT;
    return srs_check_finish(curve_id, S, S_inf, P0, Plast, count, rho_canonical4, h, beta_h, structure_ok);
}

}  // extern "C"
