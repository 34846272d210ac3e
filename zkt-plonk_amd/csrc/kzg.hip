// The KZG commitment seam (include/zkt_plonk.h "KZG commitment seam"): zkt_kzg_commit_batch and zkt_kzg_open, the two
// methods of a KZG10 wrapper (PC::commit, PC::open_individual_opening_challenges; shim/src/kzg.rs) that leaves arkworks'
// prover on the host and moves only the polynomial-commitment work to the device.
//
// commit: the k MSMs of one PC::commit go out on the prover's schedule (msm_begin_many: grouped launches where
// msm_batches_grouping says the key size gains, deferred or overlapping bucket reductions), in waves of MsmState::SLOTS,
// with ONE host wait per wave.  The host form uploads polynomial j + 1 on a copy stream while polynomial j's MSM runs on
// the context's stream.
// open: one fused pass over the coefficients (k_kzg_open_combine) writes t_i = z^i sum_j c_j p_j[i] and the per-workgroup
// partial sums of every p_j(z); the division by X - z then is the suffix scan and scaling of open_witness (poly.hip), and
// the witness is one MSM.
#include "ctx.hpp"
#include "hostinv.hpp"
#include "msm.hpp"
#include "poly.hpp"

#include <algorithm>
#include <cstring>
#include <functional>
#include <vector>

namespace zkt {

// Host uploads: hipMemcpyAsync straight from the caller's pageable memory on a copy stream of the context's own.  The
// call returns once the runtime has staged the copy, so the host stages polynomial j + 1 while the GPU runs polynomial
// j's MSM.  A pinned ring of two 4 MiB buffers filled by a host memcpy was measured against it and lost: BN254 2^20 k = 3
// 1.84 against 1.67 ms per commitment, k = 1 2.58 against 2.17 (profiles/kzg_seam_timing.txt) -- the runtime's own
// staging copies faster than one host thread.
// The fused combination reads KZG_OPEN_E elements per thread: a workgroup covers 256 KZG_OPEN_E coefficients, a whole
// number of the division's workgroups (256 open_elems(len)), whose block power table it reads.  Resource use on gfx950
// (-Rpass-analysis=kernel-resource-usage): E = 8 needs 256 VGPRs and spills 225, E = 4 204 VGPRs (2 waves per SIMD, no
// spill), E = 2 131 (3 waves) but pays the per-term wave reduction of the evaluations over half as many coefficients.
constexpr int KZG_OPEN_E = 4;

struct KzgState {
    DevSet mem;   // owns everything below
    explicit KzgState(int device) : mem(device) {}
    hipStream_t copy = nullptr;
    hipEvent_t ev_up = nullptr, ev_main = nullptr;
    DevBuf up;                         // host forms: the uploaded coefficients
    DevBuf t, tb, w, scan, pw, part, evals;   // zkt_kzg_open
};

static int kzg_state(zkt_ctx* c, KzgState** out) {
    if (!c->kzg) {
        auto K = std::make_shared<KzgState>(c->device);
        int rc;
        if ((rc = K->mem.stream(c, &K->copy)) || (rc = K->mem.event(c, &K->ev_up)) || (rc = K->mem.event(c, &K->ev_main))) return rc;
        c->kzg = K;
    }
    *out = c->kzg.get();
    return ZKT_OK;
}

// the copy stream starts behind everything on the context's stream (the upload buffer may still be read there)
static int kzg_copy_after_main(zkt_ctx* c, KzgState& K) {
    ZKT_HIP(c, hipEventRecord(K.ev_main, c->stream));
    ZKT_HIP(c, hipStreamWaitEvent(K.copy, K.ev_main, 0));
    return ZKT_OK;
}
// host -> HBM on the copy stream; the context's stream waits for it
static int kzg_upload(zkt_ctx* c, KzgState& K, const void* src, size_t bytes, void* dst) {
    ZKT_HIP(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, K.copy));
    ZKT_HIP(c, hipEventRecord(K.ev_up, K.copy));
    ZKT_HIP(c, hipStreamWaitEvent(c->stream, K.ev_up, 0));
    return ZKT_OK;
}

// everything that is refused is refused here, before any work is enqueued
static int kzg_check(zkt_ctx* c, const void* const* coeffs, const size_t* lens, int k, const void* out) {
    if (!c) return ZKT_ERR_INVALID_ARGUMENT;
    if (k < 0 || k > ZKT_KZG_BATCH_MAX) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "k: 0 .. ZKT_KZG_BATCH_MAX polynomials");
    if (k == 0) return ZKT_OK;
    if (!coeffs || !lens || !out) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    for (int j = 0; j < k; ++j)
        if (lens[j] && !coeffs[j]) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (!c->msm) return set_err(c, ZKT_ERR_NOT_LOADED, "no SRS loaded (zkt_srs_load)");
    if (c->msm->slice_off != 0 || c->msm->total != c->msm->count)
        return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "the KZG seam needs the whole key, not a slice of it");
    for (int j = 0; j < k; ++j)
        if (lens[j] > c->msm->count)
            return set_err(c, ZKT_ERR_TOO_MANY_COEFFICIENTS, "TooManyCoefficients: polynomial longer than the committer key");
    return ZKT_OK;
}

static int fq_limbs(const zkt_ctx* c) { return c->curve == ZKT_CURVE_BN254 ? 4 : 6; }
static bool xy_is_zero(const uint64_t* xy, int words) {
    for (int i = 0; i < words; ++i)
        if (xy[i]) return false;
    return true;
}

static int kzg_commit(zkt_ctx* c, const void* const* src, bool host, const size_t* lens, int k, int mont, uint64_t* out_xy,
                      int* out_inf) {
    int rc = kzg_check(c, src, lens, k, out_xy);
    if (rc || k == 0) return rc;
    (void)hipSetDevice(c->device);
    KzgState* K = nullptr;
    if ((rc = kzg_state(c, &K))) return rc;
    const int W = 2 * fq_limbs(c);
    std::vector<int> live;
    for (int j = 0; j < k; ++j)
        if (lens[j]) live.push_back(j);
    const int S = MsmState::SLOTS;
    if (host) {   // one wave's polynomials at a time
        size_t most = 0;
        for (size_t w0 = 0; w0 < live.size(); w0 += S) {
            size_t b = 0;
            for (size_t i = w0; i < std::min(live.size(), w0 + S); ++i) b += lens[live[i]] * 32;
            most = std::max(most, b);
        }
        if ((rc = grow(c, K->up, most, &K->mem))) return rc;
    }
    std::vector<uint64_t> res((size_t)k * W, 0);
    // the prover's rule: grouped launches where the key size gains from them (and not in the A/B builds that turn them off)
    const bool grouped = !c->batch_off && msm_batches_grouping(c);
    for (size_t w0 = 0; w0 < live.size(); w0 += S) {
        const int m = (int)std::min(live.size() - w0, (size_t)S);
        const void* sc[MsmState::SLOTS];
        size_t ns[MsmState::SLOTS];
        int slots[MsmState::SLOTS], tbls[MsmState::SLOTS] = {};
        size_t off = 0;
        for (int i = 0; i < m; ++i) {
            const int j = live[w0 + i];
            ns[i] = lens[j];
            slots[i] = i;
            sc[i] = host ? (const void*)((char*)K->up.p + off) : src[j];
            off += lens[j] * 32;
        }
        std::function<int(int)> ready;
        if (host) {
            if ((rc = kzg_copy_after_main(c, *K))) return rc;
            ready = [&](int i) { return kzg_upload(c, *K, src[live[w0 + i]], ns[i] * 32, const_cast<void*>(sc[i])); };
        }
        {
            ProfScope prof(c, "kzg_commit_batch", nullptr, (uint64_t)m);
            rc = msm_begin_many(c, m, sc, ns, mont, slots, tbls, grouped, ready);
        }
        if (rc) return rc;
        for (int i = 0; i < m; ++i)   // one wait: the host finishes each MSM as its tail lands
            if ((rc = msm_end(c, slots[i], res.data() + (size_t)live[w0 + i] * W))) return rc;
    }
    ZKT_HIP(c, hipStreamSynchronize(c->stream));
    memcpy(out_xy, res.data(), res.size() * 8);
    if (out_inf)
        for (int j = 0; j < k; ++j) out_inf[j] = xy_is_zero(res.data() + (size_t)j * W, W) ? 1 : 0;
    return ZKT_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// open
// ---------------------------------------------------------------------------------------------------------------------
struct KzgOpenArgs {
    const void* poly[ZKT_KZG_BATCH_MAX];
    uint64_t len[ZKT_KZG_BATCH_MAX];
    uint32_t ch[ZKT_KZG_BATCH_MAX][8];   // challenges, Montgomery
    int nterms;
};

template <class P>
ZKT_D Fe<P> wave_sum(Fe<P> x) {   // every lane of the wave gets the sum of the 64 lanes' x
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        Fe<P> y;
#pragma unroll
        for (int w = 0; w < P::N; ++w) y.v[w] = (uint32_t)__shfl_xor((int)x.v[w], d, 64);
        x = fe_add<P>(x, y);
    }
    return x;
}

// One pass over i < len_max, every coefficient read once.  Workgroup b covers i = base + 256 e + t (e < KZG_OPEN_E,
// base = 256 KZG_OPEN_E b; coalesced).  Per term j: acc_e += c_j p_j[i] (the combination) and a Horner chain in z^256 over
// e, whose value times z^t, summed over the workgroup and times z^base is the workgroup's share of p_j(z) (partials[j][b]).
// Terms are looped over inside the kernel (ragged lengths: a term that ends below the workgroup costs nothing).  Out:
// t_i = z^i acc_i, or acc_i itself when raw (z = 0: the witness is the combination shifted down by one).
// pw / blk: open_pow_tables (z^0 .. z^256; z^(256 E' b') for the division's workgroups b' = fstride b).
template <class P>
__global__ __launch_bounds__(256) void k_kzg_open_combine(KzgOpenArgs a, const Fe<P>* pw, const Fe<P>* blk, int fstride,
                                                         uint64_t len_max, int raw, Fe<P>* t_out, Fe<P>* partials, uint32_t nblk) {
    __shared__ Fe<P> wsum[ZKT_KZG_BATCH_MAX][4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint64_t base = (uint64_t)blockIdx.x * 256 * KZG_OPEN_E;
    const Fe<P> z256 = fe_load<P>(pw + 256), zt = fe_load<P>(pw + t);
    Fe<P> acc[KZG_OPEN_E];
#pragma unroll
    for (int e = 0; e < KZG_OPEN_E; ++e) acc[e] = fe_zero<P>();
#pragma unroll 1
    for (int j = 0; j < a.nterms; ++j) {
        const uint64_t len = a.len[j];
        if (base >= len) {   // uniform over the workgroup
            if (lane == 0) wsum[j][wave] = fe_zero<P>();
            continue;
        }
        const Fe<P>* p = (const Fe<P>*)a.poly[j];
        Fe<P> cj;
#pragma unroll
        for (int w = 0; w < P::N; ++w) cj.v[w] = a.ch[j][w];
        Fe<P> h = fe_zero<P>();
#pragma unroll
        for (int e = KZG_OPEN_E - 1; e >= 0; --e) {
            const uint64_t i = base + (uint64_t)e * 256 + t;
            const Fe<P> v = i < len ? fe_load<P>(p + i) : fe_zero<P>();
            h = fe_add<P>(fe_mul<P>(h, z256), v);
            acc[e] = fe_add<P>(acc[e], fe_mul<P>(cj, v));
        }
        h = wave_sum<P>(fe_mul<P>(h, zt));
        if (lane == 0) wsum[j][wave] = h;
    }
    const Fe<P> zb = fe_load<P>(blk + (size_t)fstride * blockIdx.x);   // z^base
    Fe<P> r = fe_mul<P>(zb, zt);
#pragma unroll
    for (int e = 0; e < KZG_OPEN_E; ++e) {
        const uint64_t i = base + (uint64_t)e * 256 + t;
        if (i < len_max) fe_store<P>(t_out + i, raw ? acc[e] : fe_mul<P>(acc[e], r));
        r = fe_mul<P>(r, z256);
    }
    __syncthreads();
    if (t < a.nterms) {
        Fe<P> s = fe_add<P>(fe_add<P>(wsum[t][0], wsum[t][1]), fe_add<P>(wsum[t][2], wsum[t][3]));
        fe_store<P>(partials + (size_t)t * nblk + blockIdx.x, fe_mul<P>(s, zb));
    }
}

template <class P>
static int open_combine_t(zkt_ctx* c, const KzgOpenArgs& a, const void* pw, size_t len_max, int raw, void* t_out, void* partials,
                          uint32_t nblk) {
    const Fe<P>* tab = (const Fe<P>*)pw;
    const int fstride = KZG_OPEN_E / open_elems(len_max);
    hipLaunchKernelGGL(k_kzg_open_combine<P>, dim3(nblk), dim3(256), 0, c->stream, a, tab, tab + 2 * OPEN_PW_ROW, fstride, (uint64_t)len_max,
                       raw, (Fe<P>*)t_out, (Fe<P>*)partials, nblk);
    ZKT_HIP(c, hipGetLastError());
    return ZKT_OK;
}

template <class P>
static void inv_host(const uint32_t* z, uint32_t* zi) {
    Fe<P> x;
    memcpy(x.v, z, 32);
    x = fe_inv_host<P>(x);
    memcpy(zi, x.v, 32);
}

static int kzg_open(zkt_ctx* c, const void* const* src, bool host, const size_t* lens, int k, const uint64_t* ch, const uint64_t* z4,
                    uint64_t* out_w, int* out_inf, uint64_t* out_evals) {
    int rc = kzg_check(c, src, lens, k, out_w);
    if (rc || k == 0) return rc;
    if (!ch || !z4) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    size_t L = 0, total = 0;
    for (int j = 0; j < k; ++j) {
        L = std::max(L, lens[j]);
        total += lens[j];
    }
    if (L > 0 && open_elems(L) > KZG_OPEN_E)
        return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "zkt_kzg_open: polynomials longer than 2^26 coefficients");
    const int W = 2 * fq_limbs(c);
    std::vector<uint64_t> w(W, 0), ev((size_t)k * 4, 0);
    if (L == 0) {   // all zero polynomials: the identity, zero evaluations
        memcpy(out_w, w.data(), W * 8);
        if (out_inf) *out_inf = 1;
        if (out_evals) memcpy(out_evals, ev.data(), ev.size() * 8);
        return ZKT_OK;
    }
    (void)hipSetDevice(c->device);
    KzgState* K = nullptr;
    if ((rc = kzg_state(c, &K))) return rc;
    const uint32_t nblk = (uint32_t)((L + 256 * KZG_OPEN_E - 1) / (256 * KZG_OPEN_E));
    auto need = [&](DevBuf& buf, size_t bytes) { return grow(c, buf, bytes, &K->mem); };
    if ((rc = need(K->t, L * 32)) || (rc = need(K->tb, L * 32)) || (rc = need(K->w, L * 32)) ||
        (rc = need(K->scan, (2 * (L / 1024 + 2048)) * 32)) || (rc = need(K->pw, open_witness_powers(L) * 32)) ||
        (rc = need(K->part, (size_t)k * nblk * 32)) || (rc = need(K->evals, (size_t)k * 32)))
        return rc;
    if (host && (rc = grow(c, K->up, total * 32, &K->mem))) return rc;
    KzgOpenArgs a{};
    a.nterms = k;
    size_t off = 0;
    for (int j = 0; j < k; ++j) {
        a.poly[j] = host ? (const void*)((char*)K->up.p + off) : src[j];
        a.len[j] = lens[j];
        memcpy(a.ch[j], ch + 4 * (size_t)j, 32);
        off += lens[j] * 32;
    }
    if (host) {
        if ((rc = kzg_copy_after_main(c, *K))) return rc;
        ProfScope prof(c, "kzg_open_upload", K->copy);
        for (int j = 0; j < k && !rc; ++j)
            if (lens[j]) rc = kzg_upload(c, *K, src[j], lens[j] * 32, const_cast<void*>(a.poly[j]));
        if (rc) return rc;
    }
    uint32_t z[8], zi[8] = {};
    memcpy(z, z4, 32);
    bool zero = true;
    for (int i = 0; i < 8; ++i) zero = zero && z[i] == 0;
    if (!zero) {
        if (c->curve == ZKT_CURVE_BN254) inv_host<Bn254Fr>(z, zi);
        else inv_host<Bls381Fr>(z, zi);
    }
    {
        ProfScope prof(c, "kzg_open_combine");
        if ((rc = open_pow_tables(c, z, zi, K->pw.p, L))) return rc;
        rc = c->curve == ZKT_CURVE_BN254 ? open_combine_t<Bn254Fr>(c, a, K->pw.p, L, zero, K->t.p, K->part.p, nblk)
                                         : open_combine_t<Bls381Fr>(c, a, K->pw.p, L, zero, K->t.p, K->part.p, nblk);
        if (rc) return rc;
        if (out_evals && (rc = poly_sum_rows(c, K->part.p, (int)nblk, k, K->evals.p))) return rc;
    }
    int inf = 1;
    if (L >= 2) {   // degree >= 1: the witness has L - 1 coefficients
        const void* scalars = (const char*)K->t.p + 32;   // z = 0: the combination from coefficient 1 on
        if (!zero) {
            ProfScope prof(c, "kzg_open_divide");
            if ((rc = open_divide(c, K->t.p, L, K->tb.p, K->scan.p, K->w.p, K->pw.p))) return rc;
            scalars = K->w.p;
        }
        ProfScope prof(c, "kzg_open_msm");
        if ((rc = msm_g1_dev(c, scalars, L - 1, 0, 1, w.data(), &inf))) return rc;
    }
    if (out_evals) ZKT_HIP(c, hipMemcpyAsync(ev.data(), K->evals.p, (size_t)k * 32, hipMemcpyDeviceToHost, c->stream));
    ZKT_HIP(c, hipStreamSynchronize(c->stream));
    memcpy(out_w, w.data(), W * 8);
    if (out_inf) *out_inf = inf;
    if (out_evals) memcpy(out_evals, ev.data(), ev.size() * 8);
    return ZKT_OK;
}

}  // namespace zkt

using namespace zkt;

extern "C" {

int zkt_kzg_commit_batch(zkt_ctx* c, const uint64_t* const* coeffs, const size_t* lens, int k, int scalars_montgomery,
                         uint64_t* out_xy_mont, int* out_is_infinity) {
    return kzg_commit(c, (const void* const*)coeffs, true, lens, k, scalars_montgomery, out_xy_mont, out_is_infinity);
}
int zkt_kzg_commit_batch_dev(zkt_ctx* c, const void* const* d_coeffs, const size_t* lens, int k, int scalars_montgomery,
                             uint64_t* out_xy_mont, int* out_is_infinity) {
    return kzg_commit(c, d_coeffs, false, lens, k, scalars_montgomery, out_xy_mont, out_is_infinity);
}
int zkt_kzg_open(zkt_ctx* c, const uint64_t* const* coeffs, const size_t* lens, int k, const uint64_t* challenges_mont,
                 const uint64_t* point_mont, uint64_t* out_w_xy_mont, int* out_w_is_infinity, uint64_t* out_evals_mont) {
    return kzg_open(c, (const void* const*)coeffs, true, lens, k, challenges_mont, point_mont, out_w_xy_mont, out_w_is_infinity,
                    out_evals_mont);
}
int zkt_kzg_open_dev(zkt_ctx* c, const void* const* d_coeffs, const size_t* lens, int k, const uint64_t* challenges_mont,
                     const uint64_t* point_mont, uint64_t* out_w_xy_mont, int* out_w_is_infinity, uint64_t* out_evals_mont) {
    return kzg_open(c, d_coeffs, false, lens, k, challenges_mont, point_mont, out_w_xy_mont, out_w_is_infinity, out_evals_mont);
}

}  // extern "C"
