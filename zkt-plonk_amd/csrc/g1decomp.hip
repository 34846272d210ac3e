// zkt_g1_decompress: checked GroupAffine::deserialize of ark-serialize 0.3 for a batch of compressed G1 points, one thread
// per point.  The rules are those of decompress<C> in verify.hip (the host verifier's), restated for the device; the two
// agree on every input, status for refusal:
//   - the last byte carries SWFlags: bit 7 = "y is the larger root" (PositiveY), bit 6 = infinity; both set is refused (3);
//   - the remaining bits are x as a little-endian integer, which must be below the modulus (2) -- under the infinity flag
//     as well, where it is then ignored and the point is the identity (1);
//   - rhs = x^3 + b must be a square (4): both base fields have q = 3 mod 4, so y = rhs^((q + 1) / 4) and y^2 == rhs decides;
//   - of the two roots the flag picks the larger or the smaller one as canonical integers;
//   - the point must lie in the prime-order subgroup (5; BLS12-381 only, BN254 has cofactor one).
// The input is untrusted: a thread reads its own nb bytes and writes its own point and status byte, nothing is indexed
// by data, and every refusal is a status.
//
// Subgroup test (g1_in_subgroup of verify.hip): BLS12-381's sigma(x, y) = (beta x, y), beta = 2^((q - 1) / 3), acts on G1
// as [-x^2] (x the curve parameter), and sigma(P) = [-x^2] P holds ONLY on G1: (sigma + x^2)(sigma - x^2 + 1) =
// sigma^2 + sigma + 1 - r = -r as endomorphisms.  Two multiplications by the 64-bit |x| on the XYZZ routines of ecx.hpp,
// then beta x ZZ == X and -y ZZZ == Y on [x^2] P = (X, Y, ZZ, ZZZ).
//
// Resources (gfx950, docs/EXPERIMENTS.md "g1 decompression"): no scratch on either curve.
#include "g1decomp.hpp"

#include <cstring>
#include <vector>

namespace zkt {

constexpr int G1D_THREADS = 64;   // one wave per workgroup: a batch of a few thousand points spreads over every CU

template <class C>
__global__ __launch_bounds__(G1D_THREADS) void k_g1_decompress(const uint4* __restrict__ in, uint32_t n,
                                                               Affine<typename C::Fq>* __restrict__ out,
                                                               uint8_t* __restrict__ status, Fx<typename C::Fq> beta) {
    using Q = typename C::Fq;
    constexpr int N = Q::N;
    const uint32_t i = blockIdx.x * G1D_THREADS + threadIdx.x;
    if (i >= n) return;
    Fe<Q> xw;
#pragma unroll
    for (int k = 0; k < N / 4; ++k) {
        const uint4 v = in[(size_t)i * (N / 4) + k];
        xw.v[4 * k] = v.x; xw.v[4 * k + 1] = v.y; xw.v[4 * k + 2] = v.z; xw.v[4 * k + 3] = v.w;
    }
    Fe<Q> ox, oy;
    const uint32_t st = g1d_point<C>(xw, beta, &ox, &oy);
    fe_store<Q>(&out[i].x, ox);
    fe_store<Q>(&out[i].y, oy);
    status[i] = (uint8_t)st;
}

template <class C>
static int g1_decompress_launch(zkt_ctx* c, const void* d_in, size_t n, void* d_out, void* d_status) {
    using Q = typename C::Fq;
    static const Fx<Q> beta = C::ID == 1 ? g1d_beta<Q>() : fx_zero<Q>();
    const unsigned blocks = (unsigned)((n + G1D_THREADS - 1) / G1D_THREADS);
    hipLaunchKernelGGL(k_g1_decompress<C>, dim3(blocks), dim3(G1D_THREADS), 0, c->stream, (const uint4*)d_in, (uint32_t)n,
                       (Affine<Q>*)d_out, (uint8_t*)d_status, beta);
    ZKT_HIP(c, hipGetLastError());
    return ZKT_OK;
}

int g1_decompress_enqueue(zkt_ctx* c, const void* d_in, size_t n, void* d_out, void* d_status) {
    if (c->curve == ZKT_CURVE_BN254) return g1_decompress_launch<Bn254Curve>(c, d_in, n, d_out, d_status);
    return g1_decompress_launch<Bls381Curve>(c, d_in, n, d_out, d_status);
}

}  // namespace zkt

using namespace zkt;

extern "C" {

int zkt_g1_decompress_dev(zkt_ctx* c, const void* d_compressed, size_t n, void* d_out_xy_mont, void* d_out_status) {
    if (!c) return ZKT_ERR_INVALID_ARGUMENT;
    if (n > ZKT_G1_DECOMPRESS_MAX)
        return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "g1_decompress: more points than ZKT_G1_DECOMPRESS_MAX (2^22)");
    if (n == 0) return ZKT_OK;
    if (!d_compressed || !d_out_xy_mont || !d_out_status) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (((uintptr_t)d_compressed | (uintptr_t)d_out_xy_mont) & 15u)
        return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "g1_decompress: device buffers must be 16-byte aligned");
    (void)hipSetDevice(c->device);
    return g1_decompress_enqueue(c, d_compressed, n, d_out_xy_mont, d_out_status);
}

int zkt_g1_decompress(zkt_ctx* c, const uint8_t* compressed, size_t n, uint64_t* out_xy_mont, uint8_t* out_status) {
    if (!c) return ZKT_ERR_INVALID_ARGUMENT;
    if (n > ZKT_G1_DECOMPRESS_MAX)
        return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "g1_decompress: more points than ZKT_G1_DECOMPRESS_MAX (2^22)");
    if (n == 0) return ZKT_OK;
    if (!compressed || !out_xy_mont || !out_status) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    (void)hipSetDevice(c->device);
    const size_t nb = c->curve == ZKT_CURVE_BN254 ? 32 : 48;
    auto up = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t o_out = up(n * nb), o_st = o_out + up(n * 2 * nb);
    int rc = grow(c, c->verify_scratch, o_st + up(n));
    if (rc) return rc;
    char* const base = (char*)c->verify_scratch.p;
    ZKT_HIP(c, hipMemcpyAsync(base, compressed, n * nb, hipMemcpyHostToDevice, c->stream));
    if ((rc = g1_decompress_enqueue(c, base, n, base + o_out, base + o_st))) {
        (void)hipStreamSynchronize(c->stream);   // the upload reads the caller's memory
        return rc;
    }
    ZKT_HIP(c, hipMemcpyAsync(out_xy_mont, base + o_out, n * 2 * nb, hipMemcpyDeviceToHost, c->stream));
    ZKT_HIP(c, hipMemcpyAsync(out_status, base + o_st, n, hipMemcpyDeviceToHost, c->stream));
    ZKT_HIP(c, hipStreamSynchronize(c->stream));
    return ZKT_OK;
}

}  // extern "C"
