// Batched checked deserialisation of compressed G1 points on the device (g1decomp.hip): the per-point arithmetic on the
// 29-bit limbs of fx.hpp and the XYZZ routines of ecx.hpp, every function with its limb bounds, and the enqueue entry.
#pragma once
#include "ctx.hpp"
#include "ec.hpp"
#include "ecx.hpp"

namespace zkt {

// (q + 1) / 4 as 32-bit words (q = 3 mod 4, and every modulus here leaves a spare bit, so q + 1 cannot overflow)
template <class Q>
constexpr Words<Q::N> g1d_sqrt_exponent() {
    Words<Q::N> m = words_modulus<Q>();
    uint32_t carry = 1;
    for (int i = 0; i < Q::N; ++i) {
        const uint64_t x = (uint64_t)m.w[i] + carry;
        m.w[i] = (uint32_t)x;
        carry = (uint32_t)(x >> 32);
    }
    Words<Q::N> r{};
    for (int i = 0; i < Q::N; ++i) r.w[i] = (m.w[i] >> 2) | (i + 1 < Q::N ? m.w[i + 1] << 30 : 0u);
    return r;
}
template <class Q>
struct G1dK {
    static_assert((Q::mod(0) & 3u) == 3u, "sqrt by one exponentiation needs q = 3 mod 4");
    ZKT_HD static constexpr uint32_t sqrt_exp(int w) {
        constexpr Words<Q::N> e = g1d_sqrt_exponent<Q>();
        return e.w[w];
    }
    // R'^2 mod q, limb i: fx_mul(x, this) takes a canonical integer x to its R' Montgomery form
    ZKT_HD static constexpr uint32_t rr(int i) {
        constexpr Words<Q::N> v = pow2_mod<Q>(2 * 29 * FxP<Q>::L);
        return FxP<Q>::limb_of(v, i);
    }
};

// a >= q for normalised limbs, value < 2^(29 L)
template <class Q>
ZKT_HD bool fx_geq_p(const Fx<Q>& a) {
    constexpr int L = FxP<Q>::L;
    int32_t c = 0;
#pragma unroll
    for (int i = 0; i < L - 1; ++i) c = ((int32_t)a.l[i] - (int32_t)FxP<Q>::mod(i) + c) >> 29;
    return (int32_t)a.l[L - 1] - (int32_t)FxP<Q>::mod(L - 1) + c >= 0;
}
template <class Q>
ZKT_HD bool fx_eq_limbs(const Fx<Q>& a, const Fx<Q>& b) {   // both canonical
    uint32_t d = 0;
#pragma unroll
    for (int i = 0; i < FxP<Q>::L; ++i) d |= a.l[i] ^ b.l[i];
    return d == 0;
}

// a^((q + 1) / 4): plain square-and-multiply over all 32 N exponent bits, the same walk in every lane (the exponent is a
// compile-time constant held in scalar registers; the leading zero bits square the Montgomery one).
// In: a canonical (< q).  Every square is of a value < 2q (4 q^2 < R' q), every product 2q * q.  Out: < 2q, normalised.
template <class Q>
ZKT_HD Fx<Q> g1d_sqrt_candidate(const Fx<Q>& a) {
    Fx<Q> r = fx_one<Q>();
#pragma unroll
    for (int w = Q::N - 1; w >= 0; --w) {
        const uint32_t e = G1dK<Q>::sqrt_exp(w);
#pragma nounroll
        for (int b = 31; b >= 0; --b) {
            r = fx_mul<Q>(r, r);
            if ((e >> b) & 1u) r = fx_mul<Q>(r, a);
        }
    }
    return r;
}

// [|x|] p for BLS12-381's |x| = 0xd201000000010000: 63 doublings and 5 additions, the same in every lane.
// In / out: the bounds of XyzzX (ecx.hpp).
template <class Q>
ZKT_HD XyzzX<Q> g1d_mul_x(const XyzzX<Q>& p) {
    const uint64_t xabs = 0xd201000000010000ULL;
    XyzzX<Q> acc = p;
#pragma nounroll
    for (int i = 62; i >= 0; --i) {
        acc = xx_double<Q>(acc);
        if ((xabs >> i) & 1) acc = xx_add<Q>(acc, p);
    }
    return acc;
}

// P = (x, y) affine, canonical, R' form, on the curve, not the identity: is P in G1?  In: x, y < q.
template <class Q>
ZKT_HD bool g1d_in_subgroup(const Fx<Q>& x, const Fx<Q>& y, const Fx<Q>& beta) {
    XyzzX<Q> acc;
    acc.x = x;
    acc.y = y;
    acc.zz = fx_one<Q>();
    acc.zzz = fx_one<Q>();
    acc.inf = false;
#pragma nounroll
    for (int rep = 0; rep < 2; ++rep) acc = g1d_mul_x<Q>(acc);   // [x^2] P: X < 8q, Y < 4q, ZZ, ZZZ < 2q
    if (acc.inf) return false;                                    // sigma(P) is never the identity
    const Fx<Q> lx = fx_mul<Q>(fx_mul<Q>(beta, x), acc.zz);       // q * q, then 2q * 2q; < 2q
    const Fx<Q> ny = fx_sub<Q, 1>(fx_zero<Q>(), y);               // q - y <= q
    const Fx<Q> ly = fx_mul<Q>(ny, acc.zzz);                      // q * 2q; < 2q
    return fx_eq_limbs<Q>(fx_canon<Q>(lx), fx_canon<Q>(acc.x)) && fx_eq_limbs<Q>(fx_canon<Q>(ly), fx_canon<Q>(acc.y));
}

// One point: the words of its nb bytes -> status; *ox, *oy = the point in arkworks' Montgomery form, (0, 0) unless the
// status is ZKT_G1_VALID.  beta: g1d_beta (BLS12-381; unused on BN254).  Host and device run the same code.
template <class C>
ZKT_HD uint32_t g1d_point(Fe<typename C::Fq> xw, const Fx<typename C::Fq>& beta, Fe<typename C::Fq>* ox, Fe<typename C::Fq>* oy) {
    using Q = typename C::Fq;
    constexpr int N = Q::N, L = FxP<Q>::L;
    const uint32_t flags = xw.v[N - 1] >> 30;     // bit 1: PositiveY, bit 0: infinity
    xw.v[N - 1] &= 0x3FFFFFFFu;
    *ox = fe_zero<Q>();
    *oy = fe_zero<Q>();
    const Fx<Q> xi = fx_unpack<Q>(xw);            // normalised; < 2^(32 N - 2) < 2^(29 L)
    if (flags == 3u) return ZKT_G1_BOTH_FLAGS;
    if (fx_geq_p<Q>(xi)) return ZKT_G1_NOT_CANONICAL;
    if (flags & 1u) return ZKT_G1_IDENTITY;
    Fx<Q> rr;
#pragma unroll
    for (int k = 0; k < L; ++k) rr.l[k] = G1dK<Q>::rr(k);
    const Fx<Q> x = fx_cond_sub_p<Q>(fx_mul<Q>(xi, rr));                     // q * q; canonical, R' form
    const Fx<Q> x3 = fx_mul<Q>(fx_mul<Q>(x, x), x);                          // q * q, 2q * q; < 2q
    Fx<Q> rhs = x3;
#pragma unroll
    for (uint32_t k = 0; k < C::B; ++k) rhs = fx_add<Q>(rhs, fx_one<Q>());   // b <= 4: < 6q
    rhs = fx_canon<Q>(rhs);
    Fx<Q> y = g1d_sqrt_candidate<Q>(rhs);                                    // < 2q
    if (!fx_eq_limbs<Q>(fx_cond_sub_p<Q>(fx_mul<Q>(y, y)), rhs)) return ZKT_G1_NOT_ON_CURVE;   // 4 q^2
    y = fx_cond_sub_p<Q>(y);
    // the flag speaks about y as an integer: y / R' (a product with the integer one), then 2y > q
    Fx<Q> unit = fx_zero<Q>();
    unit.l[0] = 1;
    const Fx<Q> yint = fx_cond_sub_p<Q>(fx_mul<Q>(y, unit));
    const bool larger = fx_geq_p<Q>(fx_dbl<Q>(yint));                        // 2y < 2q < 2^(29 L); q is odd, 2y != q
    if (larger != ((flags & 2u) != 0)) y = fx_cond_sub_p<Q>(fx_sub<Q, 1>(fx_zero<Q>(), y));   // q - y; y = 0 stays 0
    if constexpr (C::ID == 1) {
        if (!g1d_in_subgroup<Q>(x, y, beta)) return ZKT_G1_NOT_IN_SUBGROUP;
    }
    *ox = fx_to_ark<Q>(x);
    *oy = fx_to_ark<Q>(y);
    return ZKT_G1_VALID;
}

// One UNCOMPRESSED point (zkt_g1_check, g1check.hip): the raw words of x and y as zkt_srs_load takes them (arkworks'
// Montgomery limbs, (0, 0) = the identity) -> status, the first that applies of NOT_CANONICAL, IDENTITY, NOT_ON_CURVE,
// NOT_IN_SUBGROUP (BLS12-381), VALID.  No square root: y is given.  beta as in g1d_point.  Host and device run the same code.
template <class C>
ZKT_HD uint32_t g1c_point(const Fe<typename C::Fq>& xw, const Fe<typename C::Fq>& yw, const Fx<typename C::Fq>& beta) {
    using Q = typename C::Fq;
    static_assert(32 * Q::N <= 29 * FxP<Q>::L, "raw words fit the limbs");
    const Fx<Q> xi = fx_unpack<Q>(xw), yi = fx_unpack<Q>(yw);                // normalised; any words: < 2^(32 N) <= 2^(29 L)
    if (fx_geq_p<Q>(xi) || fx_geq_p<Q>(yi)) return ZKT_G1_NOT_CANONICAL;
    if (fx_is_zero_canon<Q>(xi) && fx_is_zero_canon<Q>(yi)) return ZKT_G1_IDENTITY;
    // the curve equation holds in one Montgomery form as in another; R' is the one fx_mul and g1d_in_subgroup work in
    const Fx<Q> x = fx_cond_sub_p<Q>(fx_mul<Q>(xi, fx_const_from_ark<Q>()));   // q * q; < 2q -> canonical, R' form
    const Fx<Q> y = fx_cond_sub_p<Q>(fx_mul<Q>(yi, fx_const_from_ark<Q>()));   // the same
    Fx<Q> rhs = fx_mul<Q>(fx_mul<Q>(x, x), x);                               // q * q, 2q * q; < 2q
#pragma unroll
    for (uint32_t k = 0; k < C::B; ++k) rhs = fx_add<Q>(rhs, fx_one<Q>());   // b <= 4: < 6q
    if (!fx_eq_limbs<Q>(fx_cond_sub_p<Q>(fx_mul<Q>(y, y)), fx_canon<Q>(rhs))) return ZKT_G1_NOT_ON_CURVE;   // q * q; < 2q
    if constexpr (C::ID == 1) {
        if (!g1d_in_subgroup<Q>(x, y, beta)) return ZKT_G1_NOT_IN_SUBGROUP;  // x, y < q, on the curve, not the identity
    }
    return ZKT_G1_VALID;
}

// beta = 2^((q - 1) / 3) in R' form, canonical (host, once per process)
template <class Q>
inline Fx<Q> g1d_beta() {
    uint32_t e[Q::N];
    uint64_t rem = 0;
    for (int i = Q::N - 1; i >= 0; --i) {
        const uint64_t cur = (rem << 32) | (uint64_t)(Q::mod(i) - (i == 0 ? 1u : 0u));
        e[i] = (uint32_t)(cur / 3);
        rem = cur % 3;
    }
    const Fe<Q> two = fe_from_u32<Q>(2);
    Fe<Q> r = fe_one<Q>();
    for (int i = Q::N * 32 - 1; i >= 0; --i) {
        r = fe_sqr<Q>(r);
        if ((e[i / 32] >> (i % 32)) & 1u) r = fe_mul<Q>(r, two);
    }
    return fx_cond_sub_p<Q>(fx_from_ark<Q>(r));
}

// Enqueues the decompression of n points on the context's stream: d_in = n x nb bytes, d_out = n affine points (x || y
// Montgomery limbs), d_status = n bytes (ZKT_G1_* of the public header).  All three device pointers, 16-byte aligned;
// 1 <= n <= ZKT_G1_DECOMPRESS_MAX is the caller's to check.  No synchronisation.
int g1_decompress_enqueue(zkt_ctx* c, const void* d_in, size_t n, void* d_out, void* d_status);

}  // namespace zkt
