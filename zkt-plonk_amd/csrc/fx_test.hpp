// Raw-limb test dispatch over the routines of fx.hpp and ecx.hpp (zkt_host_fx_op / zkt_debug_fx_op and the xyzz pair in
// capi.hip).  The same __host__ __device__ dispatcher runs in a host loop and in a plain kernel, one record per thread, so
// the host build executes the #else branches of the products and the device build the ordered v_mad_u64_u32 chains.
// Operands are taken as the caller wrote them: nothing is normalised on the way in, so a test can hand a product a lazy
// operand with limbs above 2^29.
//
// fx record:   in  = a, b, c, d (L words each; a packed operand uses the first N words of its slot)
//              out = up to 4 L words (a packed result in the first N, a predicate in word 0), the rest zero
// xyzz record: in  = two points of 4 L + 1 words: x, y, zz, zzz (L each) and an identity word; an affine operand uses
//              the x, y slots of its point.  out = one such point.
#pragma once
#include "../../include/zkt_plonk.h"
#include "ecx.hpp"

namespace zkt {

template <class P>
ZKT_HD Fx<P> fxt_load(const uint32_t* s) {
    Fx<P> r;
#pragma unroll
    for (int i = 0; i < FxP<P>::L; ++i) r.l[i] = s[i];
    return r;
}
template <class P>
ZKT_HD void fxt_store(uint32_t* d, const Fx<P>& a) {
#pragma unroll
    for (int i = 0; i < FxP<P>::L; ++i) d[i] = a.l[i];
}
template <class P>
ZKT_HD Fe<P> fxt_load_fe(const uint32_t* s) {
    Fe<P> r;
#pragma unroll
    for (int i = 0; i < P::N; ++i) r.v[i] = s[i];
    return r;
}
template <class P>
ZKT_HD void fxt_store_fe(uint32_t* d, const Fe<P>& a) {
#pragma unroll
    for (int i = 0; i < P::N; ++i) d[i] = a.v[i];
}

// fx_reduce_lazy estimates the quotient from the top limb of p, which is too narrow on the 381-bit field; the Shoup
// product's columns of nine 2^31.33 x 2^29 terms would overflow 64 bits with fourteen limbs (it serves the scalar fields)
template <class P>
constexpr bool fx_test_op_valid(int op) {
    if (op < 0 || op >= ZKT_FX_OP_COUNT) return false;
    if (op == ZKT_FX_REDUCE_LAZY) return FxP<P>::mod(FxP<P>::L - 1) >= (1u << 16);
    if (op == ZKT_FX_MUL_SHOUP) return FxP<P>::L <= 9;
    return true;
}

template <class P>
ZKT_HD void fx_test_op(int op, const uint32_t* in, uint32_t* out) {
    constexpr int L = FxP<P>::L;
    const Fx<P> a = fxt_load<P>(in), b = fxt_load<P>(in + L), c = fxt_load<P>(in + 2 * L), d = fxt_load<P>(in + 3 * L);
    for (int i = 0; i < 4 * L; ++i) out[i] = 0;
    switch (op) {
        case ZKT_FX_UNPACK: fxt_store<P>(out, fx_unpack<P>(fxt_load_fe<P>(in))); break;
        case ZKT_FX_UNPACK_SHIFT: fxt_store<P>(out, fx_unpack_shift<P>(fxt_load_fe<P>(in))); break;
        case ZKT_FX_PACK: fxt_store_fe<P>(out, fx_pack<P>(a)); break;
        case ZKT_FX_FROM_ARK: fxt_store<P>(out, fx_from_ark<P>(fxt_load_fe<P>(in))); break;
        case ZKT_FX_TO_ARK: fxt_store_fe<P>(out, fx_to_ark<P>(a)); break;
        case ZKT_FX_NORMALIZE: fxt_store<P>(out, fx_normalize<P>(a)); break;
        case ZKT_FX_ADD: fxt_store<P>(out, fx_add<P>(a, b)); break;
        case ZKT_FX_DBL: fxt_store<P>(out, fx_dbl<P>(a)); break;
        case ZKT_FX_SUB_1: fxt_store<P>(out, fx_sub<P, 1>(a, b)); break;
        case ZKT_FX_SUB_2: fxt_store<P>(out, fx_sub<P, 2>(a, b)); break;
        case ZKT_FX_SUB_4: fxt_store<P>(out, fx_sub<P, 4>(a, b)); break;
        case ZKT_FX_SUB_8: fxt_store<P>(out, fx_sub<P, 8>(a, b)); break;
        case ZKT_FX_SUB2_6: fxt_store<P>(out, fx_sub2<P, 6>(a, b, c)); break;
        case ZKT_FX_ADD_LAZY: fxt_store<P>(out, fx_add_lazy<P>(a, b)); break;
        case ZKT_FX_SUB_LAZY_3: fxt_store<P>(out, fx_sub_lazy<P, 3>(a, b)); break;
        case ZKT_FX_SUB_LAZY_4: fxt_store<P>(out, fx_sub_lazy<P, 4>(a, b)); break;
        case ZKT_FX_SUB_LAZY_5: fxt_store<P>(out, fx_sub_lazy<P, 5>(a, b)); break;
        case ZKT_FX_SUB_LAZY_9: fxt_store<P>(out, fx_sub_lazy<P, 9>(a, b)); break;
        case ZKT_FX_SUB_LAZY_WIDE_8_30: fxt_store<P>(out, fx_sub_lazy_wide<P, 8, 30>(a, b)); break;
        case ZKT_FX_MUL: fxt_store<P>(out, fx_mul<P>(a, b)); break;
        case ZKT_FX_MUL_INL: fxt_store<P>(out, fx_mul_inl<P>(a, b)); break;
        case ZKT_FX_SQR: fxt_store<P>(out, fx_sqr<P>(a)); break;
        case ZKT_FX_SQR_INL: fxt_store<P>(out, fx_sqr_inl<P>(a)); break;
        case ZKT_FX_MUL2_INL: fxt_store<P>(out, fx_mul2_inl<P>(a, b, c, d)); break;
        case ZKT_FX_MUL_SHOUP:
            if constexpr (fx_test_op_valid<P>(ZKT_FX_MUL_SHOUP)) fxt_store<P>(out, fx_mul_shoup<P>(a, b, c));
            break;
        case ZKT_FX_MUL_LOW: fxt_store<P>(out, fx_mul_low<P>(a, b)); break;
        case ZKT_FX_REDUCE_SMALL: fxt_store<P>(out, fx_reduce_small<P>(a)); break;
        case ZKT_FX_REDUCE_LAZY:
            if constexpr (fx_test_op_valid<P>(ZKT_FX_REDUCE_LAZY)) fxt_store<P>(out, fx_reduce_lazy<P>(a));
            break;
        case ZKT_FX_COND_SUB_P: fxt_store<P>(out, fx_cond_sub_p<P>(a)); break;
        case ZKT_FX_CANON: fxt_store<P>(out, fx_canon<P>(a)); break;
        case ZKT_FX_IS_ZERO_CANON: out[0] = fx_is_zero_canon<P>(a) ? 1u : 0u; break;
        case ZKT_FX_IS_ZERO_LT2P: out[0] = fx_is_zero_lt2p<P>(a) ? 1u : 0u; break;
        default: break;
    }
}

template <class Q>
ZKT_HD XyzzX<Q> xxt_load(const uint32_t* s) {
    constexpr int L = FxP<Q>::L;
    XyzzX<Q> r;
    r.x = fxt_load<Q>(s);
    r.y = fxt_load<Q>(s + L);
    r.zz = fxt_load<Q>(s + 2 * L);
    r.zzz = fxt_load<Q>(s + 3 * L);
    r.inf = s[4 * L] != 0;
    return r;
}
template <class Q>
ZKT_HD void xxt_store(uint32_t* d, const XyzzX<Q>& a) {
    constexpr int L = FxP<Q>::L;
    fxt_store<Q>(d, a.x);
    fxt_store<Q>(d + L, a.y);
    fxt_store<Q>(d + 2 * L, a.zz);
    fxt_store<Q>(d + 3 * L, a.zzz);
    d[4 * L] = a.inf ? 1u : 0u;
}

template <class Q>
ZKT_HD void xyzz_test_op(int op, const uint32_t* in, uint32_t* out) {
    constexpr int W = 4 * FxP<Q>::L + 1;
    const XyzzX<Q> p = xxt_load<Q>(in), q = xxt_load<Q>(in + W);
    AffineX<Q> pa, qa;
    pa.x = p.x;
    pa.y = p.y;
    qa.x = q.x;
    qa.y = q.y;
    XyzzX<Q> r = xx_identity<Q>();
    switch (op) {
        case ZKT_XYZZ_ADD_MIXED: r = xx_add_mixed<Q, false>(p, qa); break;
        case ZKT_XYZZ_ADD_MIXED_INL: r = xx_add_mixed<Q, true>(p, qa); break;
        case ZKT_XYZZ_ADD: r = xx_add<Q, false>(p, q); break;
        case ZKT_XYZZ_ADD_INL: r = xx_add<Q, true>(p, q); break;
        case ZKT_XYZZ_DOUBLE: r = xx_double<Q>(p); break;
        case ZKT_XYZZ_DOUBLE_AFFINE: r = xx_double_affine<Q>(pa); break;
        default: break;
    }
    xxt_store<Q>(out, r);
}

}  // namespace zkt
