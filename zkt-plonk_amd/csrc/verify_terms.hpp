// The per-proof stage of the batch verifier between the decompression and the two MSMs (verify.hip stage 2 and the
// per-proof half of stage 4): the Fiat-Shamir replay of Verifier::terms, xi_point, compute_r0, the 13 linearisation
// scalars, both fold lists and the sums by source -- written once for the kernel of verify_terms.hip (one lane per proof,
// zkt_ctx_set_verify_terms(ctx, 1)) and for the host rehearsal (zkt_debug_verify_terms_host route 1).  The yardstick is
// the host route (transcript.cpp, Verifier::terms, batch_terms): every value here equals its value there.
//
// Memory.  A transcript is byte-addressed and a lane's position in it depends on its data, so nothing of it is a local
// array: the 25 sponge words, a 13-word message buffer and the 8 words of an Ethereum transcript's two states live
// behind a pointer and a stride (VtSponge) -- LDS laid out [word][lane] in the kernel, a plain array on the host -- and
// are reached by word index alone.  Keccak-f[1600] loads the 25 words into registers, permutes, and stores them back.
// Per-proof vectors (evaluations, public inputs, the sums) stay in the caller's memory and are indexed there.
#pragma once
#include "ctx.hpp"
#include "ec.hpp"
#include "linearisation.hpp"
#include "transcript.hpp"

namespace zkt {

#define ZKT_VT_FN static __host__ __device__ __attribute__((noinline))

constexpr int VT_THREADS = 64;
constexpr int VT_ST_WORDS = 25, VT_MSG_WORDS = 13, VT_ETH_WORDS = 8;
constexpr int VT_LANE_WORDS = VT_ST_WORDS + VT_MSG_WORDS + VT_ETH_WORDS;
constexpr uint32_t VT_RATE = 166;                       // STROBE-128: 200 - 128 / 4 - 2
constexpr uint32_t VT_FLAG_I = 1, VT_FLAG_A = 2, VT_FLAG_C = 4, VT_FLAG_M = 16, VT_FLAG_K = 32;

// word w of the sponge is st[w * stride], of the message buffer msg[w * stride], of the Ethereum states eth[w * stride]
struct VtSponge {
    uint64_t *st, *msg, *eth;
    uint32_t stride;
};
// a transcript at work: TranscriptState with its bytes in a VtSponge
struct VtTr {
    VtSponge s;
    uint32_t kind, pos, pos_begin, cur_flags, counter;
};

ZKT_HD uint32_t vt_get_byte(const uint64_t* a, uint32_t stride, uint32_t at) {
    return (uint32_t)(a[(at >> 3) * stride] >> (8 * (at & 7))) & 0xffu;
}
ZKT_HD void vt_xor_byte(uint64_t* a, uint32_t stride, uint32_t at, uint32_t b) {
    a[(at >> 3) * stride] ^= (uint64_t)(b & 0xffu) << (8 * (at & 7));
}
ZKT_HD void vt_set_byte(uint64_t* a, uint32_t stride, uint32_t at, uint32_t b) {
    const int sh = 8 * (at & 7);
    uint64_t& w = a[(at >> 3) * stride];
    w = (w & ~((uint64_t)0xff << sh)) | ((uint64_t)(b & 0xffu) << sh);
}

// ---- Keccak-f[1600] (transcript.cpp keccak_f1600, the same tables) ------------------------------------------------
struct VtK {
    ZKT_HD static constexpr uint64_t rc(int i) {
        constexpr uint64_t t[24] = {
            0x0000000000000001ULL, 0x0000000000008082ULL, 0x800000000000808aULL, 0x8000000080008000ULL,
            0x000000000000808bULL, 0x0000000080000001ULL, 0x8000000080008081ULL, 0x8000000000008009ULL,
            0x000000000000008aULL, 0x0000000000000088ULL, 0x0000000080008009ULL, 0x000000008000000aULL,
            0x000000008000808bULL, 0x800000000000008bULL, 0x8000000000008089ULL, 0x8000000000008003ULL,
            0x8000000000008002ULL, 0x8000000000000080ULL, 0x000000000000800aULL, 0x800000008000000aULL,
            0x8000000080008081ULL, 0x8000000000008080ULL, 0x0000000080000001ULL, 0x8000000080008008ULL};
        return t[i];
    }
    ZKT_HD static constexpr int rot(int i) {   // every offset is in 1 .. 63
        constexpr int t[24] = {1, 3, 6, 10, 15, 21, 28, 36, 45, 55, 2, 14, 27, 41, 56, 8, 25, 43, 62, 18, 39, 61, 20, 44};
        return t[i];
    }
    ZKT_HD static constexpr int pil(int i) {
        constexpr int t[24] = {10, 7, 11, 17, 18, 3, 5, 16, 8, 21, 24, 4, 15, 23, 19, 13, 12, 2, 20, 14, 22, 9, 6, 1};
        return t[i];
    }
};
ZKT_HD uint64_t vt_rotl(uint64_t x, int n) { return (x << n) | (x >> (64 - n)); }   // 1 <= n <= 63

ZKT_VT_FN void vt_keccak_f1600(uint64_t* st, uint32_t stride) {
    uint64_t a[25];
#pragma unroll
    for (int i = 0; i < 25; ++i) a[i] = st[i * stride];
#pragma nounroll
    for (int round = 0; round < 24; ++round) {
        uint64_t c[5];
#pragma unroll
        for (int x = 0; x < 5; ++x) c[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];
#pragma unroll
        for (int x = 0; x < 5; ++x) {
            const uint64_t d = c[(x + 4) % 5] ^ vt_rotl(c[(x + 1) % 5], 1);
#pragma unroll
            for (int y = 0; y < 25; y += 5) a[y + x] ^= d;
        }
        uint64_t cur = a[1];
#pragma unroll
        for (int i = 0; i < 24; ++i) {
            const uint64_t tmp = a[VtK::pil(i)];
            a[VtK::pil(i)] = vt_rotl(cur, VtK::rot(i));
            cur = tmp;
        }
#pragma unroll
        for (int y = 0; y < 25; y += 5) {
            const uint64_t r0 = a[y], r1 = a[y + 1], r2 = a[y + 2], r3 = a[y + 3], r4 = a[y + 4];
            a[y] = r0 ^ (~r1 & r2);
            a[y + 1] = r1 ^ (~r2 & r3);
            a[y + 2] = r2 ^ (~r3 & r4);
            a[y + 3] = r3 ^ (~r4 & r0);
            a[y + 4] = r4 ^ (~r0 & r1);
        }
        a[0] ^= VtK::rc(round);
    }
#pragma unroll
    for (int i = 0; i < 25; ++i) st[i * stride] = a[i];
}

// ---- STROBE-128 as merlin uses it (transcript.cpp Strobe128) ------------------------------------------------------
ZKT_VT_FN void vt_run_f(VtTr& t) {
    vt_xor_byte(t.s.st, t.s.stride, t.pos, t.pos_begin);
    vt_xor_byte(t.s.st, t.s.stride, t.pos + 1, 0x04);
    vt_xor_byte(t.s.st, t.s.stride, VT_RATE + 1, 0x80);
    vt_keccak_f1600(t.s.st, t.s.stride);
    t.pos = 0;
    t.pos_begin = 0;
}
ZKT_HD void vt_absorb_byte(VtTr& t, uint32_t b) {
    vt_xor_byte(t.s.st, t.s.stride, t.pos, b);
    if (++t.pos == VT_RATE) vt_run_f(t);
}
ZKT_HD uint32_t vt_squeeze_byte(VtTr& t) {
    const uint32_t b = vt_get_byte(t.s.st, t.s.stride, t.pos);
    vt_set_byte(t.s.st, t.s.stride, t.pos, 0);
    if (++t.pos == VT_RATE) vt_run_f(t);
    return b;
}
ZKT_VT_FN void vt_begin_op(VtTr& t, uint32_t flags) {
    const uint32_t old_begin = t.pos_begin;
    t.pos_begin = t.pos + 1;
    t.cur_flags = flags;
    vt_absorb_byte(t, old_begin);
    vt_absorb_byte(t, flags);
    if ((flags & (VT_FLAG_C | VT_FLAG_K)) != 0 && t.pos != 0) vt_run_f(t);
}
// bytes [0, len) of the message buffer
ZKT_VT_FN void vt_absorb_msg(VtTr& t, uint32_t len) {
#pragma nounroll
    for (uint32_t i = 0; i < len; ++i) vt_absorb_byte(t, vt_get_byte(t.s.msg, t.s.stride, i));
}
// merlin's meta_ad(label || LE32(len)) in front of a message or a challenge
ZKT_VT_FN void vt_merlin_header(VtTr& t, const char* label, uint32_t len) {
    vt_begin_op(t, VT_FLAG_M | VT_FLAG_A);
#pragma nounroll
    for (const char* p = label; *p; ++p) vt_absorb_byte(t, (uint8_t)*p);
#pragma nounroll
    for (int i = 0; i < 4; ++i) vt_absorb_byte(t, len >> (8 * i));
}

// ---- EthereumTranscript (transcript.cpp EthereumHostTranscript) ---------------------------------------------------
// Keccak-256 (legacy padding 0x01) of tag || state0 || state1 || item, the item = bytes [off, off + len) of the message
// buffer in REVERSE order (the buffer holds little-endian values, the transcript hashes big-endian ones).  65 + len < 136.
ZKT_VT_FN void vt_eth_hash(VtTr& t, uint32_t tag, uint32_t off, uint32_t len, uint64_t out[4]) {
    uint64_t* st = t.s.st;
    const uint32_t sd = t.s.stride;
#pragma unroll
    for (int i = 0; i < 25; ++i) st[i * sd] = 0;
    vt_xor_byte(st, sd, 0, tag);
#pragma nounroll
    for (uint32_t i = 0; i < 64; ++i) vt_xor_byte(st, sd, 1 + i, vt_get_byte(t.s.eth, sd, i));
#pragma nounroll
    for (uint32_t i = 0; i < len; ++i) vt_xor_byte(st, sd, 65 + i, vt_get_byte(t.s.msg, sd, off + len - 1 - i));
    vt_xor_byte(st, sd, 65 + len, 0x01);
    vt_xor_byte(st, sd, 135, 0x80);
    vt_keccak_f1600(st, sd);
#pragma unroll
    for (int i = 0; i < 4; ++i) out[i] = st[i * sd];
}
ZKT_VT_FN void vt_eth_append(VtTr& t, uint32_t off, uint32_t len) {
    uint64_t n0[4], n1[4];
    vt_eth_hash(t, 0, off, len, n0);
    vt_eth_hash(t, 1, off, len, n1);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        t.s.eth[i * t.s.stride] = n0[i];
        t.s.eth[(4 + i) * t.s.stride] = n1[i];
    }
}
ZKT_HD uint64_t vt_bswap64(uint64_t x) {
    x = ((x & 0x00ff00ff00ff00ffULL) << 8) | ((x >> 8) & 0x00ff00ff00ff00ffULL);
    x = ((x & 0x0000ffff0000ffffULL) << 16) | ((x >> 16) & 0x0000ffff0000ffffULL);
    return (x << 32) | (x >> 32);
}

// ---- the TranscriptProtocol calls of Verifier::terms, on either kind ----------------------------------------------
// `count` scalars follow, 32 bytes each: ONE merlin message (transcript.rs:69-79), or one item each
ZKT_VT_FN void vt_tr_scalars_begin(VtTr& t, const char* label, uint64_t count) {
    if (t.kind != 0) return;
    vt_merlin_header(t, label, (uint32_t)(count * 32));
    vt_begin_op(t, VT_FLAG_A);
}
// one scalar: canonical, little-endian, in words 0 .. 3 of the message buffer
ZKT_VT_FN void vt_tr_scalars_item(VtTr& t) {
    if (t.kind == 0) vt_absorb_msg(t, 32);
    else vt_eth_append(t, 0, 32);
}
// a commitment: x || y || infinity byte in the message buffer, nb bytes per coordinate, the identity as (0, 1, true)
ZKT_VT_FN void vt_tr_commit_msg(VtTr& t, const char* label, uint32_t nb) {
    if (t.kind == 0) {
        vt_merlin_header(t, label, 2 * nb + 1);
        vt_begin_op(t, VT_FLAG_A);
        vt_absorb_msg(t, 2 * nb + 1);
    } else {
        vt_eth_append(t, 0, nb);
        vt_eth_append(t, nb, nb);
    }
}
// a challenge as eight canonical little-endian words: merlin (fr_bits + 7) / 8 - 1 bytes of prf (transcript.rs:102),
// ethereum the hash under tag 2 and the big-endian counter, reversed, its top byte masked with 0x1f
ZKT_VT_FN void vt_tr_challenge(VtTr& t, const char* label, uint32_t fr_bits, uint32_t out[8]) {
    uint64_t* msg = t.s.msg;
    const uint32_t sd = t.s.stride;
    if (t.kind == 0) {
        const uint32_t nbytes = (fr_bits + 7) / 8 - 1;
        vt_merlin_header(t, label, nbytes);
        vt_begin_op(t, VT_FLAG_I | VT_FLAG_A | VT_FLAG_C);
#pragma unroll
        for (int i = 0; i < 4; ++i) msg[i * sd] = 0;
#pragma nounroll
        for (uint32_t i = 0; i < nbytes; ++i) vt_xor_byte(msg, sd, i, vt_squeeze_byte(t));
    } else {
        uint64_t h[4];
        msg[0] = t.counter;
        vt_eth_hash(t, 2, 0, 4, h);
        ++t.counter;
#pragma unroll
        for (int i = 0; i < 4; ++i) msg[i * sd] = vt_bswap64(h[3 - i]);
        msg[3 * sd] &= 0x1fffffffffffffffULL;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint64_t w = msg[i * sd];
        out[2 * i] = (uint32_t)w;
        out[2 * i + 1] = (uint32_t)(w >> 32);
    }
}

ZKT_HD void vt_load_state(VtTr& t, const TranscriptState* in) {
    t.kind = in->kind;
    t.pos = in->pos < VT_RATE ? in->pos : 0;
    t.pos_begin = in->pos_begin <= VT_RATE ? in->pos_begin : 0;
    t.cur_flags = in->cur_flags;
    t.counter = in->counter;
    const uint64_t* w = reinterpret_cast<const uint64_t*>(in->bytes);
#pragma unroll
    for (int i = 0; i < VT_ST_WORDS; ++i) t.s.st[i * t.s.stride] = t.kind == 0 ? w[i] : 0;
#pragma unroll
    for (int i = 0; i < VT_ETH_WORDS; ++i) t.s.eth[i * t.s.stride] = t.kind == 0 ? 0 : w[i];
#pragma unroll
    for (int i = 0; i < VT_MSG_WORDS; ++i) t.s.msg[i * t.s.stride] = 0;
}
ZKT_HD void vt_store_state(const VtTr& t, TranscriptState* out) {
    out->kind = t.kind;
    out->pos = t.pos;
    out->pos_begin = t.pos_begin;
    out->cur_flags = t.cur_flags;
    out->counter = t.counter;
    uint64_t* w = reinterpret_cast<uint64_t*>(out->bytes);
#pragma unroll
    for (int i = 0; i < VT_ST_WORDS; ++i)
        w[i] = t.kind == 0 ? t.s.st[i * t.s.stride] : (i < VT_ETH_WORDS ? t.s.eth[i * t.s.stride] : 0);
}

// ---- field elements into the message buffer -----------------------------------------------------------------------
template <class P>
ZKT_HD void vt_msg_put(VtTr& t, int word, const Fe<P>& canonical) {
#pragma unroll
    for (int i = 0; i < P::N / 2; ++i)
        t.s.msg[(word + i) * t.s.stride] = (uint64_t)canonical.v[2 * i] | ((uint64_t)canonical.v[2 * i + 1] << 32);
}
template <class R>
ZKT_HD void vt_scalar(VtTr& t, const char* label, const Fe<R>& mont) {
    vt_tr_scalars_begin(t, label, 1);
    vt_msg_put<R>(t, 0, fe_from_mont<R>(mont));
    vt_tr_scalars_item(t);
}
template <class Q>
__host__ __device__ __attribute__((noinline)) void vt_commit(VtTr& t, const char* label, const Affine<Q>* point) {
    const Affine<Q> a = *point;
    const bool inf = aff_is_inf<Q>(a);
    Fe<Q> x = fe_zero<Q>(), y = fe_zero<Q>();
    if (inf) {
        y.v[0] = 1;
    } else {
        x = fe_from_mont<Q>(a.x);
        y = fe_from_mont<Q>(a.y);
    }
    vt_msg_put<Q>(t, 0, x);
    vt_msg_put<Q>(t, Q::N / 2, y);
    t.s.msg[Q::N * t.s.stride] = inf ? 1 : 0;
    vt_tr_commit_msg(t, label, Q::N * 4);
}
template <class R>
__host__ __device__ __attribute__((noinline)) Fe<R> vt_challenge(VtTr& t, const char* label) {
    uint32_t w[8];
    vt_tr_challenge(t, label, R::BITS, w);
    Fe<R> c;
#pragma unroll
    for (int i = 0; i < 8; ++i) c.v[i] = w[i];
    return fe_to_mont<R>(c);
}
// EV_LABEL of linearisation.hpp, reachable from the device
ZKT_HD const char* vt_ev_label(int k) {
    switch (k) {
        case EV_A: return "a_eval";
        case EV_B: return "b_eval";
        case EV_C: return "c_eval";
        case EV_S1: return "sigma1_eval";
        case EV_S2: return "sigma2_eval";
        case EV_Z1N: return "z1_next_eval";
        case EV_QL: return "q_lookup_eval";
        case EV_T: return "t_eval";
        case EV_TN: return "t_next_eval";
        case EV_Z2N: return "z2_next_eval";
        case EV_H1N: return "h1_next_eval";
        default: return "h2_eval";
    }
}

// ---- the scalar stage ---------------------------------------------------------------------------------------------
template <class R>
__host__ __device__ __attribute__((noinline)) Fe<R> vt_inv(const Fe<R>& a) { return fe_inv<R>(a); }
template <class R>
ZKT_HD Fe<R> vt_from_u64(uint64_t x) {
    Fe<R> a = fe_zero<R>();
    a.v[0] = (uint32_t)x;
    a.v[1] = (uint32_t)(x >> 32);
    return fe_to_mont<R>(a);
}
// xi_point of linearisation.hpp with the kernels' inversion (an inverse is one value, whoever computes it)
template <class R>
ZKT_HD bool vt_xi_point(const Challenges<R>& ch, uint64_t n, XiPoint<R>& at) {
    const Fe<R> one = fe_one<R>();
    at.zh = fe_sub<R>(fe_pow_u64<R>(ch.xi, n), one);
    at.nn = vt_from_u64<R>(n);
    at.a2 = fe_sqr<R>(ch.alpha); at.a3 = fe_mul<R>(at.a2, ch.alpha);
    at.a4 = fe_mul<R>(at.a3, ch.alpha); at.a5 = fe_mul<R>(at.a4, ch.alpha);
    at.eopd = fe_mul<R>(ch.epsilon, fe_add<R>(ch.delta, one));
    const Fe<R> l1den = fe_mul<R>(at.nn, fe_sub<R>(ch.xi, one));
    if (fe_is_zero<R>(l1den)) return false;
    at.l1 = fe_mul<R>(at.zh, vt_inv<R>(l1den));
    return true;
}
// compute_r0 of linearisation.hpp without an allocation: before[] (k elements, the caller's) keeps the running products,
// a denominator is formed again on the way back
template <class R>
ZKT_HD bool vt_compute_r0(const Challenges<R>& ch, const XiPoint<R>& at, const Fe<R>* ev, const Fe<R>* roots, const Fe<R>* vals,
                          uint64_t k, Fe<R>* before, Fe<R>* out) {
    typedef Fe<R> F;
    F r0 = fe_zero<R>();
    bool zero_den = false;
    F run_prod = fe_one<R>();
#pragma nounroll
    for (uint64_t i = 0; i < k; ++i) {
        const F den = fe_mul<R>(at.nn, fe_sub<R>(ch.xi, roots[i]));
        before[i] = run_prod;
        if (!fe_is_zero<R>(den)) run_prod = fe_mul<R>(run_prod, den);
    }
    F inv_all = k ? vt_inv<R>(run_prod) : run_prod;
#pragma nounroll
    for (uint64_t i = k; i-- > 0;) {
        const F root = roots[i], val = vals[i];
        const F den = fe_mul<R>(at.nn, fe_sub<R>(ch.xi, root));
        if (fe_is_zero<R>(den)) {
            zero_den = true;
            r0 = fe_sub<R>(r0, val);
            continue;
        }
        const F di = fe_mul<R>(inv_all, before[i]);
        inv_all = fe_mul<R>(inv_all, den);
        r0 = fe_sub<R>(r0, fe_mul<R>(fe_mul<R>(fe_mul<R>(at.zh, root), di), val));
    }
    const F &beta = ch.beta, &gamma = ch.gamma, &delta = ch.delta;
    F p2 = fe_mul<R>(ch.alpha, ev[EV_Z1N]);
    p2 = fe_mul<R>(p2, fe_add<R>(fe_add<R>(ev[EV_A], fe_mul<R>(beta, ev[EV_S1])), gamma));
    p2 = fe_mul<R>(p2, fe_add<R>(fe_add<R>(ev[EV_B], fe_mul<R>(beta, ev[EV_S2])), gamma));
    p2 = fe_mul<R>(p2, fe_add<R>(ev[EV_C], gamma));
    F p4 = fe_mul<R>(at.a3, ev[EV_Z2N]);
    p4 = fe_mul<R>(p4, fe_add<R>(at.eopd, fe_mul<R>(delta, ev[EV_H2])));
    p4 = fe_mul<R>(p4, fe_add<R>(fe_add<R>(at.eopd, ev[EV_H2]), fe_mul<R>(delta, ev[EV_H1N])));
    *out = fe_add<R>(fe_add<R>(r0, p2), fe_add<R>(fe_mul<R>(at.l1, at.a2), fe_add<R>(p4, fe_mul<R>(at.l1, at.a4))));
    return zero_den;
}

// One proof.  Everything behind a pointer is the caller's memory (global memory in the kernel).
template <class C>
struct VtProof {
    using R = typename C::Fr;
    using Q = typename C::Fq;
    uint64_t n, n_pi;
    Fe<R> w;                    // the generator of the domain of n points, Montgomery
    Fe<R> rho[2];               // the proof's two coefficients, Montgomery
    const Affine<Q>* cm;        // 13 decompressed commitments, wire order
    const Fe<R>* ev;            // 12 evaluations, Montgomery
    const Fe<R>*roots, *vals;   // n_pi each, Montgomery
    const Fe<R>* forced;        // NULL, or 7 values that replace the drawn beta gamma delta epsilon alpha xi eta
    Fe<R>* before;              // n_pi elements of scratch
    Fe<R>* acc;                 // out: 24 sums by source (Verifier::SRC_*), all zero on a refusal
    Fe<R>* dbg;                 // NULL, or out: the challenges as far as they were drawn, then r0; the rest zero
};

// Verifier::terms and the sums of batch_terms.  Returns ZKT_OK, ZKT_ERR_EQUAL_CHALLENGES or ZKT_ERR_ZERO_DENOMINATOR; the
// transcript is left where the host route leaves it, also on a refusal.
template <class C>
__host__ __device__ __attribute__((noinline)) int vt_terms(VtTr& t, const VtProof<C>& p) {
    using R = typename C::Fr;
    using Q = typename C::Fq;
    using F = Fe<R>;
    enum { A, B, Cc, T, H1, H2, Z1, Z2, QLO, QMID, QHI, AW, SAW };
    enum { QM, QL, QR, QO, QC, S1, S2, S3, QLOOKUP, QTABLE };
    enum { SRC_CM = 0, SRC_VK = 13, SRC_G = 23, SRC_COUNT = 24 };
#pragma nounroll
    for (int s = 0; s < SRC_COUNT; ++s) p.acc[s] = fe_zero<R>();
    if (p.dbg) {
#pragma nounroll
        for (int s = 0; s < 8; ++s) p.dbg[s] = fe_zero<R>();
    }
    auto draw = [&](const char* label, int idx) {
        F c = vt_challenge<R>(t, label);
        if (p.forced) c = p.forced[idx];
        if (p.dbg) p.dbg[idx] = c;
        return c;
    };
    // ---- transcript (proof.rs:308-360) ----
    vt_tr_scalars_begin(t, "pi", p.n_pi);
#pragma nounroll
    for (uint64_t i = 0; i < p.n_pi; ++i) {
        vt_msg_put<R>(t, 0, fe_from_mont<R>(p.vals[i]));
        vt_tr_scalars_item(t);
    }
    vt_commit<Q>(t, "a_commit", p.cm + A); vt_commit<Q>(t, "b_commit", p.cm + B); vt_commit<Q>(t, "c_commit", p.cm + Cc);
    vt_commit<Q>(t, "t_commit", p.cm + T); vt_commit<Q>(t, "h1_commit", p.cm + H1); vt_commit<Q>(t, "h2_commit", p.cm + H2);
    const F beta = draw("beta", 0), gamma = draw("gamma", 1), delta = draw("delta", 2), epsilon = draw("epsilon", 3);
    if (fe_eq<R>(beta, gamma) || fe_eq<R>(beta, delta) || fe_eq<R>(beta, epsilon) || fe_eq<R>(gamma, delta) ||
        fe_eq<R>(gamma, epsilon) || fe_eq<R>(delta, epsilon))
        return ZKT_ERR_EQUAL_CHALLENGES;
    vt_commit<Q>(t, "z1_commit", p.cm + Z1); vt_commit<Q>(t, "z2_commit", p.cm + Z2);
    const F alpha = draw("alpha", 4);
    vt_commit<Q>(t, "q_lo_commit", p.cm + QLO); vt_commit<Q>(t, "q_mid_commit", p.cm + QMID); vt_commit<Q>(t, "q_hi_commit", p.cm + QHI);
    const F xi = draw("xi", 5);
    // ---- scalars; both refusals come before the evaluations are appended ----
    const Challenges<R> ch{beta, gamma, delta, epsilon, alpha, xi, fe_zero<R>()};
    XiPoint<R> at;
    if (!vt_xi_point<R>(ch, p.n, at)) return ZKT_ERR_ZERO_DENOMINATOR;
    F r0;
    if (vt_compute_r0<R>(ch, at, p.ev, p.roots, p.vals, p.n_pi, p.before, &r0)) return ZKT_ERR_ZERO_DENOMINATOR;
    F ev[EV_COUNT];
#pragma unroll
    for (int k = 0; k < EV_COUNT; ++k) ev[k] = p.ev[k];
    F sc[LIN_COUNT];
    linearisation_scalars<R>(ch, at, ev, sc);
#pragma nounroll
    for (int k = 0; k < EV_COUNT; ++k) vt_scalar<R>(t, vt_ev_label(k), p.ev[k]);
    const F eta = draw("eta", 6);
    if (p.dbg) p.dbg[7] = r0;
    // ---- both openings' terms, each times its rho, added up by source ----
    auto add = [&](int src, int o, const F& s) { p.acc[src] = fe_add<R>(p.acc[src], fe_mul<R>(p.rho[o], s)); };
    {
        constexpr int pt[13] = {SRC_VK + QM, SRC_VK + QL, SRC_VK + QR, SRC_VK + QO, SRC_VK + QC, SRC_CM + Z1, SRC_VK + S3, SRC_CM + Z2,
                                SRC_CM + H1, SRC_VK + QTABLE, SRC_CM + QLO, SRC_CM + QMID, SRC_CM + QHI};
#pragma unroll
        for (int k = 0; k < 13; ++k) add(pt[k], 0, sc[k]);
        constexpr int cs[8] = {SRC_CM + A, SRC_CM + B, SRC_CM + Cc, SRC_VK + S1, SRC_VK + S2, SRC_VK + QLOOKUP, SRC_CM + T, SRC_CM + H2};
        constexpr int vs[8] = {EV_A, EV_B, EV_C, EV_S1, EV_S2, EV_QL, EV_T, EV_H2};
        F c = eta, comb_v = r0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            add(cs[i], 0, c);
            comb_v = fe_add<R>(comb_v, fe_mul<R>(c, ev[vs[i]]));
            c = fe_mul<R>(c, eta);
        }
        add(SRC_G, 0, fe_neg<R>(comb_v));
        add(SRC_CM + AW, 0, xi);
    }
    {
        constexpr int cs[4] = {SRC_CM + Z1, SRC_CM + Z2, SRC_CM + T, SRC_CM + H1};
        constexpr int vs[4] = {EV_Z1N, EV_Z2N, EV_TN, EV_H1N};
        F c = fe_one<R>(), comb_v = fe_zero<R>();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            add(cs[i], 1, c);
            comb_v = fe_add<R>(comb_v, fe_mul<R>(c, ev[vs[i]]));
            c = fe_mul<R>(c, eta);
        }
        add(SRC_G, 1, fe_neg<R>(comb_v));
        add(SRC_CM + SAW, 1, fe_mul<R>(xi, p.w));
    }
    return ZKT_OK;
}

// ---- the kernel's memory: one region of verify_scratch, every part a multiple of 256 bytes -------------------------
// what the host writes per proof in front of the packed vectors
template <class R>
struct alignas(16) VtDesc {
    uint64_t n, n_pi, pi_off, reserved;   // pi_off: where the proof's roots / values / scratch start in the packed arrays
    Fe<R> w, rho[2];
};
static_assert(sizeof(VtDesc<Bn254Fr>) == 128 && sizeof(VtDesc<Bls381Fr>) == 128, "vt_layout counts 128 bytes per description");
static_assert(sizeof(TranscriptState) == 232 && sizeof(TranscriptState) % 8 == 0, "the sponge is read as 64-bit words");
static_assert(8 * VT_MSG_WORDS >= 2 * 48 + 1, "the message buffer holds a BLS12-381 commitment");
struct VtLayout {
    // upload: desc .. states (the states included); download: states .. end of acc (or of dbg)
    size_t desc, ev, roots, vals, forced, states, status, acc, dbg, before, end;
};
inline VtLayout vt_layout(size_t start, size_t count, size_t total_pi, bool forced, bool dbg) {
    auto up = [](size_t b) { return (b + 255) / 256 * 256; };
    VtLayout l;
    l.desc = up(start);
    l.ev = l.desc + up(count * 128);
    l.roots = l.ev + up(count * 12 * 32);
    l.vals = l.roots + up(total_pi * 32);
    l.forced = l.vals + up(total_pi * 32);
    l.states = l.forced + up(forced ? count * 7 * 32 : 0);
    l.status = l.states + up(count * sizeof(TranscriptState));
    l.acc = l.status + up(count * 4);
    l.dbg = l.acc + up(count * 24 * 32);
    l.before = l.dbg + up(dbg ? count * 8 * 32 : 0);
    l.end = l.before + up(total_pi * 32);
    return l;
}
// Enqueue on the context's stream, no synchronisation: one lane per proof over the region at d_base laid out by `lay`
// (forced / dbg as the layout was made), d_points the 13 * count decompressed commitments.
int verify_terms_enqueue(zkt_ctx* c, void* d_base, const VtLayout& lay, const void* d_points, size_t count, bool forced, bool dbg);

}  // namespace zkt
