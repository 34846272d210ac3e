// The transcripts' one implementation: Keccak-f[1600], STROBE-128 as merlin 3.0 uses it ("Merlin v1.0") and the
// Keccak-256 EthereumTranscript (gadgets/src/transcript.rs:8-90), written once for the kernel of verify_terms.hip (one
// lane per proof) and for the host's built-in transcripts (transcript.hip), which run it at a stride of one.
//
// Memory.  A transcript is byte-addressed and a lane's position in it depends on its data, so nothing of it is a local
// array: the 25 sponge words, a 13-word message buffer and the 8 words of an Ethereum transcript's two states live
// behind a pointer and a stride (VtSponge) -- LDS laid out [word][lane] in the kernel, a plain array on the host -- and
// are reached by word index alone.  Keccak-f[1600] loads the 25 words into registers, permutes, and stores them back.
// The message buffer bounds ONE item (a scalar, a commitment); a longer message streams through vt_absorb_byte.
#pragma once
#include "fp.hpp"

namespace zkt {

#define ZKT_VT_FN static __host__ __device__ __attribute__((noinline))

// A built-in transcript's whole state, as it crosses to the device and back.  kind 0, Merlin: bytes = the 200 bytes of the
// STROBE sponge, with pos / pos_begin / cur_flags.  kind 1, Ethereum: bytes[0 .. 64) = state0 || state1, with counter.
// The sponge is read as 25 little-endian 64-bit words.
struct alignas(8) TranscriptState {
    uint32_t kind = 0, pos = 0, pos_begin = 0, cur_flags = 0, counter = 0, reserved[3] = {0, 0, 0};
    uint8_t bytes[200] = {0};
};
static_assert(sizeof(TranscriptState) == 232 && sizeof(TranscriptState) % 8 == 0, "the sponge is read as 64-bit words");

constexpr int VT_ST_WORDS = 25, VT_MSG_WORDS = 13, VT_ETH_WORDS = 8;
constexpr int VT_LANE_WORDS = VT_ST_WORDS + VT_MSG_WORDS + VT_ETH_WORDS;
constexpr uint32_t VT_RATE = 166;                       // STROBE-128: 200 - 128 / 4 - 2
constexpr uint32_t VT_FLAG_I = 1, VT_FLAG_A = 2, VT_FLAG_C = 4, VT_FLAG_M = 16, VT_FLAG_K = 32;   // T = 8 (transport): never used by merlin
// One Keccak-256 block (rate 136) takes tag || state0 || state1 || item || padding: 65 + len + 1 <= 136.  Every item of
// the protocol is a little-endian value of at most 48 bytes or the 4-byte counter; a caller with other lengths checks this.
constexpr uint32_t VT_ETH_ITEM_MAX = 136 - 65 - 1;
static_assert(8 * VT_MSG_WORDS >= 2 * 48 + 1, "the message buffer holds a BLS12-381 commitment");

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

// ---- Keccak-f[1600] -----------------------------------------------------------------------------------------------
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
    // rho offsets and pi lanes in the usual "walk (x, y) -> (y, 2x + 3y)" order; every offset is in 1 .. 63
    ZKT_HD static constexpr int rot(int i) {
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

// ---- STROBE-128 as merlin uses it ---------------------------------------------------------------------------------
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

// ---- EthereumTranscript -------------------------------------------------------------------------------------------
// Keccak-256 (legacy padding 0x01, not FIPS-202's 0x06) of tag || state0 || state1 || item, the item = bytes
// [off, off + len) of the message buffer in REVERSE order (the buffer holds little-endian values, the transcript hashes
// big-endian ones).  len <= VT_ETH_ITEM_MAX.
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

// ---- the TranscriptProtocol calls (plonk-core/src/transcript.rs:46-109), on either kind ---------------------------
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
// a commitment: x || y || infinity byte in the message buffer (GroupAffine::write, transcript.rs:81-86), nb bytes per
// coordinate, the identity as (0, 1, true)
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

}  // namespace zkt
