// Host-side transcripts: Keccak-256 over whole messages and the built-in Merlin / Ethereum transcript, both on
// transcript_core.hpp at a stride of one, and the zkt_transcript_* C API over them.  See transcript.hpp for the reference
// files they mirror.
#include "transcript.hpp"
#include "../../include/zkt_plonk.h"

#include <cstring>

namespace zkt {

void keccak256(const uint8_t* data, size_t len, uint8_t out[32]) {
    const size_t rate = 136;
    uint64_t st[25] = {0};
    while (len >= rate) {
        for (uint32_t i = 0; i < rate; ++i) vt_xor_byte(st, 1, i, data[i]);
        vt_keccak_f1600(st, 1);
        data += rate;
        len -= rate;
    }
    for (uint32_t i = 0; i < len; ++i) vt_xor_byte(st, 1, i, data[i]);
    vt_xor_byte(st, 1, (uint32_t)len, 0x01);  // legacy Keccak padding (sha3::Keccak256), not FIPS-202's 0x06
    vt_xor_byte(st, 1, rate - 1, 0x80);
    vt_keccak_f1600(st, 1);
    memcpy(out, st, 32);
}

BuiltinTranscript::BuiltinTranscript(int kind, const char* label) {
    tr_.s = VtSponge{words_, words_ + VT_ST_WORDS, words_ + VT_ST_WORDS + VT_MSG_WORDS, 1};
    tr_.kind = (uint32_t)kind;
    tr_.pos = tr_.pos_begin = tr_.cur_flags = tr_.counter = 0;
    if (kind != 0) return;
    // Strobe128::new("Merlin v1.0"), then merlin's Transcript::new(label)
    const uint8_t init[18] = {1, (uint8_t)(VT_RATE + 2), 1, 0, 1, 96, 'S', 'T', 'R', 'O', 'B', 'E', 'v', '1', '.', '0', '.', '2'};
    for (uint32_t i = 0; i < sizeof init; ++i) vt_xor_byte(words_, 1, i, init[i]);
    vt_keccak_f1600(words_, 1);
    vt_begin_op(tr_, VT_FLAG_M | VT_FLAG_A);
    for (const char* p = "Merlin v1.0"; *p; ++p) vt_absorb_byte(tr_, (uint8_t)*p);
    append_message("dom-sep", reinterpret_cast<const uint8_t*>(label), strlen(label));
}

bool BuiltinTranscript::append_message(const char* label, const uint8_t* msg, size_t len) {
    if (tr_.kind != 0) return false;
    vt_merlin_header(tr_, label, (uint32_t)len);
    vt_begin_op(tr_, VT_FLAG_A);
    for (size_t i = 0; i < len; ++i) vt_absorb_byte(tr_, msg[i]);
    return true;
}
bool BuiltinTranscript::challenge_bytes(const char* label, uint8_t* out, size_t len) {
    if (tr_.kind != 0) return false;
    vt_merlin_header(tr_, label, (uint32_t)len);
    vt_begin_op(tr_, VT_FLAG_I | VT_FLAG_A | VT_FLAG_C);
    for (size_t i = 0; i < len; ++i) out[i] = (uint8_t)vt_squeeze_byte(tr_);
    return true;
}

// ---- plonk-core/src/transcript.rs:46-109, gadgets/src/transcript.rs:8-90 ---------------------------------------------
void BuiltinTranscript::append_u64(const char* label, uint64_t v) {
    words_[VT_ST_WORDS] = v;   // little-endian in the message buffer
    if (tr_.kind == 0) {
        vt_merlin_header(tr_, label, 8);
        vt_begin_op(tr_, VT_FLAG_A);
        vt_absorb_msg(tr_, 8);
    } else {
        vt_eth_append(tr_, 0, 8);   // hashed big-endian
    }
}
void BuiltinTranscript::append_scalars(const char* label, const uint8_t* le, size_t count, size_t fr_bytes, bool) {
    if (fr_bytes != 32) return;
    vt_tr_scalars_begin(tr_, label, count);
    for (size_t k = 0; k < count; ++k) {
        memcpy(words_ + VT_ST_WORDS, le + 32 * k, 32);
        vt_tr_scalars_item(tr_);
    }
}
void BuiltinTranscript::append_commitment(const char* label, const uint8_t* x_le, const uint8_t* y_le, size_t fq_bytes,
                                          bool infinity) {
    if (fq_bytes == 0 || fq_bytes > 48) return;   // 2 * 48 + 1 bytes of message buffer; 65 + 48 + 1 <= 136 in vt_eth_hash
    uint8_t* buf = reinterpret_cast<uint8_t*>(words_ + VT_ST_WORDS);
    memset(buf, 0, 2 * fq_bytes + 1);
    if (infinity) {   // GroupAffine::zero() is (0, 1, true)
        buf[fq_bytes] = 1;
        buf[2 * fq_bytes] = 1;
    } else {
        memcpy(buf, x_le, fq_bytes);
        memcpy(buf + fq_bytes, y_le, fq_bytes);
    }
    vt_tr_commit_msg(tr_, label, (uint32_t)fq_bytes);
}
void BuiltinTranscript::challenge_scalar(const char* label, size_t fr_bits, uint8_t out_le[32]) {
    memset(out_le, 0, 32);
    if (tr_.kind == 0 && (fr_bits == 0 || fr_bits > 264)) return;   // merlin squeezes (fr_bits + 7) / 8 - 1 bytes into the 32
    uint32_t w[8];
    vt_tr_challenge(tr_, label, (uint32_t)fr_bits, w);
    memcpy(out_le, w, 32);
}

bool BuiltinTranscript::export_state(TranscriptState& out) const {
    out = TranscriptState();
    vt_store_state(tr_, &out);
    return true;
}
bool BuiltinTranscript::import_state(const TranscriptState& in) {
    if (in.kind != tr_.kind) return false;
    if (in.kind == 0 && (in.pos >= VT_RATE || in.pos_begin > VT_RATE || in.cur_flags > 255)) return false;
    vt_load_state(tr_, &in);
    if (in.kind == 0) tr_.counter = 0;                               // what the other kind alone has is not taken over
    else tr_.pos = tr_.pos_begin = tr_.cur_flags = 0;
    return true;
}

}  // namespace zkt

// ---- the zkt_transcript_* C API over the built-in transcripts ------------------------------------------------------------
using namespace zkt;

extern "C" {

zkt_transcript* zkt_transcript_new(int kind, const char* label) {
    if (kind != ZKT_TRANSCRIPT_MERLIN && kind != ZKT_TRANSCRIPT_ETHEREUM) return nullptr;
    zkt_transcript* t = new zkt_transcript();
    auto* b = new BuiltinTranscript(kind == ZKT_TRANSCRIPT_MERLIN ? 0 : 1, label ? label : "");
    t->impl.reset(b);
    if (kind == ZKT_TRANSCRIPT_MERLIN) t->merlin = b;
    return t;
}
void zkt_transcript_free(zkt_transcript* t) { delete t; }
void zkt_transcript_append_u64(zkt_transcript* t, const char* label, uint64_t v) { t->impl->append_u64(label, v); }
void zkt_transcript_append_scalars(zkt_transcript* t, const char* label, const uint8_t* le32, size_t count, int single) {
    t->impl->append_scalars(label, le32, count, 32, single != 0);
}
void zkt_transcript_append_commitment(zkt_transcript* t, const char* label, const uint8_t* x_le, const uint8_t* y_le,
                                      size_t fq_bytes, int is_infinity) {
    t->impl->append_commitment(label, x_le, y_le, fq_bytes, is_infinity != 0);
}
void zkt_transcript_seed(zkt_transcript* t, uint64_t circuit_size, const uint8_t* xy_le, const uint8_t* is_infinity,
                         size_t fq_bytes) {
    static const char* labels[10] = {"q_m_commit", "q_l_commit", "q_r_commit", "q_o_commit", "q_c_commit",
                                     "sigma1_commit", "sigma2_commit", "sigma3_commit", "q_lookup_commit", "q_table_commit"};
    t->impl->append_u64("circuit_size", circuit_size);
    for (int k = 0; k < 10; ++k) {
        const uint8_t* x = xy_le + (size_t)k * 2 * fq_bytes;
        t->impl->append_commitment(labels[k], x, x + fq_bytes, fq_bytes, is_infinity && is_infinity[k]);
    }
}
void zkt_transcript_challenge_scalar(zkt_transcript* t, const char* label, int fr_bits, uint8_t out_le32[32]) {
    t->impl->challenge_scalar(label, (size_t)fr_bits, out_le32);
}
int zkt_transcript_challenge_bytes(zkt_transcript* t, const char* label, uint8_t* out, size_t len) {
    return t->merlin && t->merlin->challenge_bytes(label, out, len) ? ZKT_OK : ZKT_ERR_INVALID_ARGUMENT;
}
int zkt_transcript_append_message(zkt_transcript* t, const char* label, const uint8_t* msg, size_t len) {
    return t->merlin && t->merlin->append_message(label, msg, len) ? ZKT_OK : ZKT_ERR_INVALID_ARGUMENT;
}

}  // extern "C"
