// Host-side transcripts: Keccak-256 over whole messages and the built-in Merlin / Ethereum transcript, both on
// transcript_core.hpp at a stride of one.  See transcript.hpp for the reference files they mirror.
#include "transcript.hpp"

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
