// Host-side Fiat-Shamir transcripts (the north star keeps Fiat-Shamir on the host).
//
// * Merlin (merlin 3.0: STROBE-128 over Keccak-f[1600], protocol label "Merlin v1.0") wrapped the
//   way plonk-core/src/transcript.rs:46-109 wraps it (MerlinTranscript).
// * EthereumTranscript of gadgets/src/transcript.rs:8-90 (Keccak-256, BN254 only).
// Both are ONE class over transcript_core.hpp, the code the batch verifier's kernel runs, at a stride of one; they sit
// behind the zkt_transcript callback table of include/zkt_plonk.h, which is also what a Rust caller implements on top of
// its own `T: TranscriptProtocol`.
#pragma once
#include "transcript_core.hpp"

#include <stddef.h>
#include <memory>

namespace zkt {

void keccak256(const uint8_t* data, size_t len, uint8_t out[32]);

// Byte-level transcript interface used by the prover: everything is already serialised the way the
// reference's TranscriptProtocol impls see it (canonical field elements, affine coordinates).
struct HostTranscript {
    virtual ~HostTranscript() {}
    virtual void append_u64(const char* label, uint64_t v) = 0;
    // scalars: count canonical little-endian values of `fr_bytes` bytes each, back to back
    virtual void append_scalars(const char* label, const uint8_t* le, size_t count, size_t fr_bytes, bool single) = 0;
    // affine point: canonical x, y little-endian (fq_bytes each) + infinity flag
    virtual void append_commitment(const char* label, const uint8_t* x_le, const uint8_t* y_le, size_t fq_bytes,
                                   bool infinity) = 0;
    // 32 bytes little-endian canonical challenge
    virtual void challenge_scalar(const char* label, size_t fr_bits, uint8_t out_le[32]) = 0;
    // the whole state out and in again; false: this transcript has no state of its own to give (a caller's callbacks)
    virtual bool export_state(TranscriptState&) const { return false; }
    virtual bool import_state(const TranscriptState&) { return false; }
};

// The built-in transcripts: a core transcript over its own VT_LANE_WORDS words.  A scalar has 32 bytes and a coordinate
// at most 48 (one item of the message buffer, one Keccak-256 block); a call with other sizes is refused: nothing changes.
struct BuiltinTranscript final : HostTranscript {
    BuiltinTranscript(int kind, const char* label);   // TranscriptState::kind: 0 Merlin, seeded with `label`; 1 Ethereum
    BuiltinTranscript(const BuiltinTranscript&) = delete;
    void append_u64(const char* label, uint64_t v) override;
    void append_scalars(const char* label, const uint8_t* le, size_t count, size_t fr_bytes, bool single) override;
    void append_commitment(const char* label, const uint8_t* x_le, const uint8_t* y_le, size_t fq_bytes,
                           bool infinity) override;
    void challenge_scalar(const char* label, size_t fr_bits, uint8_t out_le[32]) override;
    bool export_state(TranscriptState& out) const override;
    bool import_state(const TranscriptState& in) override;   // false: another kind, or a position outside the rate
    // merlin's own two calls, a message of any length (the seeding, the conformance vector); false on Ethereum
    bool append_message(const char* label, const uint8_t* msg, size_t len);
    bool challenge_bytes(const char* label, uint8_t* out, size_t len);

  private:
    uint64_t words_[VT_LANE_WORDS] = {0};
    VtTr tr_;
};

}  // namespace zkt

// the opaque handle of include/zkt_plonk.h
struct zkt_transcript {
    std::unique_ptr<zkt::HostTranscript> impl;
    zkt::BuiltinTranscript* merlin = nullptr;  // impl when it is a built-in Merlin: raw access for the conformance KAT
};
