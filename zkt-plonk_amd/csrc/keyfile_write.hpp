// Writers for the key files of the reference CLI's `Compile` (bin/src/main.rs:105-111 --ck / --pk / --vk / --epk):
// `serialize_to_file` = CanonicalSerialize::serialize_unchecked (bin/src/parser.rs:14-22).  The byte layout is the one
// keyfile.hip reads (ark-serialize 0.3 / ark-poly-commit 0.3, restated from their published derive rules; no
// reference-held file exists to pin it against: "parity unpinned", the layout is pinned to the test-side writer and to
// this library's own readers).
// Host only, and nothing of HIP: standard headers alone, so that a stand-alone program can compile it.  Values arrive as
// arkworks Montgomery limbs (what every entry of the C-ABI speaks) and leave as canonical little-endian bytes.
#pragma once
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <unistd.h>

namespace zkt {
namespace kw {

// the four moduli as 32-bit words, little endian (keyfile.hip checks them against fp.hpp's at compile time)
struct Field {
    int n32;
    uint32_t mod[12];
};
inline const Field& field(int curve_id, bool fq) {
    static const Field bn_fr{8, {0xf0000001u, 0x43e1f593u, 0x79b97091u, 0x2833e848u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u}};
    static const Field bn_fq{8, {0xd87cfd47u, 0x3c208c16u, 0x6871ca8du, 0x97816a91u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u}};
    static const Field bls_fr{8, {0x00000001u, 0xffffffffu, 0xfffe5bfeu, 0x53bda402u, 0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u}};
    static const Field bls_fq{12, {0xffffaaabu, 0xb9feffffu, 0xb153ffffu, 0x1eabfffeu, 0xf6b0f624u, 0x6730d2a0u, 0xf38512bfu, 0x64774b84u,
                                   0x434bacd7u, 0x4b1ba7b6u, 0x397fe69au, 0x1a0111eau}};
    return curve_id == 0 ? (fq ? bn_fq : bn_fr) : (fq ? bls_fq : bls_fr);
}

inline bool below_modulus(const Field& f, const uint32_t* v) {
    for (int i = f.n32 - 1; i >= 0; --i) {
        if (v[i] < f.mod[i]) return true;
        if (v[i] > f.mod[i]) return false;
    }
    return false;   // equal to the modulus
}

// a R mod p (n32 words, as the u64 limbs lie in memory) -> a, canonical little-endian bytes; false when the limbs are
// not below the modulus (our readers refuse such a value, so no file holds one)
inline bool canonical(const Field& f, const uint64_t* mont, uint8_t* out) {
    const int n = f.n32;
    uint32_t t[13];
    memcpy(t, mont, (size_t)n * 4);
    t[n] = 0;
    if (!below_modulus(f, t)) return false;
    uint32_t ninv = 1;   // -p^-1 mod 2^32 by Newton's iteration on the odd low word
    for (int i = 0; i < 5; ++i) ninv *= 2u - f.mod[0] * ninv;
    ninv = 0u - ninv;
    for (int i = 0; i < n; ++i) {   // one word of Montgomery reduction: t = (t + m p) / 2^32
        const uint32_t m = t[0] * ninv;
        uint64_t carry = 0;
        for (int j = 0; j < n; ++j) {
            const uint64_t s = (uint64_t)m * f.mod[j] + t[j] + carry;
            if (j) t[j - 1] = (uint32_t)s;
            carry = s >> 32;
        }
        const uint64_t s = (uint64_t)t[n] + carry;
        t[n - 1] = (uint32_t)s;
        t[n] = (uint32_t)(s >> 32);
    }
    // a < p on entry keeps the result below p: (a + m p) / R < p + 1, and p itself would need a = 0 (mod p)
    memcpy(out, t, (size_t)n * 4);   // little-endian words on a little-endian host
    return true;
}

// A key file in the making: the bytes go to a temporary sibling of `path` that takes the file's place only in commit().
// A writer that fails, or is dropped before commit(), leaves neither a truncated key file nor the temporary one.
class File {
  public:
    explicit File(const char* path) : path_(path), tmp_(std::string(path) + ".tmp." + std::to_string((long)getpid())) {
        f_ = fopen(tmp_.c_str(), "wb");
        created_ = f_ != nullptr;
        if (!f_) fail("cannot create");
    }
    File(const File&) = delete;
    File& operator=(const File&) = delete;
    ~File() {
        if (f_) fclose(f_);
        if (!done_ && created_) (void)remove(tmp_.c_str());
    }
    bool ok() const { return err_.empty(); }
    const std::string& error() const { return err_; }
    void bytes(const void* p, size_t len) {
        if (ok() && len && fwrite(p, 1, len, f_) != len) fail("cannot write");
    }
    void u8(uint8_t v) { bytes(&v, 1); }
    void u64(uint64_t v) {
        uint8_t b[8];
        for (int i = 0; i < 8; ++i) b[i] = (uint8_t)(v >> (8 * i));
        bytes(b, 8);
    }
    void none() { u8(0); }   // Option::None
    void reject(const std::string& what) {
        if (ok()) err_ = what + " (" + path_ + " not written)";
    }
    // one field element; a value not below the modulus ends the file
    void fe(const Field& f, const uint64_t* mont) {
        uint8_t b[48];
        if (!canonical(f, mont, b)) return reject("a value is not below the modulus");
        bytes(b, (size_t)f.n32 * 4);
    }
    // GroupAffine, unchecked: x, y, SWFlags in the top bits of y's last byte.  (0, 0) is the identity as the readers
    // return it; GroupAffine::zero() is (0, 1) with the infinity flag (bit 6)
    void g1(const Field& fq, const uint64_t* xy_mont, bool infinity) {
        const size_t nb = (size_t)fq.n32 * 4;
        uint8_t b[96] = {};
        bool zero = true;
        for (size_t i = 0; i < 2 * nb / 8; ++i) zero = zero && xy_mont[i] == 0;
        if (infinity || zero) {
            b[nb] = 1;
            b[2 * nb - 1] |= 0x40;
        } else if (!canonical(fq, xy_mont, b) || !canonical(fq, xy_mont + nb / 8, b + nb)) {
            return reject("a coordinate is not below the modulus");
        }
        bytes(b, 2 * nb);
    }
    bool commit() {
        if (!ok()) return false;
        const bool flushed = fflush(f_) == 0;
        const bool closed = fclose(f_) == 0;
        f_ = nullptr;
        if (!flushed || !closed) return fail("cannot write");
        if (rename(tmp_.c_str(), path_.c_str()) != 0) return fail("cannot rename the temporary file to");
        done_ = true;
        return true;
    }

  private:
    bool fail(const char* what) {
        if (ok()) err_ = std::string(what) + " " + path_ + ": " + strerror(errno);
        return false;
    }
    std::string path_, tmp_, err_;
    FILE* f_ = nullptr;
    bool created_ = false, done_ = false;
};

// --ck (bin/src/main.rs:105): sonic_pc::CommitterKey as PC::trim leaves it (plonk.rs:79-85): powers_of_g, an empty
// powers_of_gamma_g, shifted_powers_of_g / shifted_powers_of_gamma_g / enforced_degree_bounds = None, max_degree
inline void committer_key_head(File& w, size_t count) { w.u64(count); }
inline void committer_key_tail(File& w, size_t count) {
    w.u64(0);
    w.none();
    w.none();
    w.none();
    w.u64(count - 1);
}
inline bool write_committer_key(File& w, int curve_id, const uint64_t* g1_xy_mont, size_t count) {
    const Field& fq = field(curve_id, true);
    const size_t words = (size_t)fq.n32;   // u64 limbs of one point: two coordinates of n32 / 2
    committer_key_head(w, count);
    for (size_t i = 0; i < count && w.ok(); ++i) w.g1(fq, g1_xy_mont + i * words, false);
    committer_key_tail(w, count);
    return w.ok();
}

// --pk (bin/src/main.rs:107): ProverKey<F> (keys/mod.rs:29-41) = ten LabeledPolynomial in zkt_circuit_load order, labelled
// as in setup.rs:92-101, degree_bound and hiding_bound None
inline const char* const* prover_key_labels() {
    static const char* const l[10] = {"q_m", "q_l", "q_r", "q_o", "q_c", "sigma1", "sigma2", "sigma3", "q_lookup", "q_table"};
    return l;
}
inline bool write_prover_key(File& w, int curve_id, const uint64_t* const* polys, const size_t* lens10) {
    const Field& fr = field(curve_id, false);
    for (int k = 0; k < 10 && w.ok(); ++k) {
        const char* label = prover_key_labels()[k];
        w.u64(strlen(label));
        w.bytes(label, strlen(label));
        w.u64(lens10[k]);
        for (size_t i = 0; i < lens10[k] && w.ok(); ++i) w.fe(fr, polys[k] + 4 * i);
        w.none();
        w.none();
    }
    return w.ok();
}

// --vk (bin/src/main.rs:111): VerifierKey (keys/mod.rs:180-210) = n, pi_roots, the ten commitments
inline bool write_verifier_key(File& w, int curve_id, uint64_t n, const uint64_t* pi_roots_mont, size_t n_pi,
                               const uint64_t* commitments_xy_mont, const int* is_infinity10) {
    const Field &fr = field(curve_id, false), &fq = field(curve_id, true);
    const size_t words = (size_t)fq.n32;
    w.u64(n);
    w.u64(n_pi);
    for (size_t i = 0; i < n_pi && w.ok(); ++i) w.fe(fr, pi_roots_mont + 4 * i);
    for (int k = 0; k < 10 && w.ok(); ++k) w.g1(fq, commitments_xy_mont + (size_t)k * words, is_infinity10 && is_infinity10[k]);
    return w.ok();
}

}  // namespace kw
}  // namespace zkt
