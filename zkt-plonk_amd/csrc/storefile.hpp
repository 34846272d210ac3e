// The byte layouts of the two files the reference CLI keeps its state in (bin/src/main.rs: ProveWithdraw, Deposit, InitStore,
// ListNotes), both written by `serialize_to_file` = CanonicalSerialize::serialize_unchecked (bin/src/parser.rs):
//   --merkle-tree  MerkleTreeStore<F> { tree: BTreeMap<(usize, usize), F>, root: F, next_index: usize }
//                  (gadgets/src/merkle_tree.rs:8-13)
//       u64 E | E x (u64 layer, u64 idx, scalar), ascending (layer, idx) | scalar root | u64 next_index
//       MerkleTreeStore::default() is 48 bytes: no entry, root 0, index 0.  After add_leaf of `count` leaves the map is dense:
//       for every layer L in [0, HEIGHT) exactly the indices 0 .. ceil(count / 2^L) - 1 (merkle_tree.rs:92-95).  HEIGHT is not
//       in the file: it is max layer + 1.
//   --notes        Notes<F> = Vec<Note<F>>, Note { leaf_index: usize, identifier: F, amount: u64, secret: F }
//                  (gadgets/src/note.rs)
//       u64 count | count x (u64 leaf_index, scalar identifier, u64 amount, scalar secret): 80 bytes a note
// Both layouts are DERIVED from ark-serialize 0.3's rules, the ones keyfile.hip relies on: usize and u64 are 8 bytes little
// endian, a scalar is 32 canonical little-endian bytes on both curves, a Vec or BTreeMap is a u64 length followed by its items
// (a map's in ascending key order, a tuple's fields one after the other).  The reference holds no such file, so no
// reference-made file has ever been compared ("parity unpinned", as with the key files).
// The --cvk file is not covered: its type comes from ark-poly-commit, whose source is not in the reference tree.
// Host only, and nothing of HIP: standard headers and keyfile_write.hpp (which includes standard headers alone), so that a
// stand-alone program can compile it.  Scalars cross the C-ABI as arkworks Montgomery limbs.
#pragma once
#include "keyfile_write.hpp"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace zkt {
namespace sf {

constexpr size_t TREE_ENTRY_BYTES = 48, TREE_FIXED_BYTES = 48, NOTE_BYTES = 80;

inline uint64_t le64(const uint8_t* p) {
    uint64_t v = 0;
    for (int i = 0; i < 8; ++i) v |= (uint64_t)p[i] << (8 * i);
    return v;
}
inline void put64(uint8_t* p, uint64_t v) {
    for (int i = 0; i < 8; ++i) p[i] = (uint8_t)(v >> (8 * i));
}

// canonical little-endian bytes below the modulus?
inline bool scalar_below_modulus(const kw::Field& fr, const uint8_t* le) {
    uint32_t w[12];
    memcpy(w, le, (size_t)fr.n32 * 4);
    return kw::below_modulus(fr, w);
}

// a b / 2^(32 n) mod p over n32 words, a and b below p
inline void mont_mul(const kw::Field& f, const uint32_t* a, const uint32_t* b, uint32_t* out) {
    const int n = f.n32;
    uint32_t ninv = 1;   // -p^-1 mod 2^32
    for (int i = 0; i < 5; ++i) ninv *= 2u - f.mod[0] * ninv;
    ninv = 0u - ninv;
    uint32_t t[14] = {};
    for (int i = 0; i < n; ++i) {
        uint64_t carry = 0;
        for (int j = 0; j < n; ++j) {
            const uint64_t s = (uint64_t)a[i] * b[j] + t[j] + carry;
            t[j] = (uint32_t)s;
            carry = s >> 32;
        }
        uint64_t s = (uint64_t)t[n] + carry;
        t[n] = (uint32_t)s;
        t[n + 1] = (uint32_t)(s >> 32);
        const uint32_t m = t[0] * ninv;
        carry = ((uint64_t)m * f.mod[0] + t[0]) >> 32;
        for (int j = 1; j < n; ++j) {
            s = (uint64_t)m * f.mod[j] + t[j] + carry;
            t[j - 1] = (uint32_t)s;
            carry = s >> 32;
        }
        s = (uint64_t)t[n] + carry;
        t[n - 1] = (uint32_t)s;
        t[n] = t[n + 1] + (uint32_t)(s >> 32);
        t[n + 1] = 0;
    }
    if (t[n] || !kw::below_modulus(f, t)) {   // one subtraction brings a value below 2 p under p
        uint64_t borrow = 0;
        for (int j = 0; j < n; ++j) {
            const uint64_t d = (uint64_t)t[j] - f.mod[j] - borrow;
            t[j] = (uint32_t)d;
            borrow = (d >> 32) & 1;
        }
    }
    memcpy(out, t, (size_t)n * 4);
}

// canonical little-endian bytes -> Montgomery limbs; false when the value is not below the modulus
inline bool to_mont(const kw::Field& f, const uint8_t* le, uint64_t* out_mont) {
    const int n = f.n32;
    if (!scalar_below_modulus(f, le)) return false;
    uint32_t r2[13] = {1};   // 2^(64 n) mod p by doubling
    for (int k = 0; k < 64 * n; ++k) {
        uint32_t top = 0;
        for (int j = 0; j < n; ++j) {
            const uint32_t next = r2[j] >> 31;
            r2[j] = (r2[j] << 1) | top;
            top = next;
        }
        r2[n] = top;
        if (top || !kw::below_modulus(f, r2)) {
            uint64_t borrow = 0;
            for (int j = 0; j < n; ++j) {
                const uint64_t d = (uint64_t)r2[j] - f.mod[j] - borrow;
                r2[j] = (uint32_t)d;
                borrow = (d >> 32) & 1;
            }
            r2[n] = 0;
        }
    }
    uint32_t a[12], m[12];
    memcpy(a, le, (size_t)n * 4);
    mont_mul(f, a, r2, m);
    memcpy(out_mont, m, (size_t)n * 4);
    return true;
}

// ---- what a reader refuses ---------------------------------------------------------------------------------------------
enum Refusal {
    ACCEPTED = 0,
    UNREADABLE,     // the file cannot be opened or read
    TRUNCATED,      // the file ends before its length fields say it does; offset: the file's size
    TRAILING,       // bytes after the last field; offset: the first of them
    NOT_BELOW_MODULUS,   // offset: the scalar
    NOT_ASCENDING,  // a key that is not above the one before it; offset: its entry
    NOT_DENSE,      // a key outside the dense set of next_index leaves under the height; offset: its entry
    TOO_FEW,        // every key belongs to the dense set, and some of it are missing; offset 0: the entry count
    OVER_CAPACITY,  // next_index above the capacity; offset: next_index
    TOO_MANY_NOTES  // more notes than the caller's buffers hold; offset 0
};
inline const char* refusal_text(int kind) {
    static const char* const t[] = {"accepted", "cannot read", "truncated", "trailing bytes", "a scalar is not below the modulus",
                                    "keys are not ascending", "a key outside the dense set of next_index leaves under this height",
                                    "fewer entries than the dense set of next_index leaves under this height",
                                    "next_index is above the capacity", "more notes than the buffers hold"};
    return t[kind];
}
inline std::string refusal_message(const char* path, int kind, uint64_t offset) {
    return std::string(path) + ": " + refusal_text(kind) + " (offset " + std::to_string(offset) + ")";
}

// ---- MerkleTreeStore ---------------------------------------------------------------------------------------------------
// nodes of layer L in the dense tree of `count` leaves: ceil(count / 2^L)
inline uint64_t dense_layer_len(uint64_t count, int L) {
    if (count == 0) return 0;
    return L >= 64 ? 1 : ((count - 1) >> L) + 1;
}
inline uint64_t dense_entries(uint64_t count, int height) {
    uint64_t e = 0;
    for (int L = 0; L < height; ++L) e += dense_layer_len(count, L);   // below 2 count + height
    return e;
}

inline void write_tree_head(kw::File& w, uint64_t entries) { w.u64(entries); }
inline void write_tree_entry(kw::File& w, const kw::Field& fr, uint64_t layer, uint64_t idx, const uint64_t* mont) {
    w.u64(layer);
    w.u64(idx);
    w.fe(fr, mont);
}
inline void write_tree_tail(kw::File& w, const kw::Field& fr, const uint64_t* root_mont, uint64_t next_index) {
    w.fe(fr, root_mont);
    w.u64(next_index);
}

// A MerkleTreeStore file read front to back in chunks: open() takes the size, the entry count and the two closing fields,
// next() hands out the entries as they lie in the file, each checked, finish() closes the account.  After a refusal
// kind() / offset() say which and where, and every later call does nothing.
class TreeFile {
  public:
    TreeFile() = default;
    TreeFile(const TreeFile&) = delete;
    TreeFile& operator=(const TreeFile&) = delete;
    ~TreeFile() {
        if (f_) fclose(f_);
    }
    bool open(const char* path, const kw::Field& fr, int height, uint64_t capacity) {
        fr_ = &fr;
        height_ = height;
        capacity_ = capacity;
        f_ = fopen(path, "rb");
        if (!f_ || fseeko(f_, 0, SEEK_END) != 0) return refuse(UNREADABLE, 0);
        const off_t sz = ftello(f_);
        if (sz < 0) return refuse(UNREADABLE, 0);
        const uint64_t size = (uint64_t)sz;
        uint8_t b[40];
        if (size < 8) return refuse(TRUNCATED, size);
        if (fseeko(f_, 0, SEEK_SET) != 0 || fread(b, 1, 8, f_) != 8) return refuse(UNREADABLE, 0);
        entries_ = le64(b);
        if (size < TREE_FIXED_BYTES || entries_ > (size - TREE_FIXED_BYTES) / TREE_ENTRY_BYTES) return refuse(TRUNCATED, size);
        const uint64_t want = TREE_FIXED_BYTES + entries_ * TREE_ENTRY_BYTES;
        if (size > want) return refuse(TRAILING, want);
        if (fseeko(f_, (off_t)(want - 40), SEEK_SET) != 0 || fread(b, 1, 40, f_) != 40) return refuse(UNREADABLE, want - 40);
        memcpy(root_, b, 32);
        next_index_ = le64(b + 32);
        if (fseeko(f_, 8, SEEK_SET) != 0) return refuse(UNREADABLE, 8);
        return true;
    }
    // up to max_entries further entries into dst, 48 bytes each as in the file; 0 at the end and after a refusal
    size_t next(uint8_t* dst, size_t max_entries) {
        if (kind_ || done_ == entries_) return 0;
        const size_t cnt = (size_t)(entries_ - done_ < max_entries ? entries_ - done_ : max_entries);
        if (fread(dst, TREE_ENTRY_BYTES, cnt, f_) != cnt) {
            refuse(UNREADABLE, 8 + done_ * TREE_ENTRY_BYTES);
            return 0;
        }
        for (size_t i = 0; i < cnt; ++i) {
            const uint8_t* e = dst + i * TREE_ENTRY_BYTES;
            const uint64_t at = 8 + (done_ + i) * TREE_ENTRY_BYTES, layer = le64(e), idx = le64(e + 8);
            bool ok = true;
            if (!scalar_below_modulus(*fr_, e + 16)) ok = refuse(NOT_BELOW_MODULUS, at + 16);
            else if (have_prev_ && (layer < prev_layer_ || (layer == prev_layer_ && idx <= prev_idx_))) ok = refuse(NOT_ASCENDING, at);
            else if (layer >= (uint64_t)height_ || idx >= dense_layer_len(next_index_, (int)layer)) ok = refuse(NOT_DENSE, at);
            if (!ok) return 0;
            have_prev_ = true;
            prev_layer_ = layer;
            prev_idx_ = idx;
        }
        done_ += cnt;
        return cnt;
    }
    // after the last entry: ascending keys, all of the dense set, are that set exactly when they are as many
    bool finish() {
        if (kind_) return false;
        const uint64_t root_at = 8 + entries_ * TREE_ENTRY_BYTES;
        if (done_ != entries_) return refuse(UNREADABLE, 8 + done_ * TREE_ENTRY_BYTES);
        if (entries_ != dense_entries(next_index_, height_)) return refuse(TOO_FEW, 0);
        if (!scalar_below_modulus(*fr_, root_)) return refuse(NOT_BELOW_MODULUS, root_at);
        if (next_index_ > capacity_) return refuse(OVER_CAPACITY, root_at + 32);
        return true;
    }
    uint64_t entries() const { return entries_; }
    uint64_t next_index() const { return next_index_; }
    const uint8_t* root() const { return root_; }
    int kind() const { return kind_; }
    uint64_t offset() const { return offset_; }

  private:
    bool refuse(int kind, uint64_t offset) {
        if (!kind_) {
            kind_ = kind;
            offset_ = offset;
        }
        return false;
    }
    FILE* f_ = nullptr;
    const kw::Field* fr_ = nullptr;
    int height_ = 0, kind_ = 0;
    uint64_t capacity_ = 0, entries_ = 0, next_index_ = 0, done_ = 0, offset_ = 0, prev_layer_ = 0, prev_idx_ = 0;
    bool have_prev_ = false;
    uint8_t root_[32] = {};
};

// ---- Notes ---------------------------------------------------------------------------------------------------------------
inline bool write_notes(kw::File& w, int curve_id, const uint64_t* leaf_indices, const uint64_t* identifiers_mont, const uint64_t* amounts,
                        const uint64_t* secrets_mont, size_t count) {
    const kw::Field& fr = kw::field(curve_id, false);
    w.u64(count);
    for (size_t i = 0; i < count && w.ok(); ++i) {
        w.u64(leaf_indices[i]);
        w.fe(fr, identifiers_mont + 4 * i);
        w.u64(amounts[i]);
        w.fe(fr, secrets_mont + 4 * i);
    }
    return w.ok();
}

// the whole file's bytes -> the notes; with any output null only *count.  Returns a Refusal, *offset with it.
inline int parse_notes(const uint8_t* buf, uint64_t len, int curve_id, size_t cap, uint64_t* leaf_indices, uint64_t* identifiers_mont,
                       uint64_t* amounts, uint64_t* secrets_mont, size_t* count, uint64_t* offset) {
    const kw::Field& fr = kw::field(curve_id, false);
    *offset = len;
    if (len < 8) return TRUNCATED;
    const uint64_t n = le64(buf);
    if (n > (len - 8) / NOTE_BYTES) return TRUNCATED;
    *offset = 8 + n * NOTE_BYTES;
    if (len > *offset) return TRAILING;
    for (uint64_t i = 0; i < n; ++i)
        for (int k = 0; k < 2; ++k) {
            *offset = 8 + i * NOTE_BYTES + (k ? 48 : 8);
            if (!scalar_below_modulus(fr, buf + *offset)) return NOT_BELOW_MODULUS;
        }
    *offset = 0;
    *count = (size_t)n;
    if (!leaf_indices || !identifiers_mont || !amounts || !secrets_mont) return ACCEPTED;
    if (n > cap) return TOO_MANY_NOTES;
    for (uint64_t i = 0; i < n; ++i) {
        const uint8_t* p = buf + 8 + i * NOTE_BYTES;
        leaf_indices[i] = le64(p);
        to_mont(fr, p + 8, identifiers_mont + 4 * i);
        amounts[i] = le64(p + 40);
        to_mont(fr, p + 48, secrets_mont + 4 * i);
    }
    return ACCEPTED;
}

inline bool read_whole_file(const char* path, std::vector<uint8_t>& out) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    bool ok = fseeko(f, 0, SEEK_END) == 0;
    const off_t sz = ok ? ftello(f) : -1;
    ok = ok && sz >= 0 && fseeko(f, 0, SEEK_SET) == 0;
    if (ok) {
        out.resize((size_t)sz);
        ok = sz == 0 || fread(out.data(), 1, (size_t)sz, f) == (size_t)sz;
    }
    fclose(f);
    return ok;
}

}  // namespace sf
}  // namespace zkt
