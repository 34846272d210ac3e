// The keys that setup makes, handed back (setup.rs:42-166 returns ProverKey, VerifierKey, ExtendedProverKey): the
// polynomials, their commitments, the extended key's vectors one at a time, and the reference CLI's key files written or
// compared (bin/src/main.rs:105-111).  Host orchestration only: every launch is another unit's.
#include "circuit.hpp"
#include "keyfile.hpp"
#include "keyfile_write.hpp"
#include "msm.hpp"

#include <algorithm>

namespace zkt {

// ---- the ExtendedProverKey's vectors, one at a time (keys/mod.rs:78-146 as zkt_circuit_load runs it) ----------------------
// The derivation zkt_circuit_check_epk_file compares a file with and zkt_circuit_export_epk / _write_epk_file hand out: every
// vector is recomputed in arkworks' own form (the resident cosets partly live in the quotient kernel's radix).
static bool epk_is_evals(int k) { return k == EPK_QLOOKUP || k == EPK_S1 || k == EPK_S2 || k == EPK_S3; }
// Vector k (not zh_coset: circuit_zh4) on the device: *out is a resident table or `plain` (4n elements, written here;
// S.ev[0] as well for l_1_coset), Montgomery form; with `canon` (4n elements) the canonical values, written there.
template <class C>
static int epk_vector_dev(zkt_ctx* c, CircuitState& S, int k, void* plain, void* canon, const void** out) {
    using R = typename C::Fr;
    static const int pk_of[EPK_VECTORS] = {PK_QM, PK_QL, PK_QR, PK_QO, PK_QC, -1, PK_QLOOKUP, PK_QTABLE, -1, PK_S1, -1, PK_S2, -1, PK_S3,
                                           -1, -1, -1};
    const size_t n = S.n;
    const size_t expect = epk_is_evals(k) ? n : 4 * n;
    int rc;
    const void* src = plain;
    if (pk_of[k] >= 0) {
        if ((rc = ntt_run(c, S.log_n + 2, 0, 1, S.pk[pk_of[k]], n, plain))) return rc;
    } else if (k == EPK_QLOOKUP) {
        src = S.q_lookup_ev;
    } else if (epk_is_evals(k)) {
        src = S.sigma_ev[k == EPK_S1 ? 0 : k == EPK_S2 ? 1 : 2];
    } else if (k == EPK_X_C) {
        src = S.coset[CS_X];
    } else {              // l_1_coset, as the load derives it (the resident one went on to the quotient kernel's radix)
        if ((rc = circuit_l1_coset<R>(c, S, plain))) return rc;
    }
    *out = src;
    if (!canon) return ZKT_OK;
    LinCombArgs lc{};     // times the word 1 = R^-1 as a Montgomery operand: the canonical value
    lc.poly[0] = src;
    lc.len[0] = expect;
    lc.scalar[0][0] = 1;
    lc.nterms = 1;
    if ((rc = poly_lincomb(c, lc, canon, expect))) return rc;
    *out = canon;
    return ZKT_OK;
}

// A file the reference CLI wrote with --epk (bin/src/main.rs:108-109: ExtendedProverKey<F>, keys/mod.rs:148-174) against the
// extended key this circuit's ProverKey gives on the device: every vector is derived (epk_vector_dev), turned canonical,
// brought to the host and compared with the file's bytes as they stream by.
template <class C>
static int circuit_check_epk_t(zkt_ctx* c, const char* path, int* vec_out, size_t* at_out) {
    using R = typename C::Fr;
    using F = Fe<R>;
    CircuitState& S = *c->circuit;
    const size_t n = S.n, m = 4 * n;
    *vec_out = -1;
    *at_out = 0;
    EpkReader rd;
    struct Closer {
        EpkReader& r;
        ~Closer() { r.close(); }
    } closer{rd};
    if (!rd.open(path)) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, std::string("cannot open ") + path);
    void* plain = S.qev;          // 4n work buffers, free between proofs
    void* canon = S.wcos[W_A];
    uint8_t zh4[4][32];
    {
        F zh[4];
        circuit_zh4<R>(S.log_n, zh);
        for (int j = 0; j < 4; ++j) HostF<R>::to_le_bytes(zh[j], zh4[j]);
    }
    std::vector<uint8_t> want, got;
    const size_t step = (size_t)1 << 16;
    got.resize(step * 32);
    int rc;
    for (int k = 0; k < EPK_VECTORS; ++k) {
        uint64_t len = 0;
        if (!rd.next(&len)) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, std::string("not an ExtendedProverKey file: ") + path);
        const size_t expect = epk_is_evals(k) ? n : m;
        if (len != expect) {      // another circuit size: no element to point at
            *vec_out = k;
            *at_out = (size_t)-1;
            return ZKT_OK;
        }
        if (k != EPK_ZH_C) {
            const void* src = nullptr;
            if ((rc = epk_vector_dev<C>(c, S, k, plain, canon, &src))) return rc;
            want.resize(expect * 32);
            ZKT_HIP(c, hipMemcpyAsync(want.data(), src, expect * 32, hipMemcpyDeviceToHost, c->stream));
            ZKT_HIP(c, hipStreamSynchronize(c->stream));
        }
        for (size_t i = 0; i < expect; i += step) {
            const size_t cnt = std::min(step, expect - i);
            if (!rd.read(got.data(), cnt)) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, std::string("short read from ") + path);
            bool same = true;
            if (k != EPK_ZH_C) {
                same = memcmp(want.data() + i * 32, got.data(), cnt * 32) == 0;
            } else {
                for (size_t j = 0; j < cnt && same; ++j) same = memcmp(zh4[(i + j) & 3], got.data() + j * 32, 32) == 0;
            }
            if (!same) {
                size_t j = 0;
                while (memcmp(k != EPK_ZH_C ? want.data() + (i + j) * 32 : zh4[(i + j) & 3], got.data() + j * 32, 32) == 0) ++j;
                *vec_out = k;
                *at_out = i + j;
                return ZKT_OK;
            }
        }
    }
    if (!rd.at_end()) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, std::string("bytes after the seventeenth vector of ") + path);
    return ZKT_OK;
}

// zkt_circuit_export_epk: vector `which` in Montgomery limbs, straight from the derivation above
template <class C>
static int circuit_export_epk_t(zkt_ctx* c, int which, uint64_t* out, size_t cap, size_t* lens17) {
    using R = typename C::Fr;
    CircuitState& S = *c->circuit;
    for (int k = 0; k < EPK_VECTORS; ++k) lens17[k] = epk_is_evals(k) ? S.n : 4 * S.n;
    if (which < 0) return ZKT_OK;
    const size_t len = lens17[which];
    if (!out || cap < len) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "zkt_circuit_export_epk: the buffer is shorter than the vector");
    if (which == EPK_ZH_C) {
        Fe<R> zh[4];
        circuit_zh4<R>(S.log_n, zh);
        for (size_t i = 0; i < len; ++i) memcpy(out + 4 * i, zh[i & 3].v, 32);
        return ZKT_OK;
    }
    const void* src = nullptr;
    if (int rc = epk_vector_dev<C>(c, S, which, S.qev, nullptr, &src)) return rc;
    ZKT_HIP(c, hipMemcpyAsync(out, src, len * 32, hipMemcpyDeviceToHost, c->stream));
    ZKT_HIP(c, hipStreamSynchronize(c->stream));
    return ZKT_OK;
}

// zkt_circuit_write_epk_file (bin/src/main.rs:108-109 --epk): the seventeen vectors, canonical, streamed into `w`.  Vector
// k drains from one of two 4n device buffers through two pinned chunks -- the copy of chunk i + 1 is in flight on the copy
// stream while chunk i is written -- and vector k + 1 is derived into the other buffer on the main stream meanwhile.  The
// host holds the two chunks and never a whole vector.
constexpr size_t EPK_WRITE_CHUNK = (size_t)1 << 16;   // elements: 2 MiB, the step the check reads the file in
template <class C>
static int circuit_write_epk_t(zkt_ctx* c, kw::File& w) {
    using R = typename C::Fr;
    CircuitState& S = *c->circuit;
    const size_t n = S.n, step = EPK_WRITE_CHUNK;
    DevSet tmp(c->device);            // the call's own: the staging chunks and the events of the drain
    // whatever ends this call, nothing may still read or write the chunks or the work buffers when `tmp` goes
    struct Drain {
        zkt_ctx* c;
        hipStream_t copy;
        ~Drain() {
            (void)hipStreamSynchronize(copy);
            (void)hipStreamSynchronize(c->stream);
        }
    } drain{c, S.copy_stream};
    void* pin[2] = {};
    hipEvent_t copied[2] = {}, derived[2] = {};
    int rc;
    for (int j = 0; j < 2; ++j) {
        if ((rc = tmp.pinned(c, &pin[j], std::min(step, 4 * n) * 32))) return rc;
        if ((rc = tmp.event(c, &copied[j]))) return rc;
        if ((rc = tmp.event(c, &derived[j]))) return rc;
    }
    void* canon[2] = {S.wcos[W_A], S.wcos[W_B]};   // 4n each, free between proofs
    const void* src[2] = {};
    auto derive = [&](int k) -> int {   // enqueue vector k on the main stream (zh_coset needs no device work)
        if (k >= EPK_VECTORS || k == EPK_ZH_C) return ZKT_OK;
        // canon[k & 1] held vector k - 2, whose last chunk the host has waited for; `plain` is read on the main stream only
        if (int r = epk_vector_dev<C>(c, S, k, S.qev, canon[k & 1], &src[k & 1])) return r;
        ZKT_HIP(c, hipEventRecord(derived[k & 1], c->stream));
        return ZKT_OK;
    };
    if ((rc = derive(0))) return rc;
    for (int k = 0; k < EPK_VECTORS && w.ok(); ++k) {
        const size_t len = epk_is_evals(k) ? n : 4 * n;
        const size_t chunks = (len + step - 1) / step;
        w.u64(len);
        if (k == EPK_ZH_C) {      // the four values, over and over (a chunk is a multiple of four elements)
            if ((rc = derive(k + 1))) return rc;
            Fe<R> zh[4];
            circuit_zh4<R>(S.log_n, zh);
            const size_t fill = std::min(step, len);
            for (size_t i = 0; i < fill; ++i) HostF<R>::to_le_bytes(zh[i & 3], (uint8_t*)pin[0] + 32 * i);
            for (size_t i = 0; i < len; i += step) w.bytes(pin[0], std::min(step, len - i) * 32);
            continue;
        }
        ZKT_HIP(c, hipStreamWaitEvent(S.copy_stream, derived[k & 1], 0));
        auto issue = [&](size_t i) -> int {
            const size_t at = i * step, cnt = std::min(step, len - at);
            ZKT_HIP(c, hipMemcpyAsync(pin[i & 1], (const char*)src[k & 1] + at * 32, cnt * 32, hipMemcpyDeviceToHost, S.copy_stream));
            ZKT_HIP(c, hipEventRecord(copied[i & 1], S.copy_stream));
            return ZKT_OK;
        };
        if ((rc = issue(0))) return rc;
        if ((rc = derive(k + 1))) return rc;   // the next vector's transform runs while this one drains
        for (size_t i = 0; i < chunks; ++i) {
            if (i + 1 < chunks && (rc = issue(i + 1))) return rc;   // chunk i - 1, in the same half, is written
            ZKT_HIP(c, hipEventSynchronize(copied[i & 1]));
            w.bytes(pin[i & 1], std::min(step, len - i * step) * 32);
        }
    }
    return ZKT_OK;
}

// the VerifierKey's pi_roots (keys/mod.rs:186-188): w^pos
template <class R>
static void pi_roots_t(int log_n, const size_t* pi_pos, size_t n_pi, uint64_t* out) {
    const Fe<R> w = root_of_unity<R>(log_n);   // zkt_domain_group_gen
    for (size_t i = 0; i < n_pi; ++i) {
        const Fe<R> r = fe_pow_u64<R>(w, (uint64_t)pi_pos[i]);
        memcpy(out + 4 * i, r.v, 32);
    }
}

// the ten commitments of the loaded keys at their trimmed lengths (the caller has passed circuit_entry)
static int circuit_commitments(zkt_ctx* c, uint64_t* out_commitments, int* out_is_infinity) {
    if (!c->msm) return set_err(c, ZKT_ERR_NOT_LOADED, "no SRS loaded (zkt_srs_load)");
    CircuitState& S = *c->circuit;
    size_t lens[PK_COUNT];
    if (int rc = circuit_key_lens(c, S, lens)) return rc;
    return circuit_commit_keys(c, S, lens, out_commitments, out_is_infinity);
}

static int circuit_write_epk(zkt_ctx* c, const char* epk_path) {
    kw::File w(epk_path);
    const int rc = by_curve(c->curve, [&](auto C) { return circuit_write_epk_t<decltype(C)>(c, w); });
    if (rc) return rc;   // (the temporary file goes with `w`)
    return keyfile_write_done(c, w);
}

}  // namespace zkt

using namespace zkt;

extern "C" {

int zkt_circuit_export(zkt_ctx* c, uint64_t* const* out_polys, size_t* lens10) {
    if (!c || !lens10) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (int rc = circuit_entry(c, ENTRY_DEVICE)) return rc;
    const CircuitState& S = *c->circuit;   // read-only on the keys: forks, sharded contexts (the polynomials are replicated)
    if (int rc = circuit_key_lens(c, S, lens10)) return rc;
    if (!out_polys) return ZKT_OK;
    for (int k = 0; k < PK_COUNT; ++k)
        if (out_polys[k] && lens10[k])
            ZKT_HIP(c, hipMemcpyAsync(out_polys[k], S.pk[k], lens10[k] * 32, hipMemcpyDeviceToHost, c->stream));
    ZKT_HIP(c, hipStreamSynchronize(c->stream));
    return ZKT_OK;
}

int zkt_circuit_commitments(zkt_ctx* c, uint64_t* out_commitments, int* out_is_infinity) {
    if (!c || !out_commitments) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (int rc = circuit_entry(c, ENTRY_WORK, "zkt_circuit_commitments")) return rc;
    return circuit_commitments(c, out_commitments, out_is_infinity);
}

int zkt_circuit_export_epk(zkt_ctx* c, int which, uint64_t* out_mont, size_t cap, size_t* lens17) {
    if (!c || !lens17) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (which < -1 || which >= EPK_VECTORS) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "which: -1 (lengths) or 0 .. 16");
    if (int rc = circuit_entry(c, ENTRY_WORK, "zkt_circuit_export_epk")) return rc;
    return by_curve(c->curve, [&](auto C) { return circuit_export_epk_t<decltype(C)>(c, which, out_mont, cap, lens17); });
}

int zkt_circuit_check_epk_file(zkt_ctx* c, const char* epk_path, int* first_mismatch_vector, size_t* mismatch_at) {
    if (!c || !epk_path || !first_mismatch_vector || !mismatch_at) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (int rc = circuit_entry(c, ENTRY_DEVICE | ENTRY_WITHDRAW)) return rc;
    if (c->circuit->G != 1) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "a sharded context holds one class of every coset: check the file on an unsharded one");
    return by_curve(c->curve, [&](auto C) { return circuit_check_epk_t<decltype(C)>(c, epk_path, first_mismatch_vector, mismatch_at); });
}

int zkt_circuit_check_vk_file(zkt_ctx* c, const char* vk_path, int* first_mismatch) {
    if (!c || !vk_path || !first_mismatch) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (int rc = circuit_entry(c, ENTRY_WORK, "zkt_circuit_check_vk_file")) return rc;
    uint64_t n = 0, theirs[10 * 12] = {}, ours[10 * 12] = {};
    size_t n_pi = 0;
    int their_inf[10] = {}, our_inf[10] = {};
    if (int rc = zkt_keyfile_verifier_key(vk_path, c->curve, &n, nullptr, 0, &n_pi, theirs, their_inf))
        return set_err(c, rc, std::string("cannot read a VerifierKey from ") + vk_path);
    *first_mismatch = -1;
    if (n != c->circuit->n) {
        *first_mismatch = 10;
        return ZKT_OK;
    }
    if (int rc = circuit_commitments(c, ours, our_inf)) return rc;
    const size_t words = c->curve == ZKT_CURVE_BN254 ? 8 : 12;
    for (int k = 9; k >= 0; --k)
        if (their_inf[k] != our_inf[k] || memcmp(theirs + k * words, ours + k * words, words * 8) != 0) *first_mismatch = k;
    return ZKT_OK;
}

int zkt_circuit_write_epk_file(zkt_ctx* c, const char* epk_path) {
    if (!c || !epk_path) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (int rc = circuit_entry(c, ENTRY_WORK, "zkt_circuit_write_epk_file")) return rc;
    return circuit_write_epk(c, epk_path);
}

// bin/src/main.rs:105-111: the files `Compile` writes beside --ck (zkt_srs_save_file)
int zkt_circuit_save_files(zkt_ctx* c, const char* pk_path, const char* vk_path, const char* epk_path, const size_t* pi_pos,
                           size_t n_pi) {
    if (!c || (n_pi && !pi_pos)) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (int rc = circuit_entry(c, 0)) return rc;
    const size_t n = c->circuit->n;
    for (size_t i = 0; i < n_pi; ++i)
        if (pi_pos[i] >= n || (i && pi_pos[i] <= pi_pos[i - 1]))
            return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "public-input positions must be ascending, distinct and below n");
    if (vk_path && !c->msm) return set_err(c, ZKT_ERR_NOT_LOADED, "no SRS loaded (zkt_srs_load)");
    if (vk_path || epk_path) {
        if (int rc = circuit_entry(c, ENTRY_WORK, "zkt_circuit_save_files")) return rc;
    }
    (void)hipSetDevice(c->device);
    if (pk_path) {   // --pk: ProverKey (keys/mod.rs:29-41)
        size_t lens[PK_COUNT];
        if (int rc = zkt_circuit_export(c, nullptr, lens)) return rc;
        std::vector<std::vector<uint64_t>> polys(PK_COUNT);
        uint64_t* ptrs[PK_COUNT];
        for (int k = 0; k < PK_COUNT; ++k) {
            polys[k].resize(lens[k] * 4 + 4);
            ptrs[k] = polys[k].data();
        }
        if (int rc = zkt_circuit_export(c, ptrs, lens)) return rc;
        kw::File w(pk_path);
        kw::write_prover_key(w, c->curve, ptrs, lens);
        if (int rc = keyfile_write_done(c, w)) return rc;
    }
    if (vk_path) {   // --vk: VerifierKey (keys/mod.rs:180-210), pi_roots = w^pos
        uint64_t commits[10 * 12] = {};
        int inf[10] = {};
        if (int rc = circuit_commitments(c, commits, inf)) return rc;
        std::vector<uint64_t> roots(4 * n_pi + 4);
        by_curve(c->curve, [&](auto C) { pi_roots_t<typename decltype(C)::Fr>(c->circuit->log_n, pi_pos, n_pi, roots.data()); });
        kw::File w(vk_path);
        kw::write_verifier_key(w, c->curve, (uint64_t)n, roots.data(), n_pi, commits, inf);
        if (int rc = keyfile_write_done(c, w)) return rc;
    }
    if (epk_path) return circuit_write_epk(c, epk_path);
    return ZKT_OK;
}

}  // extern "C"
