// The loaded circuit's life cycle (circuit.hpp): the per-proof work set, load (ProverKey + ExtendedProverKey on the device,
// keys/mod.rs:78-146), fork, release, setup from evaluation vectors (setup.rs:42-166) and the key commitments.  Host
// orchestration only: every launch is another unit's.
#include "circuit.hpp"
#include "msm.hpp"

#include <algorithm>

namespace zkt {

// ---- circuit (ProverKey + ExtendedProverKey) ------------------------------------------------------
// the work set, the keys and the class tables go together (the tables unless a fork still reads them)
void circuit_release(zkt_ctx* c) {
    if (!c->circuit) return;
    (void)hipStreamSynchronize(c->stream);
    wire_bases_drop(c);   // the wiring is the circuit's
    c->circuit.reset();
}
bool circuit_tables_have_readers(const zkt_ctx* c) {
    return c->circuit && (dev_shared_has_readers(c->circuit->keys_mem) || dev_shared_has_readers(c->circuit->class_mem));
}

// Everything a context needs PER PROOF (work buffers, staging, streams, events) for the circuit shape in S (log_n, G, cls
// set): what a forked context allocates for itself while the keys stay its parent's.
static int circuit_alloc_work(zkt_ctx* c, CircuitState& S) {
    const size_t n = S.n, m = S.m;
    int rc;
    auto alloc = [&](void** p, size_t elems) { return S.work.alloc(c, p, elems * 32); };
    if ((rc = alloc(&S.qev, 4 * n))) return rc;
    if (S.G > 1) {
        if ((rc = alloc(&S.fold, m))) return rc;
        if ((rc = alloc(&S.qgather, 4 * n))) return rc;
        if (S.G == 8) for (auto& p : S.wnext) if ((rc = alloc(&p, m))) return rc;
    }
    for (auto& p : S.ev) if ((rc = alloc(&p, n + 8))) return rc;
    for (auto& p : S.sc) if ((rc = alloc(&p, n + 8))) return rc;
    if ((rc = alloc(&S.scan_tmp, 2 * ((n + 8) / 1024 + 4096)))) return rc;
    for (auto& p : S.poly) if ((rc = alloc(&p, n + 8))) return rc;
    for (int k = 0; k < W_COUNT; ++k)   // the z1 slot doubles as 2n elements of scan scratch in round 3
        if ((rc = alloc(&S.wcos[k], k == W_Z1 ? std::max(std::max(m, 2 * n), 3 * (n + 8)) : m))) return rc;   // (round 5's second opening borrows 3 (n + 8))
    const size_t eval_blocks = (n + 8 + 2047) / 2048 + 1;
    if ((rc = alloc(&S.small, 64 + 16 * eval_blocks))) return rc;
    if ((rc = alloc(&S.lag_scalars, n + 16))) return rc;   // n + 8 scalars, then the blinders of zkt_commit_evals_dev
    for (auto& q : S.lag_scalars_q) if ((rc = alloc(&q, n + 16))) return rc;
    if (S.G == 1) {   // quotient on classes
        if ((rc = alloc(&S.heads, 3 * NTT_MAX_BATCH * NTT_HEAD))) return rc;
        if ((rc = alloc(&S.d_win, QC_WIN_POLYS * QC_WIN))) return rc;
        if ((rc = S.work.pinned(c, &S.pinned_win, QC_WIN_POLYS * QC_WIN * 32))) return rc;
        if ((rc = S.work.event(c, &S.ev_win))) return rc;
    }
    if ((rc = S.work.alloc(c, (void**)&S.status, 64 * 4))) return rc;
    if ((rc = S.work.alloc(c, (void**)&S.status_alt, 64 * 4))) return rc;
    for (auto& p : S.poly_alt) if ((rc = alloc(&p, n + 8))) return rc;
    S.lk_cap = n + 2;
    if ((rc = S.work.alloc(c, (void**)&S.lk_u32, 5 * S.lk_cap * 4 + 16))) return rc;
    if ((rc = alloc(&S.lk_keys, 2 * S.lk_cap))) return rc;
    if ((rc = S.work.pinned(c, &S.pinned, 64 * 32))) return rc;
    if ((rc = S.work.stream(c, &S.copy_stream))) return rc;
    if (S.G > 1) {
        if ((rc = S.work.stream(c, &S.comm_stream))) return rc;
        for (auto& e : S.ev_piece) if ((rc = S.work.event(c, &e))) return rc;
        if ((rc = S.work.event(c, &S.ev_gathered))) return rc;
    }
    for (auto& e : S.ev_copy) if ((rc = S.work.event(c, &e))) return rc;
    if ((rc = S.work.pinned(c, &S.pinned_pi, QUOTIENT_PI_DIRECT_MAX * 40))) return rc;
    if ((rc = S.work.alloc(c, (void**)&S.pi_tab, QUOTIENT_PI_DIRECT_MAX * 40))) return rc;
    if ((rc = alloc(&S.eval_pw, std::max((size_t)EVAL_MAX * (257 + eval_blocks), 2 * open_witness_powers(n + 8))))) return rc;
    if (S.G == 1) {
        if ((rc = alloc(&S.aux_scan_tmp, 2 * ((n + 8) / 1024 + 4096)))) return rc;
        if ((rc = alloc(&S.aux_pw, open_witness_powers(n + 8)))) return rc;
        if ((rc = S.work.stream(c, &S.aux_stream))) return rc;
        if ((rc = S.work.event(c, &S.ev_aux_go))) return rc;
        if ((rc = S.work.event(c, &S.ev_aux_done))) return rc;
    }
    return ZKT_OK;
}

// zkt_ctx_fork: the parent's keys and, where they exist, its class tables; this context's own work set
int circuit_fork(zkt_ctx* child, const zkt_ctx* parent) {
    circuit_release(child);
    if (!parent->circuit) return ZKT_OK;
    const CircuitState& P0 = *parent->circuit;
    auto st = std::make_shared<CircuitState>(child->device);
    CircuitState& S = *st;
    S.log_n = P0.log_n; S.n = P0.n; S.G = P0.G; S.cls = P0.cls; S.log_m = P0.log_m; S.m = P0.m;
    static_cast<CircuitKeys&>(S) = P0;
    S.keys_mem = dev_shared_reader(P0.keys_mem);
    if (P0.ccoset_ready) {
        static_cast<ClassTables&>(S) = P0;
        S.class_mem = dev_shared_reader(P0.class_mem);
    }
    if (int rc = circuit_alloc_work(child, S)) return rc;
    child->circuit = st;
    return ZKT_OK;
}

int circuit_key_coset(zkt_ctx* c, CircuitState& S, const void* poly, size_t len, void* out) {
    return S.G == 1 ? ntt_run(c, S.log_n + 2, 0, 1, poly, len, out)
                    : ntt_run_class(c, S.log_m, S.log_n + 2, S.cls, poly, len, out, S.fold);
}

template <class C>
static int circuit_load_t(zkt_ctx* c, int log_n, const uint64_t* const* polys, const size_t* lens, bool from_evals = false,
                          unsigned evals_dev_mask = 0) {   // bit k: evaluation vector k is a device pointer
    using R = typename C::Fr;
    using F = Fe<R>;
    if (log_n < 3 || log_n + 2 > R::TWO_ADICITY || log_n + 2 > 27)
        return set_err(c, ZKT_ERR_INVALID_DOMAIN_SIZE, "InvalidEvalDomainSize: 4n domain unsupported");
    if (int rf = refuse_if_forked(c, "loading a circuit")) return rf;
    circuit_release(c);
    auto st = std::make_shared<CircuitState>(c->device);
    // a refused load lets `st` go: what it enqueued on the stream reads the half-built state, so the stream drains first
    struct Drain {
        zkt_ctx* c;
        ~Drain() { if (!c->circuit) (void)hipStreamSynchronize(c->stream); }
    } drain{c};
    CircuitState& S = *st;
    S.log_n = log_n;
    const size_t n = (size_t)1 << log_n;
    S.n = n;
    // sharded proof: this GPU keeps (and later transforms) only its class of the 4n coset
    S.G = c->sharded() ? c->comm.vt.world : 1;
    S.cls = c->sharded() ? c->comm.vt.rank : 0;
    S.log_m = log_n + 2 - (S.G == 8 ? 3 : S.G == 4 ? 2 : S.G == 2 ? 1 : 0);
    S.m = (size_t)1 << S.log_m;
    const size_t m = S.m;
    int rc;
    S.keys_mem = std::make_shared<DevShared>(c->device);
    auto alloc = [&](void** p, size_t elems) { return S.keys_mem->alloc(c, p, elems * 32); };
    if ((rc = circuit_alloc_work(c, S))) return rc;   // (the quotient vector doubles as staging below)
    for (int k = 0; k < PK_COUNT; ++k) {
        if (lens[k] > n) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "prover-key polynomial longer than n");
        if ((rc = alloc(&S.pk[k], n))) return rc;
        if (from_evals) {
            // setup.rs:72-90: poly_from_evals of the padded selector / sigma / table-mask evaluations
            const void* src = polys[k];
            const bool on_device = (evals_dev_mask >> k) & 1u;
            if (!on_device) {
                ZKT_HIP(c, hipMemsetAsync(S.qev, 0, n * 32, c->stream));   // the quotient vector doubles as staging
                if (lens[k]) ZKT_HIP(c, hipMemcpyAsync(S.qev, polys[k], lens[k] * 32, hipMemcpyHostToDevice, c->stream));
                src = S.qev;
            }
            if ((rc = ntt_run(c, log_n, 1, 0, src, on_device ? lens[k] : n, S.pk[k]))) return rc;
            S.pk_len[k] = n;
        } else {
            ZKT_HIP(c, hipMemsetAsync(S.pk[k], 0, n * 32, c->stream));
            if (lens[k]) ZKT_HIP(c, hipMemcpyAsync(S.pk[k], polys[k], lens[k] * 32, hipMemcpyHostToDevice, c->stream));
            S.pk_len[k] = lens[k];
        }
    }
    for (int k = 0; k < CS_COUNT; ++k) if ((rc = alloc(&S.coset[k], m))) return rc;
    for (int k = 0; k < 3; ++k) if ((rc = alloc(&S.sigma_ev[k], n))) return rc;
    if ((rc = alloc(&S.q_lookup_ev, n))) return rc;
    if ((rc = alloc(&S.roots, n))) return rc;

    // extend_prover_key (keys/mod.rs:78-146) on the device
    const int pk_of_cs[10] = {PK_QM, PK_QL, PK_QR, PK_QO, PK_QC, PK_QLOOKUP, PK_QTABLE, PK_S1, PK_S2, PK_S3};
    for (int k = 0; k < 10; ++k)
        if ((rc = circuit_key_coset(c, S, S.pk[pk_of_cs[k]], n, S.coset[k]))) return rc;
    // sigma / q_lookup evaluations on the n domain (prove.rs:91-94)
    if ((rc = ntt_run(c, log_n, 0, 0, S.pk[PK_S1], n, S.sigma_ev[0]))) return rc;
    if ((rc = ntt_run(c, log_n, 0, 0, S.pk[PK_S2], n, S.sigma_ev[1]))) return rc;
    if ((rc = ntt_run(c, log_n, 0, 0, S.pk[PK_S3], n, S.sigma_ev[2]))) return rc;
    if ((rc = ntt_run(c, log_n, 0, 0, S.pk[PK_QLOOKUP], n, S.q_lookup_ev))) return rc;
    const F one = fe_one<R>();
    const F w = root_of_unity<R>(log_n), w4n = root_of_unity<R>(log_n + 2);
    const F g = fe_from_u32<R>(R::GENERATOR);
    if ((rc = gen_powers(c, S.roots, n, w.v, one.v))) return rc;                 // domain.elements()
    {   // x_coset = g * w4n^t (keys/mod.rs:110-113), t = cls + G i on this GPU
        const F step = fe_pow_u64<R>(w4n, (uint64_t)S.G), first = fe_mul<R>(g, fe_pow_u64<R>(w4n, (uint64_t)S.cls));
        if ((rc = gen_powers(c, S.coset[CS_X], m, step.v, first.v))) return rc;
    }
    if ((rc = circuit_l1_coset<R>(c, S, S.coset[CS_L1]))) return rc;
    // the tables that only ever multiply go to the quotient kernel's own Montgomery radix (poly.hpp)
    if ((rc = to_hat_form(c, S.coset[CS_QM], m, 1))) return rc;
    for (int k : {CS_QL, CS_QR, CS_QO, CS_QLOOKUP, CS_QTABLE, CS_L1})
        if ((rc = to_hat_form(c, S.coset[k], m, 0))) return rc;
    F zh[4];
    circuit_zh4<R>(log_n, zh);
    for (int j = 0; j < 4; ++j) {
        if (fe_is_zero<R>(zh[j])) return set_err(c, ZKT_ERR_ZERO_DENOMINATOR, "vanishing polynomial is zero on the coset");
        const F inv = fe_inv_host<R>(zh[j]);
        memcpy(S.zh_inv[j], inv.v, 32);
    }
    ZKT_HIP(c, hipStreamSynchronize(c->stream));
    c->circuit = st;
    return ZKT_OK;
}

// setup.rs:104-121: PC::commit of the ten labelled polynomials of the loaded circuit, ProverKey order, in batches of the
// MSM's slot count: the one commit stage of zkt_circuit_setup (lens[k] = n) and of zkt_circuit_commitments / _check_vk_file
// (the trimmed lengths; the zero polynomial commits to the identity without an MSM).  Identity = (0, 0) and the flag.
int circuit_commit_keys(zkt_ctx* c, CircuitState& S, const size_t* lens, uint64_t* out_commitments, int* out_is_inf) {
    const int L = c->curve == ZKT_CURVE_BN254 ? 4 : 6;
    int rc;
    size_t off = 0, cnt = 0, total = 0;
    msm_slice(c, &off, &cnt, &total);
    for (int k = 0; k < PK_COUNT; ++k)
        if (lens[k] > S.n || (c->sharded() && lens[k] > total))
            return set_err(c, ZKT_ERR_TOO_MANY_COEFFICIENTS, "TooManyCoefficients: polynomial longer than the committer key");
    for (int k0 = 0; k0 < PK_COUNT; k0 += 5) {
        const int kk = std::min(5, PK_COUNT - k0);
        uint64_t xy[5 * 12] = {};
        if (!c->sharded()) {
            for (int k = 0; k < kk; ++k)
                if (lens[k0 + k] && (rc = msm_begin(c, S.pk[k0 + k], lens[k0 + k], 0, 1, k))) return rc;
            for (int k = 0; k < kk; ++k)
                if (lens[k0 + k] && (rc = msm_end(c, k, xy + 12 * k))) return rc;
        } else {   // this rank's slice of the coefficients; one all-gather per batch
            int slots[5];
            bool have[5];
            for (int k = 0; k < kk; ++k) {
                const size_t len = lens[k0 + k];
                slots[k] = k;
                have[k] = len > off;
                if (have[k] && (rc = msm_begin(c, (const char*)S.pk[k0 + k] + off * 32, std::min(len, off + cnt) - off, 0, 1, k)))
                    return rc;
            }
            if ((rc = msm_end_sharded(c, slots, have, kk, xy))) return rc;
        }
        for (int k = 0; k < kk; ++k) {
            bool inf = true;   // the identity comes back as (0, 0)
            for (int i = 0; i < 2 * L; ++i) inf = inf && xy[12 * k + i] == 0;
            if (out_is_inf) out_is_inf[k0 + k] = inf ? 1 : 0;
            for (int i = 0; i < 2 * L; ++i) out_commitments[(size_t)(k0 + k) * 2 * L + i] = xy[12 * k + i];
        }
    }
    return ZKT_OK;
}

// setup.rs:42-166 on the device: polynomials from the evaluation vectors, ExtendedProverKey, the ten commitments
static int circuit_setup(zkt_ctx* c, int log_n, const uint64_t* const* evals, const size_t* lens, unsigned evals_dev_mask,
                         uint64_t* out_commitments, int* out_is_inf) {
    int rc = by_curve(c->curve, [&](auto C) { return circuit_load_t<decltype(C)>(c, log_n, evals, lens, true, evals_dev_mask); });
    if (rc) return rc;
    CircuitState& S = *c->circuit;
    size_t full[PK_COUNT];
    for (auto& l : full) l = S.n;   // the polynomials as the inverse transforms left them, untrimmed
    return circuit_commit_keys(c, S, full, out_commitments, out_is_inf);
}

// The ten ProverKey polynomials' lengths as DensePolynomial::from_coefficients_vec leaves them (trailing zeros stripped, the
// zero polynomial 0), taken on the device, whatever lengths the load was given.  Reads the keys and a word vector of its
// own: no work buffer, so it may run beside an announced proof's early rounds, on a fork and on a sharded context.
int circuit_key_lens(zkt_ctx* c, const CircuitState& S, size_t* lens10) {
    DevSet tmp(c->device);
    void* d = nullptr;
    int rc = tmp.alloc(c, &d, PK_COUNT * 4);
    if (rc) return rc;
    uint32_t h[PK_COUNT] = {};
    ZKT_HIP(c, hipMemsetAsync(d, 0, PK_COUNT * 4, c->stream));
    for (int k = 0; k < PK_COUNT && !rc; ++k) rc = poly_trim_len(c, S.pk[k], S.n, (uint32_t*)d + k);
    if (!rc && hipMemcpyAsync(h, d, PK_COUNT * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess)
        rc = set_err(c, ZKT_ERR_HIP, "downloading the key lengths failed");
    const hipError_t e = hipStreamSynchronize(c->stream);   // before `tmp` goes, whatever happened
    if (rc) return rc;
    ZKT_HIP(c, e);
    for (int k = 0; k < PK_COUNT; ++k) lens10[k] = h[k];
    return ZKT_OK;
}

// With a communicator attached every rank must hold exactly its zkt_shard_range of the key: a rank that loaded the
// whole key (or somebody else's slice) would make the combined commitments a multiple of the right ones.
int check_sharded_key(zkt_ctx* c) {
    if (!c->sharded()) return ZKT_OK;
    size_t off = 0, cnt = 0, total = 0, lo = 0, hi = 0;
    msm_slice(c, &off, &cnt, &total);
    (void)zkt_shard_range(total, c->comm.vt.rank, c->comm.vt.world, &lo, &hi);
    if (off != lo || off + cnt != hi)
        return set_err(c, ZKT_ERR_INVALID_ARGUMENT,
                       "sharded proof: this rank must load powers zkt_shard_range(total, rank, world) with zkt_srs_load_slice");
    if (c->circuit && c->circuit->G != c->comm.vt.world)
        return set_err(c, ZKT_ERR_NOT_LOADED, "the circuit was loaded for another communicator");
    return ZKT_OK;
}

}  // namespace zkt

using namespace zkt;

extern "C" {

int zkt_circuit_load(zkt_ctx* c, int log_n, const uint64_t* const* pk_polys, const size_t* pk_lens) {
    if (!c || !pk_polys || !pk_lens) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    (void)hipSetDevice(c->device);
    return by_curve(c->curve, [&](auto C) { return circuit_load_t<decltype(C)>(c, log_n, pk_polys, pk_lens); });
}

int zkt_circuit_setup(zkt_ctx* c, int log_n, const uint64_t* const* evals, const size_t* eval_lens, int evals_on_device,
                      uint64_t* out_commitments, int* out_is_infinity) {
    if (!c || !evals || !eval_lens || !out_commitments) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (!c->msm) return set_err(c, ZKT_ERR_NOT_LOADED, "no SRS loaded (zkt_srs_load)");
    (void)hipSetDevice(c->device);
    if (log_n < 3 || log_n > 26) return set_err(c, ZKT_ERR_INVALID_DOMAIN_SIZE, "circuit bound out of range");
    if (int rc0 = check_sharded_key(c)) return rc0;
    const unsigned mask = evals_on_device ? (1u << PK_COUNT) - 1u : 0u;
    return circuit_setup(c, log_n, evals, eval_lens, mask, out_commitments, out_is_infinity);
}

int zkt_circuit_setup_wiring(zkt_ctx* c, int log_n, const uint64_t* const* evals, const size_t* eval_lens, int evals_on_device,
                             const uint32_t* w_l, const uint32_t* w_r, const uint32_t* w_o, size_t n_rows, size_t n_vars,
                             int wiring_on_device, uint64_t* out_commitments, int* out_is_infinity) {
    if (!c || !evals || !eval_lens || !out_commitments) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (!c->msm) return set_err(c, ZKT_ERR_NOT_LOADED, "no SRS loaded (zkt_srs_load)");
    (void)hipSetDevice(c->device);
    const int max_log_n = (c->curve == ZKT_CURVE_BN254 ? Bn254Fr::TWO_ADICITY : Bls381Fr::TWO_ADICITY) - 2;
    if (log_n < 3 || log_n > 25 || log_n > max_log_n)   // what zkt_circuit_load accepts (the 4n domain), 32-bit wire positions
        return set_err(c, ZKT_ERR_INVALID_DOMAIN_SIZE, "circuit bound out of range");
    if (int rc0 = check_sharded_key(c)) return rc0;
    if (int rf = refuse_if_forked(c, "loading a circuit")) return rf;
    // from here on as a failing zkt_circuit_setup: the previous circuit is gone
    circuit_release(c);
    const size_t n = (size_t)1 << log_n;
    if (n_rows > n) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "more wiring rows than the domain size");
    for (int k = PK_S1; k <= PK_S3; ++k)
        if (evals[k] || eval_lens[k])
            return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "zkt_circuit_setup_wiring makes sigma1..3 itself: entries 5, 6, 7 must be NULL / 0");
    if (n_rows && (!w_l || !w_r || !w_o)) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null wiring pointer");
    // the call's own buffers: the three sigma vectors and, for host wiring, the uploaded indices
    DevSet tmp(c->device);
    void* held[6] = {};
    int rc = ZKT_OK;
    for (int k = 0; k < 3 && !rc; ++k) rc = tmp.alloc(c, &held[k], n * 32);
    const uint32_t* w[3] = {w_l, w_r, w_o};
    if (!wiring_on_device && n_rows) {
        for (int k = 0; k < 3 && !rc; ++k) {
            rc = tmp.alloc(c, &held[3 + k], n_rows * 4);
            if (!rc && hipMemcpyAsync(held[3 + k], w[k], n_rows * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess)
                rc = set_err(c, ZKT_ERR_HIP, "uploading the wiring failed");
            w[k] = (const uint32_t*)held[3 + k];
        }
    }
    if (!rc) rc = sigma_build(c, log_n, w[0], w[1], w[2], n_rows, n_vars, held);
    if (!rc) {
        const uint64_t* ev[PK_COUNT];
        size_t lens[PK_COUNT];
        for (int k = 0; k < PK_COUNT; ++k) { ev[k] = evals[k]; lens[k] = eval_lens[k]; }
        unsigned mask = evals_on_device ? (1u << PK_COUNT) - 1u : 0u;
        for (int k = 0; k < 3; ++k) {
            ev[PK_S1 + k] = (const uint64_t*)held[k];
            lens[PK_S1 + k] = n;
            mask |= 1u << (PK_S1 + k);
        }
        rc = circuit_setup(c, log_n, ev, lens, mask, out_commitments, out_is_infinity);
    }
    (void)hipStreamSynchronize(c->stream);   // before `tmp` goes
    return rc;
}

}  // extern "C"
