// Device-resident PLONK+Plookup prover: host orchestration of the five rounds of
// plonk-core/src/proof_system/prove.rs:59-470.  Witness vectors are uploaded once; every
// polynomial stays in HBM between rounds; only commitments (affine points), the 12 evaluations and
// two scalars (the grand-product denominators) cross PCIe, for the host-side Fiat-Shamir transcript.
#include "ctx.hpp"
#include "hostinv.hpp"
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include "ec.hpp"
#include "keyfile.hpp"
#include "keyfile_write.hpp"
#include "linearisation.hpp"
#include "msm.hpp"
#include "poly.hpp"
#include "quotient_classes.hpp"
#include "transcript.hpp"

#include <algorithm>
#include <functional>
#include <cstring>
#include <memory>
#include <optional>
#include <vector>

namespace zkt {

enum { PK_QM = 0, PK_QL, PK_QR, PK_QO, PK_QC, PK_S1, PK_S2, PK_S3, PK_QLOOKUP, PK_QTABLE, PK_COUNT };
// coset vectors kept on the device (keys/mod.rs:153-174; x and l_1 are stored, zh is 4 scalars)
enum { CS_QM = 0, CS_QL, CS_QR, CS_QO, CS_QC, CS_QLOOKUP, CS_QTABLE, CS_S1, CS_S2, CS_S3, CS_X, CS_L1, CS_COUNT };
enum { W_A = 0, W_B, W_C, W_PI, W_Z1, W_Z2, W_T, W_H1, W_H2, W_COUNT };  // witness cosets of quotient_poly.rs:52-96

// The keys (ProverKey polynomials, ExtendedProverKey cosets, sigma / q_lookup evaluations, domain roots): read-only for a
// prover, so a fork reads its source's (circuit_fork)
struct CircuitKeys {
    std::shared_ptr<DevShared> keys_mem;   // owns every array below
    void* pk[PK_COUNT] = {};
    size_t pk_len[PK_COUNT] = {};
    void* coset[CS_COUNT] = {};
    void* sigma_ev[3] = {};
    void* q_lookup_ev = nullptr;
    void* roots = nullptr;
    uint32_t zh_inv[4][8] = {};
};
// The tables of the quotient on classes 0, 1, 2 of the 4n coset (quotient_classes.hpp): ccoset[] are coset[] as [3][n]
// class arrays, key_win the windows of sigma1..3 and q_lookup.  Built on first use (ensure_class_tables), keys as well:
// contexts forked afterwards read them.
struct ClassTables {
    std::shared_ptr<DevShared> class_mem;   // owns ccoset[]
    void* ccoset[CS_COUNT] = {};
    bool ccoset_ready = false;
    uint32_t key_win[4][QCW][8] = {};
    uint32_t qc_gamma[4][8] = {}, qc_vinv[9][8] = {}, qc_g3[3][8] = {};
};

struct CircuitState : CircuitKeys, ClassTables {
    // owns everything circuit_alloc_work makes: the per-proof buffers, pinned staging, streams and events below
    DevSet work;
    explicit CircuitState(int device) : work(device) {}
    int log_n = 0;
    size_t n = 0;
    // A proof sharded over G GPUs (zkt_ctx_set_comm): this GPU owns the 4n-coset points of global index cls modulo G,
    // m = 4n / G of them; coset[] and wcos[] hold that class only.  G = 1: the whole coset, as the reference has it.
    int G = 1, cls = 0, log_m = 0;
    size_t m = 0;
    void* wnext[4] = {};       // G = 8: z1, z2, t, h1 on the class (cls + 4) mod 8, where "omega-next" lives
    void* fold = nullptr;      // m elements: a polynomial folded modulo X^m - shift^m before its class transform
    void* qgather = nullptr;   // 4n elements: every rank's quotient evaluations, class-major (the all-gather's target)
    bool have[16] = {};        // commitment slot -> this rank's SRS slice takes part (an MSM was started)
    // per-proof work buffers
    void* ev[8] = {};       // a, b, c, t, f, h1, h2, pi   (n each)
    void* sc[4] = {};       // scan scratch: num, den, PN, SD (n each)
    void* scan_tmp = nullptr;
    void* poly[13] = {};    // a b c t h1 h2 z1 z2 pi q_lo q_mid q_hi work   (n + 8 each)
    void* wcos[W_COUNT] = {};
    void* qev = nullptr;    // 4n
    // scalars of a commitment taken in the Lagrange basis (read by the MSM's level-1 kernels only): n + 16 each; one per
    // commitment that may wait in the queue of a round (t, h1, h2; z2), the last also stages zkt_commit_evals_dev's blinders
    void* lag_scalars = nullptr;
    void* lag_scalars_q[3] = {};
    void* small = nullptr;  // blinders (19), eval partials, eval results
    uint32_t* status = nullptr;  // [0] error bits, [1] len scratch ... [4..7] quotient lens, [8..] poly lens
    uint32_t* lk_u32 = nullptr;  // lookup: perm, base counts, starts of the even half, of the odd half, hit counts
    uint32_t lk_nkeys = 0;       // keys of the resident lookup tables (0 = none)
    std::vector<uint32_t> lk_host_keys, lk_host_sorted, lk_host_counts, lk_host_order;   // host staging (8 words per key)
    // zkt_prove_set_next: rounds 1 and 2 of the NEXT proof depend on no challenge; they are issued behind the last
    // commitments of the current proof, so the GPU never drains between two proofs
    // Round 1 of the next proof goes behind the quotient commitments of round 4, round 2 behind the opening commitments
    // of round 5.  Round 1 overwrites what round 5 of the current proof still reads (the wire polynomials) and both
    // use the status words, so those exist twice; `*_alt` is the set the early work writes.
    bool has_next = false, prefetch_same_table = false;
    int prefetch_stage = 0;        // 0 nothing, 1 round 1 issued, 2 rounds 1 and 2 issued (only then it is usable)
    uint64_t prefetch_epoch = 0;   // zkt_ctx::msm_epoch right after the early work was issued
    zkt_prove_inputs next_in{}, prefetch_in{};
    void* poly_alt[3] = {};
    uint32_t* status_alt = nullptr;
    void* lk_keys = nullptr;     // insertion-order keys then sorted keys
    size_t lk_cap = 0;
    void* pinned = nullptr;
    hipStream_t comm_stream = nullptr;   // sharded proof, asynchronous communicator: the quotient exchange's pieces travel here
    hipEvent_t ev_piece[ZKT_QUOTIENT_CHUNKS] = {}, ev_gathered = nullptr;
    // Round 5: the second opening's polynomial work (a linear combination and a division: memory-bound) runs on this stream
    // beside the first opening's commitment (integer-ALU bound), in buffers of its own
    hipStream_t aux_stream = nullptr;
    hipEvent_t ev_aux_go = nullptr, ev_aux_done = nullptr;
    void* aux_scan_tmp = nullptr;
    void* aux_pw = nullptr;
    hipStream_t copy_stream = nullptr;   // host witness uploads travel beside the main stream's work (cold path)
    hipEvent_t ev_copy[4] = {};          // a, b, c uploaded; [3]: main stream reached the upload point
    void* pinned_pi = nullptr;      // host staging of pi_tab
    uint32_t* pi_tab = nullptr;     // device: QUOTIENT_PI_DIRECT_MAX entries of {rotation, 9 limbs}
    void* eval_pw = nullptr;        // round 5: EVAL_MAX x 257 powers of the evaluation points, or (fused passes) the opening tables of xi and xi w
    // The table polynomial depends on the lookup table only: while consecutive proofs pass the same table its
    // evaluations, coefficients, 4n-coset and commitment are reused (one MSM and two transforms less).
    std::vector<uint64_t> cached_table;
    bool t_cached = false, t_coset_valid = false;
    uint64_t t_srs_generation = 0;   // zkt_ctx::srs_generation the cached commitment was made under
    uint64_t t_commit_xy[12] = {};
    // wire base tables (lagrange.hip): the wires of the round 1 last enqueued that were committed over them; their digest
    // and trimmed lengths are compared when that round is collected (collect_wires)
    bool wire_route[3] = {};
    bool wire_dense_only = false;   // zkt_debug_commit_wires_dev route 0
    int wire_elim_force = -1;       // zkt_debug_commit_wires_dev: 0 = per-variable tables only (route 1), 1 = over free variables (route 2)
    // The quotient on classes 0, 1, 2 of the 4n coset (single GPU, zkt_ctx_set_quotient_route; ClassTables above): wcos[]
    // then hold [3][n] as well.
    bool use_classes = false;       // the route of the proof in flight: layout of wcos[] and of the resident t coset
    void* heads = nullptr;          // 3 x NTT_MAX_BATCH x NTT_HEAD folded head coefficients of the batch being transformed
    void* d_win = nullptr;          // QC_WIN_POLYS windows (a b c z1 z2 t), gathered in round 3 ...
    void* pinned_win = nullptr;     // ... and copied here behind them
    hipEvent_t ev_win = nullptr;
    uint32_t last_u[6][8] = {};     // zkt_debug_quotient_top
    bool last_u_valid = false;
};

// ---- host field helpers ------------------------------------------------------------------------------
template <class P>
struct HostF {
    using F = Fe<P>;
    static F from_words(const uint64_t* w) {
        F r;
        memcpy(r.v, w, 32);
        return r;
    }
    static void to_le_bytes(const F& mont, uint8_t out[32]) {
        F c = fe_from_mont<P>(mont);
        memcpy(out, c.v, 32);
    }
    static F from_le_bytes(const uint8_t in[32]) {
        F c;
        memcpy(c.v, in, 32);
        return fe_to_mont<P>(c);
    }
};

template <class Q>
static void fq_to_le(const Fe<Q>& mont, uint8_t* out) {
    Fe<Q> c = fe_from_mont<Q>(mont);
    memcpy(out, c.v, Q::N * 4);
}

// ark-serialize 0.3 compressed short-Weierstrass point (proof wire format, proof.rs:98-155):
// x little-endian, bit 7 of the last byte = y > -y, bit 6 = infinity.
template <class Q>
static void serialize_point(const Affine<Q>& p, std::vector<uint8_t>& out) {
    const size_t nb = Q::N * 4;
    std::vector<uint8_t> b(nb, 0);
    if (aff_is_inf<Q>(p)) {
        b[nb - 1] |= 0x40;
    } else {
        fq_to_le<Q>(p.x, b.data());
        Fe<Q> y = fe_from_mont<Q>(p.y);
        Fe<Q> ny = fe_from_mont<Q>(fe_neg<Q>(p.y));
        bool greater = false;
        for (int i = Q::N - 1; i >= 0; --i) {
            if (y.v[i] != ny.v[i]) {
                greater = y.v[i] > ny.v[i];
                break;
            }
        }
        if (greater) b[nb - 1] |= 0x80;
    }
    out.insert(out.end(), b.begin(), b.end());
}

// Public inputs the quotient kernel evaluates itself (poly.hpp): rows of {rotation, nine 29-bit limbs of the value}; the
// rotation 4 pos / G is in entries of a class of a coset split G ways (1: the whole coset)
template <class R>
static void pi_rows(const uint64_t* pi_pos, const uint64_t* pi_vals, size_t n_pi, size_t G, uint32_t* tab) {
    for (size_t i = 0; i < n_pi; ++i) {
        tab[10 * i] = (uint32_t)(4 * pi_pos[i] / G);
        const Fx<R> v = fx_unpack<R>(HostF<R>::from_words(pi_vals + 4 * i));
        for (int w = 0; w < 9; ++w) tab[10 * i + 1 + w] = v.l[w];
    }
}

// The quotient kernel's arguments (quotient_poly.rs:52-224).  _vectors: the twelve coset tables and the nine witness cosets,
// each `off` bytes into its vector (the classes route's [3][n] arrays); quotient_args: the whole-coset keys, the witness,
// the challenges (8 Montgomery words each) and zh_inv.  Output, size and public inputs are the caller's.
static void quotient_vectors(QuotientArgs& q, void* const cs[CS_COUNT], void* const w[W_COUNT], size_t off) {
    auto at = [&](void* const* v, int k) { return (const void*)((const char*)v[k] + off); };
    q.q_m = at(cs, CS_QM); q.q_l = at(cs, CS_QL); q.q_r = at(cs, CS_QR); q.q_o = at(cs, CS_QO); q.q_c = at(cs, CS_QC);
    q.q_lookup = at(cs, CS_QLOOKUP); q.q_table = at(cs, CS_QTABLE); q.x = at(cs, CS_X); q.l1 = at(cs, CS_L1);
    q.sigma1 = at(cs, CS_S1); q.sigma2 = at(cs, CS_S2); q.sigma3 = at(cs, CS_S3);
    q.a = at(w, W_A); q.b = at(w, W_B); q.c = at(w, W_C); q.pi = at(w, W_PI);
    q.z1 = at(w, W_Z1); q.z2 = at(w, W_Z2); q.t = at(w, W_T); q.h1 = at(w, W_H1); q.h2 = at(w, W_H2);
}
static QuotientArgs quotient_args(const CircuitState& S, void* const w[W_COUNT], const void* alpha, const void* beta,
                                  const void* gamma, const void* delta, const void* epsilon) {
    QuotientArgs q{};
    quotient_vectors(q, S.coset, w, 0);
    memcpy(q.alpha, alpha, 32); memcpy(q.beta, beta, 32); memcpy(q.gamma, gamma, 32);
    memcpy(q.delta, delta, 32); memcpy(q.epsilon, epsilon, 32);
    memcpy(q.zh_inv, S.zh_inv, sizeof(q.zh_inv));
    return q;
}

constexpr int WIRE_ELIM_MIN_LOG_N = 17;   // zkt_ctx_set_wire_elimination mode 1: circuits from this size on
// zkt_ctx_set_quotient_route mode 0: the quotient on three classes from this size on (docs/EXPERIMENTS.md "Round 4 on
// classes: one launch per stage": with the class in the grid every run of the route beats every run of the whole coset at
// 2^18 and 2^19; nothing below 2^18 was measured)
constexpr int QUOTIENT_CLASSES_MIN_LOG_N = 18;

template <class C>
struct Prover {
    using R = typename C::Fr;
    using Q = typename C::Fq;
    using F = Fe<R>;
    using H = HostF<R>;

    zkt_ctx* c;
    CircuitState& S;
    HostTranscript& tr;
    const size_t cap;   // elements of a polynomial's buffer
    void *const d_partials, *const d_results;   // round 5's small device results; the openings' totals go behind the evaluations
    Prover(zkt_ctx* ctx, CircuitState& st, HostTranscript& t)
        : c(ctx), S(st), tr(t), cap(st.n + 8), d_partials((char*)st.small + 64 * 32), d_results((char*)st.small + 32 * 32) {
        trace_on = exp_env("ZKT_HOST_TRACE") != nullptr;
    }
    bool copy_fenced = false;   // the copy stream already waits for the main stream's earlier work (run(), cold path)
    // ZKT_HOST_TRACE=1: wall-clock marks of the host control path (where the GPU may be waiting for the host)
    bool trace_on = false;
    std::vector<std::pair<const char*, std::chrono::steady_clock::time_point>> marks;
    void mark(const char* what) {
        if (trace_on) marks.emplace_back(what, std::chrono::steady_clock::now());
    }
    void dump_marks() {
        if (!trace_on || marks.empty()) return;
        for (size_t i = 1; i < marks.size(); ++i)
            fprintf(stderr, "[zkt host] %-28s %8.1f us\n", marks[i].first,
                    std::chrono::duration<double, std::micro>(marks[i].second - marks[i - 1].second).count());
        marks.clear();
    }

    void tr_commit(const char* label, const Affine<Q>& p) {
        uint8_t x[64], y[64];
        bool inf = aff_is_inf<Q>(p);
        if (!inf) {
            fq_to_le<Q>(p.x, x);
            fq_to_le<Q>(p.y, y);
        }
        tr.append_commitment(label, x, y, Q::N * 4, inf);
    }
    void tr_scalar(const char* label, const F& v) {
        uint8_t b[32];
        H::to_le_bytes(v, b);
        tr.append_scalars(label, b, 1, 32, true);
    }
    F tr_challenge(const char* label) {
        uint8_t b[32];
        tr.challenge_scalar(label, R::BITS, b);
        return H::from_le_bytes(b);
    }
    static void put(uint32_t dst[8], const F& v) { memcpy(dst, v.v, 32); }

    // Idle time of the main stream across a host round trip (zkt_profile_get "host_wait"): the first event is recorded
    // behind everything enqueued when the host starts to wait (it fires when the stream drains), the second right
    // before the next launch.  bench.py's gpu_active is the wall clock minus these.
    std::optional<ProfScope> idle;
    void wait_begin() {
        if (c->prof_on && !idle) idle.emplace(c, "host_wait");
    }
    void wait_end() { idle.reset(); }

    // commitments of one round are enqueued back to back (the bucket-reduction tail of one overlaps the
    // accumulation of the next) and collected together
    // With the committer key sharded by index range, a commitment is this rank's partial sum over
    // coefficients [slice_off, slice_off + slice_count) -- nothing at all when the polynomial ends below the slice.
    int commit_begin(const void* d_poly, size_t len, int slot) {
        if (!c->sharded()) return msm_begin(c, d_poly, len, 0, 1, slot);
        size_t off, cnt, total;
        msm_slice(c, &off, &cnt, &total);
        if (len > total)
            return set_err(c, ZKT_ERR_TOO_MANY_COEFFICIENTS, "TooManyCoefficients: polynomial longer than the committer key");
        S.have[slot] = len > off;
        if (!S.have[slot]) return ZKT_OK;
        const size_t l = std::min(len, off + cnt) - off;
        return msm_begin(c, (const char*)d_poly + off * 32, l, 0, 1, slot);
    }
    // Commitments wait in a queue until the round has begun them all (commit_flush), then go out in batches of up to
    // MSM_BATCH launches-as-one (msm.hip msm_enqueue_batch: blockIdx.y = MSM, either base table per entry).  Large and sharded
    // keys issue every commitment at once instead (msm_batches_grouping says which sizes gain).
    struct Pending {
        const void* scalars;
        size_t len;
        int slot, tbl;
    };
    Pending queue[6];
    int n_queue = 0, n_lag_queued = 0;
    bool queueing() const { return !c->sharded() && !c->batch_off && msm_batches_grouping(c); }
    int commit_flush() {
        const int k = n_queue;
        const void* sc[6];
        size_t lens[6];
        int slots[6], tbls[6];
        for (int j = 0; j < k; ++j) {
            sc[j] = queue[j].scalars; lens[j] = queue[j].len; slots[j] = queue[j].slot; tbls[j] = queue[j].tbl;
        }
        n_queue = 0;
        n_lag_queued = 0;
        return msm_begin_many(c, k, sc, lens, 1, slots, tbls, true);
    }
    int commit_push(const void* scalars, size_t len, int slot, int tbl) {
        if (n_queue == 6)
            if (int rc = commit_flush()) return rc;
        queue[n_queue++] = Pending{scalars, len, slot, tbl};
        return ZKT_OK;
    }
    int commit_begin_many(void* const* d_polys, const size_t* lens, const int* slots, int k) {
        for (int j = 0; j < k; ++j) {
            const int rc = queueing() ? commit_push(d_polys[j], lens[j], slots[j], 0) : commit_begin(d_polys[j], lens[j], slots[j]);
            if (rc) return rc;
        }
        return ZKT_OK;
    }
    // Commitment of the polynomial with evaluations `ev` plus k blinders (prove.rs:166-180,249-251), whose blinded
    // coefficients are in d_poly.  With the Lagrange-basis table (lagrange.hip) the scalars are the differences of
    // neighbouring evaluations: for t, h1, h2 and z2 all but a few thousand of them are zero and the MSM costs next to
    // nothing; without it (sharded key, key shorter than n + 1) the coefficients are committed as the reference does.
    int commit_evals_begin(const void* ev, const void* d_poly, int blinder_off, int k, int len_slot, int slot) {
        const bool q = queueing();
        if (!lagrange_ready(c, S.log_n) || c->lagrange_off)
            return q ? commit_push(d_poly, S.n + (size_t)k, slot, 0) : commit_begin(d_poly, S.n + (size_t)k, slot);
        if (q && n_lag_queued == 3)
            if (int rc0 = commit_flush()) return rc0;
        void* d = q ? S.lag_scalars_q[n_lag_queued] : S.lag_scalars;   // a queued commitment keeps its scalars until the flush
        int rc = lagrange_scalars(c, ev, S.n, S.status + 8 + len_slot, (const char*)S.small + (size_t)blinder_off * 32, k, S.roots, d);
        if (rc) return rc;
        if (!q) return msm_begin(c, d, S.n + (size_t)k, 0, 1, slot, 1);
        ++n_lag_queued;
        return commit_push(d, S.n + (size_t)k, slot, 1);
    }
    // The commitments of one prover round, collected together; skip[j]: nothing was started for entry j (out[j] is left
    // alone).  Sharded: ONE all-gather of the round's partial sums (msm.hip msm_collect_sharded).
    int commit_collect(const int* slots, const bool* skip, int k, Affine<Q>* out) {
        wait_begin();
        if (!c->sharded()) {
            for (int j = 0; j < k; ++j) {
                if (skip && skip[j]) continue;
                uint64_t xy[12];
                int rc = msm_end(c, slots[j], xy);
                if (rc) return rc;
                memcpy(out[j].x.v, xy, Q::N * 4);
                memcpy(out[j].y.v, xy + Q::N / 2, Q::N * 4);
            }
            return ZKT_OK;
        }
        bool have[16];
        uint64_t xy[16 * 12];
        for (int j = 0; j < k; ++j) have[j] = !(skip && skip[j]) && S.have[slots[j]];
        int rc = msm_end_sharded(c, slots, have, k, xy);   // the message has k entries on every rank, whatever `have` says
        if (rc) return rc;
        for (int j = 0; j < k; ++j) {
            if (skip && skip[j]) continue;
            memcpy(out[j].x.v, xy + 12 * j, Q::N * 4);
            memcpy(out[j].y.v, xy + 12 * j + Q::N / 2, Q::N * 4);
        }
        return ZKT_OK;
    }

    // Round 1 over wire base tables, once its commitments are collected (the stream has then passed the digest of the
    // index vectors and the trimmed lengths): a wire whose table was built from other index contents, or whose polynomial
    // was trimmed (its blinders then sit below X^n), is committed again through the coefficients in S.poly[k], before
    // anything is absorbed into the transcript.  took[k], when given: wire k kept its table's commitment.
    int collect_wires(Affine<Q>* cm, int* took = nullptr) {
        for (int k = 0; k < 3; ++k) {
            const bool routed = S.wire_route[k];
            S.wire_route[k] = false;
            if (took) took[k] = 0;
            if (!routed) continue;
            if (wire_bases_check(c, k, S.n)) {
                if (took) took[k] = wire_bases_route(c, k);
                continue;
            }
            static const int slot[1] = {0};
            int rc = msm_begin(c, S.poly[k], S.n + 2, 0, 1, 0);
            if (rc || (rc = commit_collect(slot, nullptr, 1, cm + k))) return rc;
        }
        return ZKT_OK;
    }

    // iNTT of n evaluations into a zero-tailed coefficient buffer, trim, blind (prove.rs:120-127 etc.); the polynomials
    // of one round go through the transform as ONE batch (one launch per pass)
    struct PolyJob {
        const void* ev;
        void* poly;
        int blinder_off, k, len_slot;
    };
    int evals_to_blinded_polys(const PolyJob* jobs, int nb) {
        const size_t n = S.n;
        int rc;
        const void* ins[NTT_MAX_BATCH];
        void* outs[NTT_MAX_BATCH];
        size_t lens[NTT_MAX_BATCH];
        for (int y = 0; y < nb; ++y) {
            ins[y] = jobs[y].ev;
            outs[y] = jobs[y].poly;
            lens[y] = n;
        }
        if ((rc = ntt_run_batch(c, S.log_n, 1, 0, nb, ins, lens, outs))) return rc;
        if (c->fused(4)) {   // one launch for the batch: slack, trimmed lengths, blinders
            TrimBlindSpec tb[NTT_MAX_BATCH];
            for (int y = 0; y < nb; ++y)
                tb[y] = TrimBlindSpec{jobs[y].poly, (const char*)S.small + (size_t)jobs[y].blinder_off * 32, S.status + 8 + jobs[y].len_slot,
                                      jobs[y].k > 0 ? jobs[y].k : -1};
            return poly_trim_blind(c, tb, nb, n, 8);
        }
        for (int y = 0; y < nb; ++y) {
            void* poly = jobs[y].poly;
            if (jobs[y].k > 0) {
                if ((rc = poly_trim_len(c, poly, n, S.status + 8 + jobs[y].len_slot, (char*)poly + n * 32, 8))) return rc;
                if ((rc = poly_add_blinders(c, poly, S.status + 8 + jobs[y].len_slot,
                                            (const char*)S.small + (size_t)jobs[y].blinder_off * 32, jobs[y].k, n + 8)))
                    return rc;
            } else {
                ZKT_HIP(c, hipMemsetAsync((char*)poly + n * 32, 0, 8 * 32, c->stream));
            }
        }
        return ZKT_OK;
    }
    int evals_to_blinded_poly(const void* ev, void* poly, int blinder_off, int k, int len_slot) {
        const PolyJob j{ev, poly, blinder_off, k, len_slot};
        return evals_to_blinded_polys(&j, 1);
    }

    int check_status() {
        uint32_t st = 0;
        ZKT_HIP(c, hipMemcpyAsync(&st, S.status, 4, hipMemcpyDeviceToHost, c->stream));
        wait_begin();
        ZKT_HIP(c, hipStreamSynchronize(c->stream));
        if (st & 16u) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "wire index outside the variable map");
        if (st & 4u) return set_err(c, ZKT_ERR_NOT_IN_TABLE, "ElementNotIndexedInTable: a looked-up value is not in the table");
        if (st & 8u) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "combine_split: h1/h2 length differs from n");
        if (st & 2u) return set_err(c, ZKT_ERR_QUOTIENT_TOO_SHORT, "quotient degree exceeds 3n+5: the circuit is not satisfied");
        if (st & 1u) return set_err(c, ZKT_ERR_QUOTIENT_TOO_SHORT, "quotient polynomial too short to split (prove.rs:287-300)");
        return ZKT_OK;
    }

    // lookup/multiset.rs:103-146 on the device; table = distinct values in insertion order
    // `fresh` = the lookup table differs from the previous proof's: its keys (insertion order and sorted), the
    // sort permutation and the base multiplicities are rebuilt and uploaded; otherwise they are still resident.
    int combine_split(const uint64_t* table, size_t table_len, bool fresh) {
        const size_t n = S.n;
        F* d_keys = (F*)S.lk_keys;
        F* d_sorted = d_keys + S.lk_cap;
        uint32_t* d_perm = S.lk_u32;
        uint32_t* d_base = S.lk_u32 + S.lk_cap;
        uint32_t* d_even = S.lk_u32 + 2 * S.lk_cap;
        uint32_t* d_odd = S.lk_u32 + 3 * S.lk_cap;
        uint32_t* d_hits = S.lk_u32 + 4 * S.lk_cap;   // zero between proofs (k_lookup_starts clears what it reads)
        if (fresh || S.lk_nkeys == 0) {
            S.lk_nkeys = 0;   // no resident keys until the new ones are checked and uploaded
            // host staging lives in the circuit state (the copies below are asynchronous and nothing here waits)
            static_assert(sizeof(F) == 32, "scalar field element = 8 words");
            S.lk_host_keys.resize((table_len + 1) * 8);
            S.lk_host_sorted.resize((table_len + 1) * 8);
            std::vector<uint32_t>& counts = S.lk_host_counts;
            std::vector<uint32_t>& order = S.lk_host_order;
            struct Span {   // a growable view of F over the word vectors
                std::vector<uint32_t>& w;
                size_t len;
                F& operator[](size_t i) { return *reinterpret_cast<F*>(w.data() + 8 * i); }
                void resize(size_t k) { len = k; }
                void push_back(const F& v) { (*this)[len] = v; ++len; }
                size_t size() const { return len; }
                F* data() { return reinterpret_cast<F*>(w.data()); }
            };
            Span keys{S.lk_host_keys, 0}, sorted{S.lk_host_sorted, 0};
            keys.resize(table_len);
            for (size_t i = 0; i < table_len; ++i) keys[i] = H::from_words(table + 4 * i);
            counts.assign(table_len, 1u);
            // t is padded with zeros to n (lookup/table.rs:52-61): they join the zero key or create it
            size_t zero_idx = table_len;
            for (size_t i = 0; i < table_len; ++i)
                if (fe_is_zero<R>(keys[i])) {
                    zero_idx = i;
                    break;
                }
            if (n > table_len) {
                if (zero_idx == table_len) {
                    keys.push_back(fe_zero<R>());
                    counts.push_back(0);
                }
                counts[zero_idx] += (uint32_t)(n - table_len);
            }
            const uint32_t nk = (uint32_t)keys.size();
            if (nk + 2 > S.lk_cap) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "lookup table larger than the circuit bound");
            order.resize(nk);
            for (uint32_t i = 0; i < nk; ++i) order[i] = i;
            auto less = [&](uint32_t a, uint32_t b) {
                for (int i = R::N - 1; i >= 0; --i) {
                    if (keys[a].v[i] != keys[b].v[i]) return keys[a].v[i] < keys[b].v[i];
                }
                return false;
            };
            std::sort(order.begin(), order.end(), less);
            // a LookupTable is an IndexSet (lookup/table.rs:19): equal values, now adjacent, would each get their own
            // count and split the hits between them, a multiset the reference cannot build
            for (uint32_t i = 1; i < nk; ++i)
                if (!less(order[i - 1], order[i]))
                    return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "lookup table holds a repeated value");
            sorted.resize(nk);
            for (uint32_t i = 0; i < nk; ++i) sorted[i] = keys[order[i]];
            ZKT_HIP(c, hipMemcpyAsync(d_keys, keys.data(), nk * 32, hipMemcpyHostToDevice, c->stream));
            ZKT_HIP(c, hipMemcpyAsync(d_sorted, sorted.data(), nk * 32, hipMemcpyHostToDevice, c->stream));
            ZKT_HIP(c, hipMemcpyAsync(d_perm, order.data(), nk * 4, hipMemcpyHostToDevice, c->stream));
            ZKT_HIP(c, hipMemcpyAsync(d_base, counts.data(), nk * 4, hipMemcpyHostToDevice, c->stream));
            ZKT_HIP(c, hipMemsetAsync(d_hits, 0, (size_t)nk * 4, c->stream));   // a failed proof may have left counts behind
            S.lk_nkeys = nk;
        }
        const uint32_t nk = S.lk_nkeys;
        int rc;
        // a looked-up value outside the table sets status bit 4 (ElementNotIndexedInTable); like the other status
        // bits it is read at the next host round trip
        if ((rc = lookup_count(c, S.ev[4], n, d_sorted, d_perm, nk, d_hits, S.status))) return rc;
        if ((rc = lookup_starts(c, d_base, d_hits, nk, n, d_even, d_odd, S.status))) return rc;   // multiset.rs:126-143
        if ((rc = lookup_expand(c, d_keys, d_even, nk, S.ev[5], n))) return rc;
        if ((rc = lookup_expand(c, d_keys, d_odd, nk, S.ev[6], n))) return rc;
        return ZKT_OK;
    }

    static bool same_inputs(const zkt_prove_inputs& a, const zkt_prove_inputs& b) {
        return a.a_evals == b.a_evals && a.b_evals == b.b_evals && a.c_evals == b.c_evals && a.n_rows == b.n_rows &&
               a.table == b.table && a.table_len == b.table_len && a.pi_pos == b.pi_pos && a.pi_vals == b.pi_vals &&
               a.n_pi == b.n_pi && a.blinders == b.blinders && a.wires_on_device == b.wires_on_device &&
               a.variables == b.variables && a.n_vars == b.n_vars && a.w_l == b.w_l && a.w_r == b.w_r && a.w_o == b.w_o;
    }
    static constexpr int coset_src[W_COUNT] = {0, 1, 2, 8, 6, 7, 3, 4, 5};  // S.poly[] of a b c pi z1 z2 t h1 h2
    int to_coset(int k) {
        // quotient_poly.rs:52-96 needs every witness polynomial on the 4n coset.  None of those transforms depends on a
        // challenge, so each is issued right behind the commitment of its polynomial, where it hides the latency-bound
        // tail of the last MSM of the round (which runs on the side stream).
        if (S.use_classes) return to_coset_classes(&k, 1);
        if (S.G == 1) return ntt_run(c, S.log_n + 2, 0, 1, S.poly[coset_src[k]], S.n + 8, S.wcos[k]);
        // sharded proof: only this GPU's class of the 4n coset, one m-point transform, no exchange
        int rc = ntt_run_class(c, S.log_m, S.log_n + 2, S.cls, S.poly[coset_src[k]], S.n + 8, S.wcos[k], S.fold);
        if (rc || S.G < 8) return rc;
        static const int next_of[W_COUNT] = {-1, -1, -1, -1, 0, 1, 2, 3, -1};     // z1 z2 t h1 are read at "omega-next"
        if (next_of[k] < 0) return ZKT_OK;
        return ntt_run_class(c, S.log_m, S.log_n + 2, (S.cls + 4) & 7, S.poly[coset_src[k]], S.n + 8, S.wnext[next_of[k]], S.fold);
    }

    // Quotient on classes: the polynomials onto classes 0, 1, 2 of the 4n coset, wcos[k] as [3][n].  Per class ONE batched
    // n-point coset transform; the n + 8 coefficients folded modulo X^n - gamma_j differ from the first n in eight places,
    // which one small launch per batch prepares for all three classes (ntt_fold_heads).
    int to_coset_classes(const int* ks, int nb) {
        const void* ins[NTT_MAX_BATCH];
        void* outs[NTT_MAX_BATCH];
        size_t lens[NTT_MAX_BATCH];
        int rc;
        for (int y = 0; y < nb; ++y) {
            ins[y] = S.poly[coset_src[ks[y]]];
            lens[y] = S.n;
        }
        if ((rc = ntt_fold_heads(c, nb, ins, S.n, &S.qc_gamma[0][0], S.heads))) return rc;
        if (c->fused(8)) {   // the class in the grid: one launch per pass for the three classes, class j into wcos[k] + j n
            const int codes[3] = {ntt_class_code(S.log_n + 2, 0), ntt_class_code(S.log_n + 2, 1), ntt_class_code(S.log_n + 2, 2)};
            for (int y = 0; y < nb; ++y) outs[y] = S.wcos[ks[y]];
            return ntt_run_classes(c, S.log_n, 0, codes, nb, ins, lens, outs, 0, S.n, S.heads);
        }
        for (int j = 0; j < 3; ++j) {
            for (int y = 0; y < nb; ++y) outs[y] = (char*)S.wcos[ks[y]] + (size_t)j * S.n * 32;
            const void* head = (const char*)S.heads + (size_t)j * NTT_MAX_BATCH * NTT_HEAD * 32;
            if ((rc = ntt_run_batch(c, S.log_n, 0, ntt_class_code(S.log_n + 2, j), nb, ins, lens, outs, head))) return rc;
        }
        return ZKT_OK;
    }

    // several witness polynomials onto the 4n coset in one launch per pass (single GPU; a sharded proof transforms its
    // classes one by one)
    int to_coset_many(std::initializer_list<int> ks) {
        int rc;
        if (S.use_classes && ks.size() <= (size_t)NTT_MAX_BATCH) return ks.size() ? to_coset_classes(ks.begin(), (int)ks.size()) : ZKT_OK;
        if (S.G != 1 || ks.size() > (size_t)NTT_MAX_BATCH) {
            for (int k : ks) if ((rc = to_coset(k))) return rc;
            return ZKT_OK;
        }
        const void* ins[NTT_MAX_BATCH];
        void* outs[NTT_MAX_BATCH];
        size_t lens[NTT_MAX_BATCH];
        int nb = 0;
        for (int k : ks) {
            ins[nb] = S.poly[coset_src[k]];
            outs[nb] = S.wcos[k];
            lens[nb] = S.n + 8;
            ++nb;
        }
        return nb ? ntt_run_batch(c, S.log_n + 2, 0, 1, nb, ins, lens, outs) : ZKT_OK;
    }

    // ---- quotient on classes: which route this proof takes, and the route's tables ----
    // [3][n] class arrays of the twelve coset tables (the same elements, so whatever form a table is kept in carries over),
    // the windows of the key polynomials and the constants.  Once per circuit; a fork made afterwards shares the arrays.
    int ensure_class_tables() {
        if (S.ccoset_ready) return ZKT_OK;
        const size_t n = S.n;
        int rc;
        if (!S.class_mem) S.class_mem = std::make_shared<DevShared>(c->device);
        for (int k = 0; k < CS_COUNT; ++k) {
            if (!S.ccoset[k] && (rc = S.class_mem->alloc(c, &S.ccoset[k], 3 * n * 32))) return rc;
            if ((rc = quotient_classes_of_coset(c, S.coset[k], S.ccoset[k], n))) return rc;
        }
        static const int key_of[4] = {PK_S1, PK_S2, PK_S3, PK_QLOOKUP};
        memset(S.key_win, 0, sizeof(S.key_win));   // the key polynomials end at n: coefficients n - 6 .. n - 1
        for (int k = 0; k < 4; ++k)
            ZKT_HIP(c, hipMemcpyAsync(S.key_win[k], (const char*)S.pk[key_of[k]] + (n - 6) * 32, 6 * 32, hipMemcpyDeviceToHost, c->stream));
        ZKT_HIP(c, hipStreamSynchronize(c->stream));
        const QuotientClassConsts<R> q = quotient_class_consts<R>(S.log_n);
        for (int j = 0; j < 4; ++j) put(S.qc_gamma[j], q.gamma[j]);
        for (int j = 0; j < 9; ++j) put(S.qc_vinv[j], q.vinv[j]);
        for (int j = 0; j < 3; ++j) put(S.qc_g3[j], q.g3[j]);
        S.ccoset_ready = true;
        return ZKT_OK;
    }
    int choose_route() {
        int mode = c->quotient_route;
        if (const char* e = exp_env("ZKT_QUOTIENT_ROUTE")) mode = atoi(e);   // A/B runs of bench.py (experiment library only)
        const bool want = !c->sharded() && S.G == 1 && (mode == 1 || (mode == 0 && S.log_n >= QUOTIENT_CLASSES_MIN_LOG_N));
        if (want)
            if (int rc = ensure_class_tables()) return rc;
        if (want != S.use_classes) {   // what was transformed ahead of time has the other route's layout
            S.use_classes = want;
            S.t_coset_valid = false;
            S.prefetch_stage = 0;
        }
        return ZKT_OK;
    }

    void swap_work_sets() {   // current <-> alternate copies of what early work of the next proof overwrites
        for (int k = 0; k < 3; ++k) std::swap(S.poly[k], S.poly_alt[k]);
        std::swap(S.status, S.status_alt);
    }

    // Everything of rounds 1 and 2 that runs on the device (prove.rs:116-185): no challenge is needed before beta, so
    // these two parts touch no transcript and can be issued ahead of time (zkt_prove_set_next).  Commitments: slots 0-5.
    int enqueue_round_1(const zkt_prove_inputs& in) {
        const size_t n = S.n;
        int rc;
        ProfScope prof_round(c, "round1");
        if (in.n_rows > n) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "more rows than the circuit bound");
        if (in.table_len >= n) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "max table size is equal or larger than n");
        if (n < 8) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "circuit bound below 8");
        if (!in.blinders) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null blinders");
        ZKT_HIP(c, hipMemsetAsync(S.status, 0, 64 * 4, c->stream));
        ZKT_HIP(c, hipMemcpyAsync(S.small, in.blinders, 19 * 32, hipMemcpyHostToDevice, c->stream));

        // ---- round 1 (prove.rs:116-140) ----
        const uint64_t* wires[3] = {in.a_evals, in.b_evals, in.c_evals};
        const bool from_vars = in.a_evals == nullptr && in.variables != nullptr;
        const void* d_vars = in.variables;
        const uint32_t* d_idx[3] = {in.w_l, in.w_r, in.w_o};
        if (from_vars) {
            if (in.n_rows && (!in.w_l || !in.w_r || !in.w_o)) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null wire index vector");
            if (in.n_vars > 0xFFFFFFFEull) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "too many variables");
            if (!in.wires_on_device) {   // stage the composer's arrays: values in the (still unused) quotient vector
                if (in.n_vars > 4 * n || 3 * in.n_rows * 4 > (n + 8) * 32)
                    return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "witness larger than the staging buffers");
                if (in.n_vars)
                    ZKT_HIP(c, hipMemcpyAsync(S.qev, in.variables, in.n_vars * 32, hipMemcpyHostToDevice, c->stream));
                d_vars = S.qev;
                for (int k = 0; k < 3; ++k) {
                    uint32_t* dst = (uint32_t*)S.poly[12] + (size_t)k * in.n_rows;   // the round-5 work buffer
                    if (in.n_rows)
                        ZKT_HIP(c, hipMemcpyAsync(dst, d_idx[k], in.n_rows * 4, hipMemcpyHostToDevice, c->stream));
                    d_idx[k] = dst;
                }
            }
        }
        const bool host_wires = !from_vars && !in.wires_on_device;
        // Wire base tables (lagrange.hip): a device-resident variable map and index vectors, a whole key with its
        // Lagrange-basis table, commitments of evaluations not switched off.  Their digest goes out ahead of the round.
        for (bool& r : S.wire_route) r = false;
        bool wire_tables = from_vars && in.wires_on_device && !c->sharded() && !c->lagrange_off && !S.wire_dense_only &&
                           lagrange_ready(c, S.log_n) && in.n_rows > 0;
        if (wire_tables) {
            // Over the circuit's free variables (lagrange.hip) in the large-key regime, where an MSM's time is its additions
            // (DESIGN.md 3.1); below it a proof is a chain of latencies and a shorter MSM buys nothing.
            const bool eliminate = S.wire_elim_force >= 0 ? S.wire_elim_force != 0
                                                          : c->wire_elim_mode == 2 || (c->wire_elim_mode == 1 && S.log_n >= WIRE_ELIM_MIN_LOG_N);
            WireElimKeys ek{};
            for (int k = 0; k < 5; ++k) ek.pk[k] = S.pk[PK_QM + k];
            ek.pi_pos = in.pi_pos;
            ek.n_pi = in.pi_pos ? in.n_pi : 0;
            if ((rc = wire_bases_prepare(c, S.log_n, d_idx, in.n_rows, in.n_vars, eliminate ? &ek : nullptr))) return rc;
            wire_tables = wire_bases_use(c, 0) || wire_bases_use(c, 1) || wire_bases_use(c, 2);
            if (wire_tables && (rc = wire_bases_digest(c, d_idx, in.n_rows))) return rc;
        }
        if (host_wires) {
            // cold path: the three wire vectors cross PCIe inside the call.  They travel on the copy stream while the main
            // stream already transforms and commits the wire before, so only the first upload is exposed.
            if (!copy_fenced) {
                ZKT_HIP(c, hipEventRecord(S.ev_copy[3], c->stream));   // the targets are free once earlier work has drained
                ZKT_HIP(c, hipStreamWaitEvent(S.copy_stream, S.ev_copy[3], 0));
            }
            copy_fenced = false;
            for (int k = 0; k < 3; ++k) {
                if (in.n_rows < n)
                    ZKT_HIP(c, hipMemsetAsync((char*)S.ev[k] + in.n_rows * 32, 0, (n - in.n_rows) * 32, S.copy_stream));
                if (in.n_rows)
                    ZKT_HIP(c, hipMemcpyAsync(S.ev[k], wires[k], in.n_rows * 32, hipMemcpyHostToDevice, S.copy_stream));
                ZKT_HIP(c, hipEventRecord(S.ev_copy[k], S.copy_stream));
                ZKT_HIP(c, hipStreamWaitEvent(c->stream, S.ev_copy[k], 0));
                if ((rc = evals_to_blinded_poly(S.ev[k], S.poly[k], 2 * k, 2, k))) return rc;
                if ((rc = commit_begin(S.poly[k], n + 2, k))) return rc;
            }
        } else {
            for (int k = 0; k < 3; ++k) {
                if (from_vars) {
                    if ((rc = poly_gather_pad(c, d_vars, in.n_vars, d_idx[k], in.n_rows, S.ev[k], n, S.status))) return rc;
                } else {
                    if ((rc = poly_copy_pad(c, wires[k], in.n_rows, S.ev[k], n))) return rc;   // prove.rs:39-55 pad_to
                }
            }
            const PolyJob jobs[3] = {{S.ev[0], S.poly[0], 0, 2, 0}, {S.ev[1], S.poly[1], 2, 2, 1}, {S.ev[2], S.poly[2], 4, 2, 2}};
            if ((rc = evals_to_blinded_polys(jobs, 3))) return rc;
            if (wire_tables && (rc = wire_bases_lens(c, S.status + 8))) return rc;
            for (int k = 0; k < 3; ++k) {
                // a wire with a base table: one scalar per distinct variable (and the two blinders) instead of n + 2
                // coefficients; the evaluation vector above is still needed by the transforms, z1 and the index check
                const void* sc = S.poly[k];
                size_t len = n + 2;
                int tbl = 0;
                if (wire_tables && wire_bases_use(c, k)) {
                    if ((rc = wire_bases_scalars(c, k, d_vars, (const char*)S.small + (size_t)(2 * k) * 32, n, &sc, &len))) return rc;
                    tbl = MSM_TBL_WIRE + k;
                    S.wire_route[k] = true;
                }
                rc = queueing() ? commit_push(sc, len, k, tbl) : tbl ? msm_begin(c, sc, len, 0, 1, k, tbl) : commit_begin(sc, len, k);
                if (rc) return rc;
            }
        }
        if ((rc = commit_flush())) return rc;
        return to_coset_many({W_A, W_B, W_C});
    }

    // ---- round 2 (prove.rs:145-185): its three commitments join the batch of round 1
    // The table polynomial's part of round 2 (prove.rs:145-156,178-180): evaluations, coefficients, commitment, coset.
    // It depends on nothing but the lookup table, so a direct (unannounced) proof issues it FIRST: it then covers the
    // upload of the first wire vector of a cold proof.  Returns whether the resident table polynomial is reused.
    bool table_is_cached(const zkt_prove_inputs& in) const {
        // the cached commitment belongs to the SRS it was made under: a reloaded key invalidates it (the polynomial and
        // its coset would survive, but one flag keeps the three together)
        return S.t_cached && S.t_srs_generation == c->srs_generation && S.cached_table.size() == 4 * in.table_len &&
               (in.table_len == 0 || memcmp(S.cached_table.data(), in.table, in.table_len * 32) == 0);
    }
    int enqueue_table(const zkt_prove_inputs& in, bool with_coset) {
        const size_t n = S.n;
        int rc;
        if (in.table_len >= n) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "max table size is equal or larger than n");
        S.t_cached = false;
        S.t_coset_valid = false;
        ZKT_HIP(c, hipMemsetAsync(S.ev[3], 0, n * 32, c->stream));
        if (in.table_len) ZKT_HIP(c, hipMemcpyAsync(S.ev[3], in.table, in.table_len * 32, hipMemcpyHostToDevice, c->stream));
        if ((rc = evals_to_blinded_poly(S.ev[3], S.poly[3], 0, 0, 3))) return rc;      // t: no blinders
        if ((rc = commit_evals_begin(S.ev[3], S.poly[3], 0, 0, 3, 3))) return rc;
        if (with_coset && (rc = to_coset(W_T))) return rc;
        return ZKT_OK;
    }

    // table_done: enqueue_table has already run for this proof (direct path)
    int enqueue_round_2(const zkt_prove_inputs& in, bool* same_table_out, bool table_done = false) {
        const size_t n = S.n;
        int rc;
        ProfScope prof_round(c, "round2");
        const bool same_table = !table_done && table_is_cached(in);
        *same_table_out = same_table;
        if (!same_table && !table_done && (rc = enqueue_table(in, false))) return rc;
        if ((rc = poly_mul_vec(c, S.q_lookup_ev, S.ev[2], S.ev[4], n))) return rc;         // f = q_lookup . c
        if ((rc = combine_split(in.table, in.table_len, !same_table))) return rc;
        {
            const PolyJob jobs[2] = {{S.ev[5], S.poly[4], 6, 3, 4}, {S.ev[6], S.poly[5], 9, 2, 5}};   // h1: 3 blinders, h2: 2
            if ((rc = evals_to_blinded_polys(jobs, 2))) return rc;
        }
        if ((rc = commit_evals_begin(S.ev[5], S.poly[4], 6, 3, 4, 4))) return rc;
        if ((rc = commit_evals_begin(S.ev[6], S.poly[5], 9, 2, 5, 5))) return rc;
        if ((rc = commit_flush())) return rc;
        if (!S.t_coset_valid && !table_done) return to_coset_many({W_T, W_H1, W_H2});
        return to_coset_many({W_H1, W_H2});   // unchanged table: its coset is still resident
    }

    // ---- the proof in flight: what run()'s steps hand to each other ----
    Challenges<R> ch;
    XiPoint<R> at;              // zh(xi), L_1(xi), the powers of alpha, epsilon (1 + delta)
    F ev[EV_COUNT];             // the twelve evaluations
    Affine<Q> cm[11], wit[2];   // the eleven commitments, the witnesses aw and saw of the openings
    F w, shifted;               // the domain's generator, xi w
    bool same_table = false, classes = false, pi_direct = false, fused3 = false, fused5 = false;

    // Rounds 1 and 2: in flight already when the proof was announced (zkt_prove_set_next), issued here otherwise
    int rounds_1_2(const zkt_prove_inputs& in) {
        int rc;
        if (S.prefetch_stage == 2 && S.prefetch_epoch == c->msm_epoch && same_inputs(S.prefetch_in, in)) {
            same_table = S.prefetch_same_table;   // in the alternate work set
            swap_work_sets();
            S.prefetch_stage = 0;
            return ZKT_OK;
        }
        S.prefetch_stage = 0;
        // nobody announced this proof: a fresh lookup table's polynomial goes first (it waits for nothing, and its
        // commitment covers the first wire upload of a cold proof)
        const bool table_first = !table_is_cached(in);
        if (table_first && in.a_evals && !in.wires_on_device) {
            // host wire vectors: the copy stream is fenced HERE, so that the uploads run beside the table's work
            ZKT_HIP(c, hipEventRecord(S.ev_copy[3], c->stream));
            ZKT_HIP(c, hipStreamWaitEvent(S.copy_stream, S.ev_copy[3], 0));
            copy_fenced = true;
        }
        if (table_first && (rc = enqueue_table(in, true))) return rc;
        if ((rc = enqueue_round_1(in))) return rc;
        return enqueue_round_2(in, &same_table, table_first);
    }

    // The six commitments of rounds 1 and 2; the table's is kept for the proofs that pass the same table
    int collect_rounds_1_2(const zkt_prove_inputs& in) {
        static const int slots[6] = {0, 1, 2, 3, 4, 5};
        const bool skip[6] = {false, false, false, same_table, false, false};
        int rc;
        if ((rc = commit_collect(slots, skip, 6, cm))) return rc;
        if ((rc = collect_wires(cm))) return rc;
        mark("wait commits of rounds 1+2");
        if (!same_table) {
            memcpy(S.t_commit_xy, cm[3].x.v, Q::N * 4);
            memcpy(S.t_commit_xy + Q::N / 2, cm[3].y.v, Q::N * 4);
            S.cached_table.assign(in.table, in.table + 4 * in.table_len);
            S.t_cached = true;
            S.t_srs_generation = c->srs_generation;
        } else {
            memcpy(cm[3].x.v, S.t_commit_xy, Q::N * 4);
            memcpy(cm[3].y.v, S.t_commit_xy + Q::N / 2, Q::N * 4);
        }
        return ZKT_OK;
    }

    // ---- round 3 (prove.rs:190-255) ----
    // Both grand products are prefix products of num/den ratios; the division is one inversion of the total
    // denominator on the host.  The two products are independent, so both pairs of scans run before the single
    // host round trip (the second pair borrows the still unused z1 coset buffer).
    // _begin: the scans and the copies of the two totals; the caller synchronises; _finish: the inversion and the
    // combines, z1 into ev[7] and z2 into sc[0].  zkt_debug_grand_products runs the same two.
    void* pn2() const { return S.wcos[W_Z1]; }
    void* sd2() const { return (char*)S.wcos[W_Z1] + S.n * 32; }
    int grand_products_begin() {
        const size_t n = S.n;
        int rc;
        ZTermsArgs za{};
        za.a = S.ev[0]; za.b = S.ev[1]; za.c = S.ev[2];
        za.s1 = S.sigma_ev[0]; za.s2 = S.sigma_ev[1]; za.s3 = S.sigma_ev[2]; za.roots = S.roots;
        za.f = S.ev[4]; za.t = S.ev[3]; za.h1 = S.ev[5]; za.h2 = S.ev[6];
        za.num = S.sc[0]; za.den = S.sc[1]; za.n = n;
        put(za.beta, ch.beta); put(za.gamma, ch.gamma); put(za.delta, ch.delta); put(za.epsilon, ch.epsilon);
        F* pin = (F*)S.pinned;
        // Fused (zkt_ctx_set_fused_passes): the terms are never stored, so num / den hold the scans' block totals and prefixes
        fused3 = c->fused(2) && grand_product_tmp_elems(n) <= n + 8;
        const void *tot1 = S.sc[3], *tot2 = sd2();
        if (fused3) {
            const bool later = c->fused(32) && grand_product_totals_fit(n);   // the four scans of the totals as one launch
            if ((rc = grand_product_scan(c, za, 1, S.sc[2], S.sc[3], S.sc[0], &tot1, later))) return rc;
            if ((rc = grand_product_scan(c, za, 2, pn2(), sd2(), S.sc[1], &tot2, later))) return rc;
            if (later && (rc = grand_product_totals2(c, n, S.sc[0], S.sc[1]))) return rc;
        } else {
            if ((rc = z1_terms(c, za))) return rc;
            if ((rc = scan_mul(c, S.sc[0], S.sc[2], n, false, S.scan_tmp))) return rc;   // PN
            if ((rc = scan_mul(c, S.sc[1], S.sc[3], n, true, S.scan_tmp))) return rc;    // SD
            if ((rc = z2_terms(c, za))) return rc;
            if ((rc = scan_mul(c, S.sc[0], pn2(), n, false, S.scan_tmp))) return rc;
            if ((rc = scan_mul(c, S.sc[1], sd2(), n, true, S.scan_tmp))) return rc;
        }
        ZKT_HIP(c, hipMemcpyAsync(pin, tot1, 32, hipMemcpyDeviceToHost, c->stream));
        ZKT_HIP(c, hipMemcpyAsync(pin + 1, tot2, 32, hipMemcpyDeviceToHost, c->stream));
        return ZKT_OK;
    }
    int grand_products_finish() {
        const size_t n = S.n;
        const F* pin = (const F*)S.pinned;
        int rc;
        if (fe_is_zero<R>(pin[0])) return set_err(c, ZKT_ERR_ZERO_DENOMINATOR, "zero denominator in the permutation grand product");
        if (fe_is_zero<R>(pin[1])) return set_err(c, ZKT_ERR_ZERO_DENOMINATOR, "zero denominator in the lookup grand product");
        const F inv12 = fe_inv_host<R>(fe_mul<R>(pin[0], pin[1]));
        const F inv1 = fe_mul<R>(inv12, pin[1]), inv2 = fe_mul<R>(inv12, pin[0]);
        wait_end();
        if (fused3) {
            if ((rc = grand_product_combine(c, S.sc[2], S.sc[3], S.sc[0], inv1.v, S.ev[7], n))) return rc;
            return grand_product_combine(c, pn2(), sd2(), S.sc[1], inv2.v, S.sc[0], n);
        }
        if ((rc = z_combine(c, S.sc[2], S.sc[3], inv1.v, S.ev[7], n))) return rc;
        return z_combine(c, pn2(), sd2(), inv2.v, S.sc[0], n);              // num / den are free again
    }

    // Classes route: the coefficients n - 6 .. n + 7 of a b c z1 z2 t (the six top coefficients of the quotient come from
    // them): one small launch and one copy, on the host well before this round's commitments are
    int gather_windows() {
        const void* const wp[QC_WIN_POLYS] = {S.poly[0], S.poly[1], S.poly[2], S.poly[6], S.poly[7], S.poly[3]};
        if (int rc = quotient_gather_windows(c, wp, S.n - 6, S.d_win)) return rc;
        ZKT_HIP(c, hipMemcpyAsync(S.pinned_win, S.d_win, QC_WIN_POLYS * QC_WIN * 32, hipMemcpyDeviceToHost, c->stream));
        ZKT_HIP(c, hipEventRecord(S.ev_win, c->stream));
        return ZKT_OK;
    }

    // The public-input polynomial of round 4 (prove.rs:258-262) is challenge-free as well.  With a handful of
    // public inputs it is never built: the quotient kernel evaluates it from rotations of l1 (poly.hpp).
    int public_inputs(const zkt_prove_inputs& in) {
        const size_t n = S.n;
        int rc;
        for (size_t i = 0; i < in.n_pi; ++i)
            if (in.pi_pos[i] >= n) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "public input position out of range");
        // (with 8 GPUs a rotation by 4 pos leaves the class for odd pos: the polynomial is transformed instead)
        pi_direct = in.n_pi <= (size_t)QUOTIENT_PI_DIRECT_MAX && S.G <= 4;
        if (pi_direct) {
            uint32_t* tab = (uint32_t*)S.pinned_pi;
            pi_rows<R>(in.pi_pos, in.pi_vals, in.n_pi, classes ? 4 : (size_t)S.G, tab);   // rotations in entries of the class
            if (in.n_pi)
                ZKT_HIP(c, hipMemcpyAsync(S.pi_tab, tab, in.n_pi * 40, hipMemcpyHostToDevice, c->stream));
            return ZKT_OK;
        }
        ZKT_HIP(c, hipMemsetAsync(S.ev[7], 0, n * 32, c->stream));
        for (size_t i = 0; i < in.n_pi; ++i)
            ZKT_HIP(c, hipMemcpyAsync((char*)S.ev[7] + in.pi_pos[i] * 32, in.pi_vals + 4 * i, 32, hipMemcpyHostToDevice, c->stream));
        if ((rc = evals_to_blinded_poly(S.ev[7], S.poly[8], 0, 0, 8))) return rc;      // pi
        return to_coset(W_PI);
    }

    int round_3(const zkt_prove_inputs& in) {
        const size_t n = S.n;
        int rc;
        if ((rc = grand_products_begin())) return rc;
        mark("enqueue grand products");
        if ((rc = check_status())) return rc;   // synchronises; reports a lookup outside the table (round 2)
        mark("wait grand products");
        if ((rc = grand_products_finish())) return rc;
        const PolyJob jobs[2] = {{S.ev[7], S.poly[6], 11, 3, 6}, {S.sc[0], S.poly[7], 14, 3, 7}};   // z1, z2: 3 blinders each
        if ((rc = evals_to_blinded_polys(jobs, 2))) return rc;
        if (classes && (rc = gather_windows())) return rc;
        void* const z1p[1] = {S.poly[6]};
        const size_t z1l[1] = {n + 3};
        static const int slots[2] = {0, 1};
        if ((rc = commit_begin_many(z1p, z1l, slots, 1))) return rc;
        if ((rc = commit_evals_begin(S.sc[0], S.poly[7], 14, 3, 7, 1))) return rc;
        if ((rc = commit_flush())) return rc;
        if ((rc = to_coset_many({W_Z1, W_Z2}))) return rc;
        if ((rc = public_inputs(in))) return rc;
        return commit_collect(slots, nullptr, 2, cm + 6);
    }

    // ---- round 4 (prove.rs:258-313): the quotient's 4n coefficients into qev, by one of three routes ----

    // Classes 0, 1, 2 of the coset, each as a sharded proof over four GPUs computes its own (the class mode of
    // the kernel), then back class by class: E_j = t mod (X^n - gamma_j); the top coefficients and the combine give t
    // closed (out): the closing pass has split the quotient into its three chunks as well (quotient_split_blind skips that)
    int quotient_on_classes(QuotientArgs q, bool* closed) {
        const size_t n = S.n;
        const int log_n = S.log_n;
        int rc;
        q.G = 4;
        q.next_off = 1;
        q.n4 = n;
        const bool grid = c->fused(8);   // the class in the grid: one launch per stage for the three classes
        for (int j = 0; j < (grid ? 1 : 3); ++j) {
            const size_t off = (size_t)j * n * 32;
            quotient_vectors(q, S.ccoset, S.wcos, off);
            q.cls = (uint32_t)j;
            q.ncls = grid ? 3 : 0;
            q.cls_stride = n;
            q.z1_next = q.z1; q.z2_next = q.z2; q.t_next = q.t; q.h1_next = q.h1;
            q.out = (char*)S.qev + off;
            if ((rc = quotient_pointwise(c, q))) return rc;
        }
        if (grid) {
            const int codes[3] = {ntt_class_code(log_n + 2, 0), ntt_class_code(log_n + 2, 1), ntt_class_code(log_n + 2, 2)};
            const void* in = S.qev;
            void* out = S.qev;
            if ((rc = ntt_run_classes(c, log_n, 1, codes, 1, &in, &n, &out, n, n))) return rc;
        } else {
            for (int j = 0; j < 3; ++j) {
                void* e = (char*)S.qev + (size_t)j * n * 32;
                if ((rc = ntt_run(c, log_n, 1, ntt_class_code(log_n + 2, j), e, n, e))) return rc;
            }
        }
        // the six top coefficients, from the windows that came with round 3 (the launches above are under way)
        ZKT_HIP(c, hipEventSynchronize(S.ev_win));
        const uint32_t* pw = (const uint32_t*)S.pinned_win;
        QuotientWindows W{};
        W.a = pw; W.b = pw + QCW * 8; W.c = pw + 2 * QCW * 8; W.z1 = pw + 3 * QCW * 8; W.z2 = pw + 4 * QCW * 8;
        W.t = pw + 5 * QCW * 8;
        W.sigma1 = &S.key_win[0][0][0]; W.sigma2 = &S.key_win[1][0][0]; W.sigma3 = &S.key_win[2][0][0];
        W.q_lookup = &S.key_win[3][0][0];
        F u[6];
        quotient_top_coefficients<R>(log_n, W, ch.alpha, ch.beta, ch.delta, u);
        for (int e = 0; e < 6; ++e) put(S.last_u[e], u[e]);
        S.last_u_valid = true;
        *closed = c->fused(16);
        if (*closed)
            return quotient_classes_close(c, S.qev, n, &S.qc_vinv[0][0], &S.last_u[0][0], &S.qc_g3[0][0], S.poly[9], S.poly[10], S.poly[11]);
        return quotient_classes_combine(c, S.qev, n, &S.qc_vinv[0][0], &S.last_u[0][0], &S.qc_g3[0][0]);
    }

    // This GPU's class of the coset, written where the all-gather wants it; then the one real exchange of a
    // sharded proof: 4n x 32 B in total, and the classes go back to natural order for the inverse transform
    int quotient_sharded(QuotientArgs q) {
        const size_t n = S.n;
        int rc;
        q.G = (uint32_t)S.G;
        q.cls = (uint32_t)S.cls;
        q.next_off = S.G <= 4 ? 4u / (uint32_t)S.G : (uint32_t)((S.cls + 4) >> 3);
        q.z1_next = S.G == 8 ? S.wnext[0] : q.z1;
        q.z2_next = S.G == 8 ? S.wnext[1] : q.z2;
        q.t_next = S.G == 8 ? S.wnext[2] : q.t;
        q.h1_next = S.G == 8 ? S.wnext[3] : q.h1;
        const size_t pieces = ZKT_QUOTIENT_CHUNKS;
        if (!(comm_async_available(c) && S.comm_stream && S.m % pieces == 0 && S.m / pieces >= 1024)) {
            q.out = (char*)S.qgather + (size_t)S.cls * S.m * 32;
            if ((rc = quotient_pointwise(c, q))) return rc;
            if ((rc = comm_all_gather_dev(c, q.out, S.qgather, S.m * 32))) return rc;
            return quotient_interleave(c, S.qgather, S.qev, 4 * n, (uint32_t)S.G);
        }
        // the exchange in pieces, stream-ordered, on a stream of its own: piece j's collective travels while
        // piece j + 1 is computed, and the host never waits (zkt_comm_vtable::all_gather_async).  The gathered
        // layout is [piece][class][m / pieces]; this rank's share of a piece is written where RCCL's in-place
        // form wants it (recv + rank * bytes).
        const size_t mp = S.m / pieces;
        for (size_t j = 0; j < pieces; ++j) {
            char* recv = (char*)S.qgather + j * (size_t)S.G * mp * 32;
            char* mine = recv + (size_t)S.cls * mp * 32;
            q.first = j * mp;
            q.count = mp;
            q.out = mine - q.first * 32;     // out[i] for i in the piece lands in `mine`
            if ((rc = quotient_pointwise(c, q))) return rc;
            ZKT_HIP(c, hipEventRecord(S.ev_piece[j], c->stream));
            ZKT_HIP(c, hipStreamWaitEvent(S.comm_stream, S.ev_piece[j], 0));
            if ((rc = comm_all_gather_async(c, mine, recv, mp * 32, S.comm_stream))) return rc;
        }
        ZKT_HIP(c, hipEventRecord(S.ev_gathered, S.comm_stream));
        ZKT_HIP(c, hipStreamWaitEvent(c->stream, S.ev_gathered, 0));
        return quotient_interleave(c, S.qgather, S.qev, 4 * n, (uint32_t)S.G, (uint32_t)pieces);
    }

    void issue_next_round_1() {   // zkt_prove_set_next: round 1 of the next proof hides the tail of the quotient commitments
        if (!S.has_next) return;
        S.has_next = false;
        swap_work_sets();
        const int r1 = enqueue_round_1(S.next_in);
        swap_work_sets();
        S.prefetch_stage = (r1 == ZKT_OK) ? 1 : 0;   // on failure the next zkt_prove redoes the work and reports
    }
    void issue_next_round_2() {   // ... and its round 2 keeps the GPU fed across the proof boundary
        if (S.prefetch_stage != 1) return;
        bool st = false;
        swap_work_sets();
        const int r2 = enqueue_round_2(S.next_in, &st);
        swap_work_sets();
        S.prefetch_stage = 0;
        if (r2 != ZKT_OK) return;
        S.prefetch_stage = 2;
        S.prefetch_in = S.next_in;
        S.prefetch_same_table = st;
        S.prefetch_epoch = c->msm_epoch;   // any other MSM before the next proof invalidates it
    }

    int round_4(const zkt_prove_inputs& in) {
        const size_t n = S.n;
        int rc;
        S.t_coset_valid = S.t_cached;
        QuotientArgs q = quotient_args(S, S.wcos, ch.alpha.v, ch.beta.v, ch.gamma.v, ch.delta.v, ch.epsilon.v);
        q.out = S.qev;
        q.n4 = S.m;
        q.pi_tab = pi_direct ? S.pi_tab : nullptr;
        q.n_pi_direct = pi_direct ? (uint32_t)in.n_pi : 0;
        bool closed = false;
        if ((rc = classes ? quotient_on_classes(q, &closed) : S.G > 1 ? quotient_sharded(q) : quotient_pointwise(c, q))) return rc;
        if (!classes && (rc = ntt_run(c, S.log_n + 2, 1, 1, S.qev, 4 * n, S.qev))) return rc;         // quotient_poly.rs:226
        // an unsatisfied circuit shows up as status bits here; they are read with the evaluations of round 5
        if ((rc = quotient_split_blind(c, S.qev, n, (const char*)S.small + 17 * 32, S.poly[9], S.poly[10], S.poly[11], S.status,
                                       c->fused(4), closed)))
            return rc;
        void* const polys[3] = {S.poly[9], S.poly[10], S.poly[11]};
        const size_t lens[3] = {n + 3, n + 3, n + 3};
        static const int slots[3] = {8, 9, 10};
        if ((rc = commit_begin_many(polys, lens, slots, 3))) return rc;
        if ((rc = commit_flush())) return rc;
        issue_next_round_1();
        return commit_collect(slots, nullptr, 3, cm + 8);
    }

    // ---- round 5 (prove.rs:318-451, linearization_poly.rs:19-121) ----
    // The twelve evaluations at xi and xi w, on the host when this returns
    int evaluations() {
        int rc;
        w = root_of_unity<R>(S.log_n);
        shifted = fe_mul<R>(ch.xi, w);
        EvalArgs ea{};
        // order of ProofEvaluations: a b c | sigma1 sigma2 z1_next | q_lookup t t_next z2_next h1_next h2
        const void* ep[12] = {S.poly[0], S.poly[1], S.poly[2], S.pk[PK_S1], S.pk[PK_S2], S.poly[6],
                              S.pk[PK_QLOOKUP], S.poly[3], S.poly[3], S.poly[7], S.poly[4], S.poly[5]};
        const size_t el[12] = {cap, cap, cap, S.pk_len[PK_S1], S.pk_len[PK_S2], cap, S.pk_len[PK_QLOOKUP], cap, cap, cap, cap, cap};
        const bool sh[12] = {false, false, false, false, false, true, false, false, true, true, true, false};
        ea.count = 12;
        for (int k = 0; k < 12; ++k) {
            ea.poly[k] = ep[k];
            ea.len[k] = el[k];
            put(ea.point[k], sh[k] ? shifted : ch.xi);
        }
        // Fused (zkt_ctx_set_fused_passes): the powers of xi and xi w the evaluations need are those of the openings' tables,
        // so both tables (and those of the inverses) are built here in one launch and stay in eval_pw for the openings
        fused5 = c->fused(1);
        if (fused5) {
            const F xi_inv = fe_is_zero<R>(ch.xi) ? ch.xi : fe_inv_host<R>(ch.xi);
            const F shifted_inv = fe_mul<R>(xi_inv, fe_inv_host<R>(w));
            for (int k = 0; k < 12; ++k) ea.table[k] = sh[k] ? 1 : 0;
            if ((rc = poly_eval_open_tables(c, ea, ch.xi.v, xi_inv.v, shifted.v, shifted_inv.v, cap, d_partials, d_results, S.eval_pw)))
                return rc;
        } else if ((rc = poly_eval_many(c, ea, d_partials, d_results, S.eval_pw))) {
            return rc;
        }
        const F* pin = (const F*)S.pinned;
        ZKT_HIP(c, hipMemcpyAsync(S.pinned, d_results, 12 * 32, hipMemcpyDeviceToHost, c->stream));
        mark("enqueue evaluations");
        if ((rc = check_status())) return rc;   // synchronises the stream
        mark("wait evaluations");
        for (int k = 0; k < 12; ++k) ev[k] = pin[k];
        return ZKT_OK;
    }

    static void term(LinCombArgs& L, const void* p, size_t len, const F& s) {
        L.poly[L.nterms] = p; L.len[L.nterms] = len;
        put(L.scalar[L.nterms], s);
        ++L.nterms;
    }
    // r(X): the thirteen scalars of linearisation.hpp against the prover's polynomials
    LinCombArgs linearisation() {
        F sc[LIN_COUNT];
        linearisation_scalars<R>(ch, at, ev, sc);
        const void* const p[LIN_COUNT] = {S.pk[PK_QM], S.pk[PK_QL], S.pk[PK_QR], S.pk[PK_QO], S.pk[PK_QC], S.poly[6], S.pk[PK_S3],
                                          S.poly[7], S.poly[4], S.pk[PK_QTABLE], S.poly[9], S.poly[10], S.poly[11]};
        const size_t l[LIN_COUNT] = {S.pk_len[PK_QM], S.pk_len[PK_QL], S.pk_len[PK_QR], S.pk_len[PK_QO], S.pk_len[PK_QC], cap,
                                     S.pk_len[PK_S3], cap, cap, S.pk_len[PK_QTABLE], cap, cap, cap};
        LinCombArgs lr{};
        for (int k = 0; k < LIN_COUNT; ++k) term(lr, p[k], l[k], sc[k]);
        return lr;
    }

    // The witness of an opening at z is (p(X) - p(z)) / (X - z).  At z = 0 (xi = 0 makes both points zero; the reference
    // proves there) that is p shifted down by one coefficient, and no power of 1/z is needed: one copy on the stream
    // the opening uses.
    int witness(const void* comb, const F& z, void* ta, void* tb, void* scan, void* out, void* pw) {
        if (fe_is_zero<R>(z)) {
            ZKT_HIP(c, hipMemcpyAsync(out, (const char*)comb + 32, (cap - 1) * 32, hipMemcpyDeviceToDevice, c->stream));
            return ZKT_OK;
        }
        const F zi = fe_inv_host<R>(z);
        return open_witness(c, comb, cap, z.v, zi.v, ta, tb, scan, out, pw);
    }
    // Fused (zkt_ctx_set_fused_passes): an opening is one pass over its polynomials (for the first, r's 13 and the 8
    // others; r is never formed) that also scales by z^i (`pw`: the point's tables, made with the evaluations), then the
    // suffix scan, whose block prefixes the last scaling adds itself; the scan's total is the combination's value at z.
    int opening(const LinCombArgs& L, const F& z, void* comb, void* ta, void* tb, void* scan, void* out, void* pw, void* d_total) {
        int rc;
        if (fe_is_zero<R>(z)) {   // the raw combination: its witness as above, its value the constant coefficient
            if ((rc = poly_lincomb(c, L, comb, cap))) return rc;
            if ((rc = witness(comb, z, ta, tb, scan, out, pw))) return rc;
            ZKT_HIP(c, hipMemcpyAsync(d_total, comb, 32, hipMemcpyDeviceToDevice, c->stream));
            return ZKT_OK;
        }
        if ((rc = open_combine(c, L, ta, cap, pw))) return rc;
        return open_divide(c, ta, cap, tb, scan, out, pw, d_total);
    }

    // Classes route, issue side of check_identity.  An unsatisfied circuit leaves no trace in the quotient's coefficients
    // on this route (there are no evaluations on a fourth class for it to spill into).  The verifier's identity at xi
    // takes over: one more value, r(xi) or (fused) (r + sum_k eta^k p_k)(xi), comes back with the round's last collect.
    int identity_value(const void* d_value) {
        ZKT_HIP(c, hipMemcpyAsync((F*)S.pinned + 16, d_value, 32, hipMemcpyDeviceToHost, c->stream));
        ZKT_HIP(c, hipEventRecord(S.ev_win, c->stream));
        return ZKT_OK;
    }

    // aw opening (prove.rs:381-420): sum_k eta^k p_k over (r, a, b, c, sigma1, sigma2, q_lookup, t, h2), witness into sc[3].
    // r(X) lives in the work buffer; its own commitment (prove.rs:372-375) is never part of the proof or the transcript.
    int first_opening() {
        int rc;
        const LinCombArgs lr = linearisation();
        void *work = S.poly[12], *d_f1 = (char*)d_results + 15 * 32;
        LinCombArgs lo{};
        F pw = fe_one<R>();
        wait_end();
        if (fused5) {
            lo = lr;
        } else {
            if ((rc = poly_lincomb(c, lr, work, cap))) return rc;
            if (classes) {
                EvalArgs er{};
                er.count = 1;
                er.poly[0] = work;
                er.len[0] = cap;
                put(er.point[0], ch.xi);
                if ((rc = poly_eval_many(c, er, d_partials, d_results, S.eval_pw))) return rc;
                if ((rc = identity_value(d_results))) return rc;
            }
            term(lo, work, cap, pw);
        }
        const void* ps[8] = {S.poly[0], S.poly[1], S.poly[2], S.pk[PK_S1], S.pk[PK_S2], S.pk[PK_QLOOKUP], S.poly[3], S.poly[5]};
        const size_t pl[8] = {cap, cap, cap, S.pk_len[PK_S1], S.pk_len[PK_S2], S.pk_len[PK_QLOOKUP], cap, cap};
        for (int k = 0; k < 8; ++k) {
            pw = fe_mul<R>(pw, ch.eta);
            term(lo, ps[k], pl[k], pw);
        }
        void* comb = S.sc[0];  // n + 8 fits: sc buffers hold n + 8 elements
        if (fused5) {
            if ((rc = opening(lo, ch.xi, comb, S.sc[1], S.sc[2], S.scan_tmp, S.sc[3], S.eval_pw, d_f1))) return rc;
            return classes ? identity_value(d_f1) : ZKT_OK;
        }
        if ((rc = poly_lincomb(c, lo, comb, cap))) return rc;
        return witness(comb, ch.xi, S.sc[1], S.sc[2], S.scan_tmp, S.sc[3], S.eval_pw);
    }

    // saw opening (prove.rs:427-451): (z1, z2, t, h1) at xi * omega.  Its linear combination and division depend on
    // nothing the first opening computes: on a single GPU they run on a second stream beside the first opening's
    // commitment (memory-bound work beside an integer-ALU-bound kernel), in the z cosets' buffers, which are dead since
    // the quotient pass.
    void* second_witness(bool aux) const { return aux ? S.wcos[W_Z2] : S.sc[3]; }
    int second_opening(bool aux) {
        void* comb2 = aux ? S.wcos[W_Z1] : S.sc[0];
        void* ta2 = aux ? (void*)((char*)S.wcos[W_Z1] + cap * 32) : S.sc[1];
        void* tb2 = aux ? (void*)((char*)S.wcos[W_Z1] + 2 * cap * 32) : S.sc[2];
        void* scan = aux ? S.aux_scan_tmp : S.scan_tmp;
        LinCombArgs lo{};
        F pw = fe_one<R>();
        const void* ps[4] = {S.poly[6], S.poly[7], S.poly[3], S.poly[4]};
        for (int k = 0; k < 4; ++k) {
            term(lo, ps[k], cap, pw);
            pw = fe_mul<R>(pw, ch.eta);
        }
        if (fused5) return opening(lo, shifted, comb2, ta2, tb2, scan, second_witness(aux), (char*)S.eval_pw + open_witness_powers(cap) * 32,
                                   (char*)d_results + 14 * 32);   // xi w's tables lie behind xi's
        if (int rc = poly_lincomb(c, lo, comb2, cap)) return rc;
        return witness(comb2, shifted, ta2, tb2, scan, second_witness(aux), aux ? S.aux_pw : S.eval_pw);
    }
    int second_opening_on_aux_stream() {
        ZKT_HIP(c, hipEventRecord(S.ev_aux_go, c->stream));
        ZKT_HIP(c, hipStreamWaitEvent(S.aux_stream, S.ev_aux_go, 0));
        hipStream_t main_stream = c->stream;
        c->stream = S.aux_stream;           // the polynomial kernels launch on the context's stream
        const int rc = second_opening(true);
        c->stream = main_stream;
        if (rc) return rc;
        ZKT_HIP(c, hipEventRecord(S.ev_aux_done, S.aux_stream));
        return ZKT_OK;
    }

    // Both openings and their commitments aw, saw; the next proof's round 2 goes behind them
    int openings() {
        int rc;
        if ((rc = first_opening())) return rc;
        const bool aux = S.aux_stream != nullptr && !c->aux_off;
        if (aux && (rc = second_opening_on_aux_stream())) return rc;
        // (small and mid-size keys: both commitments as one batch, which the second witness' own buffers allow)
        const bool both = aux && queueing();
        if (!both && (rc = commit_begin(S.sc[3], cap - 1, 6))) return rc;  // the scalars are consumed by the first kernels
        if (aux) ZKT_HIP(c, hipStreamWaitEvent(c->stream, S.ev_aux_done, 0));
        else if ((rc = second_opening(false))) return rc;
        static const int slots[2] = {6, 7};
        if (both) {
            void* const wp[2] = {S.sc[3], second_witness(aux)};
            const size_t wl[2] = {cap - 1, cap - 1};
            if ((rc = commit_begin_many(wp, wl, slots, 2))) return rc;
        } else if ((rc = commit_begin(second_witness(aux), cap - 1, 7))) {
            return rc;
        }
        if ((rc = commit_flush())) return rc;
        issue_next_round_2();
        return commit_collect(slots, nullptr, 2, wit);
    }

    // Classes route, check side: r(xi) against compute_r0 (proof.rs:163-217) made from the prover's own values.  A public
    // input's root equal to xi has L_j = 1 there and the proof goes on.
    int check_identity(const zkt_prove_inputs& in) {
        std::vector<F> root(in.n_pi), vals(in.n_pi), before(in.n_pi);
        for (size_t i = 0; i < in.n_pi; ++i) root[i] = fe_pow_u64<R>(w, (uint64_t)in.pi_pos[i]);
        if (in.n_pi) memcpy((void*)vals.data(), in.pi_vals, in.n_pi * sizeof(F));
        F r0;
        (void)compute_r0<R, fe_inv_host<R>>(ch, at, ev, root.data(), vals.data(), in.n_pi, before.data(), &r0);
        ZKT_HIP(c, hipEventSynchronize(S.ev_win));
        F r_xi = ((const F*)S.pinned)[16];
        if (fused5) {   // the first opening's combination at xi, less eta^k times a b c sigma1 sigma2 q_lookup t h2 at xi
            static const int at_xi[8] = {EV_A, EV_B, EV_C, EV_S1, EV_S2, EV_QL, EV_T, EV_H2};
            F pw = fe_one<R>();
            for (int k = 0; k < 8; ++k) {
                pw = fe_mul<R>(pw, ch.eta);
                r_xi = fe_sub<R>(r_xi, fe_mul<R>(pw, ev[at_xi[k]]));
            }
        }
        if (!fe_eq<R>(r_xi, r0))
            return set_err(c, ZKT_ERR_QUOTIENT_TOO_SHORT, "the opening identity fails at xi: the circuit is not satisfied");
        return ZKT_OK;
    }

    // ---- Proof (proof.rs:106-155), CanonicalSerialize ----
    void serialize(std::vector<uint8_t>& proof) const {
        proof.clear();
        for (int k = 0; k < 11; ++k) serialize_point<Q>(cm[k], proof);
        serialize_point<Q>(wit[0], proof);
        proof.push_back(0);   // kzg10::Proof::random_v = None
        serialize_point<Q>(wit[1], proof);
        proof.push_back(0);
        for (int k = 0; k < EV_COUNT; ++k) {
            uint8_t b[32];
            H::to_le_bytes(ev[k], b);
            proof.insert(proof.end(), b, b + 32);
        }
    }

    // The five rounds, with the transcript's traffic between them.  prof_round: stream time of a round, first launch to
    // last (zkt_profile_get "round3" ...)
    int run(const zkt_prove_inputs& in, std::vector<uint8_t>& proof) {
        int rc;
        mark("start");
        if ((rc = choose_route())) return rc;
        classes = S.use_classes;
        if ((rc = rounds_1_2(in))) return rc;
        // prove.rs:110 -- public inputs (BTreeMap order = ascending position)
        {
            std::vector<uint8_t> b(in.n_pi * 32);
            for (size_t i = 0; i < in.n_pi; ++i) H::to_le_bytes(H::from_words(in.pi_vals + 4 * i), b.data() + 32 * i);
            tr.append_scalars("pi", b.data(), in.n_pi, 32, false);
        }
        mark("enqueue rounds 1+2");
        if ((rc = collect_rounds_1_2(in))) return rc;
        static const char* L12[6] = {"a_commit", "b_commit", "c_commit", "t_commit", "h1_commit", "h2_commit"};
        for (int k = 0; k < 6; ++k) tr_commit(L12[k], cm[k]);
        mark("transcript rounds 1+2");

        ch.beta = tr_challenge("beta"); ch.gamma = tr_challenge("gamma");
        ch.delta = tr_challenge("delta"); ch.epsilon = tr_challenge("epsilon");
        if (fe_eq<R>(ch.beta, ch.gamma) || fe_eq<R>(ch.beta, ch.delta) || fe_eq<R>(ch.beta, ch.epsilon) ||
            fe_eq<R>(ch.gamma, ch.delta) || fe_eq<R>(ch.gamma, ch.epsilon) || fe_eq<R>(ch.delta, ch.epsilon))
            return set_err(c, ZKT_ERR_EQUAL_CHALLENGES, "challenges must be different (prove.rs:202-207)");
        mark("challenges round 3");
        std::optional<ProfScope> prof_round;
        wait_end();
        prof_round.emplace(c, "round3");
        if ((rc = round_3(in))) return rc;
        prof_round.reset();
        tr_commit("z1_commit", cm[6]);
        tr_commit("z2_commit", cm[7]);
        mark("round 3 finish + commits");

        ch.alpha = tr_challenge("alpha");
        wait_end();
        prof_round.emplace(c, "round4");
        if ((rc = round_4(in))) return rc;
        prof_round.reset();
        tr_commit("q_lo_commit", cm[8]);
        tr_commit("q_mid_commit", cm[9]);
        tr_commit("q_hi_commit", cm[10]);
        mark("round 4");

        ch.xi = tr_challenge("xi");
        wait_end();
        prof_round.emplace(c, "round5");
        if ((rc = evaluations())) return rc;
        // zh(xi) = xi^n - 1 ; L_1(xi) = zh * 1 / (n * (xi - 1))   (util.rs:185-195)
        if (!xi_point<R, fe_inv_host<R>>(ch, (uint64_t)S.n, at)) return set_err(c, ZKT_ERR_ZERO_DENOMINATOR, "xi = 1");
        for (int k = 0; k < EV_COUNT; ++k) tr_scalar(ev_label(k), ev[k]);
        ch.eta = tr_challenge("eta");
        if ((rc = openings())) return rc;
        wait_end();
        prof_round.reset();
        if (classes && (rc = check_identity(in))) return rc;

        serialize(proof);
        mark("round 5 finish");
        dump_marks();
        return ZKT_OK;
    }
};

// One proof; a failed one drains every stream it may have left work on
template <class C>
static int run_prover(zkt_ctx* c, const zkt_prove_inputs& in, HostTranscript& tr, std::vector<uint8_t>& proof) {
    Prover<C> p(c, *c->circuit, tr);
    const int rc = p.run(in, proof);
    if (rc) {   // an early return may leave staged copies in flight
        (void)hipStreamSynchronize(c->circuit->copy_stream);
        if (c->circuit->comm_stream) (void)hipStreamSynchronize(c->circuit->comm_stream);
        if (c->circuit->aux_stream) (void)hipStreamSynchronize(c->circuit->aux_stream);
        (void)hipStreamSynchronize(c->stream);
    }
    return rc;
}

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
    auto key_coset = [&](const void* poly, size_t len, void* out) {   // keys/mod.rs:98-120 coset_fft, this GPU's class
        return S.G == 1 ? ntt_run(c, log_n + 2, 0, 1, poly, len, out)
                        : ntt_run_class(c, S.log_m, log_n + 2, S.cls, poly, len, out, S.fold);
    };
    for (int k = 0; k < 10; ++k)
        if ((rc = key_coset(S.pk[pk_of_cs[k]], n, S.coset[k]))) return rc;
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
    {   // l_1_coset = coset_fft(L_1), L_1 = ifft(1, 0, ..., 0) = (1/n, ..., 1/n)  (keys/mod.rs:119-120)
        const F ninv = fe_inv_host<R>(fe_from_u64<R>(n));
        if ((rc = gen_powers(c, S.ev[0], n, one.v, ninv.v))) return rc;
        if ((rc = key_coset(S.ev[0], n, S.coset[CS_L1]))) return rc;
    }
    // the tables that only ever multiply go to the quotient kernel's own Montgomery radix (poly.hpp)
    if ((rc = to_hat_form(c, S.coset[CS_QM], m, 1))) return rc;
    for (int k : {CS_QL, CS_QR, CS_QO, CS_QLOOKUP, CS_QTABLE, CS_L1})
        if ((rc = to_hat_form(c, S.coset[k], m, 0))) return rc;
    {   // zh_coset takes four values: (g * w4n^i)^n - 1 = g^n * w4^(i mod 4) - 1   (keys/mod.rs:115-117)
        const F gn = fe_pow_u64<R>(g, (uint64_t)n);
        const F w4 = fe_pow_u64<R>(w4n, (uint64_t)n);
        F cur = gn;
        for (int j = 0; j < 4; ++j) {
            F zh = fe_sub<R>(cur, one);
            if (fe_is_zero<R>(zh)) return set_err(c, ZKT_ERR_ZERO_DENOMINATOR, "vanishing polynomial is zero on the coset");
            F inv = fe_inv_host<R>(zh);
            memcpy(S.zh_inv[j], inv.v, 32);
            cur = fe_mul<R>(cur, w4);
        }
    }
    ZKT_HIP(c, hipStreamSynchronize(c->stream));
    c->circuit = st;
    return ZKT_OK;
}

// setup.rs:104-121: PC::commit of the ten labelled polynomials of the loaded circuit, ProverKey order, in batches of the
// MSM's slot count: the one commit stage of zkt_circuit_setup (lens[k] = n) and of zkt_circuit_commitments / _check_vk_file
// (the trimmed lengths; the zero polynomial commits to the identity without an MSM).  Identity = (0, 0) and the flag.
static int circuit_commit_keys(zkt_ctx* c, CircuitState& S, const size_t* lens, uint64_t* out_commitments, int* out_is_inf) {
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
template <class C>
static int circuit_setup_t(zkt_ctx* c, int log_n, const uint64_t* const* evals, const size_t* lens, unsigned evals_dev_mask,
                           uint64_t* out_commitments, int* out_is_inf) {
    int rc = circuit_load_t<C>(c, log_n, evals, lens, true, evals_dev_mask);
    if (rc) return rc;
    CircuitState& S = *c->circuit;
    size_t full[PK_COUNT];
    for (auto& l : full) l = S.n;   // the polynomials as the inverse transforms left them, untrimmed
    return circuit_commit_keys(c, S, full, out_commitments, out_is_inf);
}

// The ten ProverKey polynomials' lengths as DensePolynomial::from_coefficients_vec leaves them (trailing zeros stripped, the
// zero polynomial 0), taken on the device, whatever lengths the load was given.  Reads the keys and a word vector of its
// own: no work buffer, so it may run beside an announced proof's early rounds, on a fork and on a sharded context.
static int circuit_key_lens(zkt_ctx* c, const CircuitState& S, size_t* lens10) {
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

struct VtableTranscript;  // capi glue below

}  // namespace zkt

using namespace zkt;

namespace zkt {
// Adapter over a foreign transcript (the Rust shim's `T: TranscriptProtocol`): values cross in
// arkworks' Montgomery limbs, exactly what the shim can hand to T::append_scalar / append_commitment.
template <class C>
struct VtableAdapter : HostTranscript {
    using R = typename C::Fr;
    using Q = typename C::Fq;
    const zkt_transcript_vtable* vt;
    explicit VtableAdapter(const zkt_transcript_vtable* v) : vt(v) {}
    void append_u64(const char* label, uint64_t v) override { vt->append_u64(vt->user, label, v); }
    void append_scalars(const char* label, const uint8_t* le, size_t count, size_t, bool single) override {
        std::vector<uint64_t> m(4 * count);
        for (size_t i = 0; i < count; ++i) {
            Fe<R> x = HostF<R>::from_le_bytes(le + 32 * i);
            memcpy(&m[4 * i], x.v, 32);
        }
        vt->append_scalars(vt->user, label, m.data(), count, single ? 1 : 0);
    }
    void append_commitment(const char* label, const uint8_t* x_le, const uint8_t* y_le, size_t, bool inf) override {
        uint64_t xy[12] = {0};
        if (!inf) {
            Fe<Q> x, y;
            memcpy(x.v, x_le, Q::N * 4);
            memcpy(y.v, y_le, Q::N * 4);
            x = fe_to_mont<Q>(x);
            y = fe_to_mont<Q>(y);
            memcpy(xy, x.v, Q::N * 4);
            memcpy(xy + Q::N / 2, y.v, Q::N * 4);
        }
        vt->append_commitment(vt->user, label, xy, inf ? 1 : 0);
    }
    void challenge_scalar(const char* label, size_t, uint8_t out_le[32]) override {
        uint64_t m[4];
        vt->challenge_scalar(vt->user, label, m);
        HostF<R>::to_le_bytes(HostF<R>::from_words(m), out_le);
    }
};
}  // namespace zkt

// The two grand products alone (rows a8 / a9 of SURVEY.md section 8: permutation/mod.rs:181-254, lookup/mod.rs:94-151) over
// the loaded circuit's sigma evaluations and domain: round 3's own grand_products_begin / _finish (term kernels, prefix and
// suffix product scans, ONE host inversion for both denominators, z_combine), on caller-supplied vectors.
template <class C>
static int debug_grand_products_t(zkt_ctx* c, const uint64_t* ch, const uint64_t* const* v, uint64_t* out_z1, uint64_t* out_z2) {
    using H = HostF<typename C::Fr>;
    CircuitState& S = *c->circuit;
    const size_t n = S.n;
    void* dst[7] = {S.ev[0], S.ev[1], S.ev[2], S.ev[4], S.ev[3], S.ev[5], S.ev[6]};   // a b c f t h1 h2
    for (int k = 0; k < 7; ++k) ZKT_HIP(c, hipMemcpyAsync(dst[k], v[k], n * 32, hipMemcpyHostToDevice, c->stream));
    BuiltinTranscript tr(0, "zkt_debug_grand_products");   // no challenge is drawn: they are the caller's
    Prover<C> p(c, S, tr);
    p.ch.beta = H::from_words(ch); p.ch.gamma = H::from_words(ch + 4); p.ch.delta = H::from_words(ch + 8);
    p.ch.epsilon = H::from_words(ch + 12);
    int rc;
    if ((rc = p.grand_products_begin())) return rc;
    ZKT_HIP(c, hipStreamSynchronize(c->stream));
    if ((rc = p.grand_products_finish())) return rc;
    ZKT_HIP(c, hipMemcpyAsync(out_z1, S.ev[7], n * 32, hipMemcpyDeviceToHost, c->stream));
    ZKT_HIP(c, hipMemcpyAsync(out_z2, S.sc[0], n * 32, hipMemcpyDeviceToHost, c->stream));
    ZKT_HIP(c, hipStreamSynchronize(c->stream));
    return ZKT_OK;
}

// Round 2's h1 / h2 alone: f goes where round 2 puts q_lookup . c, then the prover's own combine_split runs
template <class C>
static int debug_combine_split_t(zkt_ctx* c, const uint64_t* table, size_t table_len, const uint64_t* f, bool fresh,
                                 uint64_t* h1_out, uint64_t* h2_out) {
    CircuitState& S = *c->circuit;
    const size_t n = S.n;
    BuiltinTranscript tr(0, "zkt_debug_combine_split");   // combine_split draws no challenge
    Prover<C> p(c, S, tr);
    ZKT_HIP(c, hipMemsetAsync(S.status, 0, 4, c->stream));
    ZKT_HIP(c, hipMemcpyAsync(S.ev[4], f, n * 32, hipMemcpyHostToDevice, c->stream));
    int rc = p.combine_split(table, table_len, fresh);
    if (!rc) rc = p.check_status();   // synchronises; bit 4 -> ZKT_ERR_NOT_IN_TABLE, bit 8 -> ZKT_ERR_INVALID_ARGUMENT
    if (rc) {
        (void)hipStreamSynchronize(c->stream);   // the uploads may still read the caller's f
        return rc;
    }
    ZKT_HIP(c, hipMemcpyAsync(h1_out, S.ev[5], n * 32, hipMemcpyDeviceToHost, c->stream));
    ZKT_HIP(c, hipMemcpyAsync(h2_out, S.ev[6], n * 32, hipMemcpyDeviceToHost, c->stream));
    ZKT_HIP(c, hipStreamSynchronize(c->stream));
    return ZKT_OK;
}

// ---- the ExtendedProverKey's vectors, one at a time (keys/mod.rs:78-146 as zkt_circuit_load runs it) ----------------------
// The derivation zkt_circuit_check_epk_file compares a file with and zkt_circuit_export_epk / _write_epk_file hand out: every
// vector is recomputed in arkworks' own form (the resident cosets partly live in the quotient kernel's radix).
static bool epk_is_evals(int k) { return k == EPK_QLOOKUP || k == EPK_S1 || k == EPK_S2 || k == EPK_S3; }
// zh_coset takes four values: g^n w4^(i mod 4) - 1 (keys/mod.rs:115-117); it never exists as a vector on the device
template <class R>
static void epk_zh4(int log_n, Fe<R> out[4]) {
    const size_t n = (size_t)1 << log_n;
    const Fe<R> one = fe_one<R>(), g = fe_from_u32<R>(R::GENERATOR), w4n = root_of_unity<R>(log_n + 2);
    const Fe<R> w4 = fe_pow_u64<R>(w4n, (uint64_t)n);
    Fe<R> cur = fe_pow_u64<R>(g, (uint64_t)n);
    for (int j = 0; j < 4; ++j) {
        out[j] = fe_sub<R>(cur, one);
        cur = fe_mul<R>(cur, w4);
    }
}
// Vector k (not zh_coset) on the device: *out is a resident table or `plain` (4n elements, written here; S.ev[0] as well
// for l_1_coset), Montgomery form; with `canon` (4n elements) the canonical values, written there.
template <class C>
static int epk_vector_dev(zkt_ctx* c, CircuitState& S, int k, void* plain, void* canon, const void** out) {
    using R = typename C::Fr;
    using F = Fe<R>;
    static const int pk_of[EPK_VECTORS] = {PK_QM, PK_QL, PK_QR, PK_QO, PK_QC, -1, PK_QLOOKUP, PK_QTABLE, -1, PK_S1, -1, PK_S2, -1, PK_S3,
                                           -1, -1, -1};
    const size_t n = S.n;
    const int log_n = S.log_n;
    const size_t expect = epk_is_evals(k) ? n : 4 * n;
    int rc;
    const void* src = plain;
    if (pk_of[k] >= 0) {
        if ((rc = ntt_run(c, log_n + 2, 0, 1, S.pk[pk_of[k]], n, plain))) return rc;
    } else if (k == EPK_QLOOKUP) {
        src = S.q_lookup_ev;
    } else if (epk_is_evals(k)) {
        src = S.sigma_ev[k == EPK_S1 ? 0 : k == EPK_S2 ? 1 : 2];
    } else if (k == EPK_X_C) {
        src = S.coset[CS_X];
    } else {              // l_1_coset = coset_fft(ifft(1, 0, ..., 0)) (keys/mod.rs:119-120)
        const F one = fe_one<R>();
        const F ninv = fe_inv_host<R>(fe_from_u64<R>(n));
        if ((rc = gen_powers(c, S.ev[0], n, one.v, ninv.v))) return rc;
        if ((rc = ntt_run(c, log_n + 2, 0, 1, S.ev[0], n, plain))) return rc;
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
        epk_zh4<R>(S.log_n, zh);
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
        epk_zh4<R>(S.log_n, zh);
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
            epk_zh4<R>(S.log_n, zh);
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

int zkt_circuit_load(zkt_ctx* c, int log_n, const uint64_t* const* pk_polys, const size_t* pk_lens) {
    if (!c || !pk_polys || !pk_lens) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    (void)hipSetDevice(c->device);
    if (c->curve == ZKT_CURVE_BN254) return circuit_load_t<Bn254Curve>(c, log_n, pk_polys, pk_lens);
    return circuit_load_t<Bls381Curve>(c, log_n, pk_polys, pk_lens);
}

// With a communicator attached every rank must hold exactly its zkt_shard_range of the key: a rank that loaded the
// whole key (or somebody else's slice) would make the combined commitments a multiple of the right ones.
static int check_sharded_key(zkt_ctx* c) {
    if (!c->sharded()) return ZKT_OK;
    size_t off = 0, cnt = 0, total = 0, lo = 0, hi = 0;
    zkt::msm_slice(c, &off, &cnt, &total);
    (void)zkt_shard_range(total, c->comm.vt.rank, c->comm.vt.world, &lo, &hi);
    if (off != lo || off + cnt != hi)
        return set_err(c, ZKT_ERR_INVALID_ARGUMENT,
                       "sharded proof: this rank must load powers zkt_shard_range(total, rank, world) with zkt_srs_load_slice");
    if (c->circuit && c->circuit->G != c->comm.vt.world)
        return set_err(c, ZKT_ERR_NOT_LOADED, "the circuit was loaded for another communicator");
    return ZKT_OK;
}

static int prove_impl(zkt_ctx* c, const zkt_prove_inputs* in, HostTranscript& tr, uint8_t* out, size_t cap, size_t* len) {
    if (!c->circuit) return set_err(c, ZKT_ERR_NOT_LOADED, "no circuit loaded (zkt_circuit_load)");
    if (!c->msm) return set_err(c, ZKT_ERR_NOT_LOADED, "no SRS loaded (zkt_srs_load)");
    if (int rc0 = check_sharded_key(c)) return rc0;
    (void)hipSetDevice(c->device);
    // the Lagrange-basis table of this domain (lagrange.hip): built on the first proof after a key or circuit change
    if (!c->lagrange_off)
        if (int rc1 = lagrange_ensure(c, c->circuit->log_n)) return rc1;
    std::vector<uint8_t> proof;
    const int rc = c->curve == ZKT_CURVE_BN254 ? run_prover<Bn254Curve>(c, *in, tr, proof) : run_prover<Bls381Curve>(c, *in, tr, proof);
    if (rc) {
        // a failed proof withdraws the announcement of its successor: the next call must not issue early work from
        // pointers the caller may have released meanwhile, nor pick up half-issued early rounds
        c->circuit->has_next = false;
        c->circuit->prefetch_stage = 0;
        return rc;
    }
    if (len) *len = proof.size();
    if (proof.size() > cap) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "proof buffer too small");
    memcpy(out, proof.data(), proof.size());
    return ZKT_OK;
}

// ---- commitments of evaluation vectors (lagrange.hip) --------------------------------------------------
int zkt_ctx_set_lagrange(zkt_ctx* c, int on) {
    if (!c) return ZKT_ERR_INVALID_ARGUMENT;
    c->lagrange_off = !on;
    ++c->msm_epoch;   // early work of an announced proof was issued under the other setting
    return ZKT_OK;
}

int zkt_ctx_set_wire_elimination(zkt_ctx* c, int mode) {
    if (!c) return ZKT_ERR_INVALID_ARGUMENT;
    if (mode < 0 || mode > 2) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "mode: 0 off, 1 automatic, 2 whenever a table can be built");
    c->wire_elim_mode = mode;
    ++c->msm_epoch;   // early work of an announced proof was issued under the other setting
    return ZKT_OK;
}

int zkt_ctx_set_quotient_route(zkt_ctx* c, int mode) {
    if (!c) return ZKT_ERR_INVALID_ARGUMENT;
    if (mode < 0 || mode > 2) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "mode: 0 automatic, 1 three classes, 2 the whole coset");
    c->quotient_route = mode;   // the next proof compares its route with what was transformed ahead of time (choose_route)
    return ZKT_OK;
}

int zkt_ctx_set_fused_passes(zkt_ctx* c, int mode) {
    if (!c) return ZKT_ERR_INVALID_ARGUMENT;
    if (mode < 0 || mode > 2) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "mode: 0 automatic, 1 fused, 2 one launch per step");
    c->fused_passes = mode;   // read by every round as it is enqueued; early work of an announced proof stays valid (same values)
    return ZKT_OK;
}

int zkt_debug_quotient_top(zkt_ctx* c, uint64_t* out_u, int* out_on_classes) {
    if (!c || !out_u) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (!c->circuit) return set_err(c, ZKT_ERR_NOT_LOADED, "no circuit loaded (zkt_circuit_load)");
    const CircuitState& S = *c->circuit;
    if (out_on_classes) *out_on_classes = S.use_classes ? 1 : 0;
    memcpy(out_u, S.last_u, sizeof(S.last_u));   // zero until a proof has taken the route
    return ZKT_OK;
}

int zkt_debug_quotient_coeffs(zkt_ctx* c, uint64_t* out, size_t count) {
    if (!c || !out) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (!c->circuit) return set_err(c, ZKT_ERR_NOT_LOADED, "no circuit loaded (zkt_circuit_load)");
    const CircuitState& S = *c->circuit;
    if (count > 4 * S.n) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "the quotient vector holds 4n elements");
    (void)hipSetDevice(c->device);
    ZKT_HIP(c, hipStreamSynchronize(c->stream));
    ZKT_HIP(c, hipMemcpy(out, S.qev, count * 32, hipMemcpyDeviceToHost));
    return ZKT_OK;
}

extern "C++" template <class R>
static void debug_quotient_classes_host_t(int log_n, const uint64_t* windows, const uint64_t* challenges, uint64_t* out_u,
                                          uint64_t* out_consts) {
    typedef Fe<R> F;
    const QuotientClassConsts<R> q = quotient_class_consts<R>(log_n);
    for (int k = 0; k < 4; ++k) memcpy(out_consts + 4 * k, q.gamma[k].v, 32);
    for (int k = 0; k < 9; ++k) memcpy(out_consts + 4 * (4 + k), q.vinv[k].v, 32);
    for (int k = 0; k < 3; ++k) memcpy(out_consts + 4 * (13 + k), q.g3[k].v, 32);
    const uint32_t* w = (const uint32_t*)windows;
    QuotientWindows W{};
    const uint32_t** slot[10] = {&W.a, &W.b, &W.c, &W.z1, &W.z2, &W.t, &W.sigma1, &W.sigma2, &W.sigma3, &W.q_lookup};
    for (int k = 0; k < 10; ++k) *slot[k] = w + (size_t)k * QCW * 8;
    F alpha, beta, delta, u[6];
    memcpy(alpha.v, challenges, 32);
    memcpy(beta.v, challenges + 4, 32);
    memcpy(delta.v, challenges + 8, 32);
    quotient_top_coefficients<R>(log_n, W, alpha, beta, delta, u);
    for (int e = 0; e < 6; ++e) memcpy(out_u + 4 * e, u[e].v, 32);
}

int zkt_debug_quotient_classes_host(int curve, int log_n, const uint64_t* windows, const uint64_t* challenges, uint64_t* out_u,
                                    uint64_t* out_consts) {
    if (!windows || !challenges || !out_u || !out_consts) return ZKT_ERR_INVALID_ARGUMENT;
    if (curve == ZKT_CURVE_BN254) {
        if (log_n < 3 || log_n + 2 > Bn254Fr::TWO_ADICITY) return ZKT_ERR_INVALID_DOMAIN_SIZE;
        debug_quotient_classes_host_t<Bn254Fr>(log_n, windows, challenges, out_u, out_consts);
    } else if (curve == ZKT_CURVE_BLS12_381) {
        if (log_n < 3 || log_n + 2 > Bls381Fr::TWO_ADICITY) return ZKT_ERR_INVALID_DOMAIN_SIZE;
        debug_quotient_classes_host_t<Bls381Fr>(log_n, windows, challenges, out_u, out_consts);
    } else {
        return ZKT_ERR_INVALID_ARGUMENT;
    }
    return ZKT_OK;
}

int zkt_lagrange_info(zkt_ctx* c, int* log_n, size_t* bases) {
    if (!c) return ZKT_ERR_INVALID_ARGUMENT;
    const bool ready = c->circuit && lagrange_ready(c, c->circuit->log_n) && !c->lagrange_off;
    if (log_n) *log_n = ready ? c->circuit->log_n : -1;
    if (bases) *bases = ready ? lagrange_bases(c) : 0;
    return ZKT_OK;
}

int zkt_commit_evals_dev(zkt_ctx* c, const void* d_evals, const uint64_t* blinders, int k, int path, uint64_t* out_xy,
                         int* out_is_infinity) {
    if (!c || !d_evals || !out_xy || (k > 0 && !blinders)) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (k < 0 || k > 3) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "0 .. 3 blinders");
    if (!c->circuit) return set_err(c, ZKT_ERR_NOT_LOADED, "no circuit loaded (the domain comes from it)");
    if (!c->msm) return set_err(c, ZKT_ERR_NOT_LOADED, "no SRS loaded (zkt_srs_load)");
    if (c->sharded()) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "not available on a sharded key");
    (void)hipSetDevice(c->device);
    CircuitState& S = *c->circuit;
    const size_t n = S.n;
    int rc;
    if (path == 1) {
        if ((rc = lagrange_ensure(c, S.log_n))) return rc;
        if (!lagrange_ready(c, S.log_n)) return set_err(c, ZKT_ERR_NOT_LOADED, "the key is too short for the Lagrange-basis table");
    } else if (path != 0) {
        return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "path: 0 coefficients, 1 Lagrange basis");
    }
    c->circuit->prefetch_stage = 0;   // the work buffer below belongs to round 5 of an announced proof as well
    uint32_t* d_len = S.status + 8 + 12;
    void* d_bl = (char*)S.lag_scalars + (n + 8) * 32;
    void* poly = S.poly[12];
    ZKT_HIP(c, hipMemsetAsync(d_len, 0, 4, c->stream));
    if (k) ZKT_HIP(c, hipMemcpyAsync(d_bl, blinders, (size_t)k * 32, hipMemcpyHostToDevice, c->stream));
    // poly_from_evals + add_blinders_to_poly (util.rs:63-86, prove.rs:472-483)
    if ((rc = ntt_run(c, S.log_n, 1, 0, d_evals, n, poly))) return rc;
    if (c->fused(4)) {
        const TrimBlindSpec tb{poly, d_bl, d_len, k};
        if ((rc = poly_trim_blind(c, &tb, 1, n, 8))) return rc;
    } else {
        if ((rc = poly_trim_len(c, poly, n, d_len, (char*)poly + n * 32, 8))) return rc;
        if (k && (rc = poly_add_blinders(c, poly, d_len, d_bl, k, n + 8))) return rc;
    }
    if (path == 0) return msm_g1_dev(c, poly, n + (size_t)k, 0, 1, out_xy, out_is_infinity);
    if ((rc = lagrange_scalars(c, d_evals, n, d_len, d_bl, k, S.roots, S.lag_scalars))) return rc;
    if ((rc = msm_begin(c, S.lag_scalars, n + (size_t)k, 0, 1, 0, 1))) return rc;
    uint64_t xy[12] = {};
    if ((rc = msm_end(c, 0, xy))) return rc;
    const size_t words = c->curve == ZKT_CURVE_BN254 ? 8 : 12;
    memcpy(out_xy, xy, words * 8);
    if (out_is_infinity) {
        bool any = false;
        for (size_t i = 0; i < words; ++i) any = any || xy[i] != 0;
        *out_is_infinity = any ? 0 : 1;
    }
    return ZKT_OK;
}

int zkt_circuit_setup(zkt_ctx* c, int log_n, const uint64_t* const* evals, const size_t* eval_lens, int evals_on_device,
                      uint64_t* out_commitments, int* out_is_infinity) {
    if (!c || !evals || !eval_lens || !out_commitments) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (!c->msm) return set_err(c, ZKT_ERR_NOT_LOADED, "no SRS loaded (zkt_srs_load)");
    (void)hipSetDevice(c->device);
    if (log_n < 3 || log_n > 26) return set_err(c, ZKT_ERR_INVALID_DOMAIN_SIZE, "circuit bound out of range");
    if (int rc0 = check_sharded_key(c)) return rc0;
    const unsigned mask = evals_on_device ? (1u << PK_COUNT) - 1u : 0u;
    if (c->curve == ZKT_CURVE_BN254)
        return circuit_setup_t<Bn254Curve>(c, log_n, evals, eval_lens, mask, out_commitments, out_is_infinity);
    return circuit_setup_t<Bls381Curve>(c, log_n, evals, eval_lens, mask, out_commitments, out_is_infinity);
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
        rc = c->curve == ZKT_CURVE_BN254 ? circuit_setup_t<Bn254Curve>(c, log_n, ev, lens, mask, out_commitments, out_is_infinity)
                                         : circuit_setup_t<Bls381Curve>(c, log_n, ev, lens, mask, out_commitments, out_is_infinity);
    }
    (void)hipStreamSynchronize(c->stream);   // before `tmp` goes
    return rc;
}

// helper.rs:13-75 check_gate over every row (check.hip).  Reads the loaded keys, writes nothing of the circuit state: the
// work buffers, the resident lookup keys and an announced proof's early rounds stay as they are.
int zkt_circuit_check_witness(zkt_ctx* c, const zkt_prove_inputs* in, int flags, zkt_witness_report* out) {
    if (!c) return ZKT_ERR_INVALID_ARGUMENT;
    if (!in || !out) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (!c->circuit) return set_err(c, ZKT_ERR_NOT_LOADED, "no circuit loaded (zkt_circuit_load)");
    if (flags & ~ZKT_CHECK_WIRING) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "unknown flag bits");
    const CircuitState& S = *c->circuit;
    const size_t n = S.n;
    if (in->n_rows > n) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "more rows than the circuit bound");
    if (in->table_len >= n) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "max table size is equal or larger than n");
    if (in->table_len && !in->table) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null lookup table");
    if (in->n_pi && (!in->pi_pos || !in->pi_vals)) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null public inputs");
    for (size_t i = 0; i < in->n_pi; ++i)
        if (in->pi_pos[i] >= n) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "public input position out of range");
    if (in->a_evals) {
        if (flags & ZKT_CHECK_WIRING)
            return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "ZKT_CHECK_WIRING needs the witness as variables + w_l / w_r / w_o: evaluation vectors carry no wiring");
        if (in->n_rows && (!in->b_evals || !in->c_evals)) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null wire vector");
    } else {
        if (in->n_rows && (!in->w_l || !in->w_r || !in->w_o)) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null wire index vector");
        if (in->n_vars && !in->variables) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null variable map");
        if (in->n_vars > 0xFFFFFFFEull) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "too many variables");
        if ((flags & ZKT_CHECK_WIRING) && S.log_n > 25)
            return set_err(c, ZKT_ERR_INVALID_DOMAIN_SIZE, "InvalidEvalDomainSize: the wiring's positions are 32-bit (log_n <= 25)");
    }
    (void)hipSetDevice(c->device);
    WitnessCheckKeys keys{};
    keys.log_n = S.log_n;
    for (int k = 0; k < 5; ++k) keys.pk[k] = S.pk[PK_QM + k];   // PK_QM .. PK_QC
    keys.q_lookup_ev = S.q_lookup_ev;
    for (int k = 0; k < 3; ++k) keys.sigma_ev[k] = S.sigma_ev[k];
    return witness_check(c, keys, *in, flags, out);
}

// The plan of a witness completion over the loaded circuit's selectors (witness_plan.hip).  Reads the loaded keys, writes
// nothing of the circuit state; the plan keeps no pointer into it.
int zkt_witness_plan_create_ex(zkt_ctx* c, const uint32_t* w_l, const uint32_t* w_r, const uint32_t* w_o, size_t n_rows, size_t n_vars,
                               int wiring_on_device, const size_t* pi_pos, size_t n_pi, uint32_t rules, zkt_witness_plan** out) {
    if (!c) return ZKT_ERR_INVALID_ARGUMENT;
    if (!out) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (!c->circuit) return set_err(c, ZKT_ERR_NOT_LOADED, "no circuit loaded (zkt_circuit_load)");
    const CircuitState& S = *c->circuit;
    WitnessPlanKeys keys{};
    keys.log_n = S.log_n;
    for (int k = 0; k < 5; ++k) keys.pk[k] = S.pk[PK_QM + k];   // PK_QM .. PK_QC
    return witness_plan_create(c, keys, w_l, w_r, w_o, n_rows, n_vars, wiring_on_device, pi_pos, n_pi, rules, out);
}

int zkt_witness_plan_create(zkt_ctx* c, const uint32_t* w_l, const uint32_t* w_r, const uint32_t* w_o, size_t n_rows, size_t n_vars,
                            int wiring_on_device, const size_t* pi_pos, size_t n_pi, zkt_witness_plan** out) {
    return zkt_witness_plan_create_ex(c, w_l, w_r, w_o, n_rows, n_vars, wiring_on_device, pi_pos, n_pi, 0, out);
}

// The single check's rules over a batch of completed maps under one wiring (check.hip).  Reads the loaded keys, writes
// nothing of the circuit state, as zkt_circuit_check_witness.
int zkt_circuit_check_witness_batch(zkt_ctx* c, const zkt_witness_batch* in, int flags, zkt_witness_report* out) {
    if (!c) return ZKT_ERR_INVALID_ARGUMENT;
    if (!in || !out) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (!c->circuit) return set_err(c, ZKT_ERR_NOT_LOADED, "no circuit loaded (zkt_circuit_load)");
    if (flags & ~ZKT_CHECK_WIRING) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "unknown flag bits");
    const CircuitState& S = *c->circuit;
    const size_t n = S.n;
    if (in->batch < 1 || in->batch > ZKT_WITNESS_BATCH_MAX) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "1 <= batch <= ZKT_WITNESS_BATCH_MAX");
    if (in->stride < in->n_vars) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "stride below n_vars");
    if (in->n_tables != 0 && in->n_tables != 1 && in->n_tables != in->batch)
        return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "n_tables must be 0, 1 or batch");
    if (in->n_tables && (!in->tables || !in->table_lens)) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null lookup tables");
    if (in->n_rows > n) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "more rows than the circuit bound");
    for (size_t t = 0; t < in->n_tables; ++t) {
        if (in->table_lens[t] >= n) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "max table size is equal or larger than n");
        if (in->table_lens[t] && !in->tables[t]) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null lookup table");
    }
    if (in->n_pi && (!in->pi_pos || !in->d_pi_vals)) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null public inputs");
    for (size_t i = 0; i < in->n_pi; ++i)
        if (in->pi_pos[i] >= n) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "public input position out of range");
    if (in->n_rows && (!in->w_l || !in->w_r || !in->w_o)) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null wire index vector");
    if (in->n_vars && !in->d_variables) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null variable map");
    if (in->n_vars > 0xFFFFFFFEull) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "too many variables");
    if ((flags & ZKT_CHECK_WIRING) && S.log_n > 25)
        return set_err(c, ZKT_ERR_INVALID_DOMAIN_SIZE, "InvalidEvalDomainSize: the wiring's positions are 32-bit (log_n <= 25)");
    (void)hipSetDevice(c->device);
    WitnessCheckKeys keys{};
    keys.log_n = S.log_n;
    for (int k = 0; k < 5; ++k) keys.pk[k] = S.pk[PK_QM + k];   // PK_QM .. PK_QC
    keys.q_lookup_ev = S.q_lookup_ev;
    for (int k = 0; k < 3; ++k) keys.sigma_ev[k] = S.sigma_ev[k];
    return witness_check_batch(c, keys, *in, flags, out);
}

// Test hook: the fused quotient pass on its own (quotient_poly.rs:98-224) over the loaded circuit's key cosets and
// caller-supplied witness cosets, so that the kernel is compared point by point on inputs that satisfy nothing.
int zkt_debug_quotient(zkt_ctx* c, const uint64_t* challenges, const uint64_t* const* wit, const uint64_t* pi_pos,
                       const uint64_t* pi_vals, size_t n_pi, uint64_t* out) {
    if (!c || !challenges || !wit || !out || (n_pi && (!pi_pos || !pi_vals)))
        return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (!c->circuit) return set_err(c, ZKT_ERR_NOT_LOADED, "no circuit loaded (zkt_circuit_load)");
    CircuitState& S = *c->circuit;
    if (S.G != 1) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "zkt_debug_quotient: whole-coset circuits only");
    if (n_pi > (size_t)QUOTIENT_PI_DIRECT_MAX) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "too many direct public inputs");
    for (size_t i = 0; i < n_pi; ++i)
        if (pi_pos[i] >= S.n) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "public input position out of range");
    (void)hipSetDevice(c->device);
    const size_t bytes = 4 * S.n * 32;
    DevSet tmp(c->device);
    void* d[W_COUNT] = {};
    void* d_out = nullptr;
    uint32_t* d_tab = nullptr;
    int rc = ZKT_OK;
    for (int k = 0; k < W_COUNT && !rc; ++k) {
        if (k == W_PI && n_pi) continue;
        if (!wit[k]) rc = set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null witness coset");
        else if (!(rc = tmp.alloc(c, &d[k], bytes)) && hipMemcpy(d[k], wit[k], bytes, hipMemcpyHostToDevice) != hipSuccess)
            rc = set_err(c, ZKT_ERR_HIP, "copy of a witness coset failed");
    }
    if (!rc) rc = tmp.alloc(c, &d_out, bytes);
    if (!rc && n_pi) {
        std::vector<uint32_t> tab(10 * n_pi);
        if (c->curve == ZKT_CURVE_BN254) pi_rows<Bn254Curve::Fr>(pi_pos, pi_vals, n_pi, 1, tab.data());
        else pi_rows<Bls381Curve::Fr>(pi_pos, pi_vals, n_pi, 1, tab.data());
        if (!(rc = tmp.alloc(c, (void**)&d_tab, tab.size() * 4)) &&
            hipMemcpy(d_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
            rc = set_err(c, ZKT_ERR_HIP, "copy of the public-input rows failed");
    }
    if (!rc) {
        QuotientArgs q = quotient_args(S, d, challenges, challenges + 4, challenges + 8, challenges + 12, challenges + 16);
        q.out = d_out;
        q.n4 = 4 * S.n;
        q.pi_tab = n_pi ? d_tab : nullptr;
        q.n_pi_direct = (uint32_t)n_pi;
        rc = quotient_pointwise(c, q);
        if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = set_err(c, ZKT_ERR_HIP, "quotient kernel failed");
        if (!rc && hipMemcpy(out, d_out, bytes, hipMemcpyDeviceToHost) != hipSuccess) rc = set_err(c, ZKT_ERR_HIP, "copy back failed");
    }
    return rc;
}

int zkt_debug_grand_products(zkt_ctx* c, const uint64_t* challenges, const uint64_t* const* vectors, uint64_t* out_z1,
                             uint64_t* out_z2) {
    if (!c || !challenges || !vectors || !out_z1 || !out_z2) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    for (int k = 0; k < 7; ++k)
        if (!vectors[k]) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null vector");
    if (!c->circuit) return set_err(c, ZKT_ERR_NOT_LOADED, "no circuit loaded (zkt_circuit_load)");
    (void)hipSetDevice(c->device);
    c->circuit->prefetch_stage = 0;   // the work buffers are shared with an announced proof's early rounds
    // the caller's t replaces the evaluations of the cached table polynomial: the next proof rebuilds it
    c->circuit->t_cached = false;
    if (c->curve == ZKT_CURVE_BN254) return debug_grand_products_t<Bn254Curve>(c, challenges, vectors, out_z1, out_z2);
    return debug_grand_products_t<Bls381Curve>(c, challenges, vectors, out_z1, out_z2);
}

int zkt_debug_combine_split(zkt_ctx* c, const uint64_t* table, size_t table_len, const uint64_t* f, int fresh,
                            uint64_t* h1_out, uint64_t* h2_out) {
    if (!c || !f || !h1_out || !h2_out || (table_len && !table)) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (!c->circuit) return set_err(c, ZKT_ERR_NOT_LOADED, "no circuit loaded (zkt_circuit_load)");
    CircuitState& S = *c->circuit;
    if (S.has_next) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "zkt_debug_combine_split: a next proof is announced");
    if (table_len >= S.n) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "max table size is equal or larger than n");
    (void)hipSetDevice(c->device);
    S.prefetch_stage = 0;   // the work buffers are shared with an announced proof's early rounds
    // the keys this call leaves resident need not be those of the cached table polynomial: the next proof rebuilds both
    S.t_cached = false;
    if (c->curve == ZKT_CURVE_BN254) return debug_combine_split_t<Bn254Curve>(c, table, table_len, f, fresh != 0, h1_out, h2_out);
    return debug_combine_split_t<Bls381Curve>(c, table, table_len, f, fresh != 0, h1_out, h2_out);
}

int zkt_circuit_check_epk_file(zkt_ctx* c, const char* epk_path, int* first_mismatch_vector, size_t* mismatch_at) {
    if (!c || !epk_path || !first_mismatch_vector || !mismatch_at) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (!c->circuit) return set_err(c, ZKT_ERR_NOT_LOADED, "no circuit loaded (zkt_circuit_load)");
    if (c->circuit->G != 1) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "a sharded context holds one class of every coset: check the file on an unsharded one");
    (void)hipSetDevice(c->device);
    c->circuit->prefetch_stage = 0;   // the work buffers are shared with an announced proof's early rounds
    if (c->curve == ZKT_CURVE_BN254) return circuit_check_epk_t<Bn254Curve>(c, epk_path, first_mismatch_vector, mismatch_at);
    return circuit_check_epk_t<Bls381Curve>(c, epk_path, first_mismatch_vector, mismatch_at);
}

// ---- the keys that setup makes, handed back (setup.rs:42-166 returns ProverKey, VerifierKey, ExtendedProverKey) -------------
int zkt_circuit_export(zkt_ctx* c, uint64_t* const* out_polys, size_t* lens10) {
    if (!c || !lens10) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (!c->circuit) return set_err(c, ZKT_ERR_NOT_LOADED, "no circuit loaded (zkt_circuit_load)");
    (void)hipSetDevice(c->device);
    const CircuitState& S = *c->circuit;   // read-only on the keys: forks, sharded contexts (the polynomials are replicated)
    if (int rc = circuit_key_lens(c, S, lens10)) return rc;
    if (!out_polys) return ZKT_OK;
    for (int k = 0; k < PK_COUNT; ++k)
        if (out_polys[k] && lens10[k])
            ZKT_HIP(c, hipMemcpyAsync(out_polys[k], S.pk[k], lens10[k] * 32, hipMemcpyDeviceToHost, c->stream));
    ZKT_HIP(c, hipStreamSynchronize(c->stream));
    return ZKT_OK;
}

// what the entries below share: they use the per-proof work buffers (or the MSM's slots)
static int circuit_work_entry(zkt_ctx* c, const char* who) {
    if (!c->circuit) return set_err(c, ZKT_ERR_NOT_LOADED, "no circuit loaded (zkt_circuit_load)");
    if (c->sharded() || c->circuit->G != 1)
        return set_err(c, ZKT_ERR_INVALID_ARGUMENT, std::string(who) + ": a sharded context holds one class of every coset and a slice of the key; use an unsharded one");
    if (c->circuit->has_next) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, std::string(who) + ": a next proof is announced");
    (void)hipSetDevice(c->device);
    c->circuit->prefetch_stage = 0;   // the work buffers are shared with an announced proof's early rounds
    return ZKT_OK;
}

static int circuit_commitments(zkt_ctx* c, uint64_t* out_commitments, int* out_is_infinity) {
    if (!c->msm) return set_err(c, ZKT_ERR_NOT_LOADED, "no SRS loaded (zkt_srs_load)");
    CircuitState& S = *c->circuit;
    size_t lens[PK_COUNT];
    if (int rc = circuit_key_lens(c, S, lens)) return rc;
    return circuit_commit_keys(c, S, lens, out_commitments, out_is_infinity);
}

int zkt_circuit_commitments(zkt_ctx* c, uint64_t* out_commitments, int* out_is_infinity) {
    if (!c || !out_commitments) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (int rc = circuit_work_entry(c, "zkt_circuit_commitments")) return rc;
    return circuit_commitments(c, out_commitments, out_is_infinity);
}

int zkt_circuit_export_epk(zkt_ctx* c, int which, uint64_t* out_mont, size_t cap, size_t* lens17) {
    if (!c || !lens17) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (which < -1 || which >= EPK_VECTORS) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "which: -1 (lengths) or 0 .. 16");
    if (int rc = circuit_work_entry(c, "zkt_circuit_export_epk")) return rc;
    if (c->curve == ZKT_CURVE_BN254) return circuit_export_epk_t<Bn254Curve>(c, which, out_mont, cap, lens17);
    return circuit_export_epk_t<Bls381Curve>(c, which, out_mont, cap, lens17);
}

int zkt_circuit_check_vk_file(zkt_ctx* c, const char* vk_path, int* first_mismatch) {
    if (!c || !vk_path || !first_mismatch) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (int rc = circuit_work_entry(c, "zkt_circuit_check_vk_file")) return rc;
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

static int circuit_write_epk(zkt_ctx* c, const char* epk_path) {
    kw::File w(epk_path);
    const int rc = c->curve == ZKT_CURVE_BN254 ? circuit_write_epk_t<Bn254Curve>(c, w) : circuit_write_epk_t<Bls381Curve>(c, w);
    if (rc) return rc;   // (the temporary file goes with `w`)
    return keyfile_write_done(c, w);
}

int zkt_circuit_write_epk_file(zkt_ctx* c, const char* epk_path) {
    if (!c || !epk_path) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (int rc = circuit_work_entry(c, "zkt_circuit_write_epk_file")) return rc;
    return circuit_write_epk(c, epk_path);
}

// bin/src/main.rs:105-111: the files `Compile` writes beside --ck (zkt_srs_save_file)
int zkt_circuit_save_files(zkt_ctx* c, const char* pk_path, const char* vk_path, const char* epk_path, const size_t* pi_pos,
                           size_t n_pi) {
    if (!c || (n_pi && !pi_pos)) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (!c->circuit) return set_err(c, ZKT_ERR_NOT_LOADED, "no circuit loaded (zkt_circuit_load)");
    const size_t n = c->circuit->n;
    for (size_t i = 0; i < n_pi; ++i)
        if (pi_pos[i] >= n || (i && pi_pos[i] <= pi_pos[i - 1]))
            return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "public-input positions must be ascending, distinct and below n");
    if (vk_path && !c->msm) return set_err(c, ZKT_ERR_NOT_LOADED, "no SRS loaded (zkt_srs_load)");
    if (vk_path || epk_path) {
        if (int rc = circuit_work_entry(c, "zkt_circuit_save_files")) return rc;
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
        if (c->curve == ZKT_CURVE_BN254) pi_roots_t<Bn254Fr>(c->circuit->log_n, pi_pos, n_pi, roots.data());
        else pi_roots_t<Bls381Fr>(c->circuit->log_n, pi_pos, n_pi, roots.data());
        kw::File w(vk_path);
        kw::write_verifier_key(w, c->curve, (uint64_t)n, roots.data(), n_pi, commits, inf);
        if (int rc = keyfile_write_done(c, w)) return rc;
    }
    if (epk_path) return circuit_write_epk(c, epk_path);
    return ZKT_OK;
}

// Row a13's two kernels alone (linearization_poly.rs:55-121): k <= 12 polynomials of the prover's lengths, each evaluated at its
// own point (poly_eval_many), and their linear combination sum_j scalars[j] polys[j] (poly_lincomb)
int zkt_debug_eval_lincomb(zkt_ctx* c, const uint64_t* const* polys, const size_t* lens, int k, const uint64_t* points,
                           const uint64_t* scalars, uint64_t* out_evals, uint64_t* out_lincomb, size_t out_len) {
    if (!c || !polys || !lens || !points || !scalars || !out_evals || !out_lincomb) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (!c->circuit) return set_err(c, ZKT_ERR_NOT_LOADED, "no circuit loaded (zkt_circuit_load)");
    CircuitState& S = *c->circuit;
    const size_t cap = S.n + 8;
    if (k < 1 || k > 12 || out_len < 1 || out_len > cap) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "1 .. 12 polynomials, out_len <= n + 8");
    for (int j = 0; j < k; ++j)
        if (!polys[j] || lens[j] < 1 || lens[j] > cap) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "1 .. n + 8 coefficients each");
    (void)hipSetDevice(c->device);
    S.prefetch_stage = 0;   // the work buffers are shared with an announced proof's early rounds
    EvalArgs ea{};
    LinCombArgs lc{};
    ea.count = k;
    lc.nterms = k;
    for (int j = 0; j < k; ++j) {
        ZKT_HIP(c, hipMemcpyAsync(S.poly[j], polys[j], lens[j] * 32, hipMemcpyHostToDevice, c->stream));
        ea.poly[j] = lc.poly[j] = S.poly[j];
        ea.len[j] = lc.len[j] = lens[j];
        memcpy(ea.point[j], points + 4 * j, 32);
        memcpy(lc.scalar[j], scalars + 4 * j, 32);
    }
    void* d_partials = (char*)S.small + 64 * 32;
    void* d_results = (char*)S.small + 32 * 32;
    int rc = poly_eval_many(c, ea, d_partials, d_results, S.eval_pw);
    if (rc) return rc;
    if ((rc = poly_lincomb(c, lc, S.sc[0], out_len))) return rc;
    ZKT_HIP(c, hipMemcpyAsync(out_evals, d_results, (size_t)k * 32, hipMemcpyDeviceToHost, c->stream));
    ZKT_HIP(c, hipMemcpyAsync(out_lincomb, S.sc[0], out_len * 32, hipMemcpyDeviceToHost, c->stream));
    ZKT_HIP(c, hipStreamSynchronize(c->stream));
    return ZKT_OK;
}

// kzg10::compute_witness_polynomial alone (row a12: the division of prove.rs:381-451's aggregated polynomial by X - z)
int zkt_debug_open_witness(zkt_ctx* c, const uint64_t* coeffs, size_t len, const uint64_t* z4, uint64_t* out) {
    if (!c || !coeffs || !z4 || !out) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (!c->circuit) return set_err(c, ZKT_ERR_NOT_LOADED, "no circuit loaded (zkt_circuit_load)");
    CircuitState& S = *c->circuit;
    if (len < 2 || len > S.n + 8) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "2 .. n + 8 coefficients");
    (void)hipSetDevice(c->device);
    c->circuit->prefetch_stage = 0;
    uint32_t z[8], zi[8];
    memcpy(z, z4, 32);
    bool zero = true;
    for (int i = 0; i < 8; ++i) zero = zero && z[i] == 0;
    if (zero) return set_err(c, ZKT_ERR_ZERO_DENOMINATOR, "evaluation point is zero");
    if (c->curve == ZKT_CURVE_BN254) memcpy(zi, fe_inv_host<Bn254Fr>(HostF<Bn254Fr>::from_words(z4)).v, 32);
    else memcpy(zi, fe_inv_host<Bls381Fr>(HostF<Bls381Fr>::from_words(z4)).v, 32);
    ZKT_HIP(c, hipMemcpyAsync(S.sc[0], coeffs, len * 32, hipMemcpyHostToDevice, c->stream));
    int rc = open_witness(c, S.sc[0], len, z, zi, S.sc[1], S.sc[2], S.scan_tmp, S.sc[3], S.eval_pw);
    if (rc) return rc;
    ZKT_HIP(c, hipMemcpyAsync(out, S.sc[3], (len - 1) * 32, hipMemcpyDeviceToHost, c->stream));
    ZKT_HIP(c, hipStreamSynchronize(c->stream));
    return ZKT_OK;
}

// Test hook: round 1 of the prover (gather, transforms, the three wire commitments, their collection) on a variable map
// and index vectors that need satisfy nothing.
extern "C++" template <class C>
static int debug_commit_wires_t(zkt_ctx* c, const zkt_prove_inputs& in, int route, uint64_t* out_xy, int* out_inf, int* out_route) {
    using Q = typename C::Fq;
    CircuitState& S = *c->circuit;
    BuiltinTranscript tr(0, "zkt_debug_commit_wires_dev");
    Prover<C> p(c, S, tr);
    S.wire_dense_only = route == 0;
    S.wire_elim_force = route == 2 ? 1 : 0;
    int rc = p.enqueue_round_1(in);
    S.wire_dense_only = false;
    S.wire_elim_force = -1;
    Affine<Q> cm[3];
    static const int slots[3] = {0, 1, 2};
    int took[3] = {0, 0, 0};
    if (!rc) rc = p.commit_collect(slots, nullptr, 3, cm);
    if (!rc) rc = p.collect_wires(cm, took);
    p.wait_end();
    if (!rc) rc = p.check_status();   // synchronises; an index outside the variable map
    if (rc) {
        for (bool& r : S.wire_route) r = false;
        (void)hipStreamSynchronize(c->stream);
        return rc;
    }
    for (int k = 0; k < 3; ++k) {
        memcpy(out_xy + (size_t)k * Q::N, cm[k].x.v, Q::N * 4);
        memcpy(out_xy + (size_t)k * Q::N + Q::N / 2, cm[k].y.v, Q::N * 4);
        if (out_inf) out_inf[k] = aff_is_inf<Q>(cm[k]) ? 1 : 0;
        if (out_route) out_route[k] = took[k];
    }
    return ZKT_OK;
}

int zkt_debug_commit_wires_dev(zkt_ctx* c, const void* d_variables, size_t n_vars, const uint32_t* d_w_l, const uint32_t* d_w_r,
                               const uint32_t* d_w_o, size_t n_rows, const uint64_t* blinders, int route, uint64_t* out_xy,
                               int* out_is_infinity, int* out_route) {
    if (route != 0 && route != 1) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "route: 0 coefficients, 1 wire base tables");
    return zkt_debug_commit_wires_pi_dev(c, d_variables, n_vars, d_w_l, d_w_r, d_w_o, n_rows, blinders, route, nullptr, 0, out_xy,
                                         out_is_infinity, out_route);
}

int zkt_debug_commit_wires_pi_dev(zkt_ctx* c, const void* d_variables, size_t n_vars, const uint32_t* d_w_l, const uint32_t* d_w_r,
                                  const uint32_t* d_w_o, size_t n_rows, const uint64_t* blinders, int route, const size_t* pi_pos,
                                  size_t n_pi, uint64_t* out_xy, int* out_is_infinity, int* out_route) {
    if (!c || !d_variables || !blinders || !out_xy || (n_pi && !pi_pos)) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (route < 0 || route > 2)
        return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "route: 0 coefficients, 1 wire base tables, 2 tables over free variables");
    if (!c->circuit) return set_err(c, ZKT_ERR_NOT_LOADED, "no circuit loaded (the domain comes from it)");
    if (!c->msm) return set_err(c, ZKT_ERR_NOT_LOADED, "no SRS loaded (zkt_srs_load)");
    if (c->sharded()) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "not available on a sharded key");
    CircuitState& S = *c->circuit;
    if (S.has_next) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "zkt_debug_commit_wires_dev: a next proof is announced");
    (void)hipSetDevice(c->device);
    S.prefetch_stage = 0;   // the work buffers are shared with an announced proof's early rounds
    if (route >= 1 && !c->lagrange_off)
        if (int rc1 = lagrange_ensure(c, S.log_n)) return rc1;
    uint64_t bl[19 * 4] = {};
    memcpy(bl, blinders, 6 * 32);
    zkt_prove_inputs in{};
    in.variables = (const uint64_t*)d_variables;
    in.n_vars = n_vars;
    in.w_l = d_w_l; in.w_r = d_w_r; in.w_o = d_w_o;
    in.n_rows = n_rows;
    in.wires_on_device = 1;
    in.blinders = bl;
    in.pi_pos = pi_pos;
    in.n_pi = n_pi;
    if (c->curve == ZKT_CURVE_BN254) return debug_commit_wires_t<Bn254Curve>(c, in, route, out_xy, out_is_infinity, out_route);
    return debug_commit_wires_t<Bls381Curve>(c, in, route, out_xy, out_is_infinity, out_route);
}

int zkt_prove_set_next(zkt_ctx* c, const zkt_prove_inputs* next) {
    if (!c) return ZKT_ERR_INVALID_ARGUMENT;
    if (!c->circuit) return set_err(c, ZKT_ERR_NOT_LOADED, "no circuit loaded (zkt_circuit_load)");
    c->circuit->has_next = next != nullptr;
    if (next) c->circuit->next_in = *next;
    return ZKT_OK;
}

int zkt_prove(zkt_ctx* c, const zkt_prove_inputs* in, zkt_transcript* tr, uint8_t* proof_out, size_t proof_cap,
              size_t* proof_len) {
    if (!c || !in || !tr || !proof_out) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    return prove_impl(c, in, *tr->impl, proof_out, proof_cap, proof_len);
}

int zkt_prove_with(zkt_ctx* c, const zkt_prove_inputs* in, const zkt_transcript_vtable* vt, uint8_t* proof_out,
                   size_t proof_cap, size_t* proof_len) {
    if (!c || !in || !vt || !proof_out) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (c->curve == ZKT_CURVE_BN254) {
        VtableAdapter<Bn254Curve> a(vt);
        return prove_impl(c, in, a, proof_out, proof_cap, proof_len);
    }
    VtableAdapter<Bls381Curve> a(vt);
    return prove_impl(c, in, a, proof_out, proof_cap, proof_len);
}

}  // extern "C"
