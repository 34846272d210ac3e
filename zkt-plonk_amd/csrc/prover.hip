// Device-resident PLONK+Plookup prover: host orchestration of the five rounds of
// plonk-core/src/proof_system/prove.rs:59-470.  Witness vectors are uploaded once; every
// polynomial stays in HBM between rounds; only commitments (affine points), the 12 evaluations and
// two scalars (the grand-product denominators) cross PCIe, for the host-side Fiat-Shamir transcript.
// The circuit's state and life cycle are circuit.hpp / circuit.hip; this unit holds Prover<C>, the entries that prove and
// the test hooks that run single rounds of it.
#include "circuit.hpp"
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include "linearisation.hpp"
#include "msm.hpp"
#include "transcript.hpp"

#include <algorithm>
#include <functional>
#include <cstring>
#include <memory>
#include <optional>
#include <vector>

namespace zkt {

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

extern "C" {

static int prove_impl(zkt_ctx* c, const zkt_prove_inputs* in, HostTranscript& tr, uint8_t* out, size_t cap, size_t* len) {
    if (int rc0 = circuit_entry(c, ENTRY_SRS)) return rc0;
    if (int rc0 = check_sharded_key(c)) return rc0;
    (void)hipSetDevice(c->device);
    // the Lagrange-basis table of this domain (lagrange.hip): built on the first proof after a key or circuit change
    if (!c->lagrange_off)
        if (int rc1 = lagrange_ensure(c, c->circuit->log_n)) return rc1;
    std::vector<uint8_t> proof;
    const int rc = by_curve(c->curve, [&](auto C) { return run_prover<decltype(C)>(c, *in, tr, proof); });
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

int zkt_debug_grand_products(zkt_ctx* c, const uint64_t* challenges, const uint64_t* const* vectors, uint64_t* out_z1,
                             uint64_t* out_z2) {
    if (!c || !challenges || !vectors || !out_z1 || !out_z2) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    for (int k = 0; k < 7; ++k)
        if (!vectors[k]) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null vector");
    if (int rc = circuit_entry(c, ENTRY_DEVICE | ENTRY_WITHDRAW)) return rc;
    // the caller's t replaces the evaluations of the cached table polynomial: the next proof rebuilds it
    c->circuit->t_cached = false;
    return by_curve(c->curve, [&](auto C) { return debug_grand_products_t<decltype(C)>(c, challenges, vectors, out_z1, out_z2); });
}

int zkt_debug_combine_split(zkt_ctx* c, const uint64_t* table, size_t table_len, const uint64_t* f, int fresh,
                            uint64_t* h1_out, uint64_t* h2_out) {
    if (!c || !f || !h1_out || !h2_out || (table_len && !table)) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (int rc = circuit_entry(c, ENTRY_NO_NEXT | ENTRY_DEVICE | ENTRY_WITHDRAW, "zkt_debug_combine_split")) return rc;
    CircuitState& S = *c->circuit;
    if (table_len >= S.n) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "max table size is equal or larger than n");
    // the keys this call leaves resident need not be those of the cached table polynomial: the next proof rebuilds both
    S.t_cached = false;
    return by_curve(c->curve, [&](auto C) { return debug_combine_split_t<decltype(C)>(c, table, table_len, f, fresh != 0, h1_out, h2_out); });
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
    if (int rc0 = circuit_entry(c, ENTRY_DOMAIN | ENTRY_SRS | ENTRY_WHOLE_KEY | ENTRY_NO_NEXT | ENTRY_DEVICE | ENTRY_WITHDRAW, "zkt_debug_commit_wires_dev"))
        return rc0;
    CircuitState& S = *c->circuit;
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
    return by_curve(c->curve, [&](auto C) { return debug_commit_wires_t<decltype(C)>(c, in, route, out_xy, out_is_infinity, out_route); });
}

int zkt_prove_set_next(zkt_ctx* c, const zkt_prove_inputs* next) {
    if (!c) return ZKT_ERR_INVALID_ARGUMENT;
    if (int rc = circuit_entry(c, 0)) return rc;
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
    return by_curve(c->curve, [&](auto C) {
        VtableAdapter<decltype(C)> a(vt);
        return prove_impl(c, in, a, proof_out, proof_cap, proof_len);
    });
}

}  // extern "C"
