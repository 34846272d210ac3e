// The per-proof stage of the verifier between the decompression and the group arithmetic (verify.hip step 2; stage 2 and
// the per-proof half of stage 4 of the batch verifier): the Fiat-Shamir replay of proof.rs:308-360, xi_point, compute_r0,
// the 13 linearisation scalars and both fold lists -- ONE template, verifier_replay, over a transcript and a sink:
//   transcripts  VtCoreTr, the core's state itself (the kernel of verify_terms.hip, one lane per proof, and its host
//                rehearsal, zkt_debug_verify_terms_host route 1); VtHostTr over a HostTranscript&, whatever is behind it
//                (the single-proof verifier, the batch verifier's host route, a caller's callback table)
//   sinks        VtSums adds rho[o] * scalar into the 24 sums by source (the kernel, the batch verifier); verify.hip's
//                term lists keep every (opening, source, scalar) for the two short MSMs of one proof
// Per-proof vectors (evaluations, public inputs, the sums) stay in the caller's memory and are indexed there.
#pragma once
#include "ctx.hpp"
#include "ec.hpp"
#include "linearisation.hpp"
#include "transcript.hpp"

namespace zkt {

constexpr int VT_THREADS = 64;

// the proof's 13 commitments in wire order, the ten verifier-key commitments in theirs
enum { CM_A, CM_B, CM_C, CM_T, CM_H1, CM_H2, CM_Z1, CM_Z2, CM_QLO, CM_QMID, CM_QHI, CM_AW, CM_SAW, CM_COUNT };
enum { VK_QM, VK_QL, VK_QR, VK_QO, VK_QC, VK_S1, VK_S2, VK_S3, VK_QLOOKUP, VK_QTABLE, VK_COUNT };
// Where a term's point comes from: the proof's commitments, the verifier-key commitments, g.  Z1, Z2, T, H1, g and the
// verifier-key points occur in both openings; a consumer that adds the two lists up is left with at most SRC_COUNT bases
// per proof.  Opening o is checked against the witness SRC_CM + CM_AW + o.
enum { SRC_CM = 0, SRC_VK = CM_COUNT, SRC_G = SRC_VK + VK_COUNT, SRC_COUNT };
static_assert(SRC_VK == 13 && SRC_G == 23 && SRC_COUNT == 24, "VtLayout and verify_leaves.hpp count 24 sources");

// ---- the replay's transcript over the core's state ----------------------------------------------------------------
template <class Q>
__host__ __device__ __attribute__((noinline)) void vt_commit(VtTr& t, const char* label, const Affine<Q>* point) {
    const Affine<Q> a = *point;
    const bool inf = aff_is_inf<Q>(a);
    Fe<Q> x = fe_zero<Q>(), y = fe_zero<Q>();
    if (inf) {
        y.v[0] = 1;
    } else {
        x = fe_from_mont<Q>(a.x);
        y = fe_from_mont<Q>(a.y);
    }
    vt_msg_put<Q>(t, 0, x);
    vt_msg_put<Q>(t, Q::N / 2, y);
    t.s.msg[Q::N * t.s.stride] = inf ? 1 : 0;
    vt_tr_commit_msg(t, label, Q::N * 4);
}
template <class R>
__host__ __device__ __attribute__((noinline)) Fe<R> vt_challenge(VtTr& t, const char* label) {
    uint32_t w[8];
    vt_tr_challenge(t, label, R::BITS, w);
    Fe<R> c;
#pragma unroll
    for (int i = 0; i < 8; ++i) c.v[i] = w[i];
    return fe_to_mont<R>(c);
}
template <class C>
struct VtCoreTr {
    using R = typename C::Fr;
    using Q = typename C::Fq;
    VtTr& t;
    // `count` Montgomery scalars under one label (single: the caller's append_scalar, not append_scalars; one encoding here)
    ZKT_HD void scalars(const char* label, const Fe<R>* mont, uint64_t count, bool) {
        vt_tr_scalars_begin(t, label, count);
#pragma nounroll
        for (uint64_t i = 0; i < count; ++i) {
            vt_msg_put<R>(t, 0, fe_from_mont<R>(mont[i]));
            vt_tr_scalars_item(t);
        }
    }
    ZKT_HD void commit(const char* label, const Affine<Q>* point) { vt_commit<Q>(t, label, point); }
    ZKT_HD Fe<R> challenge(const char* label) { return vt_challenge<R>(t, label); }
    ZKT_HD static Fe<R> inv(const Fe<R>& a) { return fe_inv_call<R>(a); }
};

// One proof.  Everything behind a pointer is the caller's memory (global memory in the kernel).
template <class C>
struct VtProof {
    using R = typename C::Fr;
    using Q = typename C::Fq;
    uint64_t n, n_pi;
    Fe<R> w;                    // the generator of the domain of n points, Montgomery
    Fe<R> rho[2];               // the proof's two coefficients, Montgomery (VtSums)
    const Affine<Q>* cm;        // 13 decompressed commitments, wire order
    const Fe<R>* ev;            // 12 evaluations, Montgomery
    const Fe<R>*roots, *vals;   // n_pi each, Montgomery
    const Fe<R>* forced;        // NULL, or 7 values that replace the drawn beta gamma delta epsilon alpha xi eta
    Fe<R>* before;              // n_pi elements of scratch
    Fe<R>* acc;                 // out: 24 sums by source, all zero on a refusal (VtSums)
    Fe<R>* dbg;                 // NULL, or out: the challenges as far as they were drawn, then r0; the rest zero
};

// the sink that adds both openings' terms, each times its rho, up by source
template <class C>
struct VtSums {
    using R = typename C::Fr;
    const VtProof<C>& p;
    ZKT_HD void term(int o, int src, const Fe<R>& s) { p.acc[src] = fe_add<R>(p.acc[src], fe_mul<R>(p.rho[o], s)); }
};

// The transcript of proof.rs:308-360, r0, and every term (opening, source, scalar) of the two openings
//     L_o = sum_i eta^i C_i - (sum_i eta^i v_i) g + z W_o
// in order (the linearisation commitment, C_0 of the first opening, enters through its own 13 terms; the witness comes
// last).  No group arithmetic.  Returns ZKT_OK, ZKT_ERR_EQUAL_CHALLENGES or ZKT_ERR_ZERO_DENOMINATOR; a refused proof
// has given the sink nothing, and its transcript stops where the refusal was seen.
template <class C, class Tr, class Sink>
ZKT_HD int verifier_replay(Tr& t, const VtProof<C>& p, Sink& sink) {
    using R = typename C::Fr;
    using F = Fe<R>;
    if (p.dbg) {
#pragma nounroll
        for (int s = 0; s < 8; ++s) p.dbg[s] = fe_zero<R>();
    }
    auto draw = [&](const char* label, int idx) {
        F c = t.challenge(label);
        if (p.forced) c = p.forced[idx];
        if (p.dbg) p.dbg[idx] = c;
        return c;
    };
    // ---- transcript (proof.rs:308-360); "pi" is ONE message ----
    t.scalars("pi", p.vals, p.n_pi, false);
    t.commit("a_commit", p.cm + CM_A); t.commit("b_commit", p.cm + CM_B); t.commit("c_commit", p.cm + CM_C);
    t.commit("t_commit", p.cm + CM_T); t.commit("h1_commit", p.cm + CM_H1); t.commit("h2_commit", p.cm + CM_H2);
    const F beta = draw("beta", 0), gamma = draw("gamma", 1), delta = draw("delta", 2), epsilon = draw("epsilon", 3);
    if (fe_eq<R>(beta, gamma) || fe_eq<R>(beta, delta) || fe_eq<R>(beta, epsilon) || fe_eq<R>(gamma, delta) ||
        fe_eq<R>(gamma, epsilon) || fe_eq<R>(delta, epsilon))
        return ZKT_ERR_EQUAL_CHALLENGES;
    t.commit("z1_commit", p.cm + CM_Z1); t.commit("z2_commit", p.cm + CM_Z2);
    const F alpha = draw("alpha", 4);
    t.commit("q_lo_commit", p.cm + CM_QLO); t.commit("q_mid_commit", p.cm + CM_QMID); t.commit("q_hi_commit", p.cm + CM_QHI);
    const F xi = draw("xi", 5);
    // ---- scalars (linearisation.hpp); both refusals come before the evaluations are appended ----
    const Challenges<R> ch{beta, gamma, delta, epsilon, alpha, xi, fe_zero<R>()};
    XiPoint<R> at;
    if (!xi_point<R, Tr::inv>(ch, p.n, at)) return ZKT_ERR_ZERO_DENOMINATOR;
    F r0;
    if (compute_r0<R, Tr::inv>(ch, at, p.ev, p.roots, p.vals, p.n_pi, p.before, &r0)) return ZKT_ERR_ZERO_DENOMINATOR;
    F ev[EV_COUNT];
#pragma unroll
    for (int k = 0; k < EV_COUNT; ++k) ev[k] = p.ev[k];
    F sc[LIN_COUNT];
    linearisation_scalars<R>(ch, at, ev, sc);
#pragma nounroll
    for (int k = 0; k < EV_COUNT; ++k) t.scalars(ev_label(k), p.ev + k, 1, true);
    const F eta = draw("eta", 6);
    if (p.dbg) p.dbg[7] = r0;
    // ---- the two openings (proof.rs:420-500; the 13-point combination of commitment.rs:32-45) ----
    {
        constexpr int pt[13] = {SRC_VK + VK_QM, SRC_VK + VK_QL, SRC_VK + VK_QR, SRC_VK + VK_QO, SRC_VK + VK_QC, SRC_CM + CM_Z1,
                                SRC_VK + VK_S3, SRC_CM + CM_Z2, SRC_CM + CM_H1, SRC_VK + VK_QTABLE, SRC_CM + CM_QLO,
                                SRC_CM + CM_QMID, SRC_CM + CM_QHI};
#pragma unroll
        for (int k = 0; k < 13; ++k) sink.term(0, pt[k], sc[k]);
        constexpr int cs[8] = {SRC_CM + CM_A, SRC_CM + CM_B, SRC_CM + CM_C, SRC_VK + VK_S1, SRC_VK + VK_S2, SRC_VK + VK_QLOOKUP,
                               SRC_CM + CM_T, SRC_CM + CM_H2};
        constexpr int vs[8] = {EV_A, EV_B, EV_C, EV_S1, EV_S2, EV_QL, EV_T, EV_H2};
        F c = eta, comb_v = r0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            sink.term(0, cs[i], c);
            comb_v = fe_add<R>(comb_v, fe_mul<R>(c, ev[vs[i]]));
            c = fe_mul<R>(c, eta);
        }
        sink.term(0, SRC_G, fe_neg<R>(comb_v));
        sink.term(0, SRC_CM + CM_AW, xi);
    }
    {
        constexpr int cs[4] = {SRC_CM + CM_Z1, SRC_CM + CM_Z2, SRC_CM + CM_T, SRC_CM + CM_H1};
        constexpr int vs[4] = {EV_Z1N, EV_Z2N, EV_TN, EV_H1N};
        F c = fe_one<R>(), comb_v = fe_zero<R>();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            sink.term(1, cs[i], c);
            comb_v = fe_add<R>(comb_v, fe_mul<R>(c, ev[vs[i]]));
            c = fe_mul<R>(c, eta);
        }
        sink.term(1, SRC_G, fe_neg<R>(comb_v));
        sink.term(1, SRC_CM + CM_SAW, fe_mul<R>(xi, p.w));
    }
    return ZKT_OK;
}

// the replay into the 24 sums of p.acc, as one function: what a lane of the kernel runs
template <class C, class Tr>
__host__ __device__ __attribute__((noinline)) int vt_terms(Tr t, const VtProof<C>& p) {
#pragma nounroll
    for (int s = 0; s < SRC_COUNT; ++s) p.acc[s] = fe_zero<typename C::Fr>();
    VtSums<C> sums{p};
    return verifier_replay<C>(t, p, sums);
}

// ---- the kernel's memory: one region of verify_scratch, every part a multiple of 256 bytes -------------------------
// what the host writes per proof in front of the packed vectors
template <class R>
struct alignas(16) VtDesc {
    uint64_t n, n_pi, pi_off, reserved;   // pi_off: where the proof's roots / values / scratch start in the packed arrays
    Fe<R> w, rho[2];
};
static_assert(sizeof(VtDesc<Bn254Fr>) == 128 && sizeof(VtDesc<Bls381Fr>) == 128, "vt_layout counts 128 bytes per description");
struct VtLayout {
    // upload: desc .. states (the states included); download: states .. end of acc (or of dbg)
    size_t desc, ev, roots, vals, forced, states, status, acc, dbg, before, end;
};
inline VtLayout vt_layout(size_t start, size_t count, size_t total_pi, bool forced, bool dbg) {
    auto up = [](size_t b) { return (b + 255) / 256 * 256; };
    VtLayout l;
    l.desc = up(start);
    l.ev = l.desc + up(count * 128);
    l.roots = l.ev + up(count * 12 * 32);
    l.vals = l.roots + up(total_pi * 32);
    l.forced = l.vals + up(total_pi * 32);
    l.states = l.forced + up(forced ? count * 7 * 32 : 0);
    l.status = l.states + up(count * sizeof(TranscriptState));
    l.acc = l.status + up(count * 4);
    l.dbg = l.acc + up(count * 24 * 32);
    l.before = l.dbg + up(dbg ? count * 8 * 32 : 0);
    l.end = l.before + up(total_pi * 32);
    return l;
}
// Enqueue on the context's stream, no synchronisation: one lane per proof over the region at d_base laid out by `lay`
// (forced / dbg as the layout was made), d_points the 13 * count decompressed commitments.
int verify_terms_enqueue(zkt_ctx* c, void* d_base, const VtLayout& lay, const void* d_points, size_t count, bool forced, bool dbg);

}  // namespace zkt
