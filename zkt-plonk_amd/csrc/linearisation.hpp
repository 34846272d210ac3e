// Arithmetic of the verifier's identity at xi (proof.rs:163-282, linearization_poly.rs:19-121, util.rs:185-195):
// zh(xi), L_1(xi), the thirteen scalars of the linearisation and compute_r0.  The prover puts the scalars against its
// polynomials (round 5) and, on the quotient's classes route, checks r(xi) against r0; the verifier -- on the host and in
// the kernel of verify_terms.hip -- puts them against its commitments and folds r0 into the first opening.  One
// implementation, so they cannot drift apart; what differs is the inversion, which the caller names: the host's
// fe_inv_host, the kernels' fe_inv_call (an inverse is one value, whoever computes it).
#pragma once
#include "ctx.hpp"
#include "hostinv.hpp"

namespace zkt {

// the twelve evaluations, in ProofEvaluations order (the proof's wire order), and their transcript labels
enum { EV_A = 0, EV_B, EV_C, EV_S1, EV_S2, EV_Z1N, EV_QL, EV_T, EV_TN, EV_Z2N, EV_H1N, EV_H2, EV_COUNT };
ZKT_HD const char* ev_label(int k) {
    switch (k) {
        case EV_A: return "a_eval";
        case EV_B: return "b_eval";
        case EV_C: return "c_eval";
        case EV_S1: return "sigma1_eval";
        case EV_S2: return "sigma2_eval";
        case EV_Z1N: return "z1_next_eval";
        case EV_QL: return "q_lookup_eval";
        case EV_T: return "t_eval";
        case EV_TN: return "t_next_eval";
        case EV_Z2N: return "z2_next_eval";
        case EV_H1N: return "h1_next_eval";
        default: return "h2_eval";
    }
}
// the thirteen terms of the linearisation, in the order of commitment.rs:32-45
enum { LIN_QM = 0, LIN_QL, LIN_QR, LIN_QO, LIN_QC, LIN_Z1, LIN_S3, LIN_Z2, LIN_H1, LIN_QTABLE, LIN_QLO, LIN_QMID, LIN_QHI, LIN_COUNT };

template <class R> struct Challenges { Fe<R> beta, gamma, delta, epsilon, alpha, xi, eta; };
template <class R> struct XiPoint {
    Fe<R> zh, nn, l1;           // zh(xi) = xi^n - 1, n as a field element, L_1(xi)
    Fe<R> a2, a3, a4, a5, eopd;   // powers of alpha, epsilon (1 + delta)
};

// fe_inv (fp.hpp) as one function that device code calls, not a copy at every use
template <class R>
__host__ __device__ __attribute__((noinline)) Fe<R> fe_inv_call(const Fe<R>& a) { return fe_inv<R>(a); }

// false: n (xi - 1) = 0, L_1(xi) has no denominator and is left alone (the other members are set)
template <class R, Fe<R> (*INV)(const Fe<R>&)>
ZKT_HD bool xi_point(const Challenges<R>& ch, uint64_t n, XiPoint<R>& at) {
    const Fe<R> one = fe_one<R>();
    at.zh = fe_sub<R>(fe_pow_u64<R>(ch.xi, n), one);
    at.nn = fe_from_u64<R>(n);
    at.a2 = fe_sqr<R>(ch.alpha); at.a3 = fe_mul<R>(at.a2, ch.alpha);
    at.a4 = fe_mul<R>(at.a3, ch.alpha); at.a5 = fe_mul<R>(at.a4, ch.alpha);
    at.eopd = fe_mul<R>(ch.epsilon, fe_add<R>(ch.delta, one));
    const Fe<R> l1den = fe_mul<R>(at.nn, fe_sub<R>(ch.xi, one));
    if (fe_is_zero<R>(l1den)) return false;
    at.l1 = fe_mul<R>(at.zh, INV(l1den));
    return true;
}

template <class R> ZKT_HD void linearisation_scalars(const Challenges<R>& ch, const XiPoint<R>& at, const Fe<R>* ev, Fe<R> sc[LIN_COUNT]) {
    typedef Fe<R> F;
    const F &alpha = ch.alpha, &beta = ch.beta, &gamma = ch.gamma, &delta = ch.delta, &epsilon = ch.epsilon, &xi = ch.xi;
    const F one = fe_one<R>(), k1 = fe_from_u32<R>(7), k2 = fe_from_u32<R>(13);
    const F bxi = fe_mul<R>(beta, xi);
    sc[LIN_QM] = fe_mul<R>(ev[EV_A], ev[EV_B]);   // keys/arithmetic.rs:37-46
    sc[LIN_QL] = ev[EV_A]; sc[LIN_QR] = ev[EV_B]; sc[LIN_QO] = ev[EV_C]; sc[LIN_QC] = one;
    // keys/permutation.rs:34-69
    F s_z1 = fe_mul<R>(alpha, fe_add<R>(fe_add<R>(bxi, ev[EV_A]), gamma));
    s_z1 = fe_mul<R>(s_z1, fe_add<R>(fe_add<R>(fe_mul<R>(bxi, k1), ev[EV_B]), gamma));
    s_z1 = fe_mul<R>(s_z1, fe_add<R>(fe_add<R>(fe_mul<R>(bxi, k2), ev[EV_C]), gamma));
    sc[LIN_Z1] = fe_add<R>(s_z1, fe_mul<R>(at.l1, at.a2));
    F s_s3 = fe_mul<R>(fe_mul<R>(fe_neg<R>(alpha), beta), ev[EV_Z1N]);
    s_s3 = fe_mul<R>(s_s3, fe_add<R>(fe_add<R>(fe_mul<R>(beta, ev[EV_S1]), ev[EV_A]), gamma));
    sc[LIN_S3] = fe_mul<R>(s_s3, fe_add<R>(fe_add<R>(fe_mul<R>(beta, ev[EV_S2]), ev[EV_B]), gamma));
    // keys/lookup.rs:29-65
    F s_z2 = fe_mul<R>(fe_mul<R>(at.a3, fe_add<R>(delta, one)), fe_add<R>(epsilon, fe_mul<R>(ev[EV_QL], ev[EV_C])));
    s_z2 = fe_mul<R>(s_z2, fe_add<R>(fe_add<R>(at.eopd, ev[EV_T]), fe_mul<R>(delta, ev[EV_TN])));
    sc[LIN_Z2] = fe_add<R>(s_z2, fe_mul<R>(at.a4, at.l1));
    sc[LIN_H1] = fe_mul<R>(fe_mul<R>(fe_neg<R>(at.a3), ev[EV_Z2N]),
                           fe_add<R>(fe_add<R>(at.eopd, ev[EV_H2]), fe_mul<R>(delta, ev[EV_H1N])));
    sc[LIN_QTABLE] = fe_mul<R>(at.a5, ev[EV_T]);
    // linearization_poly.rs:100-109: -zh * (q_lo + xi^(n+2) q_mid + xi^(2n+4) q_hi)
    const F xn2 = fe_mul<R>(fe_mul<R>(fe_add<R>(at.zh, one), xi), xi), nzh = fe_neg<R>(at.zh);
    sc[LIN_QLO] = nzh;
    sc[LIN_QMID] = fe_mul<R>(nzh, xn2);
    sc[LIN_QHI] = fe_mul<R>(nzh, fe_sqr<R>(xn2));
}

// compute_r0 (proof.rs:163-217) over k public inputs `vals` at the domain points `roots` (Montgomery form):
// L_j(xi) = zh root_j / (n (xi - root_j)), all denominators inverted at once; a root equal to xi has L_j = 1 (and zh = 0
// silences the others).  No allocation: before[] (k elements, the caller's) keeps the running products of the non-zero
// denominators, and a denominator is formed again on the way back.  Returns whether any denominator was zero: the
// verifier refuses such a proof, the prover goes on.
template <class R, Fe<R> (*INV)(const Fe<R>&)>
ZKT_HD bool compute_r0(const Challenges<R>& ch, const XiPoint<R>& at, const Fe<R>* ev, const Fe<R>* roots, const Fe<R>* vals,
                       uint64_t k, Fe<R>* before, Fe<R>* out) {
    typedef Fe<R> F;
    F r0 = fe_zero<R>();
    bool zero_den = false;
    F run_prod = fe_one<R>();
#pragma nounroll
    for (uint64_t i = 0; i < k; ++i) {
        const F den = fe_mul<R>(at.nn, fe_sub<R>(ch.xi, roots[i]));
        before[i] = run_prod;
        if (!fe_is_zero<R>(den)) run_prod = fe_mul<R>(run_prod, den);
    }
    F inv_all = k ? INV(run_prod) : run_prod;
#pragma nounroll
    for (uint64_t i = k; i-- > 0;) {
        const F root = roots[i], val = vals[i];
        const F den = fe_mul<R>(at.nn, fe_sub<R>(ch.xi, root));
        if (fe_is_zero<R>(den)) {
            zero_den = true;
            r0 = fe_sub<R>(r0, val);
            continue;
        }
        const F di = fe_mul<R>(inv_all, before[i]);
        inv_all = fe_mul<R>(inv_all, den);
        r0 = fe_sub<R>(r0, fe_mul<R>(fe_mul<R>(fe_mul<R>(at.zh, root), di), val));
    }
    const F &beta = ch.beta, &gamma = ch.gamma, &delta = ch.delta;
    F p2 = fe_mul<R>(ch.alpha, ev[EV_Z1N]);
    p2 = fe_mul<R>(p2, fe_add<R>(fe_add<R>(ev[EV_A], fe_mul<R>(beta, ev[EV_S1])), gamma));
    p2 = fe_mul<R>(p2, fe_add<R>(fe_add<R>(ev[EV_B], fe_mul<R>(beta, ev[EV_S2])), gamma));
    p2 = fe_mul<R>(p2, fe_add<R>(ev[EV_C], gamma));
    F p4 = fe_mul<R>(at.a3, ev[EV_Z2N]);
    p4 = fe_mul<R>(p4, fe_add<R>(at.eopd, fe_mul<R>(delta, ev[EV_H2])));
    p4 = fe_mul<R>(p4, fe_add<R>(fe_add<R>(at.eopd, ev[EV_H2]), fe_mul<R>(delta, ev[EV_H1N])));
    *out = fe_add<R>(fe_add<R>(r0, p2), fe_add<R>(fe_mul<R>(at.l1, at.a2), fe_add<R>(p4, fe_mul<R>(at.l1, at.a4))));
    return zero_den;
}

}  // namespace zkt
