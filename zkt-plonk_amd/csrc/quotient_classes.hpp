// Host arithmetic of the quotient on three classes of the 4n coset (prover.hip "quotient on classes").
//
// The quotient t has 3n + 6 coefficients.  Its values on the classes j = 0, 1, 2 of the coset g <w_4n> (the points
// g w_4n^(j + 4 i), on which X^n = gamma_j = g^n i4^j, i4 = w_4n^n) fix t~ = t mod Z3, where
//   Z3 = (X^n - gamma_0)(X^n - gamma_1)(X^n - gamma_2) = X^3n + gamma_3 X^2n + gamma_3^2 X^n + gamma_3^3,
// and t = t~ + u Z3 with u the six top coefficients of t.  Since t (X^n - 1) = N, those are the coefficients 4n .. 4n + 5
// of the numerator N, and only three of its products reach that far (n >= 8):
//   alpha z1 (a + beta X + gamma)(b + beta k1 X + gamma)(c + beta k2 X + gamma)
//   - alpha z1(wX) (a + beta sigma1 + gamma)(b + beta sigma2 + gamma)(c + beta sigma3 + gamma)
//   alpha^3 (1 + delta) z2 (epsilon + c q_lookup)(epsilon (1 + delta) + t + delta t(wX))
// each a product of four polynomials of degree <= n + 2, so that its coefficients from 4n on need the factors'
// coefficients n - 6 and above only: "windows" of QCW = 14 coefficients, n - 6 .. n + 7, read as stored.
#pragma once
#include "ctx.hpp"
#include "hostinv.hpp"
#include <cstring>

namespace zkt {

constexpr int QCW = 14;   // coefficients n - 6 .. n + 7 of a polynomial kept in n + 8 elements

template <class R>
struct QuotientClassConsts {
    Fe<R> gamma[4];   // X^n on class j
    Fe<R> vinv[9];    // inverse of the Vandermonde matrix (gamma_j^k), j = row, k = column; row-major
    Fe<R> g3[3];      // gamma_3, gamma_3^2, gamma_3^3
};

template <class R>
static QuotientClassConsts<R> quotient_class_consts(int log_n) {
    QuotientClassConsts<R> q;
    const uint64_t n = (uint64_t)1 << log_n;
    const Fe<R> g = fe_from_u32<R>(R::GENERATOR);
    const Fe<R> i4 = fe_pow_u64<R>(root_of_unity<R>(log_n + 2), n);
    q.gamma[0] = fe_pow_u64<R>(g, n);
    for (int j = 1; j < 4; ++j) q.gamma[j] = fe_mul<R>(q.gamma[j - 1], i4);
    // column j of the inverse holds the coefficients of the Lagrange polynomial that is 1 at gamma_j and 0 at the others:
    // (Y - ga)(Y - gb) / ((gj - ga)(gj - gb))
    for (int j = 0; j < 3; ++j) {
        const Fe<R>&gj = q.gamma[j], &ga = q.gamma[(j + 1) % 3], &gb = q.gamma[(j + 2) % 3];
        const Fe<R> d = fe_inv_host<R>(fe_mul<R>(fe_sub<R>(gj, ga), fe_sub<R>(gj, gb)));
        q.vinv[0 + j] = fe_mul<R>(fe_mul<R>(ga, gb), d);
        q.vinv[3 + j] = fe_mul<R>(fe_neg<R>(fe_add<R>(ga, gb)), d);
        q.vinv[6 + j] = d;
    }
    q.g3[0] = q.gamma[3];
    q.g3[1] = fe_sqr<R>(q.gamma[3]);
    q.g3[2] = fe_mul<R>(q.g3[1], q.gamma[3]);
    return q;
}

// Coefficients 4n .. 4n + 5 of the product of four polynomials given by their windows (index i = coefficient n - 6 + i,
// nothing above the window): those of index sum 24 .. 29.  Trailing zeros of a window are skipped.
template <class R>
static void quotient_top_of_product(const Fe<R>* const w[4], Fe<R> out[6]) {
    int len[4];
    for (int k = 0; k < 4; ++k) {
        len[k] = QCW;
        while (len[k] > 0 && fe_is_zero<R>(w[k][len[k] - 1])) --len[k];
    }
    for (int e = 0; e < 6; ++e) out[e] = fe_zero<R>();
    if (!len[0] || !len[1] || !len[2] || !len[3]) return;
    Fe<R> p01[2 * QCW - 1], p23[2 * QCW - 1];
    auto conv = [&](const Fe<R>* x, int lx, const Fe<R>* y, int ly, Fe<R>* o) {
        for (int i = 0; i < lx + ly - 1; ++i) o[i] = fe_zero<R>();
        for (int i = 0; i < lx; ++i)
            for (int j = 0; j < ly; ++j) o[i + j] = fe_add<R>(o[i + j], fe_mul<R>(x[i], y[j]));
    };
    conv(w[0], len[0], w[1], len[1], p01);
    conv(w[2], len[2], w[3], len[3], p23);
    const int l01 = len[0] + len[1] - 1, l23 = len[2] + len[3] - 1;
    for (int e = 0; e < 6; ++e) {
        const int s = 4 * 6 + e;
        for (int i = 0; i < l01; ++i) {
            const int j = s - i;
            if (j >= 0 && j < l23) out[e] = fe_add<R>(out[e], fe_mul<R>(p01[i], p23[j]));
        }
    }
}

struct QuotientWindows {   // QCW elements each
    const uint32_t *a, *b, *c, *z1, *z2, *t, *sigma1, *sigma2, *sigma3, *q_lookup;
};

// u = the coefficients 4n .. 4n + 5 of the quotient's numerator
template <class R>
static void quotient_top_coefficients(int log_n, const QuotientWindows& W, const Fe<R>& alpha, const Fe<R>& beta, const Fe<R>& delta,
                                      Fe<R> u[6]) {
    typedef Fe<R> F;
    auto load = [](const uint32_t* p, F* o) {
        for (int i = 0; i < QCW; ++i)
            for (int k = 0; k < 8; ++k) o[i].v[k] = p[8 * i + k];
    };
    F a[QCW], b[QCW], c[QCW], z1[QCW], z2[QCW], t[QCW], s1[QCW], s2[QCW], s3[QCW], ql[QCW];
    load(W.a, a); load(W.b, b); load(W.c, c); load(W.z1, z1); load(W.z2, z2); load(W.t, t);
    load(W.sigma1, s1); load(W.sigma2, s2); load(W.sigma3, s3); load(W.q_lookup, ql);
    // p(wX): coefficient k times w^k, k = n - 6 + i, w^n = 1
    const F w = root_of_unity<R>(log_n);
    F wk[QCW];
    wk[6] = fe_one<R>();
    const F winv = fe_inv_host<R>(w);
    for (int i = 7; i < QCW; ++i) wk[i] = fe_mul<R>(wk[i - 1], w);
    for (int i = 5; i >= 0; --i) wk[i] = fe_mul<R>(wk[i + 1], winv);
    F z1w[QCW], as[QCW], bs[QCW], cs[QCW], tt[QCW];
    for (int i = 0; i < QCW; ++i) {
        z1w[i] = fe_mul<R>(z1[i], wk[i]);
        as[i] = fe_add<R>(a[i], fe_mul<R>(beta, s1[i]));
        bs[i] = fe_add<R>(b[i], fe_mul<R>(beta, s2[i]));
        cs[i] = fe_add<R>(c[i], fe_mul<R>(beta, s3[i]));
        tt[i] = fe_add<R>(t[i], fe_mul<R>(delta, fe_mul<R>(t[i], wk[i])));
    }
    F p1[6], p2[6], p3[6];
    {
        const F* f[4] = {z1, a, b, c};
        quotient_top_of_product<R>(f, p1);
    }
    {
        const F* f[4] = {z1w, as, bs, cs};
        quotient_top_of_product<R>(f, p2);
    }
    {
        const F* f[4] = {z2, c, ql, tt};
        quotient_top_of_product<R>(f, p3);
    }
    const F a3 = fe_mul<R>(fe_sqr<R>(alpha), alpha);
    const F k3 = fe_mul<R>(a3, fe_add<R>(delta, fe_one<R>()));
    for (int e = 0; e < 6; ++e)
        u[e] = fe_add<R>(fe_mul<R>(alpha, fe_sub<R>(p1[e], p2[e])), fe_mul<R>(k3, p3[e]));
}

}  // namespace zkt
