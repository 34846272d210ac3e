// Elimination of the circuit's linear rows (host; lagrange.hip "wire tables over free variables").
//
// Row i asserts  q_m a b + q_l a + q_r b + q_o c + q_c + PI_i = 0  with a = x[w_l[i]], b = x[w_r[i]], c = x[w_o[i]].  Walking the
// rows in ascending order, row i DEFINES v = w_o[i] when q_m[i] = 0, q_o[i] is 1 or -1, i is no public-input position, v is a
// real variable (not Variable::Zero, inside the map) and v stands on no wire of an earlier row nor on an input wire of this
// one.  A variable first seen anywhere else is FREE.  A defined v is an affine form of free variables,
//     x_v = kappa_v + sum_f M[v][f] x_f,
// obtained by substituting the forms of the row's two inputs (Variable::Zero contributes nothing).  A form with more than
// K non-zero terms is not kept: its variable is declared free instead, which bounds the work and the memory.
// Every witness that satisfies the defining rows satisfies these identities; nothing else is assumed.
#pragma once
#include "fp.hpp"

#include <cstddef>
#include <cstdint>
#include <vector>

namespace zkt {

constexpr int WIRE_ELIM_K = 16;        // the prover's support cap
constexpr int WIRE_ELIM_K_MAX = 64;

template <class R>
struct WireElim {
    using F = Fe<R>;
    std::vector<uint8_t> kind;          // per variable: 0 on no wire, 1 free, 2 defined
    std::vector<uint32_t> free_vars;    // in the order of their first appearance
    std::vector<uint32_t> def_vars;     // in the order of their defining rows
    std::vector<uint32_t> def_id;       // per variable: its index in def_vars (defined variables only)
    std::vector<uint64_t> def_start;    // def_vars.size() + 1: the terms of a defined variable, ascending free variable
    std::vector<uint32_t> term_f;       // the free variable of a term
    std::vector<F> term_c;              // its coefficient (Montgomery form, never zero)
    std::vector<F> kappa;               // per defined variable (Montgomery form)
};

// sel[0..4] = q_m q_l q_r q_o q_c, at least n_rows evaluations each (Montgomery form); w[0..2] = w_l w_r w_o, n_rows indices
// each (0xFFFFFFFF = Variable::Zero; an index >= n_vars is read as Variable::Zero: the prover refuses such a witness anyway)
template <class R>
void wire_eliminate(const Fe<R>* const* sel, const uint32_t* const* w, size_t n_rows, size_t n_vars, const size_t* pi_pos, size_t n_pi,
                    int K, WireElim<R>& E) {
    using F = Fe<R>;
    E = WireElim<R>{};
    E.kind.assign(n_vars, 0);
    E.def_id.assign(n_vars, 0);
    E.def_start.push_back(0);
    std::vector<bool> is_pi(n_rows, false);
    for (size_t k = 0; k < n_pi; ++k)
        if (pi_pos[k] < n_rows) is_pi[pi_pos[k]] = true;
    const F one = fe_one<R>(), minus_one = fe_neg<R>(fe_one<R>());
    auto touch = [&](uint32_t v) {
        if (v < n_vars && E.kind[v] == 0) {
            E.kind[v] = 1;
            E.free_vars.push_back(v);
        }
    };
    // the two inputs' scaled forms, each ascending in the free variable
    uint32_t fa[WIRE_ELIM_K_MAX], fb[WIRE_ELIM_K_MAX], fo[2 * WIRE_ELIM_K_MAX];
    F ca[WIRE_ELIM_K_MAX], cb[WIRE_ELIM_K_MAX], co[2 * WIRE_ELIM_K_MAX];
    for (size_t i = 0; i < n_rows; ++i) {
        const uint32_t a = w[0][i], b = w[1][i], o = w[2][i];
        const F qo = sel[3][i];
        const bool plus = fe_eq<R>(qo, one);
        const bool cand = o < n_vars && E.kind[o] == 0 && o != a && o != b && !is_pi[i] && fe_is_zero<R>(sel[0][i]) &&
                          (plus || fe_eq<R>(qo, minus_one));
        touch(a);
        touch(b);
        if (!cand) {
            touch(o);
            continue;
        }
        // c = -(q_l a + q_r b + q_c) / q_o
        F kap = plus ? fe_neg<R>(sel[4][i]) : sel[4][i];
        auto scaled = [&](uint32_t v, const F& q, uint32_t* f, F* cf) -> int {
            if (v >= n_vars || fe_is_zero<R>(q)) return 0;
            const F s = plus ? fe_neg<R>(q) : q;
            if (E.kind[v] == 1) {
                f[0] = v;
                cf[0] = s;
                return 1;
            }
            const uint32_t d = E.def_id[v];
            int m = 0;
            for (uint64_t t = E.def_start[d]; t < E.def_start[d + 1]; ++t, ++m) {
                f[m] = E.term_f[t];
                cf[m] = fe_mul<R>(s, E.term_c[t]);
            }
            kap = fe_add<R>(kap, fe_mul<R>(s, E.kappa[d]));
            return m;
        };
        const int na = scaled(a, sel[1][i], fa, ca), nb = scaled(b, sel[2][i], fb, cb);
        int ia = 0, ib = 0, no = 0;
        while (ia < na || ib < nb) {
            if (ib == nb || (ia < na && fa[ia] < fb[ib])) {
                fo[no] = fa[ia]; co[no++] = ca[ia++];
            } else if (ia == na || fb[ib] < fa[ia]) {
                fo[no] = fb[ib]; co[no++] = cb[ib++];
            } else {
                const F s = fe_add<R>(ca[ia], cb[ib]);
                if (!fe_is_zero<R>(s)) { fo[no] = fa[ia]; co[no++] = s; }
                ++ia; ++ib;
            }
        }
        if (no > K) {
            touch(o);
            continue;
        }
        E.kind[o] = 2;
        E.def_id[o] = (uint32_t)E.def_vars.size();
        E.def_vars.push_back(o);
        E.term_f.insert(E.term_f.end(), fo, fo + no);
        E.term_c.insert(E.term_c.end(), co, co + no);
        E.def_start.push_back(E.term_f.size());
        E.kappa.push_back(kap);
    }
}

}  // namespace zkt
