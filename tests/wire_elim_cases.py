"""Shared by tests/test_wire_elimination_host.py and tests/test_gpu_wire_elimination.py: the host pass behind the wire tables
over free variables (zkt_debug_wire_elimination, csrc/wire_elim.hpp) run on an oracle ConstraintSystem, with its results as
Python integers, and the rule that decides per wire whether such a table shrinks it (csrc/lagrange.hip)."""
import numpy as np

from oracle import plonk as P, coracle as K

ZERO = 0xFFFFFFFF
FREE, DEFINED = 1, 2
MAX_FRAC = 0.9          # WIRE_BASES_MAX_FRAC


def to_idx(ws):
    return np.array([ZERO if v == P.ZERO_VAR else v for v in ws], dtype=np.uint32)


def raw(cv, cs, K_cap=16, pi_pos=None):
    """the hook's arrays for the circuit `cs` (public inputs at cs.pi unless pi_pos is given)"""
    import zkt_plonk_amd._lib as L
    sel = [K.fr_to_mont(cv, q) for q in (cs.q_m, cs.q_l, cs.q_r, cs.q_o, cs.q_c)]
    pos = sorted(cs.pi) if pi_pos is None else list(pi_pos)
    return L.wire_elimination(cv.name, sel, to_idx(cs.w_l), to_idx(cs.w_r), to_idx(cs.w_o), len(cs.values), pos, K_cap)


def eliminate(cv, cs, K_cap=16, pi_pos=None):
    """-> (kind per variable, free list, {v: ({f: M[v][f]}, kappa_v)} for the defined variables)"""
    kind, free, tv, tf, tc, kappa = raw(cv, cs, K_cap, pi_pos)
    coef = K.fr_from_mont(cv, tc) if len(tv) else []
    kap = K.fr_from_mont(cv, kappa) if len(kappa) else []
    forms = {int(v): ({}, int(kap[v])) for v in np.nonzero(kind == DEFINED)[0]}
    for v, f, c in zip(tv.tolist(), tf.tolist(), coef):
        assert f not in forms[v][0], "a free variable twice in one form"
        forms[v][0][f] = int(c)
    return kind, [int(f) for f in free], forms


def predicted_routes(cs, kind, free, forms):
    """What lagrange.hip decides per wire: 2 when the free variables that reach the wire, plus the constant point, are fewer
    than MAX_FRAC of the bases of the wire's other route (its distinct variables when those are fewer than MAX_FRAC of the
    rows, else the rows); otherwise that other route (1 or 0)."""
    n_rows = cs.n_gates
    if not forms or not free:
        return None
    out = []
    for ws in (cs.w_l, cs.w_r, cs.w_o):
        distinct = {v for v in ws if v != P.ZERO_VAR}
        d = len(distinct)
        other = 1 if d < MAX_FRAC * n_rows else 0
        present = d if other else n_rows
        reach = set()
        for v in distinct:
            if kind[v] == FREE:
                reach.add(v)
            else:
                reach.update(forms[v][0])
        out.append(2 if d and reach and len(reach) + 1 < MAX_FRAC * present else other)
    return out
