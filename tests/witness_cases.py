"""The three rules of zkt_circuit_check_witness (check_gate, constraint_system/helper.rs:13-75, over every row) restated in
plain Python, and the builders of the cases the tests feed it.  tests/test_witness_cases_oracle.py pins the restatement
against ConstraintSystem.check_satisfied; tests/test_gpu_witness_check.py takes its expected reports from here.

A report is a dict: satisfied, checked, n_arithmetic, first_arithmetic, residual (the gate equation's value at
first_arithmetic as an integer, 0 when none), n_lookup, first_lookup, n_wiring, first_wiring ((column, row) or None);
a `first_*` without a failure is None."""
import random

import numpy as np

from oracle import plonk as P

import sigma_cases as SC

SELECTORS = ("q_m", "q_l", "q_r", "q_o", "q_c", "q_lookup")
CHECK_WIRING = 1


def _pad(v, n):
    v = list(v)
    assert len(v) <= n
    return v + [0] * (n - len(v))


def expected_report(p, n, sel, a, b, c, table, pi, key_wiring=None, wiring=None):
    """sel: the six selector vectors of the loaded key (up to n values each, zero above); a, b, c: the wire values (up
    to n, zero above); table: the lookup table as passed to the call; pi: {row: value}.  key_wiring / wiring: three index
    vectors each (0xFFFFFFFF = Variable::Zero) -- the wiring the key's permutation was made from and the one handed to
    the call; both given = the wiring rule runs."""
    q = {k: _pad(sel[k], n) for k in SELECTORS}
    a, b, c = _pad(a, n), _pad(b, n), _pad(c, n)
    tbl = set(int(t) % p for t in table)
    bad_a, bad_l, residual = [], [], 0
    for i in range(n):
        t = (q["q_m"][i] * a[i] * b[i] + q["q_l"][i] * a[i] + q["q_r"][i] * b[i] + q["q_o"][i] * c[i] + q["q_c"][i]
             + pi.get(i, 0)) % p
        if t:
            if not bad_a:
                residual = t
            bad_a.append(i)
        f = q["q_lookup"][i] * c[i] % p
        if f and f not in tbl:
            bad_l.append(i)
    bad_w = []
    if wiring is not None:
        # k_col w^row is one value per wire (the cosets of 1, 7, 13 are disjoint), so two sigma evaluations are equal
        # exactly when their targets are: the comparison is made on the targets of sigma_cases.sigma_targets
        want = SC.sigma_targets(key_wiring[0], key_wiring[1], key_wiring[2], n).reshape(-1)
        got = SC.sigma_targets(wiring[0], wiring[1], wiring[2], n).reshape(-1)
        bad_w = np.flatnonzero(want != got).tolist()          # wire numbers p = 3 row + column, ascending
    return dict(satisfied=not (bad_a or bad_l or bad_w), checked=3 | (4 if wiring is not None else 0),
                n_arithmetic=len(bad_a), first_arithmetic=bad_a[0] if bad_a else None, residual=residual,
                n_lookup=len(bad_l), first_lookup=bad_l[0] if bad_l else None,
                n_wiring=len(bad_w), first_wiring=(bad_w[0] % 3, bad_w[0] // 3) if bad_w else None)


def indices(cs):
    return [SC.to_index(w, P.ZERO_VAR) for w in (cs.w_l, cs.w_r, cs.w_o)]


def selectors(cs):
    return {k: list(getattr(cs, k)) for k in SELECTORS}


def report_of_cs(cs, key=None, wiring=False):
    """The expected report of the witness held by `cs` (values, wiring, table, public inputs) against the key made from
    `key` (selectors and wiring; default: cs itself)."""
    key = cs if key is None else key
    a, b, c = cs.wire_evals(cs.n_gates)
    return expected_report(cs.p, key.circuit_bound(), selectors(key), a, b, c, cs.table, cs.pi,
                           indices(key) if wiring else None, indices(cs) if wiring else None)


# ---- case builders: every one returns a changed copy, the original stays as it is -----------------------------------
def clone(cs):
    out = P.ConstraintSystem.__new__(P.ConstraintSystem)
    out.__dict__.update(cs.__dict__)
    for k in ("values", "table", "w_l", "w_r", "w_o") + SELECTORS:
        setattr(out, k, list(getattr(cs, k)))
    out.pi = dict(cs.pi)
    return out


def with_value(cs, var, value):
    out = clone(cs)
    out.values[var] = value % cs.p
    return out


def with_random_values(cs, seed):
    out = clone(cs)
    rnd = random.Random(seed)
    out.values = [rnd.randrange(cs.p) for _ in cs.values]
    return out


def with_qc_shift(cs, row, delta):
    out = clone(cs)
    out.q_c[row] = (out.q_c[row] + delta) % cs.p
    return out


def with_pi_value(cs, row, value):
    out = clone(cs)
    assert row in out.pi
    out.pi[row] = value % cs.p
    return out


def with_pi_moved(cs, row, to):
    out = clone(cs)
    assert row in out.pi and to not in out.pi
    out.pi[to] = out.pi.pop(row)
    return out


def with_table(cs, table):
    out = clone(cs)
    out.table = [t % cs.p for t in table]
    return out


def lookup_rows(cs):
    return [g for g in range(cs.n_gates) if cs.q_lookup[g]]


def third_kind_rows(cs):
    """rows of synthetic_circuit's third gate kind (q_l a + q_r b - c + q_c with random 254-bit selectors): satisfied
    only modulo p, every term is large"""
    big = cs.p >> 8
    return [g for g in range(cs.n_gates) if cs.q_l[g] > big and cs.q_r[g] > big and cs.q_c[g] > big and not cs.q_m[g]]


def with_equal_value_swap(cs):
    """One index replaced by another variable of equal value: lookup_constrain(x) copies x into a fresh output variable,
    so its row (x, Zero, x') may read x' on the left as well.  Gates and lookups still pass, the permutation differs.
    -> (changed copy, row)"""
    row = lookup_rows(cs)[len(lookup_rows(cs)) // 2]
    x, x2 = cs.w_l[row], cs.w_o[row]
    assert x != x2 and x != P.ZERO_VAR and cs.value_of(x) == cs.value_of(x2)
    out = clone(cs)
    out.w_l[row] = x2
    return out, row


def cs_cases(cv):
    """name -> (ConstraintSystem holding the witness, ConstraintSystem the key is made from): P.test_circuit,
    P.synthetic_circuit and each of their mutations that is still a ConstraintSystem.  Deterministic."""
    out = {}
    bases = {"test_circuit": P.test_circuit(cv, size=20),
             "synthetic_700": P.synthetic_circuit(cv, 700, 32, seed=4242),
             "synthetic_1024": P.synthetic_circuit(cv, 1024, 32, seed=1024)}
    for name, cs in bases.items():
        p = cs.p
        out[name] = (cs, cs)
        var = cs.w_l[cs.n_gates // 2] if cs.w_l[cs.n_gates // 2] != P.ZERO_VAR else cs.w_o[cs.n_gates // 2]
        out[name + "/one_value_changed"] = (with_value(cs, var, cs.values[var] + 1), cs)
        out[name + "/random_witness"] = (with_random_values(cs, 99), cs)
        for label, row in (("row0", 0), ("last_gate", cs.n_gates - 1)):
            out[name + "/qc_plus_1_" + label] = (cs, with_qc_shift(cs, row, 1))
            out[name + "/qc_minus_1_" + label] = (cs, with_qc_shift(cs, row, -1))
        pi_row = sorted(cs.pi)[0]
        out[name + "/wrong_public_input"] = (with_pi_value(cs, pi_row, cs.pi[pi_row] + 5), cs)
        free = next(g for g in range(cs.n_gates) if g not in cs.pi)
        out[name + "/moved_public_input"] = (with_pi_moved(cs, pi_row, free), cs)
        used = cs.value_of(cs.w_o[lookup_rows(cs)[0]])
        assert used % p in cs.table
        out[name + "/table_value_removed"] = (with_table(cs, [t for t in cs.table if t != used % p]), cs)
        out[name + "/table_reversed"] = (with_table(cs, cs.table[::-1]), cs)
        out[name + "/table_of_one"] = (with_table(cs, cs.table[:1]), cs)
        out[name + "/table_empty"] = (with_table(cs, []), cs)
        out[name + "/equal_value_swap"] = (with_equal_value_swap(cs)[0], cs)
    return out


def combined(wit, key):
    """The ConstraintSystem whose check_satisfied is the oracle for (witness of `wit`, selectors of `key`)."""
    out = clone(wit)
    for k in SELECTORS:
        setattr(out, k, list(getattr(key, k)))
    return out
