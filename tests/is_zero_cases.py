"""Shared by the rule-Z tests (test_is_zero_cases_oracle.py, test_witness_rule_z_host.py, test_gpu_witness_is_zero.py): the
rule of csrc/witness_plan.hpp restated in Python WITH rule Z (plan, completion), and the cases.  witness_plan_cases is
imported, not edited: with rules = 0 the planner here equals witness_plan_cases.plan (pinned by the oracle test).

Rule Z, tried at row i before rule O, only under RULE_IS_ZERO.  It fires when neither row i nor row i + 1 is public and
i + 1 < n_rows; row i = (x, y, z) with q_m != 0, q_o != 0, q_l = q_r = 0 (q_c arbitrary); y and z real, unseen at row i,
distinct from each other and from x; x real or Zero; row i + 1 = (x, z, Zero) with q_m != 0 and q_l = q_r = q_o = q_c = 0.
Row i then defines both:   x = 0: y = 0, z = -q_c / q_o;   x != 0: z = 0, y = -q_c / (q_m x).   Row i + 1 defines nothing;
level(y) = level(z) = 1 + level(x).  Any clause failing: rules O and R as without the bit.

The gadgets are restated row by row with the reference's selectors (oracle/composer.py has none of them):
  should_be_zero_with_output   plonk-core/src/constraint_system/mod.rs:243-281
  should_eq_with_output        mod.rs:285-289 (sub_gate, arithmetic.rs:45-72, then the above)
  conditional_select_one       mod.rs:415-452"""
import random

from oracle import plonk as P

import witness_plan_cases as W

RULE_IS_ZERO = 1                          # ZKT_WITNESS_RULE_IS_ZERO
ZINV, ZFLAG = 4, 5                        # zkt_witness_plan_kinds: rule Z's inverse y, its flag z
UNUSED, FREE, OUT, RIGHT, ZERO_VAR = W.UNUSED, W.FREE, W.OUT, W.RIGHT, P.ZERO_VAR
DEFINED = (OUT, RIGHT, ZINV, ZFLAG)


# ---- the rule ---------------------------------------------------------------------------------------------------------------
def plan(c, rules=0):
    n_vars, is_pi = c.n_vars, set(c.pi_pos)
    kind, def_row, level = [UNUSED] * n_vars, [W.NO_ROW] * n_vars, [0] * n_vars
    seen = [False] * n_vars
    real = lambda v: v != ZERO_VAR
    lvl = lambda v: level[v] if real(v) else 0
    sel = lambda k, i: c.sel[k][i]
    records = []                                                        # (level, row)
    for i in range(c.n_rows):
        a, b, o = c.w[0][i], c.w[1][i], c.w[2][i]
        if i not in is_pi:
            j = i + 1
            if (rules & RULE_IS_ZERO and j < c.n_rows and j not in is_pi
                    and sel(0, i) != 0 and sel(3, i) != 0 and sel(1, i) == 0 and sel(2, i) == 0
                    and real(b) and real(o) and not seen[b] and not seen[o] and b != o and b != a and o != a
                    and c.w[0][j] == a and c.w[1][j] == o and c.w[2][j] == ZERO_VAR
                    and sel(0, j) != 0 and sel(1, j) == sel(2, j) == sel(3, j) == sel(4, j) == 0):
                kind[b], kind[o] = ZINV, ZFLAG
                def_row[b] = def_row[o] = i
                level[b] = level[o] = 1 + lvl(a)
                records.append((level[o], i))
            elif sel(3, i) != 0 and real(o) and not seen[o] and o != a and o != b:
                kind[o], def_row[o], level[o] = OUT, i, 1 + max(lvl(a), lvl(b))
                records.append((level[o], i))
            elif real(b) and not seen[b] and b != a and b != o and (not real(a) or seen[a]) and (not real(o) or seen[o]):
                kind[b], def_row[b], level[b] = RIGHT, i, 1 + max(lvl(a), lvl(o))
                records.append((level[b], i))
        for v in (a, b, o):
            if real(v):
                if kind[v] == UNUSED:
                    kind[v] = FREE
                seen[v] = True
    pl = W.Plan()
    pl.kind, pl.def_row, pl.level = kind, def_row, level
    pl.depth = max(level, default=0)
    pl.rows = [r for _, r in sorted(records)]                           # one record per pair
    pl.level_rows = [0] * (pl.depth + 1)
    for l, _ in records:
        pl.level_rows[l] += 1
    pl.max_level_rows = max(pl.level_rows, default=0)
    pl.n_free, pl.n_out, pl.n_right, pl.n_unused = (kind.count(k) for k in (FREE, OUT, RIGHT, UNUSED))
    pl.n_pairs = kind.count(ZFLAG)
    return pl


def complete(c, pl, values):
    """as witness_plan_cases.complete, with the pairs: -> (the completed map, public inputs, (unsolvable rows, first or NONE))"""
    p = c.p
    x = list(values)
    val = lambda v: 0 if v == ZERO_VAR else x[v]
    bad = []
    for i in pl.rows:
        qm, ql, qr, qo, qc = (q[i] for q in c.sel)
        a, b, o = c.w[0][i], c.w[1][i], c.w[2][i]
        if o != ZERO_VAR and pl.kind[o] == ZFLAG and pl.def_row[o] == i:
            if val(a) == 0:
                x[b], x[o] = 0, -qc * pow(qo, -1, p) % p
            else:
                x[b], x[o] = -qc * pow(qm * val(a), -1, p) % p, 0
        elif o != ZERO_VAR and pl.kind[o] == OUT and pl.def_row[o] == i:
            x[o] = -(qm * val(a) * val(b) + ql * val(a) + qr * val(b) + qc) * pow(qo, -1, p) % p
        else:
            den = (qm * val(a) + qr) % p
            if den == 0:
                x[b] = 0
                bad.append(i)
            else:
                x[b] = -(ql * val(a) + qo * val(o) + qc) * pow(den, -1, p) % p
    return x, W.public_inputs(c, x), (len(bad), min(bad) if bad else W.NONE)


def prefill(c, pl, values, stride=None, salt=1):
    """witness_plan_cases.prefill, the pairs' variables overwritten as well"""
    x = W.prefill(c, pl, values, stride, salt)
    for v in range(c.n_vars):
        if pl.kind[v] in (ZINV, ZFLAG):
            x[v] = (0xBEEF << 170) + 29 * v + salt
    return x


def unsatisfied_rows(c, x, pi):
    """rows whose gate equation is not 0 on the map x with the public inputs pi (position order), by Python integers"""
    by_row = dict(zip(c.pi_pos, pi))
    val = lambda v: 0 if v == ZERO_VAR else x[v]
    out = []
    for i in range(c.n_rows):
        qm, ql, qr, qo, qc = (q[i] for q in c.sel)
        a, b, o = (val(w[i]) for w in c.w)
        if (qm * a * b + ql * a + qr * b + qo * o + qc + by_row.get(i, 0)) % c.p:
            out.append(i)
    return out


# ---- the reference's gadgets, as its proving composer assigns them -------------------------------------------------------------
def should_be_zero_with_output(cs, x, q_m=1, q_o=1, q_c=-1):                # mod.rs:243-281; other selectors: the general pair
    p = cs.p
    xv = cs.value_of(x)
    yv = 0 if xv == 0 else -q_c * pow(q_m * xv, -1, p) % p                  # mod.rs:269: inverse().unwrap_or_default()
    zv = -q_c * pow(q_o, -1, p) % p if xv == 0 else 0                       # mod.rs:270-271
    y, z = cs.assign_variable(yv), cs.assign_variable(zv)
    cs.arith_constrain(x, y, z, q_m=q_m, q_o=q_o, q_c=q_c)                  # x y + z - 1 = 0
    cs.arith_constrain(x, z, ZERO_VAR, q_m=1)                               # x z = 0
    return y, z


def sub_gate(cs, x, y):                                                     # arithmetic.rs:45-72
    z = cs.assign_variable(cs.value_of(x) - cs.value_of(y))
    cs.arith_constrain(x, y, z, q_l=1, q_r=-1, q_o=-1)
    return z


def should_eq_with_output(cs, x, y):                                        # mod.rs:285-289
    d = sub_gate(cs, x, y)
    return (d,) + should_be_zero_with_output(cs, d)


def conditional_select_one(cs, bit, value):                                 # mod.rs:415-452: bit value - bit - out + 1 = 0
    bv = cs.value_of(bit)
    assert bv in (0, 1)
    out = cs.assign_variable(1 if bv == 0 else cs.value_of(value))
    cs.arith_constrain(bit, value, out, q_m=1, q_l=-1, q_o=-1, q_c=1)
    return out


# ---- the cases -----------------------------------------------------------------------------------------------------------------
class Case:
    """c: the Circuit (its values: the first witness); witnesses: full maps, one per input set, every row satisfied;
    kinds: {var: kind} expected under RULE_IS_ZERO; near_miss: the bit changes nothing about this circuit's plan"""

    def __init__(self, c, witnesses, kinds, near_miss):
        self.c, self.witnesses, self.kinds, self.near_miss = c, witnesses, kinds, near_miss


def _make(cv, log_n, name, build, inputs, near_miss=False):
    made = []
    for vals in inputs:
        cs = W._cs(cv, log_n)
        kinds = build(cs, *vals)
        made.append(W.Circuit.of(cs, log_n, name="%s/%s/%d" % (name, cv.name, log_n)))
        assert cs.circuit_bound() == 1 << log_n
    assert all(W.same_circuit(made[0], m) for m in made[1:])
    return Case(made[0], [m.values for m in made], kinds, near_miss)


def xs(p, seed):
    """x in {0, 1, p - 1, a random value}"""
    return [0, 1, p - 1, random.Random(seed).randrange(2, p - 1)]


def cases(cv, log_n):
    p = cv.fr.p
    rnd = random.Random(0x15E0 + log_n)
    r = lambda: rnd.randrange(2, p - 1)
    out = []

    def free_x(cs, xv):                                                   # a pair on a free x
        x = cs.assign_variable(xv)
        y, z = should_be_zero_with_output(cs, x)
        return {x: FREE, y: ZINV, z: ZFLAG}
    out.append(_make(cv, log_n, "free_x", free_x, [(v,) for v in xs(p, 1)]))

    def on_zero(cs, _):                                                   # a pair on Variable::Zero
        y, z = should_be_zero_with_output(cs, ZERO_VAR)
        return {y: ZINV, z: ZFLAG}
    out.append(_make(cv, log_n, "on_zero", on_zero, [(0,)]))

    def eq(cs, av, bv):                                                   # should_eq_with_output: a pair on a sub_gate output
        a, b = cs.assign_variable(av), cs.assign_variable(bv)
        d, y, z = should_eq_with_output(cs, a, b)
        return {a: FREE, b: FREE, d: OUT, y: ZINV, z: ZFLAG}
    k = r()
    out.append(_make(cv, log_n, "eq", eq, [(k, k), (0, 0), (k, k + 1), (k, k - 1 + p), (5, r()), (0, 1), (p - 1, 0)]))

    def chained(cs, xv, vv):                                              # a rule-Z output feeds a later level
        x, v = cs.assign_variable(xv), cs.assign_variable(vv)
        y1, z1 = should_be_zero_with_output(cs, x)
        s = conditional_select_one(cs, z1, v)
        y2, z2 = should_be_zero_with_output(cs, s)
        return {x: FREE, v: FREE, y1: ZINV, z1: ZFLAG, s: OUT, y2: ZINV, z2: ZFLAG}
    out.append(_make(cv, log_n, "chained", chained, [(0, 0), (0, r()), (r(), 0), (1, p - 1), (0, 1)]))

    for qc in (7, 0):                                                     # general selectors
        def general(cs, xv, qc=qc):
            x = cs.assign_variable(xv)
            y, z = should_be_zero_with_output(cs, x, q_m=3, q_o=-5, q_c=qc)
            return {x: FREE, y: ZINV, z: ZFLAG}
        out.append(_make(cv, log_n, "general_qc%d" % qc, general, [(v,) for v in xs(p, 2)]))

    # near misses: they fall through to rules O and R, with the bit as without
    inv = lambda v: pow(v, -1, p) if v % p else 0
    flag = lambda v: 1 if v % p == 0 else 0

    def y_seen(cs, xv):
        x, y = cs.assign_variable(xv), cs.assign_variable(inv(xv))
        cs.arith_constrain(y, y, ZERO_VAR, q_l=1, q_r=-1)
        z = cs.assign_variable(flag(xv))
        cs.arith_constrain(x, y, z, q_m=1, q_o=1, q_c=-1)
        cs.arith_constrain(x, z, ZERO_VAR, q_m=1)
        return {x: FREE, y: FREE, z: OUT}
    out.append(_make(cv, log_n, "y_seen", y_seen, [(v,) for v in xs(p, 3)], True))

    def z_seen(cs, xv):                                                   # x and z seen: rule R solves for y (x != 0)
        x, z = cs.assign_variable(xv), cs.assign_variable(flag(xv))
        cs.arith_constrain(x, z, ZERO_VAR, q_m=1)
        y = cs.assign_variable(inv(xv))
        cs.arith_constrain(x, y, z, q_m=1, q_o=1, q_c=-1)
        cs.arith_constrain(x, z, ZERO_VAR, q_m=1)
        return {x: FREE, z: FREE, y: RIGHT}
    out.append(_make(cv, log_n, "z_seen", z_seen, [(v,) for v in xs(p, 4)[1:]], True))

    def x_is_y(cs, xv):                                                   # (x, x, z): x^2 + z - 1 = 0, x z = 0
        x = cs.assign_variable(xv)
        z = cs.assign_variable(1 - xv * xv)
        cs.arith_constrain(x, x, z, q_m=1, q_o=1, q_c=-1)
        cs.arith_constrain(x, z, ZERO_VAR, q_m=1)
        return {x: FREE, z: OUT}
    out.append(_make(cv, log_n, "x_is_y", x_is_y, [(0,), (1,), (p - 1,)], True))

    def with_q_l(cs, xv):                                                 # x y + 2 x + z - 1 = 0
        x = cs.assign_variable(xv)
        y = cs.assign_variable((1 - 2 * xv) * inv(xv))
        z = cs.assign_variable(flag(xv))
        cs.arith_constrain(x, y, z, q_m=1, q_l=2, q_o=1, q_c=-1)
        cs.arith_constrain(x, z, ZERO_VAR, q_m=1)
        return {x: FREE, y: FREE, z: OUT}
    out.append(_make(cv, log_n, "with_q_l", with_q_l, [(v,) for v in xs(p, 5)], True))

    def second_q_c(cs, yv):                                               # second row x z + 3 = 0: x = 1, z = -3, y = 4
        x, y = cs.assign_variable(1), cs.assign_variable(yv)
        z = cs.assign_variable(1 - yv)
        cs.arith_constrain(x, y, z, q_m=1, q_o=1, q_c=-1)
        cs.arith_constrain(x, z, ZERO_VAR, q_m=1, q_c=3)
        return {x: FREE, y: FREE, z: OUT}
    out.append(_make(cv, log_n, "second_q_c", second_q_c, [(4,)], True))

    def second_public(cs, xv, yv):                                        # the second row is public: its PI is an output
        x, y = cs.assign_variable(xv), cs.assign_variable(yv)
        z = cs.assign_variable(1 - xv * yv)
        cs.arith_constrain(x, y, z, q_m=1, q_o=1, q_c=-1)
        cs.arith_constrain(x, z, ZERO_VAR, q_m=1, pi=-xv * (1 - xv * yv))
        return {x: FREE, y: FREE, z: OUT}
    out.append(_make(cv, log_n, "second_public", second_public, [(r(), r()), (0, 9)], True))

    def split_by_end(cs, xv, yv):                                         # the first row is the last row
        x, y = cs.assign_variable(xv), cs.assign_variable(yv)
        while cs.n_gates < (1 << log_n) - 1:
            cs.arith_constrain(x, x, ZERO_VAR, q_l=1, q_r=-1)
        z = cs.assign_variable(1 - xv * yv)
        cs.arith_constrain(x, y, z, q_m=1, q_o=1, q_c=-1)
        return {x: FREE, y: FREE, z: OUT}
    out.append(_make(cv, log_n, "split_by_end", split_by_end, [(r(), r()), (0, 3)], True))
    return out


WIDE_PAIRS = 300                          # one level, more than one stride of the 256-thread workgroup
_WIDE = {}


def wide_case(cv, n_witnesses=4):
    """log_n = 10: WIDE_PAIRS independent pairs in level 1, zero and non-zero x mixed along the rows and across witnesses"""
    if (cv.name, n_witnesses) not in _WIDE:
        p = cv.fr.p

        def build(cs, seed):
            rnd = random.Random(seed)
            kinds = {}
            for k in range(WIDE_PAIRS):
                xv = (0, 1, p - 1, rnd.randrange(2, p - 1), 0, rnd.randrange(2, p - 1))[(k + seed) % 6 if k % 7 else rnd.randrange(6)]
                x = cs.assign_variable(xv)
                y, z = should_be_zero_with_output(cs, x)
                kinds.update({x: FREE, y: ZINV, z: ZFLAG})
            return kinds
        _WIDE[cv.name, n_witnesses] = _make(cv, 10, "wide", build, [(s,) for s in range(n_witnesses)])
    return _WIDE[cv.name, n_witnesses]


def host_plan(c, rules):
    """zkt_debug_witness_plan_host_ex on the case -> (kind, def_row, level) as lists"""
    import zkt_plonk_amd._lib as L
    sel = [W.mont(c.cv, q) for q in c.sel]
    kind, def_row, level = L.debug_witness_plan_host(c.cv.name, sel, c.idx(0), c.idx(1), c.idx(2), c.n_vars, list(c.pi_pos), rules=rules)
    return kind.tolist(), def_row.tolist(), level.tolist()
