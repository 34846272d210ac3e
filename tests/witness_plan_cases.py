"""Shared by the witness-completion tests (test_witness_plan_*.py, test_gpu_witness_complete*.py): a Python restatement of
the rule of csrc/witness_plan.hpp (plan, completion, public inputs; include/zkt_plonk.h states the rule) and the cases.

The rule.  Row i asserts q_m a b + q_l a + q_r b + q_o c + q_c + PI_i = 0.  Rows are walked in ascending order; a variable
is unseen at row i when it stands on no wire of an earlier row.
  - a public-input row defines nothing; PI_i = -(q_m a b + q_l a + q_r b + q_o c + q_c) is an output;
  - rule O: q_o != 0 and w_o a real variable, unseen, different from w_l and w_r:  c = -(q_m a b + q_l a + q_r b + q_c) / q_o;
  - rule R: otherwise, w_r a real variable, unseen, different from w_l and w_o, and w_l, w_o each Zero or seen:
            b = -(q_l a + q_o c + q_c) / (q_m a + q_r); a zero denominator writes 0 and reports the row;
  - every other variable first seen on a wire is free; a variable on no wire is never touched.
level(defined v) = 1 + max level of the other two wires of its row (free and Zero: 0)."""
import numpy as np

from oracle import composer as OC, fields as F, plonk as P

ZERO = 0xFFFFFFFF
UNUSED, FREE, OUT, RIGHT = 0, 1, 2, 3
NONE = (1 << 64) - 1                      # ZKT_CHECK_NONE
NO_ROW = 0xFFFFFFFF                       # def_row of a variable that no row defines
BATCH_MAX = 256                           # ZKT_WITNESS_BATCH_MAX
MAX_LAUNCHES = 64


class Circuit:
    """Selectors (integers mod p), wiring (-1 = Variable::Zero), public-input positions; `values` is a full witness when the
    case has one (the oracle's cs.values), `pi` its public inputs by position."""

    def __init__(self, cv, q_m, q_l, q_r, q_o, q_c, w_l, w_r, w_o, n_vars, pi_pos, log_n, values=None, pi=None, name=""):
        self.cv, self.p = cv, cv.fr.p
        self.sel = [[x % self.p for x in q] for q in (q_m, q_l, q_r, q_o, q_c)]
        self.w = [list(w_l), list(w_r), list(w_o)]
        self.n_rows, self.n_vars, self.pi_pos, self.log_n = len(self.w[0]), n_vars, sorted(pi_pos), log_n
        self.values, self.pi, self.name = values, pi, name
        assert all(len(q) == self.n_rows for q in self.sel) and all(len(w) == self.n_rows for w in self.w)

    @staticmethod
    def of(cs, log_n=None, name=""):
        n = cs.circuit_bound()
        c = Circuit(cs.cv, cs.q_m, cs.q_l, cs.q_r, cs.q_o, cs.q_c, cs.w_l, cs.w_r, cs.w_o, len(cs.values), sorted(cs.pi),
                    log_n if log_n is not None else n.bit_length() - 1, list(cs.values), dict(cs.pi), name)
        c.cs = cs                                              # the key is made from it (oracle.plonk.setup_evals)
        return c

    def idx(self, k):
        return np.array([ZERO if v == P.ZERO_VAR else v for v in self.w[k]], dtype=np.uint32)


class Plan:
    pass


def plan(c: Circuit) -> Plan:
    n_vars, is_pi = c.n_vars, set(c.pi_pos)
    kind, def_row, level = [UNUSED] * n_vars, [NO_ROW] * n_vars, [0] * n_vars
    seen = [False] * n_vars
    real = lambda v: v != P.ZERO_VAR
    lvl = lambda v: level[v] if real(v) else 0
    for i in range(c.n_rows):
        a, b, o = c.w[0][i], c.w[1][i], c.w[2][i]
        if i not in is_pi:
            if c.sel[3][i] != 0 and real(o) and not seen[o] and o != a and o != b:
                kind[o], def_row[o], level[o] = OUT, i, 1 + max(lvl(a), lvl(b))
            elif (real(b) and not seen[b] and b != a and b != o and (not real(a) or seen[a]) and (not real(o) or seen[o])):
                kind[b], def_row[b], level[b] = RIGHT, i, 1 + max(lvl(a), lvl(o))
        for v in (a, b, o):
            if real(v):
                if kind[v] == UNUSED:
                    kind[v] = FREE
                seen[v] = True
    pl = Plan()
    pl.kind, pl.def_row, pl.level = kind, def_row, level
    pl.depth = max(level, default=0)
    rows = sorted((level[v], def_row[v]) for v in range(n_vars) if kind[v] in (OUT, RIGHT))
    pl.rows = [r for _, r in rows]
    pl.level_rows = [0] * (pl.depth + 1)
    for l, _ in rows:
        pl.level_rows[l] += 1
    pl.max_level_rows = max(pl.level_rows, default=0)
    pl.n_free, pl.n_out, pl.n_right, pl.n_unused = (kind.count(k) for k in (FREE, OUT, RIGHT, UNUSED))
    return pl


def launches(pl: Plan, wide_min_rows: int) -> int:
    """The launches that fill the map (the closing public-input launch is not counted): a level of at least wide_min_rows rows
    is one launch, a run of narrower levels between two such is one launch; above MAX_LAUNCHES, one launch altogether."""
    if pl.depth == 0:
        return 0
    count, in_run = 0, False
    for l in range(1, pl.depth + 1):
        if pl.level_rows[l] >= wide_min_rows:
            count, in_run = count + 1, False
        elif not in_run:
            count, in_run = count + 1, True
    return 1 if count > MAX_LAUNCHES else count


def complete(c: Circuit, pl: Plan, values):
    """-> (the completed map, public inputs in position order, (unsolvable rows, first such row or NONE)).  `values` is read
    at the free variables only."""
    p = c.p
    x = list(values)
    val = lambda v: 0 if v == P.ZERO_VAR else x[v]
    bad = []
    for i in pl.rows:
        qm, ql, qr, qo, qc = (q[i] for q in c.sel)
        a, b, o = c.w[0][i], c.w[1][i], c.w[2][i]
        if pl.kind[o] == OUT and pl.def_row[o] == i:
            x[o] = -(qm * val(a) * val(b) + ql * val(a) + qr * val(b) + qc) * pow(qo, -1, p) % p
        else:
            den = (qm * val(a) + qr) % p
            if den == 0:
                x[b] = 0
                bad.append(i)
            else:
                x[b] = -(ql * val(a) + qo * val(o) + qc) * pow(den, -1, p) % p
    return x, public_inputs(c, x), (len(bad), min(bad) if bad else NONE)


def public_inputs(c: Circuit, x):
    p, out = c.p, []
    val = lambda v: 0 if v == P.ZERO_VAR else x[v]
    for i in c.pi_pos:
        if i >= c.n_rows:
            out.append(0)                                    # a padded row: every selector is 0 there
            continue
        a, b, o = (val(w[i]) for w in c.w)
        qm, ql, qr, qo, qc = (q[i] for q in c.sel)
        out.append(-(qm * a * b + ql * a + qr * b + qo * o + qc) % p)
    return out


def prefill(c: Circuit, pl: Plan, values, stride=None, salt=1):
    """The map a completion starts from: free and unused variables and the padding as given (padding: a pattern), every
    defined variable overwritten with a distinct non-zero pattern."""
    stride = c.n_vars if stride is None else stride
    x = list(values) + [(0xA5A5 << 200) + 977 * k + salt for k in range(stride - c.n_vars)]
    for v in range(c.n_vars):
        if pl.kind[v] in (OUT, RIGHT):
            x[v] = (0xDEAD << 180) + 31 * v + salt
    return x


# ---- (a) hand-made circuits ---------------------------------------------------------------------------------------------
def _cs(cv, log_n):
    return P.ConstraintSystem(cv, [1, 2, 5], (1 << log_n) - 1)          # the setup needs n > table_size


def handmade_cases(cv, log_n):
    """-> list of (Circuit, free values {var: value}, expected kinds {var: kind}, expected (unsolvable rows, first such row))"""
    p = cv.fr.p
    Z = P.ZERO_VAR
    out = []

    def case(name, cs, free, kinds, bad=(0, NONE), n_rows_full=False):
        if n_rows_full:
            u = next(iter(free))
            while cs.n_gates < (1 << log_n):
                cs.arith_constrain(u, u, Z, q_l=1, q_r=-1)               # constraint only: defines nothing
        c = Circuit.of(cs, log_n, name="%s/%s/%d" % (name, cv.name, log_n))
        assert cs.circuit_bound() == 1 << log_n
        c.values = None
        out.append((c, dict(free), dict(kinds), bad))

    for qo in (-1, 5):                                                   # add -> mul -> linear_transform
        cs = _cs(cv, log_n)
        x, y = cs.assign_variable(11), cs.assign_variable(13)
        s, m, t = (cs.assign_variable(0) for _ in range(3))
        cs.arith_constrain(x, y, s, q_l=1, q_r=1, q_o=qo)
        cs.arith_constrain(s, x, m, q_m=1, q_o=qo)
        cs.arith_constrain(m, s, t, q_l=3, q_r=-7, q_o=qo, q_c=9)
        case("chain_qo%d" % qo, cs, {x: 11, y: 13}, {x: FREE, y: FREE, s: OUT, m: OUT, t: OUT}, n_rows_full=(qo == 5))

    for divisor in (13, 0):                                              # div_gate: wires (y, z, x), y z - x = 0
        cs = _cs(cv, log_n)
        x, y = cs.assign_variable(11), cs.assign_variable(divisor)
        cs.arith_constrain(x, y, Z, q_l=0, q_r=0)                        # both seen
        z = cs.assign_variable(0)
        cs.arith_constrain(y, z, x, q_m=1, q_o=-1)
        w = cs.assign_variable(0)
        cs.arith_constrain(z, x, w, q_l=1, q_r=2, q_o=-1)                # the quotient (or the rule's 0) propagates
        case("div_by_%d" % divisor, cs, {x: 11, y: divisor}, {x: FREE, y: FREE, z: RIGHT, w: OUT}, (0, NONE) if divisor else (1, 1))

    cs = _cs(cv, log_n)                                                  # boolean row (x, x, x) defines nothing
    x = cs.assign_variable(1)
    cs.boolean_gate(x)
    case("boolean", cs, {x: 1}, {x: FREE})

    cs = _cs(cv, log_n)                                                  # an output already seen: constraint only
    x, y = cs.assign_variable(4), cs.assign_variable(9)
    z = cs.assign_variable(0)
    cs.arith_constrain(x, y, z, q_l=1, q_r=1, q_o=-1)
    cs.arith_constrain(y, x, z, q_l=1, q_r=1, q_o=-1)
    case("output_seen", cs, {x: 4, y: 9}, {x: FREE, y: FREE, z: OUT})

    cs = _cs(cv, log_n)                                                  # two rows name the same new output: the first defines
    x, y = cs.assign_variable(4), cs.assign_variable(9)
    z = cs.assign_variable(0)
    cs.arith_constrain(x, y, z, q_m=1, q_o=-1)
    cs.arith_constrain(x, y, z, q_m=2, q_o=-2)
    case("same_output_twice", cs, {x: 4, y: 9}, {z: OUT})

    cs = _cs(cv, log_n)                                                  # an output equal to one of its own inputs
    x, s = cs.assign_variable(6), cs.assign_variable(0)
    cs.arith_constrain(s, x, s, q_l=1, q_o=-1)
    t = cs.assign_variable(5)
    cs.arith_constrain(x, t, t, q_r=1, q_o=-1)
    case("output_is_input", cs, {x: 6, s: 0, t: 5}, {x: FREE, s: FREE, t: FREE})

    cs = _cs(cv, log_n)                                                  # Zero on each wire
    x, y = cs.assign_variable(21), cs.assign_variable(22)
    a, b = cs.assign_variable(0), cs.assign_variable(0)
    cs.arith_constrain(Z, y, a, q_m=4, q_l=5, q_r=3, q_o=-1, q_c=7)
    cs.arith_constrain(x, Z, b, q_m=4, q_l=5, q_r=3, q_o=2, q_c=7)
    cs.arith_constrain(x, y, Z, q_l=1, q_r=1, q_o=9, q_c=-43)
    k = cs.assign_variable(0)
    cs.arith_constrain(Z, Z, k, q_o=-1, q_c=9)
    r = cs.assign_variable(0)
    cs.arith_constrain(Z, r, Z, q_r=3, q_c=-12)                          # rule R with Zero on both other wires: r = 4
    case("zero_wires", cs, {x: 21, y: 22}, {a: OUT, b: OUT, k: OUT, r: RIGHT})

    cs = _cs(cv, log_n)                                                  # w_o and w_r both unseen: O wins, w_r is free
    x = cs.assign_variable(3)
    f, o = cs.assign_variable(8), cs.assign_variable(0)
    cs.arith_constrain(x, f, o, q_m=1, q_o=-1)
    case("o_wins", cs, {x: 3, f: 8}, {x: FREE, f: FREE, o: OUT})

    cs = _cs(cv, log_n)                                                  # rule R needs w_l and w_o seen; and no left-wire rule
    x, y = cs.assign_variable(3), cs.assign_variable(0)
    u = cs.assign_variable(5)
    cs.arith_constrain(u, y, x, q_m=1, q_o=0)                            # q_o = 0: not O; w_l, w_o unseen: not R
    l = cs.assign_variable(15)
    cs.arith_constrain(l, u, x, q_l=1, q_m=0, q_r=-3)                    # an unseen left wire with both others seen: free
    case("r_needs_seen", cs, {x: 3, y: 0, u: 5, l: 15}, {x: FREE, y: FREE, u: FREE, l: FREE})

    cs = _cs(cv, log_n)                                                  # a public-input row on an unseen variable
    v = cs.assign_variable(77)
    cs.set_variable_public(v)
    w = cs.assign_variable(0)
    cs.arith_constrain(v, v, w, q_m=1, q_l=1, q_o=-1, pi=5)              # a public row that could define does not
    case("public_rows", cs, {v: 77, w: 123}, {v: FREE, w: FREE})

    cs = _cs(cv, log_n)                                                  # a variable on no wire, below and above the used ones
    lone = cs.assign_variable(99)
    x = cs.assign_variable(2)
    s = cs.assign_variable(0)
    cs.arith_constrain(x, x, s, q_m=1, q_o=-1)
    tail = cs.assign_variable(98)
    case("on_no_wire", cs, {lone: 99, x: 2, tail: 98}, {lone: UNUSED, x: FREE, s: OUT, tail: UNUSED})

    cs = _cs(cv, log_n)                                                  # n_rows = 0
    lone = cs.assign_variable(5)
    case("no_rows", cs, {lone: 5}, {lone: UNUSED})

    cs = _cs(cv, log_n)                                                  # a public position past the rows: PI = 0 there
    x = cs.assign_variable(6)
    cs.set_variable_public(x)
    cs.pi[(1 << log_n) - 1] = 0
    case("pi_past_rows", cs, {x: 6}, {x: FREE})
    return out


def handmade_values(c: Circuit, free):
    """the free values laid into a map of n_vars entries (everything else 0)"""
    x = [0] * c.n_vars
    for v, val in free.items():
        x[v] = val % c.p
    return x


# ---- (b), (c): the withdraw circuit --------------------------------------------------------------------------------------
_WITHDRAW = {}


def withdraw(cvname, params, seed=1, inputs=2, height=3, width=4):
    """(Circuit with the oracle's values and public inputs, the CLI-order public inputs); params: "synthetic" | "shipped" """
    import merkle_path_cases as MP
    key = (cvname, params, seed, inputs, height, width)
    if key not in _WITHDRAW:
        cv = F.BN254 if cvname == "bn254" else F.BLS12_381
        prm = MP.synthetic_params(cv, width) if params == "synthetic" else MP.shipped_params(width)
        cs, pub = OC.withdraw_instance(cv, prm, inputs=inputs, height=height, seed=seed)
        _WITHDRAW[key] = (Circuit.of(cs, name="withdraw/%s/%s/%d" % (cvname, params, seed)), pub, cs)
    return _WITHDRAW[key]


def same_circuit(c1: Circuit, c2: Circuit) -> bool:
    return c1.sel == c2.sel and c1.w == c2.w and c1.pi_pos == c2.pi_pos and c1.n_vars == c2.n_vars


def withdraw_free_count(inputs, height):
    return inputs * (3 + 2 * height) + 67


def secret_variable(c: Circuit, pl: Plan) -> int:
    """The first note's secret: the divisor of the first div_gate row (wires (secret, 1 / secret, one))."""
    row = min(pl.def_row[v] for v in range(c.n_vars) if pl.kind[v] == RIGHT)
    return c.w[0][row]


# ---- the library's view of a case -----------------------------------------------------------------------------------------
def mont(cv, ints):
    from oracle import coracle as K
    return K.fr_to_mont(cv, list(ints)) if len(ints) else np.zeros((0, 4), dtype=np.uint64)


def unmont(cv, arr):
    from oracle import coracle as K
    arr = np.ascontiguousarray(arr, dtype=np.uint64).reshape(-1, 4)
    return [int(v) for v in K.fr_from_mont(cv, arr)] if arr.shape[0] else []


def host_plan(c: Circuit):
    """zkt_debug_witness_plan_host on the case -> (kind, def_row, level) as lists"""
    import zkt_plonk_amd._lib as L
    sel = [mont(c.cv, q) for q in c.sel]
    pos = [i for i in c.pi_pos]
    kind, def_row, level = L.debug_witness_plan_host(c.cv.name, sel, c.idx(0), c.idx(1), c.idx(2), c.n_vars, pos)
    return kind.tolist(), def_row.tolist(), level.tolist()
