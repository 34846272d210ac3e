"""CPU: pins the rule-Z cases (tests/is_zero_cases.py).  Every completed map satisfies every row, by direct evaluation of the
gate equation with Python integers, and equals what the gadgets' own native assignments give; with rules = 0 the extended
planner is witness_plan_cases.plan, on the cases of both modules.  The cases module is plain Python; the kind numbers it uses
are held against the package's (zkt_plonk_amd.witness), which the parent does not have."""
import pytest

from oracle import fields as F
import is_zero_cases as Z
import witness_plan_cases as W

from zkt_plonk_amd import witness as PKG

CURVES = {"bn254": F.BN254, "bls12_381": F.BLS12_381}
assert (PKG.ZINV, PKG.ZFLAG, PKG.RULE_IS_ZERO) == (Z.ZINV, Z.ZFLAG, Z.RULE_IS_ZERO)


def _same_plan(a, b):
    return all(getattr(a, k) == getattr(b, k) for k in ("kind", "def_row", "level", "depth", "rows", "level_rows", "max_level_rows",
                                                         "n_free", "n_out", "n_right", "n_unused"))


def _check_case(case):
    c = case.c
    pl = Z.plan(c, Z.RULE_IS_ZERO)
    for v, k in case.kinds.items():
        assert pl.kind[v] == k, (c.name, v)
    assert _same_plan(Z.plan(c, 0), W.plan(c)), c.name
    if case.near_miss:
        assert _same_plan(pl, W.plan(c)) and pl.n_pairs == 0, c.name
    else:
        assert pl.n_pairs == sum(1 for k in case.kinds.values() if k == Z.ZFLAG) > 0, c.name
        assert pl.n_free < W.plan(c).n_free, c.name                        # the bit takes the pairs' y off the caller
    for values in case.witnesses:
        x, pi, bad = Z.complete(c, pl, Z.prefill(c, pl, values))
        assert x == values, c.name                                         # the gadgets' own native assignments
        assert bad == (0, W.NONE), c.name
        assert Z.unsatisfied_rows(c, x, pi) == [], c.name
    return pl


@pytest.mark.parametrize("log_n", [3, 4])
@pytest.mark.parametrize("cvname", sorted(CURVES))
def test_cases_complete_to_satisfied_maps(cvname, log_n):
    cases = Z.cases(CURVES[cvname], log_n)
    assert sum(c.near_miss for c in cases) == 7 and len(cases) == 13
    for case in cases:
        _check_case(case)


def test_levels_of_the_chained_pairs_and_of_should_eq():
    by_name = {c.c.name.split("/")[0]: c for c in Z.cases(F.BN254, 3)}
    ch = by_name["chained"]
    pl = Z.plan(ch.c, Z.RULE_IS_ZERO)
    x, v, y1, z1, s, y2, z2 = sorted(ch.kinds)
    assert [pl.level[k] for k in (x, v, y1, z1, s, y2, z2)] == [0, 0, 1, 1, 2, 3, 3]
    assert pl.def_row[y1] == pl.def_row[z1] == 0 and pl.def_row[y2] == pl.def_row[z2] == 3 and pl.rows == [0, 2, 3]
    eq = by_name["eq"]
    pl = Z.plan(eq.c, Z.RULE_IS_ZERO)
    a, b, d, y, z = sorted(eq.kinds)
    assert [pl.level[k] for k in (d, y, z)] == [1, 2, 2]
    flags = [w[z] for w in eq.witnesses]
    assert flags == [1, 1, 0, 0, 0, 0, 0]                                  # zero reached as a difference of equal inputs
    assert [w[y] * w[d] % eq.c.p for w in eq.witnesses] == [0, 0, 1, 1, 1, 1, 1]


@pytest.mark.parametrize("cvname", sorted(CURVES))
def test_wide_case(cvname):
    case = Z.wide_case(CURVES[cvname])
    pl = _check_case(case)
    assert case.c.log_n == 10 and pl.n_pairs == Z.WIDE_PAIRS == pl.max_level_rows and pl.depth == 1 and Z.WIDE_PAIRS > 256
    for values in case.witnesses:                                          # zero and non-zero mixed along the rows
        zs = [values[v] for v, k in case.kinds.items() if k == Z.ZFLAG]
        assert 30 < sum(zs) < 270 and set(zs) == {0, 1}
    firsts = [[w[v] for w in case.witnesses] for v, k in case.kinds.items() if k == Z.ZFLAG]
    assert any(len(set(f)) == 2 for f in firsts)                           # and across the witnesses of a batch


@pytest.mark.parametrize("log_n", [3, 4])
@pytest.mark.parametrize("cvname", sorted(CURVES))
def test_without_the_bit_the_planner_is_the_imported_one(cvname, log_n):
    for c, _, _, _ in W.handmade_cases(CURVES[cvname], log_n):
        assert _same_plan(Z.plan(c, 0), W.plan(c)), c.name
        assert _same_plan(Z.plan(c, Z.RULE_IS_ZERO), W.plan(c)), c.name     # none of them holds a pair


@pytest.mark.parametrize("cvname,params", [("bn254", "synthetic"), ("bls12_381", "synthetic"), ("bn254", "shipped")])
def test_the_withdraw_circuit_holds_no_pair(cvname, params):
    c = W.withdraw(cvname, params, 1)[0]
    assert _same_plan(Z.plan(c, 0), W.plan(c))
    assert _same_plan(Z.plan(c, Z.RULE_IS_ZERO), W.plan(c))
