"""CPU: the Python restatement of the witness-completion rule (tests/witness_plan_cases.py) against the oracle's composer.  From
the composer's direct assign_variable values alone it must reproduce cs.values, cs.pi and the CLI-order public inputs of
oracle.composer.withdraw_instance; the free variables are exactly those assign_variable calls."""
import pytest

import witness_plan_cases as W

CASES = [("bn254", "synthetic", 2, 3, 4), ("bls12_381", "synthetic", 2, 3, 4), ("bn254", "shipped", 2, 3, 4),
         ("bn254", "synthetic", 1, 2, 5)]
FIGURES = {("bn254", "synthetic", 2, 3, 4): (2548, 2555, 245, 87, 12), ("bls12_381", "synthetic", 2, 3, 4): (2548, 2555, 245, 87, 12),
           ("bn254", "shipped", 2, 3, 4): (18214, 18221, 2240, 87, 15)}


@pytest.mark.parametrize("cvname,params,inputs,height,width", CASES)
def test_restatement_reproduces_the_composers_witness(cvname, params, inputs, height, width):
    c, pub, cs = W.withdraw(cvname, params, 1, inputs, height, width)
    assert cs.check_satisfied()
    pl = W.plan(c)
    assert pl.n_free == W.withdraw_free_count(inputs, height)
    assert pl.n_right == inputs and pl.n_unused == 0
    assert pl.n_free + pl.n_out + pl.n_right == c.n_vars
    start = W.prefill(c, pl, c.values)
    assert all(start[v] != c.values[v] for v in range(c.n_vars) if pl.kind[v] in (W.OUT, W.RIGHT))
    x, pi, bad = W.complete(c, pl, start)
    assert x == c.values
    assert pi == [c.pi[i] for i in c.pi_pos]
    assert sorted(pi) == sorted(v % c.p for v in pub)
    assert bad == (0, W.NONE)
    key = (cvname, params, inputs, height, width)
    if key in FIGURES:
        assert (c.n_rows, c.n_vars, pl.depth, pl.max_level_rows, c.log_n) == FIGURES[key]


@pytest.mark.parametrize("cvname,params", [("bn254", "synthetic"), ("bls12_381", "synthetic"), ("bn254", "shipped")])
def test_seeds_change_the_witness_not_the_circuit(cvname, params):
    c1 = W.withdraw(cvname, params, 1)[0]
    for seed in (2, 3, 4):
        c2 = W.withdraw(cvname, params, seed)[0]
        assert W.same_circuit(c1, c2)
        assert c2.values != c1.values


def test_a_zero_secret_is_one_unsolvable_row_and_propagates():
    c = W.withdraw("bn254", "synthetic", 1)[0]
    pl = W.plan(c)
    free = [v for v in range(c.n_vars) if pl.kind[v] == W.FREE]
    secret = W.secret_variable(c, pl)
    assert secret in free
    start = W.prefill(c, pl, c.values)
    start[secret] = 0
    x, pi, bad = W.complete(c, pl, start)
    row = pl.def_row[[v for v in range(c.n_vars) if pl.kind[v] == W.RIGHT][0]]
    assert bad == (1, row)
    assert x[c.w[1][row]] == 0 and x != c.values


def test_the_split_predicts_the_launches():
    c = W.withdraw("bn254", "synthetic", 1)[0]
    pl = W.plan(c)
    assert pl.level_rows[1] == 87 and max(pl.level_rows[2:]) < 87
    assert [W.launches(pl, k) for k in (1, 87, 88, 1 << 31)] == [1, 2, 1, 1]
    assert W.launches(pl, 40) > 2
