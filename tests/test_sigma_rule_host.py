"""The cycle rule of the sigma permutation as tests/sigma_cases.py restates it (a stable argsort of the gate-major keys)
against the oracle's ConstraintSystem.sigma_mappings (permutation/mod.rs:104-137): this pins the expected values of
tests/test_gpu_sigma.py.  No GPU."""
import numpy as np
import pytest

from oracle import fields as F, plonk as P

import sigma_cases as SC


def _oracle_targets(cs, n):
    sig = cs.sigma_mappings(n)
    return np.array([[3 * sig[col][g][1] + sig[col][g][0] for col in range(3)] for g in range(n)], dtype=np.int64)


def _check(cs):
    n = cs.circuit_bound()
    got = SC.sigma_targets(*(SC.to_index(w, P.ZERO_VAR) for w in (cs.w_l, cs.w_r, cs.w_o)), n)
    assert np.array_equal(got, _oracle_targets(cs, n))


def test_rule_on_the_reference_test_circuit():
    _check(P.test_circuit(F.BN254))


def test_rule_on_a_synthetic_circuit():
    _check(P.synthetic_circuit(F.BN254, 700, 32, seed=4242))


@pytest.mark.parametrize("name", sorted(SC.raw_cases()))
def test_rule_on_the_raw_cases(name):
    case = SC.raw_cases()[name]
    w, n = case["w"], 1 << case["log_n"]
    assert w.shape[0] <= n and all(v == SC.ZERO or v < case["n_vars"] for v in w.reshape(-1).tolist())
    cs = P.ConstraintSystem(F.BN254, [], 0)
    for col, name_ in enumerate(("w_l", "w_r", "w_o")):
        setattr(cs, name_, [P.ZERO_VAR if v == SC.ZERO else v for v in w[:, col].tolist()])
    cs.q_m = [0] * w.shape[0]                      # n_gates
    assert np.array_equal(SC.sigma_targets(w[:, 0], w[:, 1], w[:, 2], n), _oracle_targets(cs, n))


def test_raw_cases_have_the_shapes_they_are_named_for():
    c = SC.raw_cases()
    b = c["b_long_runs_odd_rows"]["w"]
    assert b.shape[0] == 8191 and 4000 < (b == 0).sum() < 6000 and (b == SC.ZERO).sum() > 2000
    assert all((b[:, col] == 0).sum() > 1000 for col in range(3))
    pos = np.flatnonzero(b.reshape(-1) == 0)
    assert pos[-1] - pos[0] > 4 * 2048              # the run crosses several workgroups of the sort
    assert len(set(c["c_all_distinct_no_padding"]["w"].reshape(-1).tolist())) == 3 << 12
    e = c["e_third_digit"]["w"]
    assert (e < 65536).any() and (e >= 65536).any() and c["e_third_digit"]["n_vars"] == 70000
    f = c["f_fourth_digit"]["w"].reshape(-1).tolist()
    assert all(v in f for v in (0, 255, 256, 65535, 65536, 1 << 24, (1 << 24) + 2))


def test_values_follow_the_targets():
    """k_col * w^row: the identity permutation gives (w^i, 7 w^i, 13 w^i)."""
    fr = F.BN254.fr
    root = fr.root_of_unity(8)
    vals = SC.sigma_values(fr.p, 3, SC.sigma_targets([], [], [], 8), root)
    for col, k in enumerate(SC.KS):
        assert vals[col] == [k * pow(root, i, fr.p) % fr.p for i in range(8)]
