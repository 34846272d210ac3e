"""CPU pin of the Merkle-path cases (tests/merkle_path_cases.py): the layout the device kernel writes -- level k of a path at
base + k (6 + vars_per_hash), six select variables and then the hash's -- derived WITHOUT the composer from the select
formulas and gadget_trace, against the composer's own map; and PoseidonGadget.merkle_path's bookkeeping."""
import pytest

from oracle import composer as OC, fields as F

import merkle_path_cases as MC

CASES = [("bn254", 3, False) + MC.shapes(3)[0], ("bn254", 4, False) + MC.shapes(4)[1], ("bls12_381", 5, False) + MC.shapes(5)[3],
         ("bls12_381", 8, False) + MC.shapes(8)[4], ("bn254", 4, False) + MC.shapes(4)[2], ("bn254", 4, True, 2, 2, "mixed", False, False)]


@pytest.mark.parametrize("args", CASES, ids=lambda a: "%s-x%d-%s-h%d-b%d-%s-%s" % (a[0], a[1], "shipped" if a[2] else "syn", a[3],
                                                                                  a[4], a[5], "dense" if a[6] else "scattered"))
def test_derived_levels_equal_the_composers_map(args):
    case = MC.build(*args)
    S = case.per_level
    assert S == 6 + case.prm.gates_per_hash and case.span == case.height * S and len(case.values) == case.n_vars
    written = set()
    for pth in range(case.batch):
        want, root = MC.derive_path(case, pth)
        b = case.bases[pth]
        assert case.values[b:b + case.span] == want, pth
        assert root == case.roots[pth] == case.values[case.root_vars[pth]]
        assert case.root_vars[pth] == b + (case.height - 1) * S + 6 + case.hash_var_offset
        for k in range(case.height):              # the hash of level k takes z_l and z_r: the variables 4 and 1 in front of it
            lvl = b + k * S
            assert case.values[lvl + 6:lvl + S] == OC.gadget_trace(case.prm, [case.values[lvl + 2], case.values[lvl + 5]])
        assert not written & set(range(b, b + case.span))
        written |= set(range(b, b + case.span))
    ins = [v for pth in range(case.batch) for v in [case.leaf[pth]] + case.bits[pth] + case.sibs[pth] if v != MC.ZERO]
    assert not written & set(ins) and all(v < case.n_vars for v in ins)
    if case.dense:
        assert case.bases == [case.bases[0] + k * case.span for k in range(case.batch)]
    if args[7]:
        assert case.leaf[0] == MC.ZERO and MC.ZERO in case.sibs[-1]


def test_the_cases_cover_every_bit_pattern_and_both_base_forms():
    for w in (3, 4, 5, 8):
        sh = MC.shapes(w)
        assert {s[0] for s in sh} == {1, 2, 3, 7}
        assert {s[1] for s in sh} == {1, MC.per_wave(w) + 1, 4 * MC.per_wave(w) + 1}
        assert {s[2] for s in sh} == {"zeros", "ones", "mixed"} and {s[3] for s in sh} == {True, False}
    assert [MC.lanes_per_hash(w) for w in (3, 4, 5, 8)] == [16, 16, 32, 64]
    case = MC.build("bn254", 4, False, *MC.shapes(4)[3])
    vals = {tuple(case.value(b) for b in bits) for bits in case.bits}
    assert any(0 in v and 1 in v for v in vals)


def test_the_withdraw_circuits_path_levels_are_the_hashes_fed_by_the_two_selects():
    """In WithdrawCircuit the levels of merkle_proof are exactly the hash calls whose inputs are the variables 4 and 1 in
    front of their trace (z_l and z_r), consecutive levels S apart: what the end-to-end device test relies on."""
    cv = F.BN254
    prm = MC.synthetic_params(cv, 4)
    cs, _ = OC.withdraw_instance(cv, prm, inputs=2, height=3, seed=3)
    S = 6 + prm.gates_per_hash
    levels = [base for base, ins in cs.hash_calls if [v for v, _, _ in ins] == [base - 4, base - 1]]
    assert len(levels) == 2 * 3 and len(cs.hash_calls) == 2 * (3 + 3) + 2
    for first in (levels[0], levels[3]):
        assert [first, first + S, first + 2 * S] == levels[levels.index(first):levels.index(first) + 3]


def test_gadget_refuses_what_one_path_launch_cannot_order():
    """PoseidonGadget.merkle_path's bookkeeping needs no device: the checks run on the recorded indices."""
    from zkt_plonk_amd.poseidon import PoseidonGadget, VARIABLE_ZERO
    g = PoseidonGadget.__new__(PoseidonGadget)
    g.width, g.vars_per_hash, g.vars_per_level = 4, 100, 106
    g.hash_var_offset = 100 - 1 - 2 * 4
    g.calls, g.paths = [], []
    root = g.merkle_path(1000, 3, [4, 5], [6, VARIABLE_ZERO])
    assert root == 1000 + 106 + 6 + g.hash_var_offset
    g.hash(2000, [7, 1])
    g._check_paths()
    g.hash(3000, [root])                                   # a hash fed by the root
    with pytest.raises(ValueError):
        g._check_paths()
    g.calls.pop()
    g.merkle_path(5000, 1000 + 2, [4], [6])                # a leaf another path makes
    with pytest.raises(ValueError):
        g._check_paths()
    g.paths.pop()
    g.merkle_path(5000, 3, [4], [1000 + 2 * 106 - 1])      # a sibling another path makes (its last variable)
    with pytest.raises(ValueError):
        g._check_paths()
    g.paths.pop()
    g.merkle_path(5000, 3, [4], [1000 + 2 * 106])          # the first variable behind it is free
    g._check_paths()
    with pytest.raises(ValueError):
        g.merkle_path(7000, 3, [4, 5], [6])                # one sibling per bit
    g.width = 2
    with pytest.raises(ValueError):
        g.merkle_path(7000, 3, [4], [6])                   # hash_two does not fit width 2
    assert g.levels() == [[0]]                             # hash calls are grouped as before
