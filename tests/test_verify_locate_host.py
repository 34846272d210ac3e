"""CPU: zkt_debug_verify_locate_host, the whole of zkt_verify_batch_locate on the host with the leaves and the levels
of its tree computed by the code the kernels run (csrc/verify_leaves.hpp): verdicts against zkt_verify per proof, the
number of pairing checks against its bound, and every node of the tree against the host verifier's own arithmetic
(zkt_verify_prepare, zkt_g1_msm_host, zkt_g1_sum_host).  Proofs of the CPU oracle, both curves, Merlin transcripts and
the Ethereum transcript on BN254."""
import numpy as np
import pytest

from oracle import fields as F

import verify_locate_cases as VC

CURVES = [F.BN254, F.BLS12_381]
IDS = lambda c: c.name  # noqa: E731


def _bad_sets(count):
    sets = [(), (0,), (count - 1,), (0, 1), (2, 3)]
    return sorted({s for s in sets if all(i < count for i in s)})


CASES = [(count, bad) for count in (1, 2, 3, 5, 33) for bad in _bad_sets(count)] + [(3, (0, 1, 2))]


@pytest.mark.parametrize("cv", CURVES, ids=IDS)
def test_the_host_verifier_takes_every_bad_proof_without_an_error(cv):
    made, srs, h, beta_h, wrong = VC._made(cv)
    for kind in VC.KINDS:
        for e in made:
            bad = kind(cv, e)
            VC.pairs(cv, bad)                                    # zkt_verify_prepare: no error
            assert not VC.verdict(cv, bad, beta_h), kind.__name__
    for a, b in ((made[0], made[2]), (made[0], made[1])):
        for e in VC.swapped(a, b):
            VC.pairs(cv, e)
            assert not VC.verdict(cv, e, beta_h)
    for e in made:
        assert VC.verdict(cv, e, beta_h) and not VC.verdict(cv, e, wrong)
    # the identity cases are what they are meant to be: Q_i = 0 without witnesses
    _, inf = VC.pairs(cv, VC.witnesses_identity(cv, made[0]))
    assert inf.tolist() == [False, True, False, True]


def _run(cv, entries, beta_h):
    from zkt_plonk_amd import _lib
    h = VC._made(cv)[2]
    accepted, bad, n_checks, tree = _lib.debug_verify_locate_host(cv.name, VC._items(cv, entries), h, beta_h)
    want = [not VC.verdict(cv, e, beta_h) for e in entries]
    assert bad.tolist() == want
    assert accepted == (not any(want))
    assert 1 <= n_checks <= VC.bound(len(entries), sum(want))
    if accepted or len(entries) == 1:
        assert n_checks == 1
    return tree


@pytest.mark.parametrize("count,bad", CASES, ids=lambda v: str(v).replace(" ", ""))
@pytest.mark.parametrize("cv", CURVES, ids=IDS)
def test_verdicts_checks_and_tree(cv, count, bad):
    made, srs, h, beta_h, wrong = VC._made(cv)
    entries = VC.batch(cv, count, bad)
    VC.check_tree(cv, entries, _run(cv, entries, beta_h))


@pytest.mark.parametrize("cv", CURVES, ids=IDS)
def test_every_proof_is_bad_under_the_wrong_beta_h(cv):
    made, srs, h, beta_h, wrong = VC._made(cv)
    entries = VC.batch(cv, 3, ())
    VC.check_tree(cv, entries, _run(cv, entries, wrong))


@pytest.mark.parametrize("cv", CURVES, ids=IDS)
def test_every_kind_of_bad_proof_and_the_identity_flags(cv):
    made, srs, h, beta_h, wrong = VC._made(cv)
    entries, bad = VC.mixed_batch(cv, 8)
    assert bad == {0, 1, 2, 3, 4, 6, 7}
    nodes, inf, rho = tree = _run(cv, entries, beta_h)
    VC.check_tree(cv, entries, tree)
    # proof 1 has no witnesses: its Q is the identity; proof 0 has no commitment at all, its P is made of the key's points;
    # node 8 is the parent of leaves 0 and 1
    assert not inf[0].any() and np.flatnonzero(inf[1]).tolist() == [0, 1, 8]


def test_arguments_are_checked_and_outputs_stay_untouched_on_an_error():
    import ctypes
    from zkt_plonk_amd import _lib
    cv = F.BN254
    made, srs, h, beta_h, wrong = VC._made(cv)
    L = _lib.lib()
    u = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))  # noqa: E731
    truncated = [made[0], made[1][:2] + (made[1][2][:-1],) + made[1][3:]]
    for entries, count in ((made, 0), (made, _lib.VERIFY_BATCH_DEV_MAX + 1), (truncated, 2)):
        ins, trs, k, hh, bh, keep = _lib._verify_batch_args(_lib.curve_id(cv.name), VC._items(cv, entries), h, beta_h)
        ok, nb, nc = ctypes.c_int(7), ctypes.c_size_t(7), ctypes.c_size_t(7)
        bad = np.full(4, 7, dtype=np.uint8)
        rc = L.zkt_debug_verify_locate_host(_lib.curve_id(cv.name), ins, trs, count, u(hh), u(bh), ctypes.byref(ok),
                                            bad.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), ctypes.byref(nb), ctypes.byref(nc),
                                            None, None, None)
        assert rc == 1
        assert (ok.value, nb.value, nc.value) == (7, 7, 7) and bad.tolist() == [7] * 4
