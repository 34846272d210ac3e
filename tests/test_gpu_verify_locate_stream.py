"""GPU: zkt_verify_batch_locate and zkt_debug_verify_batch_tree on a stream the CALLER owns and keeps busy, through the rig
of tests/test_gpu_caller_stream.py (tests/stream_rig.py): a bounded spin and a marker event on the context's stream, then
the call at once.  The call synchronises, so it must be ENTERED while the marker is pending; everything it puts on the
stream -- the decompression, the two MSMs, and for a rejected batch a device-to-device copy when the scratch grows, three
uploads, the leaf and level launches and the download of the tree -- then runs behind the caller's work.  held == idle ==
the host entry, exactly.  The inputs are host memory: there is no decoy to write behind the hold."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import fields as F

import verify_locate_cases as VC

CURVES = [F.BN254, F.BLS12_381]


@pytest.fixture(scope="module")
def rigs():
    import torch
    import zkt_plonk_amd as z
    import stream_rig as R
    made = {}
    for cv in CURVES:
        rig = R.Rig(z.Context(cv.name, 0), torch.cuda.Stream())
        if made:
            rig.share_calibration(next(iter(made.values())))
        else:
            rig.calibrate()
        made[cv.name] = rig
    yield made
    for rig in made.values():
        rig.ctx.close()


@pytest.mark.parametrize("cv", CURVES, ids=lambda c: c.name)
def test_locate_on_a_held_stream(rigs, cv):
    """Five proofs accepted; five with proof 3 bad; 33 with proofs 2 and 31 bad.  Then once more, held only, with 65 proofs:
    more scratch than anything before it on this context, so the copy that keeps the decompressed commitments while the
    scratch grows happens behind the hold as well."""
    import stream_rig as R
    rig = rigs[cv.name]
    ctx = rig.ctx
    made, srs, h, beta_h, wrong = VC._made(cv)
    cases = [(5, ()), (5, (3,)), (33, (2, 31))]
    batches = [VC.batch(cv, count, bad) for count, bad in cases]

    def body(m, data):
        out = []
        for entries in batches:
            m.begin()
            out.append(m.blocking("zkt_verify_batch_locate", ctx.verify_batch_locate, VC._items(cv, entries), h, beta_h))
        return out

    decoy, idle, held = rig.three_ways(body, [], [], [])
    assert held == idle == decoy
    for (count, bad), (accepted, out_bad, n_checks) in zip(cases, held):
        assert accepted == (not bad)
        assert np.flatnonzero(np.frombuffer(out_bad, dtype=np.bool_)).tolist() == list(bad)
        assert n_checks <= VC.bound(count, len(bad)) and (bad or n_checks == 1)
    items = VC._items(cv, VC.batch(cv, 65, (0, 64)))
    m = R._Mode(rig, True)
    m.begin()
    accepted, out_bad, n_checks = m.blocking("zkt_verify_batch_locate, growing", ctx.verify_batch_locate, items, h, beta_h)
    m.finish()
    assert not accepted and np.flatnonzero(out_bad).tolist() == [0, 64] and n_checks <= VC.bound(65, 2)


@pytest.mark.parametrize("cv", CURVES, ids=lambda c: c.name)
def test_tree_on_a_held_stream(rigs, cv):
    """The tree of a mixed batch of 33 built behind the hold: every node is the host entry's."""
    rig = rigs[cv.name]
    ctx = rig.ctx
    made, srs, h, beta_h, wrong = VC._made(cv)
    entries, bad, (accepted, out_bad, n_checks, want) = VC.host_reference(cv, 33)

    def body(m, data):
        m.begin()
        return m.blocking("zkt_debug_verify_batch_tree", ctx.debug_verify_batch_tree, VC._items(cv, entries), h, beta_h)

    import stream_rig as R
    decoy, idle, held = rig.three_ways(body, [], [], [])
    assert held == idle == R.norm(want)
