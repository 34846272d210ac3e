"""GPU: zkt_verify_batch_dev under zkt_ctx_set_verify_terms(ctx, 1) on a stream the CALLER owns and keeps busy, through
the rig of tests/test_gpu_caller_stream.py (tests/stream_rig.py): a bounded spin and a marker event on the context's
stream, then the call at once.  The call synchronises, so it must be ENTERED while the marker is pending; the
decompression, the term kernel behind it, their copies and the two MSMs then run behind the caller's work.
held == idle == what the call gives under mode 0.  The inputs are host memory: there is no decoy to write behind the hold."""
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
def test_verify_batch_dev_under_mode_1_on_a_held_stream(rigs, cv):
    """Five proofs accepted; five with proof 3 bad; 67 accepted; 67 under another trapdoor."""
    rig = rigs[cv.name]
    ctx = rig.ctx
    made, srs, h, beta_h, wrong = VC._made(cv)
    cases = [(VC.batch(cv, 5, ()), beta_h), (VC.batch(cv, 5, (3,)), beta_h), (VC.batch(cv, 67, ()), beta_h),
             (VC.batch(cv, 67, ()), wrong)]
    ctx.set_verify_terms(0)
    want = [ctx.verify_batch_dev(VC._items(cv, entries), h, bh) for entries, bh in cases]
    assert want == [True, False, True, False]
    ctx.set_verify_terms(1)

    def body(m, data):
        out = []
        for entries, bh in cases:
            items = VC._items(cv, entries)                   # fresh transcripts, seeded before the hold starts
            m.begin()
            out.append(m.blocking("zkt_verify_batch_dev", ctx.verify_batch_dev, items, h, bh))
        return out

    decoy, idle, held = rig.three_ways(body, [], [], [])
    assert held == idle == decoy == tuple(want)
