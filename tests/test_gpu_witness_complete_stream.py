"""GPU: zkt_witness_complete_enqueue on a stream the CALLER owns and keeps busy, through the rig of
tests/test_gpu_caller_stream.py (tests/stream_rig.py): a bounded spin and a marker event on the context's stream, then the
caller's kernel that writes the real free variables over a decoy witness, and the call at once.  The call is enqueue-only: it
must RETURN while the marker is pending, and the map and the public inputs must be those of the real witness afterwards."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import coracle as K, plonk as P

import witness_plan_cases as W


def test_witness_complete_enqueue_on_a_held_stream():
    import torch
    import zkt_plonk_amd as z
    import stream_rig as R
    c = W.withdraw("bn254", "synthetic", 1)[0]
    decoy_c = W.withdraw("bn254", "synthetic", 2)[0]
    assert W.same_circuit(c, decoy_c)
    pl = W.plan(c)
    cv = c.cv
    rig = R.Rig(z.Context(cv.name, 0), torch.cuda.Stream())
    ctx = rig.ctx
    plan = None
    try:
        be = K.CBackend(cv, K.srs_mont(cv, 3, 2))
        ev = P.setup_evals(be, c.cs)
        ctx.circuit_load(c.log_n, [W.mont(cv, be.ifft(1 << c.log_n, ev[k])) for k in z.PK_ORDER])
        plan = z.WitnessPlan(ctx, c.idx(0), c.idx(1), c.idx(2), c.n_vars, c.pi_pos)
        stride = c.n_vars + 1
        real = W.prefill(c, pl, c.values, stride)
        decoy = W.prefill(c, pl, decoy_c.values, stride, salt=5)
        want_map, want_pi, status = W.complete(c, pl, real)
        assert status == (0, W.NONE) and want_map[:c.n_vars] == c.values
        d_vars = R.dev(np.zeros((stride, 4), dtype=np.uint64))
        d_pi = R.dev(np.zeros((len(c.pi_pos), 4), dtype=np.uint64))

        def body(m, data):
            m.begin([(d_vars, data[0])])
            m.enqueue("zkt_witness_complete_enqueue", plan.complete_dev, d_vars.data_ptr(), stride, 1, d_pi.data_ptr())
            return m.consume(d_vars), m.consume(d_pi)

        results = rig.three_ways(body, [d_vars], [R.dev(W.mont(cv, decoy))], [R.dev(W.mont(cv, real))], outs=[d_pi])
        R.compare("zkt_witness_complete_enqueue", results, (W.mont(cv, want_map), W.mont(cv, want_pi)))
        assert plan.status(1) == [(0, None)]
    finally:
        if plan is not None:
            plan.close()
        ctx.close()
