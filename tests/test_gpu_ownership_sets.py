"""What a context owns alone goes back with its owner (csrc/ctx.hpp DevSet): a refused circuit load leaves nothing behind, a
context that is reloaded returns what the previous key and circuit took, and the side states (the KZG seam's, the
variable-base MSM's, the key check's) go with their context, forks included.  Measured with zkt_debug_live_allocations,
which sees device memory only; that streams, events and pinned memory travel with the same set is the type's guarantee.

Circuits of n = 16 and n = 32 under keys of n + 8 powers on both curves, on the routes that make every table group
(test_gpu_fork_ownership.Rig.root).  Every proof is compared byte for byte with the oracle's."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import coracle as K

import srs_check_cases as SC
from test_gpu_fork_ownership import CURVES, Rig, _live, fx  # noqa: F401  (fx: the module's fixture)

A_N, B_N = 16, 32
ERR_INVALID_ARGUMENT = 1


def _routes(z, cv):
    """a context on the routes Rig.root sets, with nothing loaded"""
    ctx = z.Context(cv.name, 0)
    ctx.set_quotient_route(1)
    ctx.set_wire_elimination(2)
    return ctx


@pytest.mark.parametrize("n", [A_N, B_N])
@pytest.mark.parametrize("cv", CURVES, ids=lambda c: c.name)
def test_refused_loads_leave_nothing(cv, n, fx):
    """A load that is refused after its work set was made (q_m longer than n) gives everything back: repeating it does
    not grow the library's device memory, the context then loads and proves, and closing it leaves what was there before."""
    import zkt_plonk_amd as z
    f = fx(cv, n)
    rig = Rig(z, cv)
    ctx = None
    try:
        rig.witness(f)
        before = _live()
        ctx = _routes(z, cv)
        ctx.srs_load(f.srs)
        too_long = np.zeros((n + 1, 4), dtype=np.uint64)
        polys = [too_long if k == "q_m" else f.pkm[k] for k in z.PK_ORDER]
        evals = {k: too_long if k == "q_m" else np.zeros((n, 4), dtype=np.uint64) for k in z.PK_ORDER}
        for what, call in (("circuit_load", lambda: ctx.circuit_load(f.log_n, polys)),
                           ("GpuProver.setup", lambda: z.GpuProver.setup(ctx, f.log_n, evals))):
            live = []
            for _ in range(3):
                with pytest.raises(z.ZktError) as e:
                    call()
                assert e.value.code == ERR_INVALID_ARGUMENT, what
                live.append(_live())
            print("%s n=%d %s: live (count, bytes) before the context %s, after each refusal %s" % (cv.name, n, what, before, live))
            assert live[1] == live[0] and live[2] == live[0], (what, "a refused load left device memory behind", live)
        rig.load(ctx, f)
        rig.prove(ctx, f, "after the refused loads")
        ctx.close()
        ctx = None
        assert _live() == before, "device allocations (count, bytes) left behind by the context"
    finally:
        if ctx is not None:
            ctx.close()
        rig.data.close()


@pytest.mark.parametrize("cv", CURVES, ids=lambda c: c.name)
def test_reloading_returns_what_it_took(cv, fx):
    """One context goes A B A B A (key + circuit at n = 16, then at n = 32, ...), a proof at every step.  From step 2 on the
    scratch is at its largest and both sizes' NTT plans exist, so what is alive after a step depends on the step's
    size alone: every reload released exactly what the load before it took."""
    import zkt_plonk_amd as z
    fa, fb = fx(cv, A_N), fx(cv, B_N)
    rig = Rig(z, cv)
    ctx = None
    try:
        rig.witness(fa)
        rig.witness(fb)
        before = _live()
        ctx = _routes(z, cv)
        live = []
        for step, f in enumerate((fa, fb, fa, fb, fa), 1):
            rig.load(ctx, f)
            rig.prove(ctx, f, "step %d (n = %d)" % (step, f.n))
            live.append(_live())
        print("%s: live (count, bytes) after steps 1..5 %s" % (cv.name, live))
        assert live[2] == live[4], ("A: step 3 against step 5", live)
        assert live[1] == live[3], ("B: step 2 against step 4", live)
        ctx.close()
        ctx = None
        assert _live() == before, "device allocations (count, bytes) left behind by the context"
    finally:
        if ctx is not None:
            ctx.close()
        rig.data.close()


def _side_calls(ctx, cv, f, g2):
    """zkt_kzg_open, zkt_kzg_commit_batch, zkt_msm_g1_bases and zkt_srs_check once each: every side state of `ctx` exists"""
    rng = np.random.default_rng(f.n)
    polys = [K.fr_to_mont(cv, [int(x) for x in rng.integers(1, 1 << 62, size=m)]) for m in (1, 2, f.n + 8)]
    got = ctx.kzg_commit_batch(polys)
    for p, (xy, inf) in zip(polys, got):
        want_xy, want_inf = K.msm_mont(cv, f.srs[:p.shape[0]], p)
        assert inf == want_inf and np.array_equal(xy, want_xy)
    ch, zm = polys[2][:3], polys[1][0]
    (w, inf), ev = ctx.kzg_open(polys, ch, zm)
    assert np.array_equal(ev, np.array([K.poly_eval(cv, p, zm) for p in polys], dtype=np.uint64).reshape(-1, 4))
    xy, inf = ctx.msm_bases(f.srs[:1], polys[0])
    want_xy, want_inf = K.msm_mont(cv, f.srs[:1], polys[0])
    assert inf == want_inf and np.array_equal(xy, want_xy)
    h, bh = g2
    assert ctx.srs_check(SC.key(cv)[:1], h, bh, SC.SEED_A).ok


@pytest.mark.parametrize("cv", CURVES, ids=lambda c: c.name)
def test_side_states_go_with_their_context(cv, fx):
    """The scratch of the KZG seam, of zkt_msm_g1_bases and of zkt_srs_check belongs to its state: closing the context, or
    a fork before its parent, returns the library's device memory to what it was before the context existed."""
    import zkt_plonk_amd as z
    from zkt_plonk_amd import _lib
    f = fx(cv, A_N)
    g2 = _lib.srs_generate_g2(cv.name, SC.TAU)
    before = _live()
    ctx = z.Context(cv.name, 0)
    try:
        ctx.srs_load(f.srs)
        _side_calls(ctx, cv, f, g2)
    finally:
        ctx.close()
    assert _live() == before, "a context's side states left device memory behind"
    parent = z.Context(cv.name, 0)
    fork = None
    try:
        parent.srs_load(f.srs)
        fork = parent.fork()
        _side_calls(fork, cv, f, g2)
        fork.close()
        fork = None
    finally:
        if fork is not None:
            fork.close()
        parent.close()
    assert _live() == before, "a fork's side states left device memory behind"
