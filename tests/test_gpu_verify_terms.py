"""GPU: the batch verifier's transcripts and scalar stage on the device (csrc/verify_terms.hip,
zkt_ctx_set_verify_terms(ctx, 1)).  The kernel (zkt_debug_verify_terms route 2) against the existing host code (route 0)
over the table of tests/verify_terms_cases.py, integer for integer, at counts around a wave; then the four batch calls
under mode 1 against themselves under mode 0: results, refusals, and where the transcript handles are left."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import fields as F, coracle as K

import test_gpu_verify_batch as VB
import verify_locate_cases as VC
import verify_terms_cases as TC

CURVES = [F.BN254, F.BLS12_381]
IDS = lambda c: c.name  # noqa: E731


@pytest.fixture(scope="module")
def ctxs():
    """Per curve a context under mode 0 and one under mode 1; neither holds a key or a circuit."""
    import zkt_plonk_amd as z
    made = {}
    for cv in CURVES:
        made[cv.name] = (z.Context(cv.name, 0), z.Context(cv.name, 0))
        made[cv.name][1].set_verify_terms(1)
    yield made
    for pair in made.values():
        for c in pair:
            c.close()


def _kernel_and_host(ctx, cv, rows, rho):
    """-> route 0's result after checking that the kernel's and the probes of the handles are equal"""
    forced = TC.forced_array(cv, rows)
    out, left = [], []
    for route in (0, 2):
        its = TC.items(cv, rows)
        out.append(ctx.debug_verify_terms(its, rho, forced, route))
        left.append(TC.probes(its))
    for name, a, b in zip(("challenges", "r0", "sums", "status"), out[0], out[1]):
        assert np.array_equal(a, b), name
    assert left[0] == left[1]
    return out[0]


@pytest.mark.parametrize("count", [1, 3, 64, 65, 67])
@pytest.mark.parametrize("cv", CURVES, ids=IDS)
def test_the_kernel_equals_the_host_code(ctxs, cv, count):
    """one lane, a few, a full wave, one past it, and the locate tests' odd count; the whole table is in from 22 on"""
    rows = TC.cycle(TC.ROWS(cv), count)
    ch, r0, acc, status = _kernel_and_host(ctxs[cv.name][0], cv, rows, TC.rho_array(cv, count))
    assert not status.any() and acc.reshape(count, -1).any(axis=1).all()


@pytest.mark.parametrize("cv", CURVES, ids=IDS)
def test_the_table_alone_and_without_coefficients(ctxs, cv):
    rows = list(TC.ROWS(cv))
    assert not _kernel_and_host(ctxs[cv.name][0], cv, rows, None)[3].any()


@pytest.mark.parametrize("cv", CURVES, ids=IDS)
def test_forced_refusals_and_edge_points(ctxs, cv):
    rows, want = TC.FORCED(cv)
    assert _kernel_and_host(ctxs[cv.name][0], cv, list(rows), TC.rho_array(cv, len(rows), seed=6))[3].tolist() == list(want)
    rows, want = TC.two_refusals(cv)
    status = _kernel_and_host(ctxs[cv.name][0], cv, list(rows), None)[3]
    assert status.tolist() == list(want) and np.flatnonzero(status).tolist() == [5, 9]


@pytest.mark.parametrize("cv", CURVES, ids=IDS)
def test_the_batch_calls_do_not_depend_on_the_mode(ctxs, cv):
    host, dev = ctxs[cv.name]
    made, srs, h, beta_h, wrong = VC._made(cv)
    # A, B, flags and coefficients; the handles afterwards
    for count in (1, 3, 67):
        entries = VB._cycle(made, count)
        got = []
        for ctx in (host, dev):
            its = VC._items(cv, entries)
            got.append(ctx.verify_batch_prepare_dev(its, h, beta_h) + (TC.probes(its),))
        (ab0, inf0, rho0, left0), (ab1, inf1, rho1, left1) = got
        assert np.array_equal(ab0, ab1) and inf0.tolist() == inf1.tolist() and np.array_equal(rho0, rho1) and left0 == left1
    # verdicts: a good batch, one with a flipped evaluation byte
    good, bad = VC.batch(cv, 67, ()), VC.batch(cv, 67, (33,))
    bad[33] = VC.flipped(cv, VB._cycle(made, 67)[33])
    for ctx in (host, dev):
        assert ctx.verify_batch_dev(VC._items(cv, good), h, beta_h)
        assert not ctx.verify_batch_dev(VC._items(cv, bad), h, beta_h)
        assert not ctx.verify_batch_dev(VC._items(cv, good), h, wrong)
    # locating, and the tree
    for count, where in ((5, (3,)), (33, (2, 31)), (67, ())):
        entries = VC.batch(cv, count, where)
        a0, bad0, n0 = host.verify_batch_locate(VC._items(cv, entries), h, beta_h)
        a1, bad1, n1 = dev.verify_batch_locate(VC._items(cv, entries), h, beta_h)
        assert (a0, bad0.tolist(), n0) == (a1, bad1.tolist(), n1) and np.flatnonzero(bad1).tolist() == list(where)
    entries, _ = VC.mixed_batch(cv, 33)
    t0 = host.debug_verify_batch_tree(VC._items(cv, entries), h, beta_h)
    t1 = dev.debug_verify_batch_tree(VC._items(cv, entries), h, beta_h)
    assert all(np.array_equal(x, y) for x, y in zip(t0, t1))


def _raw_prepare(ctx, cv, its, h, beta_h):
    """zkt_verify_batch_prepare_dev -> (code, message)"""
    import zkt_plonk_amd as z
    from zkt_plonk_amd import _lib
    L = z.lib()
    u = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))  # noqa: E731
    ins, trs, k, hh, bh, keep = _lib._verify_batch_args(ctx.curve, its, h, beta_h)
    ab = np.zeros((2, 2 * ctx.fq_limbs), dtype=np.uint64)
    rc = L.zkt_verify_batch_prepare_dev(ctx.handle, ins, trs, k, u(hh), u(bh), u(ab), None, None)
    return rc, L.zkt_last_error(ctx.handle).decode()


@pytest.mark.parametrize("cv", CURVES, ids=IDS)
def test_refusals_name_the_lowest_proof_and_leave_the_handles_alone(ctxs, cv):
    host, dev = ctxs[cv.name]
    made, srs, h, beta_h, wrong = VC._made(cv)
    rows = list(TC.two_natural_refusals(cv))
    fresh = TC.probes(TC.items(cv, rows))
    its0, its1 = TC.items(cv, rows), TC.items(cv, rows)
    rc0, msg0 = _raw_prepare(host, cv, its0, h, beta_h)
    rc1, msg1 = _raw_prepare(dev, cv, its1, h, beta_h)
    assert rc0 == rc1 == TC.ZERO_DENOMINATOR and msg0 == msg1 and "proof 5:" in msg1 and "denominator" in msg1
    assert TC.probes(its1) == fresh                          # on an error no state is written back
    assert TC.probes(its0)[:5] != fresh[:5]                  # (the serial loop had consumed the proofs in front)
    # a refused commitment comes before any term refusal, whatever the indices: proof 7's b is off the curve
    nb = TC._nb(cv)
    raw = bytearray(rows[7].entry[4])
    raw[nb:2 * nb] = VB._off_curve_x(cv).to_bytes(nb, "little")
    rows[7] = rows[7]._replace(name=rows[7].name + "_off_curve", entry=rows[7].entry[:4] + (bytes(raw),) + rows[7].entry[5:])
    its0, its1 = TC.items(cv, rows), TC.items(cv, rows)
    rc0, msg0 = _raw_prepare(host, cv, its0, h, beta_h)
    rc1, msg1 = _raw_prepare(dev, cv, its1, h, beta_h)
    assert rc0 == rc1 == 1 and msg0 == msg1 and "proof 7" in msg1 and "commitment 1" in msg1
    assert TC.probes(its1) == TC.probes(TC.items(cv, rows))
    # truncated bytes: stage 1's own refusal
    rows[2] = rows[2]._replace(name=rows[2].name + "_short", entry=rows[2].entry[:4] + (rows[2].entry[4][:-1],) + rows[2].entry[5:])
    assert _raw_prepare(host, cv, TC.items(cv, rows), h, beta_h) == _raw_prepare(dev, cv, TC.items(cv, rows), h, beta_h)
    assert dev.verify_batch_dev(VC._items(cv, made), h, beta_h)                         # none of it sticks


def test_the_switch_a_fork_and_the_allocations():
    import zkt_plonk_amd as z
    from zkt_plonk_amd import _lib
    cv = F.BN254
    made, srs, h, beta_h, wrong = VC._made(cv)
    rows = list(TC.two_natural_refusals(cv))
    fresh = TC.probes(TC.items(cv, rows))
    before = _lib.debug_live_allocations()
    ctx = z.Context(cv.name, 0)
    try:
        for mode in (2, -1, 3):
            with pytest.raises(z.ZktError) as e:
                ctx.set_verify_terms(mode)
            assert e.value.code == 1
        its = TC.items(cv, rows)                             # still mode 0: the loop consumes what it passes
        assert _raw_prepare(ctx, cv, its, h, beta_h)[0] == TC.ZERO_DENOMINATOR and TC.probes(its)[:5] != fresh[:5]
        ctx.set_verify_terms(1)
        fork = ctx.fork()
        try:
            ctx.set_verify_terms(0)                          # the fork keeps what it inherited
            its = TC.items(cv, rows)
            assert _raw_prepare(fork, cv, its, h, beta_h)[0] == TC.ZERO_DENOMINATOR and TC.probes(its) == fresh
            fork.profile_enable(True)
            assert fork.verify_batch_dev(VC._items(cv, VB._cycle(made, 67)), h, beta_h)
            assert fork.profile_get("verify_terms")[0] == 1
            accepted, bad, n_checks = fork.verify_batch_locate(VC._items(cv, VC.batch(cv, 33, (2, 31))), h, beta_h)
            assert not accepted and np.flatnonzero(bad).tolist() == [2, 31]
        finally:
            fork.close()
        assert _lib.debug_live_allocations()[0] > before[0]
    finally:
        ctx.close()
    assert _lib.debug_live_allocations() == before


def test_an_announced_proof_keeps_its_bytes_across_a_mode_1_call():
    """Prove, announce the next proof, verify a batch under mode 1 on the same context, run the announced proof: its bytes
    are those of the proof made with nothing in between."""
    import zkt_plonk_amd as z
    cv = F.BN254
    made, _, h, beta_h, wrong = VC._made(cv)
    entries = VC.batch(cv, 5, (3,))
    cs, n, srs, pk, vk, blinders, want = VB._small_proof_setup(cv)
    ctx = z.Context(cv.name, 0)
    try:
        ctx.set_verify_terms(1)
        ctx.srs_load(srs)
        z.GpuProver(ctx, n.bit_length() - 1, {k: K.fr_to_mont(cv, pk.polys[k]) for k in z.PK_ORDER})
        a, b, c = cs.wire_evals(cs.n_gates)
        wires = [K.fr_to_mont(cv, w) for w in (a, b, c)]
        table = K.fr_to_mont(cv, cs.table)
        pi_pos = sorted(cs.pi)
        pi_vals = K.fr_to_mont(cv, [cs.pi[k] for k in pi_pos])

        def tr():
            return z.seed_transcript(z.Transcript("merlin", "ZKT Plonk"), vk.n, vk.commits)

        d = []
        for w in wires:
            d.append(ctx.alloc(w.nbytes))
            ctx.upload(d[-1], w)
        try:
            preps = [ctx.prepare_dev(d[0], d[1], d[2], cs.n_gates, table, pi_pos, pi_vals, K.fr_to_mont(cv, x)) for x in blinders]
            assert ctx.prove_prepared(preps[0], tr(), preps[1]) == want[0]            # proof 1 is announced
            assert ctx.verify_batch_dev(VC._items(cv, made), h, beta_h)
            accepted, out_bad, n_checks = ctx.verify_batch_locate(VC._items(cv, entries), h, beta_h)
            assert not accepted and np.flatnonzero(out_bad).tolist() == [3]
            assert ctx.prove_prepared(preps[1], tr()) == want[1]
        finally:
            for x in d:
                ctx.free(x)
    finally:
        ctx.close()
