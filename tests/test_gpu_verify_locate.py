"""GPU: zkt_verify_batch_locate.  The pairs of every proof and their tree from the device (zkt_debug_verify_batch_tree)
against the host entry that runs the same code on the CPU (zkt_debug_verify_locate_host), bit for bit; the verdicts
against zkt_verify per proof and zkt_verify_batch_dev per batch; the number of pairing checks against its bound; errors;
and that the call leaves a context's key, circuit and announced proof alone."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import fields as F, coracle as K

import verify_locate_cases as VC
import test_gpu_verify_batch as VB

CURVES = [F.BN254, F.BLS12_381]
IDS = lambda c: c.name  # noqa: E731


@pytest.fixture(scope="module")
def ctxs():
    import zkt_plonk_amd as z
    c = {cv.name: z.Context(cv.name, 0) for cv in CURVES}
    yield c
    for x in c.values():
        x.close()


# no inner level; an unpaired node on one level (3, 5, 33) and on several (67); 64 / 65: the last full wave and workgroup of the
# per-proof launches and one proof more (the per-term launch has its edges at every count here: 26 * count threads)
@pytest.mark.parametrize("count", [1, 2, 3, 5, 33, 64, 65, 67])
@pytest.mark.parametrize("cv", CURVES, ids=IDS)
def test_tree_is_the_host_entrys_bit_for_bit(ctxs, cv, count):
    ctx = ctxs[cv.name]
    made, srs, h, beta_h, wrong = VC._made(cv)
    entries, bad, (accepted, out_bad, n_checks, (nodes_h, inf_h, rho_h)) = VC.host_reference(cv, count)
    assert not accepted and set(np.flatnonzero(out_bad).tolist()) == bad
    nodes, inf, rho = ctx.debug_verify_batch_tree(VC._items(cv, entries), h, beta_h)
    assert np.array_equal(rho, rho_h)
    assert np.array_equal(inf, inf_h)
    assert np.array_equal(nodes, nodes_h)
    assert inf[1, 0] and not inf[0, 0]                               # proof 0 holds no commitment: Q_0 is the identity
    ab, ab_inf, rho_p = ctx.verify_batch_prepare_dev(VC._items(cv, entries), h, beta_h)
    assert np.array_equal(rho_p, rho)
    assert np.array_equal(ab, nodes[:, -1]) and ab_inf.tolist() == inf[:, -1].tolist()


LOCATE = [(1, ()), (1, (0,)), (3, ()), (3, (0,)), (3, (0, 1, 2)), (67, ()), (67, (0,)), (67, (66,)), (67, (32, 33)), (67, (0, 33, 66))]


@pytest.mark.parametrize("count,bad", LOCATE, ids=lambda v: str(v).replace(" ", ""))
@pytest.mark.parametrize("cv", CURVES, ids=IDS)
def test_locate_names_the_bad_proofs(ctxs, cv, count, bad):
    ctx = ctxs[cv.name]
    made, srs, h, beta_h, wrong = VC._made(cv)
    entries = VC.batch(cv, count, bad)
    want = [not VC.verdict(cv, e, beta_h) for e in entries]
    assert set(np.flatnonzero(want).tolist()) == set(bad)
    accepted, out_bad, n_checks = ctx.verify_batch_locate(VC._items(cv, entries), h, beta_h)
    assert out_bad.tolist() == want and accepted == (not bad)
    assert 1 <= n_checks <= VC.bound(count, len(bad))
    if accepted or count == 1:
        assert n_checks == 1
    assert ctx.verify_batch_dev(VC._items(cv, entries), h, beta_h) == accepted


@pytest.mark.parametrize("count", [1, 3, 67])
@pytest.mark.parametrize("cv", CURVES, ids=IDS)
def test_every_proof_is_bad_under_the_wrong_beta_h(ctxs, cv, count):
    ctx = ctxs[cv.name]
    made, srs, h, beta_h, wrong = VC._made(cv)
    entries = VC.batch(cv, count, ())
    accepted, out_bad, n_checks = ctx.verify_batch_locate(VC._items(cv, entries), h, wrong)
    assert not accepted and out_bad.all() and len(out_bad) == count
    assert n_checks <= VC.bound(count, count) and (count > 1 or n_checks == 1)
    assert not VC.verdict(cv, entries[0], wrong)
    assert not ctx.verify_batch_dev(VC._items(cv, entries), h, wrong)


@pytest.mark.parametrize("cv", CURVES, ids=IDS)
def test_errors(ctxs, cv):
    import zkt_plonk_amd as z
    from zkt_plonk_amd import _lib
    ctx = ctxs[cv.name]
    made, srs, h, beta_h, wrong = VC._made(cv)
    nb = (cv.fq.bits + 2 + 7) // 8
    L = z.lib()
    u = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))  # noqa: E731

    def call(entries, count=None):
        """the raw call with marked outputs -> (code, message, outputs untouched)"""
        ins, trs, k, hh, bh, keep = _lib._verify_batch_args(ctx.curve, VC._items(cv, entries), h, beta_h)
        ok, n_bad, n_chk = ctypes.c_int(7), ctypes.c_size_t(7), ctypes.c_size_t(7)
        bad = np.full(max(len(entries), 1), 7, dtype=np.uint8)
        rc = L.zkt_verify_batch_locate(ctx.handle, ins, trs, k if count is None else count, u(hh), u(bh), ctypes.byref(ok),
                                       bad.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), ctypes.byref(n_bad),
                                       ctypes.byref(n_chk))
        untouched = (ok.value, n_bad.value, n_chk.value) == (7, 7, 7) and (bad == 7).all()
        return rc, L.zkt_last_error(ctx.handle).decode(), untouched

    def with_proof(k, raw):
        return made[:k] + [made[k][:2] + (raw,) + made[k][3:]] + made[k + 1:]

    rc, msg, untouched = call(with_proof(2, made[2][2][:-1]))                       # truncated bytes
    assert rc == 1 and "proof 2" in msg and untouched
    raw = bytearray(made[1][2])
    raw[nb:2 * nb] = VB._off_curve_x(cv).to_bytes(nb, "little")                     # the b commitment of proof 1 off the curve
    rc, msg, untouched = call(with_proof(1, bytes(raw)))
    assert rc == 1 and "proof 1" in msg and "commitment 1" in msg and "curve" in msg and untouched
    rc, msg, untouched = call(made, count=0)
    assert rc == 1 and untouched
    rc, msg, untouched = call(made[:1], count=_lib.VERIFY_BATCH_DEV_MAX + 1)        # refused before any item is read
    assert rc == 1 and "ZKT_VERIFY_BATCH_DEV_MAX" in msg and untouched
    with pytest.raises(z.ZktError) as e:
        ctx.verify_batch_locate([], h, beta_h)
    assert e.value.code == 1
    with pytest.raises(z.ZktError) as e:
        ctx.debug_verify_batch_tree(VC._items(cv, with_proof(0, made[0][2][:-1])), h, beta_h)
    assert e.value.code == 1 and "proof 0" in str(e.value)
    accepted, out_bad, n_checks = ctx.verify_batch_locate(VC._items(cv, made), h, beta_h)   # none of it sticks
    assert accepted and not out_bad.any() and n_checks == 1


def test_an_announced_proof_keeps_its_bytes():
    """Prove, announce the next proof, locate the bad proof of a rejected batch on the same context, run the announced proof:
    its bytes are those of the proof made with nothing in between.  Once more on a forked context."""
    import zkt_plonk_amd as z
    cv = F.BN254
    made, _, h, beta_h, wrong = VC._made(cv)
    entries = VC.batch(cv, 5, (3,))
    cs, n, srs, pk, vk, blinders, want = VB._small_proof_setup(cv)
    ctx = z.Context(cv.name, 0)
    try:
        ctx.srs_load(srs)
        z.GpuProver(ctx, n.bit_length() - 1, {k: K.fr_to_mont(cv, pk.polys[k]) for k in z.PK_ORDER})
        a, b, c = cs.wire_evals(cs.n_gates)
        wires = [K.fr_to_mont(cv, w) for w in (a, b, c)]
        table = K.fr_to_mont(cv, cs.table)
        pi_pos = sorted(cs.pi)
        pi_vals = K.fr_to_mont(cv, [cs.pi[k] for k in pi_pos])

        def tr():
            return z.seed_transcript(z.Transcript("merlin", "ZKT Plonk"), vk.n, vk.commits)

        def round_trip(c):
            d = []
            for w in wires:
                d.append(c.alloc(w.nbytes))
                c.upload(d[-1], w)
            try:
                preps = [c.prepare_dev(d[0], d[1], d[2], cs.n_gates, table, pi_pos, pi_vals, K.fr_to_mont(cv, x)) for x in blinders]
                assert c.prove_prepared(preps[0], tr(), preps[1]) == want[0]        # proof 1 is announced
                accepted, out_bad, n_checks = c.verify_batch_locate(VC._items(cv, entries), h, beta_h)
                assert not accepted and np.flatnonzero(out_bad).tolist() == [3] and n_checks <= VC.bound(5, 1)
                assert c.prove_prepared(preps[1], tr()) == want[1]
            finally:
                for x in d:
                    c.free(x)

        round_trip(ctx)
        fork = ctx.fork()
        try:
            z.GpuProver(fork, n.bit_length() - 1)
            round_trip(fork)
        finally:
            fork.close()
        assert ctx.msm_info()["srs_count"] == n + 8                                 # under the key it was given
    finally:
        ctx.close()
