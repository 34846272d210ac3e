"""GPU: zkt_g1_check and zkt_srs_check, a committer key validated on the device, against the CPU oracle: the statuses of
tests/srs_check_cases.py (oracle.curve) and of the host run of the same rules, exact; the challenge sum S bit for bit
against coracle's Pippenger; keys of oracle.curve.srs_powers, h and beta_h of zkt_srs_generate_g2."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import fields as F, coracle as K, curve as C

import srs_check_cases as SC

IDS = lambda v: getattr(v, "name", str(v))
LENGTHS = [0, 1, 63, 64, 65, 520, 4097]       # as tests/test_gpu_g1_decompress.py: one lane .. a ragged tail of workgroups
N = SC.N_KEY
CHUNK = 64                                    # 257 points: five chunks, the last of one point


@pytest.fixture(scope="module")
def ctxs():
    """One context per curve with NO key loaded: the calls need none."""
    import zkt_plonk_amd as z
    c = {cv.name: z.Context(cv.name, 0) for cv in SC.CURVES}
    yield c
    for x in c.values():
        x.close()


@pytest.fixture(scope="module")
def g2():
    from zkt_plonk_amd import _lib
    return {(cv.name, d): _lib.srs_generate_g2(cv.name, SC.TAU + d) for cv in SC.CURVES for d in (0, 1)}


def _on_device(ctx, pts, fn, offset=0):
    """fn(device pointer) over a device copy of pts (placed `offset` bytes into its allocation)"""
    d = ctx.alloc(pts.nbytes + 64)
    try:
        if offset:                                   # zkt_dev_upload to the shifted address
            ctx.upload(d + offset, pts)
        else:
            ctx.upload(d, pts)
        return fn(d + offset)
    finally:
        ctx.free(d)


# ---- statuses -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("cv", SC.CURVES, ids=IDS)
def test_g1_check_matches_the_oracle_and_the_host_run(ctxs, cv, n):
    from zkt_plonk_amd import _lib
    ctx = ctxs[cv.name]
    pts, want = SC.scattered(cv, n, rot=n)
    assert np.array_equal(_lib.debug_g1_check_host(cv.name, pts), want)
    got = ctx.g1_check(pts)
    assert got.shape == want.shape and np.array_equal(got, want), np.nonzero(got != want)[0][:8]
    if n:
        dev = _on_device(ctx, pts, lambda d: ctx.g1_check(d, n))
        assert np.array_equal(dev, want), np.nonzero(dev != want)[0][:8]


@pytest.mark.parametrize("cv", SC.CURVES, ids=IDS)
def test_every_bad_point_at_every_spot(ctxs, cv):
    ctx, n = ctxs[cv.name], 260
    for rot in range(len(SC.bad(cv))):
        pts, want = SC.scattered(cv, n, rot)
        got = ctx.g1_check(pts)
        assert np.array_equal(got, want), (rot, np.nonzero(got != want)[0][:8])


def test_g1_check_arguments(ctxs):
    import zkt_plonk_amd as z
    ctx = ctxs["bn254"]
    L = z.lib()
    st = (ctypes.c_uint8 * 4)()
    pts, want = SC.scattered(F.BN254, 3)
    assert L.zkt_g1_check(ctx.handle, None, 0, 0, None) == 0 and L.zkt_g1_check(ctx.handle, None, 0, 1, None) == 0   # n = 0
    assert L.zkt_g1_check(None, pts.ctypes.data, 3, 0, st) == 1
    assert L.zkt_g1_check(ctx.handle, None, 3, 0, st) == 1
    assert L.zkt_g1_check(ctx.handle, pts.ctypes.data, 3, 0, None) == 1

    def misaligned(d):
        with pytest.raises(z.ZktError) as e:
            ctx.g1_check(d, 3)
        assert e.value.code == 1 and "16-byte aligned" in str(e.value)
        return True

    assert _on_device(ctx, pts, misaligned, offset=8)
    assert np.array_equal(ctx.g1_check(pts), want)              # the context still works afterwards


# ---- true keys ----------------------------------------------------------------------------------------------------------
def _same_sum(got, want):
    (go, gi), (wo, wi) = got, want
    return (gi and not go.any()) if wi else (not gi and np.array_equal(go, wo))


@pytest.mark.parametrize("count", [1, 2, 3, 63, 64, 65, 257])
@pytest.mark.parametrize("cv", SC.CURVES, ids=IDS)
def test_true_key_in_chunks_of_64(ctxs, g2, cv, count):
    ctx = ctxs[cv.name]
    h, bh = g2[cv.name, 0]
    key = SC.key(cv)[:count]
    ctx.debug_srs_check_chunk(CHUNK)
    try:
        reps = [ctx.srs_check(key, h, bh, seed, want_status=True) for seed in (SC.SEED_A, SC.SEED_B)]
        dev = _on_device(ctx, key, lambda d: ctx.srs_check(d, h, bh, SC.SEED_A, n=count))
    finally:
        ctx.debug_srs_check_chunk(0)
    for rep, seed in zip(reps + [dev], (SC.SEED_A, SC.SEED_B, SC.SEED_A)):
        assert rep.ok and rep.points_ok and rep.structure_checked and rep.structure_ok, rep
        assert (rep.count, rep.n_bad, rep.first_bad, rep.first_bad_status) == (count, 0, count, SC.VALID)
        assert rep.by_status == [count, 0, 0, 0, 0, 0]
        assert _same_sum(rep.sum, SC.challenge_sum(cv, key, SC.rho_of(cv, seed))), (count, seed)
    assert not reps[0].status.any() and reps[0].status.shape == (count,)
    assert not np.array_equal(reps[0].sum[0], reps[1].sum[0]) or count == 1          # another seed, another S
    if count <= 3:                                                                   # the sum, once more by the plain rule
        rho = SC.rho_of(cv, SC.SEED_A)
        S = C.msm_naive(cv, SC.key_points(cv)[:count], [pow(rho, i, cv.fr.p) for i in range(count)])
        assert np.array_equal(reps[0].sum[0], K.points_to_mont(cv, [S])[0])
    if count == 1:
        assert np.array_equal(reps[0].sum[0], key[0]) and np.array_equal(reps[1].sum[0], key[0])


@pytest.mark.parametrize("cv", SC.CURVES, ids=IDS)
def test_true_key_of_4097_points_in_one_chunk(ctxs, g2, cv):
    ctx, count = ctxs[cv.name], 4097
    h, bh = g2[cv.name, 0]
    key = SC.long_key(cv, count)
    sums = []
    for seed in (SC.SEED_A, SC.SEED_B):
        rep = ctx.srs_check(key, h, bh, seed)
        assert rep.ok and rep.structure_checked and rep.by_status == [count, 0, 0, 0, 0, 0], rep
        assert _same_sum(rep.sum, SC.challenge_sum(cv, key, SC.rho_of(cv, seed)))
        sums.append(rep.sum[0])
    assert not np.array_equal(sums[0], sums[1])


# ---- one bad point, two bad points --------------------------------------------------------------------------------------
@pytest.mark.parametrize("cv", SC.CURVES, ids=IDS)
def test_one_bad_point_is_named_and_no_structure_is_judged(ctxs, g2, cv):
    ctx = ctxs[cv.name]
    h, bh = g2[cv.name, 0]
    kinds = SC.by_status(cv)
    assert sorted(kinds) == ([1, 2, 4, 5] if cv.name == "bls12_381" else [1, 2, 4])
    ctx.debug_srs_check_chunk(CHUNK)
    try:
        for st, xy in sorted(kinds.items()):
            for at in (0, 63, 64, N - 1):
                key = SC.key(cv).copy()
                key[at] = SC.rows(cv, [xy])[0]
                rep = ctx.srs_check(key, h, bh, SC.SEED_A, want_status=(at != 63))
                assert not rep.ok and not rep.points_ok and not rep.structure_checked and not rep.structure_ok and rep.sum is None, rep
                assert (rep.count, rep.n_bad, rep.first_bad, rep.first_bad_status) == (N, 1, at, st), (rep, at, st)
                want = [0] * 6
                want[SC.VALID], want[st] = N - 1, 1
                assert rep.by_status == want
                if at != 63:
                    assert np.array_equal(rep.status, ctx.g1_check(key)) and rep.status[at] == st and rep.status.sum() == st
        # two bad points in different chunks: the lower index is the first, both are counted
        a, b = sorted(kinds)[:2]
        for lo, hi in ((70, 200), (3, 256)):
            key = SC.key(cv).copy()
            key[lo], key[hi] = SC.rows(cv, [kinds[b]])[0], SC.rows(cv, [kinds[a]])[0]
            rep = ctx.srs_check(key, h, bh, SC.SEED_A)
            assert (rep.n_bad, rep.first_bad, rep.first_bad_status, rep.points_ok, rep.structure_checked) == (2, lo, b, False, False)
            assert rep.by_status[SC.VALID] == N - 2 and rep.by_status[a] == 1 and rep.by_status[b] == 1
    finally:
        ctx.debug_srs_check_chunk(0)


# ---- valid points, wrong structure --------------------------------------------------------------------------------------
@pytest.mark.parametrize("cv", SC.CURVES, ids=IDS)
def test_valid_points_in_the_wrong_structure_are_rejected(ctxs, g2, cv):
    ctx = ctxs[cv.name]
    h, bh = g2[cv.name, 0]
    true = SC.key(cv)
    cases = {}
    k = true.copy()
    k[[63, 64]] = true[[64, 63]]
    cases["P_63 and P_64 swapped"] = (k, bh)
    for at in (1, 64, N - 1):
        cases["2 P_%d" % at] = (SC.double_point(cv, true, at), bh)
    cases["beta_h of tau + 1"] = (true, g2[cv.name, 1][1])
    cases["reversed"] = (np.ascontiguousarray(true[::-1]), bh)
    other = SC.key(cv, SC.TAU + 0x1001, N)
    cases["tau up to 100, another tau after"] = (np.concatenate([true[:101], other[101:]]), bh)
    ctx.debug_srs_check_chunk(CHUNK)
    try:
        assert ctx.srs_check(true, h, bh, SC.SEED_A).ok
        for name, (key, beta) in cases.items():
            rep = ctx.srs_check(key, h, beta, SC.SEED_A)
            assert rep.points_ok and rep.structure_checked and not rep.structure_ok and not rep.ok, (name, rep)
            assert rep.n_bad == 0 and rep.first_bad == N and rep.by_status == [N, 0, 0, 0, 0, 0], name
            assert _same_sum(rep.sum, SC.challenge_sum(cv, key, SC.rho_of(cv, SC.SEED_A))), name
    finally:
        ctx.debug_srs_check_chunk(0)


# ---- refusals -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cv", SC.CURVES, ids=IDS)
def test_refusals(ctxs, g2, cv):
    import zkt_plonk_amd as z
    from zkt_plonk_amd import _lib
    ctx = ctxs[cv.name]
    h, bh = g2[cv.name, 0]
    key = SC.key(cv)[:5]
    for seed in (0, cv.fr.p):                                    # both reduce to rho = 0
        with pytest.raises(z.ZktError) as e:
            ctx.srs_check(key, h, bh, seed)
        assert e.value.code == 1 and "rho = 0" in str(e.value)
    assert ctx.srs_check(key, h, bh, cv.fr.p + 1).ok             # reduces to rho = 1
    with pytest.raises(z.ZktError) as e:
        ctx.srs_check(key[:0], h, bh, SC.SEED_A)                 # count = 0
    assert e.value.code == 1
    rep, seed = _lib.SrsReport(), (ctypes.c_uint8 * 32)(*SC.SEED_A)
    L, p = z.lib(), _lib.u64p
    # the count is judged before any memory is touched
    assert L.zkt_srs_check(ctx.handle, key.ctypes.data, _lib.SRS_CHECK_MAX + 1, 0, p(h), p(bh), seed, None, ctypes.byref(rep)) == 1
    assert b"ZKT_SRS_CHECK_MAX" in L.zkt_last_error(ctx.handle)
    assert L.zkt_srs_check(ctx.handle, key.ctypes.data, 5, 0, p(h), p(bh), seed, None, None) == 1
    assert L.zkt_srs_check(ctx.handle, key.ctypes.data, 5, 0, p(h), p(bh), None, None, ctypes.byref(rep)) == 1
    with pytest.raises(z.ZktError):
        ctx.debug_srs_check_chunk(_lib.MSM_BASES_MAX + 1)
    assert _on_device(ctx, key, lambda d: pytest.raises(z.ZktError, ctx.srs_check, d, h, bh, SC.SEED_A, n=5) is not None, offset=8)
    assert ctx.srs_check(key, h, bh, SC.SEED_A).ok


# ---- the context is left alone ------------------------------------------------------------------------------------------
def test_proofs_and_the_loaded_key_are_unchanged_by_the_call(g2):
    """The smallest circuit the prover tests use (oracle.plonk.test_circuit, n = 128): a proof's bytes before and after
    zkt_srs_check, the loaded key read back, and the call on a fork."""
    import zkt_plonk_amd as z
    from oracle import plonk as P
    cv = F.BN254
    cs = P.test_circuit(cv)
    n = cs.circuit_bound()
    srs = K.srs_mont(cv, 0x5EED, n + 8)
    be = K.CBackend(cv, srs)
    pk, epk, vk = P.setup(be, [None] * (n + 8), cs, True)
    blinders = [(i + 1) * 0x9E3779B97F4A7C15 % cv.fr.p for i in range(P.NUM_BLINDERS)]
    want = P.prove(be, [None] * (n + 8), pk, epk, vk, cs, P.new_seeded_transcript(cv, vk), blinders).serialize(cv)
    h, bh = g2[cv.name, 0]
    key = SC.key(cv)
    S = SC.challenge_sum(cv, key, SC.rho_of(cv, SC.SEED_A))
    ctx = z.Context(cv.name, 0)
    try:
        ctx.srs_load(srs)
        prover = z.GpuProver(ctx, n.bit_length() - 1, {k: K.fr_to_mont(cv, pk.polys[k]) for k in z.PK_ORDER})
        a, b, c = cs.wire_evals(cs.n_gates)
        wires = [K.fr_to_mont(cv, w) for w in (a, b, c)]
        table = K.fr_to_mont(cv, cs.table)
        pi = {p_: K.fr_to_mont(cv, [v])[0] for p_, v in cs.pi.items()}

        def prove(pr):
            tr = z.seed_transcript(z.Transcript("merlin", "ZKT Plonk"), vk.n, vk.commits)
            return pr.prove(wires[0], wires[1], wires[2], table, pi, K.fr_to_mont(cv, blinders), tr)

        assert prove(prover) == want
        rep = ctx.srs_check(key, h, bh, SC.SEED_A)
        assert rep.ok and _same_sum(rep.sum, S)
        assert prove(prover) == want
        assert np.array_equal(ctx.srs_download(0, n + 8), srs)
        bad = key.copy()
        bad[200] = 0
        assert ctx.srs_check(bad, h, bh, SC.SEED_A).first_bad == 200
        assert prove(prover) == want
        fork = ctx.fork()
        try:
            rep = fork.srs_check(key, h, bh, SC.SEED_A)
            assert rep.ok and _same_sum(rep.sum, S)
            assert np.array_equal(fork.g1_check(bad), ctx.g1_check(bad))
            assert z.GpuProver(fork, n.bit_length() - 1).prove(wires[0], wires[1], wires[2], table, pi, K.fr_to_mont(cv, blinders),
                                                               z.seed_transcript(z.Transcript("merlin", "ZKT Plonk"), vk.n, vk.commits)) == want
        finally:
            fork.close()
        assert prove(prover) == want
        assert np.array_equal(ctx.srs_download(0, n + 8), srs)
    finally:
        ctx.close()


# ---- the caller's stream ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cv", SC.CURVES, ids=IDS)
def test_points_still_being_written_on_the_callers_stream(g2, cv):
    """tests/stream_rig.py: the key is in device memory, and the caller's own copy on the context's stream is still writing
    it (behind a hold) when the calls are made.  Both must judge the finished buffer: the decoy it overwrites is a valid key
    of another tau with an identity in it, whose statuses, verdict and sum all differ."""
    import torch
    import zkt_plonk_amd as z
    import stream_rig as R
    h, bh = g2[cv.name, 0]
    real = SC.key(cv).copy()
    decoy = SC.key(cv, SC.TAU + 0x1001, N).copy()
    decoy[N - 2] = 0
    want_st = np.zeros(N, dtype=np.uint8)
    S, inf = SC.challenge_sum(cv, real, SC.rho_of(cv, SC.SEED_A))
    assert not inf
    ctx = z.Context(cv.name, 0)
    try:
        rig = R.Rig(ctx, torch.cuda.Stream())
        rig.calibrate()
        d_key = R.dev(decoy)

        def check(m, data):
            m.begin([(d_key, data[0])])
            return m.blocking("zkt_g1_check", ctx.g1_check, d_key.data_ptr(), N)

        R.compare("zkt_g1_check", rig.three_ways(check, [d_key], [R.dev(decoy)], [R.dev(real)]), want_st)

        def srs(m, data):
            m.begin([(d_key, data[0])])
            rep = m.blocking("zkt_srs_check", ctx.srs_check, d_key.data_ptr(), h, bh, SC.SEED_A, n=N, want_status=True)
            return [rep.status, rep.ok, rep.n_bad, rep.first_bad, rep.sum[0] if rep.sum else None]

        R.compare("zkt_srs_check", rig.three_ways(srs, [d_key], [R.dev(decoy)], [R.dev(real)]), [want_st, True, 0, N, S])
    finally:
        ctx.close()
