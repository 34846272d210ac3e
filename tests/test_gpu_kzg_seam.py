"""GPU: the KZG commitment seam, zkt_kzg_commit_batch / zkt_kzg_open (and their _dev forms), against the CPU oracle
(orc_msm, orc_lincomb, orc_div_linear, orc_poly_eval) and against the library's own single MSM."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import fields as F, coracle as K

CURVES = [F.BN254, F.BLS12_381]
N = 1 << 14          # powers of the test key: grouped launches and deferred tails are on at this size
TAU = 0x7A0C5EED


@pytest.fixture(scope="module")
def keyed():
    """One context per curve with a key of N powers, and the key itself (host copy for the oracle)."""
    import zkt_plonk_amd as z
    out = {}
    for cv in CURVES:
        ctx = z.Context(cv.name, 0)
        srs = K.srs_mont(cv, TAU, N)
        ctx.srs_load(srs)
        out[cv.name] = (ctx, srs)
    yield out
    for ctx, _ in out.values():
        ctx.close()


def _fr(cv, n, rng):
    """n random field elements below 2^(bits - 1) < r: valid Montgomery limbs (and canonical integers)"""
    s = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, 4), dtype=np.uint64)
    s[:, 3] &= np.uint64((1 << (cv.fr.bits - 1 - 192)) - 1)
    return s


def _lens(k, top, rng):
    """ragged lengths: 0, 1, 2, the whole key, then random ones"""
    base = [0, 1, 2, top]
    return [base[j] if j < len(base) else int(rng.integers(3, top)) for j in range(k)]


def _same(got, want):
    """same point; the call writes the identity as (0,0) (the oracle's coordinates are meaningless there)"""
    (go, gi), (wo, wi) = got, want
    if wi:
        return gi and not go.any()
    return not gi and np.array_equal(go, wo)


def _oracle_commit(cv, srs, p, mont=True):
    if p.shape[0] == 0:
        return np.zeros(2 * cv.fq.limbs64, dtype=np.uint64), True
    return K.msm_mont(cv, srs[:p.shape[0]], p, mont)


def _upload_all(ctx, polys):
    ptrs = []
    for p in polys:
        if p.shape[0]:
            d = ctx.alloc(p.nbytes)
            ctx.upload(d, p)
            ptrs.append(d)
        else:
            ptrs.append(0)
    return ptrs


def _free_all(ctx, ptrs):
    for d in ptrs:
        if d:
            ctx.free(d)


@pytest.mark.parametrize("cv", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("k", [1, 3, 7, 32])
def test_commit_batch_matches_oracle(cv, k, keyed):
    ctx, srs = keyed[cv.name]
    rng = np.random.default_rng(100 + k)
    polys = [_fr(cv, n, rng) for n in _lens(k, N, rng)]
    for mont in (True, False):
        got = ctx.kzg_commit_batch(polys, montgomery=mont)
        assert len(got) == k
        d = _upload_all(ctx, polys)
        try:
            got_dev = ctx.kzg_commit_batch_dev(d, [p.shape[0] for p in polys], montgomery=mont)
        finally:
            _free_all(ctx, d)
        for j, p in enumerate(polys):
            want = _oracle_commit(cv, srs, p, mont)
            assert _same(got[j], want), "entry %d (len %d, montgomery %s)" % (j, p.shape[0], mont)
            assert np.array_equal(got[j][0], got_dev[j][0]) and got[j][1] == got_dev[j][1]
            if p.shape[0]:
                assert _same(ctx.msm(p, montgomery=mont), want)


def test_commit_batch_bn254_2_20():
    """BN254 at 2^20 powers, k = 3: one launch sequence per MSM (no grouping), the tails overlapping the next MSM."""
    import zkt_plonk_amd as z
    cv = F.BN254
    n = 1 << 20
    ctx = z.Context(cv.name, 0)
    try:
        ctx.srs_generate(0x5EED, n)
        srs = ctx.srs_download(0, n)
        rng = np.random.default_rng(2020)
        polys = [_fr(cv, n, rng), _fr(cv, n - 5, rng), _fr(cv, 12345, rng)]
        got = ctx.kzg_commit_batch(polys)
        d = _upload_all(ctx, polys)
        try:
            got_dev = ctx.kzg_commit_batch_dev(d, [p.shape[0] for p in polys])
        finally:
            _free_all(ctx, d)
        for j, p in enumerate(polys):
            want = K.msm_mont(cv, srs[:p.shape[0]], p)
            assert _same(got[j], want) and _same(got_dev[j], want)
            assert _same(ctx.msm(p), want)
    finally:
        ctx.close()


def _points(cv, rng):
    """z: random, 0, 1 and a primitive root of unity of the key's domain (Montgomery limbs)"""
    root = cv.fr.root_of_unity(N)
    vals = [int(rng.integers(2, 1 << 62)) * int(rng.integers(2, 1 << 62)) % cv.fr.p, 0, 1, root]
    return [(name, K.fr_to_mont(cv, [v])[0]) for name, v in zip(("random", "zero", "one", "root"), vals)]


def _oracle_open(cv, srs, polys, ch, zm):
    L = max(p.shape[0] for p in polys)
    comb = K.lincomb(cv, polys, ch, max(L, 1))
    wit = K.div_linear(cv, comb[:L], zm)
    if wit.shape[0] == 0:
        w = (np.zeros(2 * cv.fq.limbs64, dtype=np.uint64), True)
    else:
        w = K.msm_mont(cv, srs[:wit.shape[0]], wit)
    ev = np.array([K.poly_eval(cv, p, zm) for p in polys], dtype=np.uint64).reshape(-1, 4)
    return w, ev


@pytest.mark.parametrize("cv", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("k", [1, 10, 32])
def test_open_matches_oracle(cv, k, keyed):
    ctx, srs = keyed[cv.name]
    rng = np.random.default_rng(200 + k)
    lens = _lens(k, N, rng)
    if k == 1:
        lens = [int(rng.integers(N // 2, N))]
    polys = [_fr(cv, n, rng) for n in lens]
    ch = _fr(cv, k, rng)
    if k > 2:
        ch[1] = 0            # a zero challenge
        ch[2] = ch[0]        # and a repeated one
    for name, zm in _points(cv, rng):
        (w, inf), ev = ctx.kzg_open(polys, ch, zm)
        want_w, want_ev = _oracle_open(cv, srs, polys, ch, zm)
        assert _same((w, inf), want_w), "witness, z = %s" % name
        assert np.array_equal(ev, want_ev), "evaluations, z = %s" % name
    # the _dev form, bit for bit; evaluations optional
    zm = _points(cv, rng)[0][1]
    want = ctx.kzg_open(polys, ch, zm)
    d = _upload_all(ctx, polys)
    try:
        got = ctx.kzg_open_dev(d, lens, ch, zm)
        got_noev = ctx.kzg_open_dev(d, lens, ch, zm, evals=False)
    finally:
        _free_all(ctx, d)
    assert np.array_equal(got[0][0], want[0][0]) and got[0][1] == want[0][1] and np.array_equal(got[1], want[1])
    assert np.array_equal(got_noev[0][0], want[0][0]) and got_noev[1] is None


@pytest.mark.parametrize("cv", CURVES, ids=lambda c: c.name)
def test_open_of_constants_is_the_identity(cv, keyed):
    ctx, srs = keyed[cv.name]
    rng = np.random.default_rng(5)
    polys = [_fr(cv, 1, rng) for _ in range(4)] + [np.zeros((0, 4), dtype=np.uint64)]
    ch = _fr(cv, 5, rng)
    zm = _fr(cv, 1, rng)[0]
    (w, inf), ev = ctx.kzg_open(polys, ch, zm)
    assert inf and not w.any()
    assert np.array_equal(ev[:4], np.concatenate(polys[:4])) and not ev[4].any()
    (w, inf), ev = ctx.kzg_open([np.zeros((0, 4), dtype=np.uint64)] * 3, ch[:3], zm)
    assert inf and not w.any() and not ev.any()
    # and k = 0: nothing to do, nothing written
    assert ctx.kzg_commit_batch([]) == []


def _raw_commit(ctx, polys, k=None):
    """direct C call with sentinel-filled outputs -> (rc, out, inf)"""
    L = ctx._L
    k = len(polys) if k is None else k
    arrs = [np.ascontiguousarray(p, dtype=np.uint64) for p in polys]
    ptrs = (ctypes.c_void_p * max(len(arrs), 1))(*[a.ctypes.data for a in arrs])
    lens = (ctypes.c_size_t * max(len(arrs), 1))(*[a.shape[0] for a in arrs])
    out = np.full(max(len(arrs), 1) * 2 * ctx.fq_limbs, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    inf = (ctypes.c_int * max(len(arrs), 1))(*([7] * max(len(arrs), 1)))
    rc = L.zkt_kzg_commit_batch(ctx._h, ptrs, lens, k, 1, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), inf)
    return rc, out, list(inf)


def _raw_open(ctx, polys, ch, zm):
    L = ctx._L
    u64 = ctypes.POINTER(ctypes.c_uint64)
    arrs = [np.ascontiguousarray(p, dtype=np.uint64) for p in polys]
    ptrs = (ctypes.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
    lens = (ctypes.c_size_t * len(arrs))(*[a.shape[0] for a in arrs])
    w = np.full(2 * ctx.fq_limbs, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    ev = np.full((len(arrs), 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    inf = ctypes.c_int(7)
    rc = L.zkt_kzg_open(ctx._h, ptrs, lens, len(arrs), ch.ctypes.data_as(u64), zm.ctypes.data_as(u64), w.ctypes.data_as(u64),
                        ctypes.byref(inf), ev.ctypes.data_as(u64))
    return rc, w, inf.value, ev


def test_errors(keyed):
    import zkt_plonk_amd as z
    cv = F.BN254
    ctx, srs = keyed[cv.name]
    rng = np.random.default_rng(9)
    ok = _fr(cv, 100, rng)
    # too long a polynomial: code 5, nothing written
    rc, out, inf = _raw_commit(ctx, [ok, _fr(cv, N + 1, rng)])
    assert rc == 5 and (out == 0xA5A5A5A5A5A5A5A5).all() and inf == [7, 7]
    ch = _fr(cv, 2, rng)
    zm = _fr(cv, 1, rng)[0].copy()
    rc, w, winf, ev = _raw_open(ctx, [ok, _fr(cv, N + 1, rng)], ch, zm)
    assert rc == 5 and (w == 0xA5A5A5A5A5A5A5A5).all() and winf == 7 and (ev == 0xA5A5A5A5A5A5A5A5).all()
    # k above ZKT_KZG_BATCH_MAX, null pointers: code 1
    assert _raw_commit(ctx, [ok] * 33)[0] == 1
    assert _raw_commit(ctx, [ok], k=-1)[0] == 1
    u64 = ctypes.POINTER(ctypes.c_uint64)
    lens = (ctypes.c_size_t * 1)(100)
    out = np.zeros(8, dtype=np.uint64)
    assert ctx._L.zkt_kzg_commit_batch(ctx._h, None, lens, 1, 1, out.ctypes.data_as(u64), None) == 1
    nullp = (ctypes.c_void_p * 1)(None)
    assert ctx._L.zkt_kzg_commit_batch(ctx._h, nullp, lens, 1, 1, out.ctypes.data_as(u64), None) == 1
    ptrs = (ctypes.c_void_p * 1)(ok.ctypes.data)
    assert ctx._L.zkt_kzg_commit_batch(ctx._h, ptrs, lens, 1, 1, None, None) == 1
    assert ctx._L.zkt_kzg_open(ctx._h, ptrs, lens, 1, None, zm.ctypes.data_as(u64), out.ctypes.data_as(u64), None, None) == 1
    # and the context still works
    assert _same(ctx.kzg_commit_batch([ok])[0], K.msm_mont(cv, srs[:100], ok))
    # no SRS: code 10; a sliced key: code 1
    bare = z.Context(cv.name, 0)
    try:
        with pytest.raises(z.ZktError) as e:
            bare.kzg_commit_batch([ok])
        assert e.value.code == 10
        with pytest.raises(z.ZktError) as e:
            bare.kzg_open([ok], ch[:1], zm)
        assert e.value.code == 10
        bare.srs_generate_slice(TAU, 64, 64, 256)
        with pytest.raises(z.ZktError) as e:
            bare.kzg_commit_batch([ok[:10]])
        assert e.value.code == 1
        with pytest.raises(z.ZktError) as e:
            bare.kzg_open([ok[:10]], ch[:1], zm)
        assert e.value.code == 1
    finally:
        bare.close()


def _small_proof_setup(cv):
    from oracle import plonk as P
    cs = P.test_circuit(cv)
    n = cs.circuit_bound()
    srs = K.srs_mont(cv, 0x5EED, n + 8)
    be = K.CBackend(cv, srs)
    pk, epk, vk = P.setup(be, [None] * (n + 8), cs, True)
    blinders = [[(i + 1 + 100 * k) * 0x9E3779B97F4A7C15 % cv.fr.p for i in range(P.NUM_BLINDERS)] for k in range(3)]
    want = [P.prove(be, [None] * (n + 8), pk, epk, vk, cs, P.new_seeded_transcript(cv, vk), b).serialize(cv) for b in blinders]
    return cs, n, srs, pk, vk, blinders, want


def test_proofs_around_the_calls_are_unchanged():
    """Prove, commit_batch and open, prove again (and on a forked context; and with the next proof announced): every
    proof's bytes equal the oracle's, and the calls' results stay right."""
    import zkt_plonk_amd as z
    cv = F.BN254
    cs, n, srs, pk, vk, blinders, want = _small_proof_setup(cv)
    rng = np.random.default_rng(77)
    polys = [_fr(cv, m, rng) for m in (n + 8, n, 3, 0, n // 2 + 1)]
    ch = _fr(cv, len(polys), rng)
    zm = _fr(cv, 1, rng)[0]
    want_c = [_oracle_commit(cv, srs, p) for p in polys]
    want_w, want_ev = _oracle_open(cv, srs, polys, ch, zm)

    def seam(c):
        got = c.kzg_commit_batch(polys)
        assert all(_same(g, w) for g, w in zip(got, want_c))
        (w, inf), ev = c.kzg_open(polys, ch, zm)
        assert _same((w, inf), want_w) and np.array_equal(ev, want_ev)

    ctx = z.Context(cv.name, 0)
    try:
        ctx.srs_load(srs)
        prover = z.GpuProver(ctx, n.bit_length() - 1, {k: K.fr_to_mont(cv, pk.polys[k]) for k in z.PK_ORDER})
        a, b, c = cs.wire_evals(cs.n_gates)
        wires = [K.fr_to_mont(cv, w) for w in (a, b, c)]
        table = K.fr_to_mont(cv, cs.table)
        pi = {p_: K.fr_to_mont(cv, [v])[0] for p_, v in cs.pi.items()}

        def tr():
            return z.seed_transcript(z.Transcript("merlin", "ZKT Plonk"), vk.n, vk.commits)

        def prove(k):
            return prover.prove(wires[0], wires[1], wires[2], table, pi, K.fr_to_mont(cv, blinders[k]), tr())

        assert prove(0) == want[0]
        seam(ctx)
        assert prove(1) == want[1]
        seam(ctx)
        assert prove(0) == want[0]
        # a forked context: its own scratch, the parent's key and circuit untouched
        fork = ctx.fork()
        try:
            seam(fork)
            assert prove(2) == want[2]
            fork_prover = z.GpuProver(fork, n.bit_length() - 1)
            assert fork_prover.prove(wires[0], wires[1], wires[2], table, pi, K.fr_to_mont(cv, blinders[1]), tr()) == want[1]
            seam(fork)
        finally:
            fork.close()
        # the next proof announced (zkt_prove_set_next), then the calls, then that proof: same bytes
        pi_pos = sorted(cs.pi)
        pi_vals = K.fr_to_mont(cv, [cs.pi[k] for k in pi_pos])
        d = []
        for w in wires:
            d.append(ctx.alloc(w.nbytes))
            ctx.upload(d[-1], w)
        try:
            preps = [ctx.prepare_dev(d[0], d[1], d[2], cs.n_gates, table, pi_pos, pi_vals, K.fr_to_mont(cv, x))
                     for x in blinders]
            assert ctx.prove_prepared(preps[0], tr(), preps[1]) == want[0]
            seam(ctx)
            assert ctx.prove_prepared(preps[1], tr(), preps[2]) == want[1]
            seam(ctx)
            assert ctx.prove_prepared(preps[2], tr()) == want[2]
        finally:
            for x in d:
                ctx.free(x)
    finally:
        ctx.close()
