"""GPU: zkt_msm_g1_bases / zkt_msm_g1_bases_dev, the device MSM over caller-supplied bases (VariableBaseMSM on arbitrary
points), against the CPU oracle (orc_msm, ark-ec's Pippenger) and against the library's own fixed-base MSM."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import fields as F, coracle as K

CURVES = [F.BN254, F.BLS12_381]
SIZES = {"bn254": [1, 2, 3, 255, (1 << 10) + 7, 1 << 14, 1 << 17, 1 << 20],
         "bls12_381": [1, 2, 3, 255, (1 << 10) + 7, 1 << 14, 1 << 18]}


@pytest.fixture(scope="module")
def ctxs():
    """One context per curve with NO key loaded: the call needs none."""
    import zkt_plonk_amd as z
    c = {cv.name: z.Context(cv.name, 0) for cv in CURVES}
    yield c
    for x in c.values():
        x.close()


@functools.lru_cache(maxsize=None)
def _bases(cv, n, seed=1):
    """n random multiples of G: the powers of a random trapdoor, shuffled (read-only: callers copy before editing)."""
    rng = np.random.default_rng(seed)
    tau = int(rng.integers(2, 1 << 62)) * int(rng.integers(2, 1 << 62)) % cv.fr.p
    pts = K.srs_mont(cv, tau, n)[rng.permutation(n)]
    pts.setflags(write=False)
    return pts


def _scalars(cv, n, seed, full=0):
    """n random scalars below 2^(bits - 1) < r (valid in either form); the first `full` are arbitrary 256-bit integers."""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, 4), dtype=np.uint64)
    s[:, 3] &= np.uint64((1 << (cv.fr.bits - 1 - 192)) - 1)
    if full:
        s[:full] = rng.integers(0, 1 << 63, size=(full, 4), dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    return s


def _reduced(cv, s, upto):
    """s with its first `upto` rows reduced mod r (the oracle reads fr_bits bits only)."""
    s = s.copy()
    if upto:
        s[:upto] = K.ints_to_limbs([v % cv.fr.p for v in K.limbs_to_ints(s[:upto])], 4)
    return s


def _neg(cv, pts):
    """-P in Montgomery limbs: y -> p - y ((0,0) stays)."""
    L = cv.fq.limbs64
    out = pts.copy()
    ys = K.limbs_to_ints(pts[:, L:])
    out[:, L:] = K.ints_to_limbs([(cv.fq.p - y) % cv.fq.p for y in ys], L)
    return out


def _same(got, want):
    """same point; the call writes the identity as (0,0) (the oracle's coordinates are meaningless there)"""
    (go, gi), (wo, wi) = got, want
    if wi:
        return gi and not go.any()
    return not gi and np.array_equal(go, wo)


@pytest.mark.parametrize("cv", CURVES, ids=lambda c: c.name)
def test_random_bases_vs_oracle(cv, ctxs):
    ctx = ctxs[cv.name]
    for n in SIZES[cv.name]:
        bases = _bases(cv, n)
        # Montgomery scalars (polynomial coefficients as they sit in memory)
        sc = _scalars(cv, n, 10 + n)
        assert _same(ctx.msm_bases(bases, sc, montgomery=True), K.msm_mont(cv, bases, sc, True)), (cv.name, n, "mont")
        # canonical 256-bit integers, the first ones >= r: every bit counts, the result is that of s mod r
        full = min(n, 64)
        sc = _scalars(cv, n, 20 + n, full=full)
        want = K.msm_mont(cv, bases, _reduced(cv, sc, full), False)
        assert _same(ctx.msm_bases(bases, sc, montgomery=False), want), (cv.name, n, "canonical")


def _boundaries(ctx, top):
    """n on both sides of every change of digit width / window count the call picks up to `top` points"""
    out, prev = [], None
    for lg in range(0, top.bit_length()):
        n = 1 << lg
        info = ctx.msm_bases_info(n)
        if prev is not None and info != prev:
            out += [n - 1, n]
        prev = info
    return [n for n in out if 1 <= n <= top]


@pytest.mark.parametrize("cv", CURVES, ids=lambda c: c.name)
def test_srs_bases_match_the_fixed_base_msm(cv):
    """Bases = the first n powers of the loaded key: the result is zkt_msm_g1's on the same scalars, at every regime
    boundary of the variable-base path and at the largest size (the call runs on a context with a key loaded)."""
    import zkt_plonk_amd as z
    top = (1 << 22) if cv is F.BN254 else (1 << 20)
    ctx = z.Context(cv.name, 0)
    try:
        ctx.srs_generate(0xB45E5 + cv.curve_id, top)
        srs = ctx.srs_download(0, top)
        sizes = sorted(set(_boundaries(ctx, top) + [top]))
        assert len(sizes) >= 4, sizes
        for n in sizes:
            sc = _scalars(cv, n, 30 + n)
            for mont in (True, False):
                want = ctx.msm(sc, 0, mont)
                assert _same(ctx.msm_bases(srs[:n], sc, montgomery=mont), want), (cv.name, n, mont, ctx.msm_bases_info(n, mont))
    finally:
        ctx.close()


@pytest.mark.parametrize("cv", CURVES, ids=lambda c: c.name)
def test_exceptional_inputs(cv, ctxs):
    ctx = ctxs[cv.name]
    p = cv.fr.p
    L = cv.fq.limbs64
    P = np.array(_bases(cv, 4)[:1])
    ident = np.zeros((1, 2 * L), dtype=np.uint64)
    one = lambda n, v: K.ints_to_limbs([v] * n, 4)
    # n = 0: the identity
    out, inf = ctx.msm_bases(np.zeros((0, 2 * L), dtype=np.uint64), np.zeros((0, 4), dtype=np.uint64))
    assert inf and not out.any()
    # every base the same point, random and equal scalars: P + P inside the buckets, one crowded bucket per window
    for n in (300, 1 << 14):
        bases = np.repeat(P, n, axis=0)
        sc = _scalars(cv, n, 40 + n)
        assert _same(ctx.msm_bases(bases, sc), K.msm_mont(cv, bases, sc, True)), (cv.name, n)
        sc = one(n, 0x1234567 + n)
        assert _same(ctx.msm_bases(bases, sc, montgomery=False), K.msm_mont(cv, bases, sc, False)), (cv.name, n, "equal")
    # P and -P in the same sum: exact cancellation, and mixed with other points and identities
    negP = _neg(cv, P)
    out, inf = ctx.msm_bases(np.concatenate([P, negP]), one(2, 77), montgomery=False)
    assert inf and not out.any()
    out, inf = ctx.msm_bases(np.concatenate([P, negP] * 500), one(1000, 12345), montgomery=False)
    assert inf and not out.any()
    pts = np.array(_bases(cv, 4096, seed=3))
    pts[1::2] = _neg(cv, pts[0::2])                      # pairs P_i, -P_i
    pts[::17] = 0                                        # identities
    for mont in (True, False):
        sc = _scalars(cv, 4096, 50)
        sc[1::2] = sc[0::2]                              # equal scalars on P and -P: those pairs cancel
        sc[3::10] = 0                                    # zero scalars
        assert _same(ctx.msm_bases(pts, sc, montgomery=mont), K.msm_mont(cv, pts, sc, mont)), (cv.name, mont)
    # identity bases only / zero scalars only: the identity
    out, inf = ctx.msm_bases(np.repeat(ident, 100, axis=0), _scalars(cv, 100, 60))
    assert inf and not out.any()
    out, inf = ctx.msm_bases(_bases(cv, 1 << 14), np.zeros((1 << 14, 4), dtype=np.uint64))
    assert inf and not out.any()
    # canonical scalars r - 1, r + 5, 2^256 - 1 (and r, 2r: the identity on a point of order r)
    big = [p - 1, p + 5, (1 << 256) - 1, p, 2 * p, 1]
    bases = np.array(_bases(cv, len(big), seed=5))
    sc = K.ints_to_limbs(big, 4)
    want = K.msm_mont(cv, bases, K.ints_to_limbs([v % p for v in big], 4), False)
    assert _same(ctx.msm_bases(bases, sc, montgomery=False), want)
    for i, v in enumerate(big):
        want = K.msm_mont(cv, bases[i:i + 1], K.ints_to_limbs([v % p], 4), False)
        assert _same(ctx.msm_bases(bases[i:i + 1], sc[i:i + 1], montgomery=False), want), hex(v)
    out, inf = ctx.msm_bases(bases[3:5], sc[3:5], montgomery=False)
    assert inf and not out.any()


@pytest.mark.parametrize("cv", CURVES, ids=lambda c: c.name)
def test_host_and_device_variants_agree(cv):
    """Same bytes from host and HBM inputs, on a fresh context that never saw a key."""
    import zkt_plonk_amd as z
    ctx = z.Context(cv.name, 0)
    try:
        for n in (5, 1 << 12, 1 << 16):
            bases = np.ascontiguousarray(_bases(cv, n, seed=7))
            for mont in (True, False):
                full = 0 if mont else min(n, 8)
                sc = _scalars(cv, n, 70 + n, full=full)
                db, ds = ctx.alloc(bases.nbytes), ctx.alloc(sc.nbytes)
                try:
                    ctx.upload(db, bases)
                    ctx.upload(ds, sc)
                    dev = ctx.msm_bases_dev(db, ds, n, montgomery=mont)
                finally:
                    ctx.free(db)
                    ctx.free(ds)
                host = ctx.msm_bases(bases, sc, montgomery=mont)
                assert _same(dev, host), (n, mont)
                want = K.msm_mont(cv, bases, _reduced(cv, sc, full), mont)
                assert _same(host, want), (n, mont)
        assert ctx.msm_info()["srs_count"] == 0           # still no key
    finally:
        ctx.close()


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


def test_proofs_around_the_call_are_unchanged():
    """Prove, msm_bases, prove again (and on a forked context; and with the next proof announced): every proof's bytes
    equal the oracle's, and the calls' results stay right."""
    import zkt_plonk_amd as z
    cv = F.BN254
    cs, n, srs, pk, vk, blinders, want = _small_proof_setup(cv)
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

        bases = _bases(cv, 1 << 14, seed=9)
        sc = _scalars(cv, 1 << 14, 90)
        ref = K.msm_mont(cv, bases, sc, True)
        assert prove(0) == want[0]
        assert _same(ctx.msm_bases(bases, sc), ref)
        assert prove(1) == want[1]
        assert _same(ctx.msm_bases(bases, sc), ref)
        assert prove(0) == want[0]
        # a forked context: its own scratch, the parent's key and circuit untouched
        fork = ctx.fork()
        try:
            assert _same(fork.msm_bases(bases, sc), ref)
            assert prove(2) == want[2]
            fork_prover = z.GpuProver(fork, n.bit_length() - 1)
            assert fork_prover.prove(wires[0], wires[1], wires[2], table, pi, K.fr_to_mont(cv, blinders[1]), tr()) == want[1]
            assert _same(fork.msm_bases(bases, sc), ref)
        finally:
            fork.close()
        # the next proof announced (zkt_prove_set_next), then the call, then that proof: same bytes
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
            assert _same(ctx.msm_bases(bases, sc), ref)
            assert ctx.prove_prepared(preps[1], tr(), preps[2]) == want[1]
            assert _same(ctx.msm_bases(bases, sc), ref)
            assert ctx.prove_prepared(preps[2], tr()) == want[2]
        finally:
            for x in d:
                ctx.free(x)
    finally:
        ctx.close()


def test_errors(ctxs):
    import zkt_plonk_amd as z
    ctx = ctxs["bn254"]
    L = z.lib()
    out = np.zeros(8, dtype=np.uint64)
    inf = ctypes.c_int(0)
    pts = np.ascontiguousarray(_bases(F.BN254, 4))
    sc = _scalars(F.BN254, 4, 1)
    P64 = ctypes.POINTER(ctypes.c_uint64)
    u = lambda a: a.ctypes.data_as(P64)
    assert L.zkt_msm_g1_bases(None, u(pts), u(sc), 4, 1, u(out), ctypes.byref(inf)) == 1
    assert L.zkt_msm_g1_bases(ctx.handle, None, u(sc), 4, 1, u(out), ctypes.byref(inf)) == 1
    assert L.zkt_msm_g1_bases(ctx.handle, u(pts), None, 4, 1, u(out), ctypes.byref(inf)) == 1
    assert L.zkt_msm_g1_bases(ctx.handle, u(pts), u(sc), 4, 1, None, ctypes.byref(inf)) == 1
    assert L.zkt_msm_g1_bases_dev(ctx.handle, None, None, 4, 1, u(out), ctypes.byref(inf)) == 1
    # NULL inputs are fine with n = 0, and out_is_infinity is optional
    assert L.zkt_msm_g1_bases(ctx.handle, None, None, 0, 1, u(out), None) == 0 and not out.any()
    # more points than the maximum: refused before anything is read
    with pytest.raises(z.ZktError) as e:
        ctx.msm_bases_dev(pts.ctypes.data, sc.ctypes.data, z._lib.MSM_BASES_MAX + 1)
    assert e.value.code == 1 and "ZKT_MSM_BASES_MAX" in str(e.value)
    assert L.zkt_msm_g1_bases(ctx.handle, u(pts), u(sc), z._lib.MSM_BASES_MAX + 1, 0, u(out), ctypes.byref(inf)) == 1
    with pytest.raises(z.ZktError):
        ctx.msm_bases_info(z._lib.MSM_BASES_MAX + 1)
    # the largest size is accepted: the digit layout it needs fits the sort
    for cvn in ("bn254", "bls12_381"):
        for mont in (True, False):
            info = ctxs[cvn].msm_bases_info(z._lib.MSM_BASES_MAX, mont)
            assert 8 <= info["window_bits"] <= 16 and info["windows"] * info["window_bits"] >= 255
    # mismatched lengths in the Python wrapper
    with pytest.raises(ValueError):
        ctx.msm_bases(pts, sc[:3])
    # the context still works after the refusals
    assert _same(ctx.msm_bases(pts, sc), K.msm_mont(F.BN254, pts, sc, True))
