"""Plookup's h1 / h2 on the device (csrc/poly.hip k_lookup_count / k_lookup_starts / k_lookup_expand, driven by the
prover's own combine_split, csrc/prover.hip) at tables that span several 1024-key scan chunks and outgrow the 8192-key
LDS histogram, with the zero key of the padding absent or already in the table, against the C++ oracle element by
element; and whole proofs over such tables -- chained, reordered, failed and interleaved with the split alone -- against
the CPU oracle's bytes, each verified."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import fields as F, plonk as P, coracle as K
from helpers import field_elems
import lookup_cases as LC

LOG_N = 14
N = 1 << LOG_N


@pytest.fixture(scope="module")
def ctxs():
    import zkt_plonk_amd as z
    c = {cv.name: z.Context(cv.name, 0) for cv in (F.BN254, F.BLS12_381)}
    yield c
    for x in c.values():
        x.close()


def _split_ctx(ctxs, cv):
    """The context of `cv` with a circuit of n = 2^14 loaded (bench.py's; the split only needs its n and buffers)."""
    import bench as B
    import zkt_plonk_amd as z
    ctx = ctxs[cv.name]
    if ctx.circuit_log_n != LOG_N:
        ctx.srs_generate(0x10C0 + LOG_N, N + 8)
        circ = B.synthetic_circuit(B.FIELDS[cv.name], LOG_N)
        z.GpuProver.setup(ctx, LOG_N, {k: K.fr_to_mont(cv, circ["sel"][k]) for k in z.PK_ORDER})
    return ctx


def _first_diff(a, b):
    d = np.flatnonzero((a != b).any(axis=1))
    return int(d[0]) if d.shape[0] else -1


def _check(ctx, table, f, fresh, label):
    n = f.shape[0]
    w1, w2 = K.combine_split(LC.pad(table, n), f)
    assert w1.shape[0] == n and w2.shape[0] == n, label
    g1, g2 = ctx.debug_combine_split(table, f, fresh)
    assert np.array_equal(g1, w1), "%s: h1 differs first at %d" % (label, _first_diff(g1, w1))
    assert np.array_equal(g2, w2), "%s: h2 differs first at %d" % (label, _first_diff(g2, w2))


def _split_cases(ctx, rng, counts, zero_at=LC.ZERO_AT):
    """Every f pattern over each table: the first call uploads the keys, the others reuse them (fresh = 0, the path of
    proofs over an unchanged table), which needs the hit counts of the call before cleared."""
    seen = 0
    for label, table, fs in LC.cases(rng, N, counts, zero_at):
        for i, (kind, f) in enumerate(fs):
            _check(ctx, table, f, i == 0, "%s f=%s" % (label, kind))
            seen += 1
    return seen


@pytest.mark.parametrize("nkeys", LC.key_counts(N))
def test_split_matches_oracle_bn254(nkeys, ctxs):
    """Key counts on both sides of the scan chunks (1024, 2048), the LDS limit (8192) and n; 0 absent (the padding appends
    the zero key: with one key, an empty table), first, in the middle, last (the padding joins it)."""
    ctx = _split_ctx(ctxs, F.BN254)
    seen = _split_cases(ctx, np.random.default_rng(0x1000 + nkeys), [nkeys])
    assert seen == len(LC.F_KINDS) * (1 if nkeys == N else 4)


def test_split_largest_tables(ctxs):
    """table_len = n - 1, the largest a LookupTable<F, SIZE> may be (SIZE < n): 0 absent (n keys), first, middle, last."""
    ctx = _split_ctx(ctxs, F.BN254)
    rng = np.random.default_rng(0x1001)
    for z in LC.ZERO_AT:
        table = LC.make_table(rng, N if z == "absent" else N - 1, z)
        assert table.shape[0] == N - 1
        keys = LC.padded_keys(table)
        for i, kind in enumerate(LC.F_KINDS):
            _check(ctx, table, LC.make_f(rng, N, keys, kind), i == 0, "table_len=n-1 zero=%s f=%s" % (z, kind))


@pytest.mark.parametrize("nkeys", [1025, 8193])
def test_split_after_a_value_outside_the_table(nkeys, ctxs):
    """A looked-up value outside the table, first or last in f: ElementNotIndexedInTable (8).  The hits of the values
    that were found must not survive: the next call over the resident keys gives the oracle's halves (LDS histogram and
    global counters)."""
    import zkt_plonk_amd as z
    ctx = _split_ctx(ctxs, F.BN254)
    rng = np.random.default_rng(0x1002 + nkeys)
    table = LC.make_table(rng, nkeys, "middle")
    keys = LC.padded_keys(table)
    bad = LC.random_values(rng, 1, avoid=keys)[0]
    for at, fresh in ((0, True), (N - 1, False)):
        f = LC.make_f(rng, N, keys, "uniform")
        f[at] = bad
        with pytest.raises(z.ZktError) as e:
            ctx.debug_combine_split(table, f, fresh)
        assert e.value.code == 8, (at, e.value)
        _check(ctx, table, LC.make_f(rng, N, keys, "uniform"), False, "after code 8 (f[%d])" % at)
    # fresh = 0 with new f after good calls, then a fresh upload of the same table
    for i, kind in enumerate(("odd_straddle", "each_once", "uniform")):
        _check(ctx, table, LC.make_f(rng, N, keys, kind), i == 2, "again f=%s" % kind)


def test_split_refusals(ctxs):
    """table_len = n is refused with code 1 before anything runs (the resident keys stay); a table that holds a value
    twice (neighbours, far apart, 0 twice) with code 1 and no keys left resident, so that a following fresh = 0 call
    builds them from its own table.  So is a call while a next proof is announced, and one without a circuit (10)."""
    import zkt_plonk_amd as z
    from zkt_plonk_amd._lib import u64p
    ctx = _split_ctx(ctxs, F.BN254)
    rng = np.random.default_rng(0x1003)
    good = LC.make_table(rng, 2049, "first")
    keys = LC.padded_keys(good)
    _check(ctx, good, LC.make_f(rng, N, keys, "uniform"), True, "good table")
    f0 = np.zeros((N, 4), dtype=np.uint64)
    for i, table in enumerate([LC.make_table(rng, N, "middle"), LC.random_values(rng, N)]):
        with pytest.raises(z.ZktError) as e:
            ctx.debug_combine_split(table, f0, True)
        assert e.value.code == 1, (i, e.value)
        _check(ctx, good, LC.make_f(rng, N, keys, "uniform"), False, "after table_len = n (%d)" % i)
    rep = LC.make_table(rng, 9000, "absent")
    twins = [rep.copy(), rep.copy(), LC.make_table(rng, 1030, "last")]
    twins[0][101] = twins[0][100]
    twins[1][8500] = twins[1][3]
    twins[2][5] = 0
    for i, table in enumerate(twins):
        with pytest.raises(z.ZktError) as e:
            ctx.debug_combine_split(table, f0, True)
        assert e.value.code == 1 and "repeated" in str(e.value), (i, e.value)
        other = LC.make_table(rng, 1100 + i, "middle")
        _check(ctx, other, LC.make_f(rng, N, LC.padded_keys(other), "uniform"), False, "after repeated value %d" % i)
    # an announced next proof owns the work buffers
    prep = ctx.prepare_host(f0[:8], f0[:8], f0[:8], good, [], np.zeros((0, 4), dtype=np.uint64),
                            np.zeros((19, 4), dtype=np.uint64))
    ctx.check(ctx._L.zkt_prove_set_next(ctx.handle, ctypes.byref(prep.struct)))
    try:
        with pytest.raises(z.ZktError) as e:
            ctx.debug_combine_split(good, f0, True)
        assert e.value.code == 1 and "announced" in str(e.value)
    finally:
        ctx.check(ctx._L.zkt_prove_set_next(ctx.handle, None))
    _check(ctx, good, f0, True, "after the announcement is withdrawn")
    bare = z.Context(F.BN254.name, 0)
    try:
        h = np.empty((N, 4), dtype=np.uint64)
        P64 = ctypes.POINTER(ctypes.c_uint64)
        bare._L.zkt_debug_combine_split.argtypes = [ctypes.c_void_p, P64, ctypes.c_size_t, P64, ctypes.c_int, P64, P64]
        assert bare._L.zkt_debug_combine_split(bare.handle, u64p(good), good.shape[0], u64p(f0), 1, u64p(h), u64p(h)) == 10
        with pytest.raises(ValueError):
            bare.debug_combine_split(good, f0)
    finally:
        bare.close()


def test_split_matches_oracle_bls12_381(ctxs):
    """BLS12-381: past one chunk (1025 keys), past the LDS histogram (8193) and the largest table, 0 in the middle."""
    cv = F.BLS12_381
    ctx = _split_ctx(ctxs, cv)
    rng = np.random.default_rng(0x1004)
    assert _split_cases(ctx, rng, [1025, 8193], ("middle",)) == 2 * len(LC.F_KINDS)
    table = LC.make_table(rng, N - 1, "middle")
    for i, kind in enumerate(LC.F_KINDS):
        _check(ctx, table, LC.make_f(rng, N, LC.padded_keys(table), kind), i == 0, "table_len=n-1 f=%s" % kind)


# ---- whole proofs -------------------------------------------------------------------------------------------------

def _workload(z, ctx, cv, log_n, table_size, value_seeds, tau):
    """bench.py's synthetic circuit with a `table_size` table, set up on the device; one witness per value seed (same
    selectors and table).  -> (evals, [witness dicts], vk, srs)."""
    import bench as B
    n = 1 << log_n
    ctx.srs_generate(tau, n + 8)
    circs = [B.synthetic_circuit(B.FIELDS[cv.name], log_n, table_size=table_size, value_seed=v) for v in value_seeds]
    for c in circs[1:]:
        assert c["sel"] == circs[0]["sel"] and c["table"] == circs[0]["table"]
    assert len(circs[0]["table"]) == table_size - 1
    evals = {name: K.fr_to_mont(cv, circs[0]["sel"][name]) for name in z.PK_ORDER}
    _, commits = z.GpuProver.setup(ctx, log_n, evals)
    L, q = cv.fq.limbs64, cv.fq.p
    rinv = pow(1 << (64 * L), -1, q)
    pts = {}
    for name in z.PK_ORDER:
        xy, inf = commits[name]
        pts[name] = None if inf else (sum(int(v) << (64 * i) for i, v in enumerate(xy[:L])) * rinv % q,
                                      sum(int(v) << (64 * i) for i, v in enumerate(xy[L:])) * rinv % q)
    table = K.fr_to_mont(cv, circs[0]["table"])
    ws = []
    for circ in circs:
        gates = circ["gates"]
        pi_pos = sorted(circ["pi"])
        ws.append(dict(a=K.fr_to_mont(cv, circ["a"][:gates]), b=K.fr_to_mont(cv, circ["b"][:gates]),
                       c=K.fr_to_mont(cv, circ["c"][:gates]), table=table, pi=circ["pi"], pi_pos=pi_pos,
                       pi_vals=K.fr_to_mont(cv, [circ["pi"][k] for k in pi_pos]),
                       lookup_rows=[i for i, v in enumerate(circ["sel"]["q_lookup"]) if v]))
    vk = P.VerifierKey(n, [pow(cv.fr.root_of_unity(n), i, cv.fr.p) for i in ws[0]["pi_pos"]], pts)
    return evals, ws, vk, ctx.srs_download(0, n + 8)


class _Prover:
    """The GPU and the CPU oracle on one circuit: prepared inputs of a witness, the oracle's bytes (verified)."""

    def __init__(self, z, ctx, cv, log_n, evals, vk, srs, tau):
        from oracle import fastplonk as FP
        self.z, self.ctx, self.cv, self.vk, self.srs, self.tau, self.FP = z, ctx, cv, vk, srs, tau, FP
        self.keys = FP.setup(cv, srs, log_n, evals, commitments=False)

    def tr(self):
        t = self.z.Transcript("merlin", "ZKT Plonk", fr_bits=self.cv.fr.bits, fq_bytes=8 * self.cv.fq.limbs64)
        return self.z.seed_transcript(t, self.vk.n, self.vk.commits)

    def prep(self, w, blinders):
        return self.ctx.prepare_host(w["a"], w["b"], w["c"], w["table"], w["pi_pos"], w["pi_vals"],
                                     K.fr_to_mont(self.cv, blinders))

    def want(self, w, blinders):
        cv = self.cv
        got = self.FP.prove(cv, self.srs, self.keys, w["a"], w["b"], w["c"], w["table"], w["pi"],
                            P.new_seeded_transcript(cv, self.vk), blinders)
        assert P.verify(cv, self.tau, self.vk, P.proof_deserialize(cv, got), P.new_seeded_transcript(cv, self.vk),
                        [w["pi"][k] for k in w["pi_pos"]])
        return got


def test_proofs_over_a_65536_key_table_bn254(ctxs):
    """n = 2^17 with a 2^16-entry table (65 535 values + the zero key: 64 scan chunks, global counters), every proof equal
    to the oracle's bytes: an announced second witness; the same values in another insertion order (a new table to
    table_is_cached); a looked-up value outside the table (8) over the resident keys, then the first witness over them;
    the split alone on another table in between (stale-key guard); the first proof sharded over two thread ranks."""
    import zkt_plonk_amd as z
    from test_gpu_prove import _sharded_legs
    cv = F.BN254
    ctx = ctxs[cv.name]
    log_n, tau = 17, 0x7AB1E17
    n = 1 << log_n
    evals, (w0, w1), vk, srs = _workload(z, ctx, cv, log_n, 1 << 16, (1, 2), tau)
    pv = _Prover(z, ctx, cv, log_n, evals, vk, srs, tau)
    bl = [field_elems(cv.fr.p, 1700 + k, P.NUM_BLINDERS) for k in range(3)]
    want0, want1 = pv.want(w0, bl[0]), pv.want(w1, bl[1])
    p0, p1 = pv.prep(w0, bl[0]), pv.prep(w1, bl[1])
    assert ctx.prove_prepared(p0, pv.tr(), p1) == want0
    assert ctx.prove_prepared(p1, pv.tr()) == want1
    # the same values in another insertion order: t, h1, h2 change, their lengths do not
    wr = dict(w0, table=w0["table"][np.random.default_rng(17).permutation(w0["table"].shape[0])])
    assert not np.array_equal(wr["table"], w0["table"])
    assert ctx.prove_prepared(pv.prep(wr, bl[2]), pv.tr()) == pv.want(wr, bl[2])
    assert ctx.prove_prepared(p0, pv.tr()) == want0      # the original order is a new table again
    # a failed proof over the resident keys: its hits must not reach the next proof over them
    row = w0["lookup_rows"][len(w0["lookup_rows"]) // 2]
    bad_v = LC.random_values(np.random.default_rng(18), 1, avoid=w0["table"])[0]
    wb = dict(w0, a=w0["a"].copy(), c=w0["c"].copy())
    wb["a"][row] = bad_v
    wb["c"][row] = bad_v
    with pytest.raises(z.ZktError) as e:
        ctx.prove_prepared(pv.prep(wb, bl[0]), pv.tr())
    assert e.value.code == 8, e.value
    assert ctx.prove_prepared(p0, pv.tr()) == want0
    # the split alone on another table leaves other keys resident: the next proof must not take them for its own
    other = LC.make_table(np.random.default_rng(19), 3000, "absent")
    ctx.debug_combine_split(other, np.zeros((n, 4), dtype=np.uint64))
    assert ctx.prove_prepared(p0, pv.tr()) == want0
    _sharded_legs(z, cv, n, srs, evals, vk, w0, bl[0], want0, (2,))


def test_proof_over_a_32768_key_table_bls12_381(ctxs):
    """BLS12-381, n = 2^16, bench.py's table at table_size 2^15 (32 767 values + the zero key)."""
    import zkt_plonk_amd as z
    cv = F.BLS12_381
    ctx = ctxs[cv.name]
    log_n, tau = 16, 0xB15AB1E
    evals, (w,), vk, srs = _workload(z, ctx, cv, log_n, 1 << 15, (3,), tau)
    pv = _Prover(z, ctx, cv, log_n, evals, vk, srs, tau)
    bl = field_elems(cv.fr.p, 1800, P.NUM_BLINDERS)
    assert ctx.prove_prepared(pv.prep(w, bl), pv.tr()) == pv.want(w, bl)


def test_proof_with_zero_in_the_table_bn254(ctxs):
    """n = 2^14, the 1023 values of bench.py's table with 0 inserted (table_len = table_size = 1024 < n): the padding
    joins the zero key inside the table.  First or last (where it is the proof without it), the proof equals the
    oracle's.  At table_size // 2 the
    reference itself has no proof: combine_split gathers every padding zero at the table's 0, so h1 / h2 are no longer
    t with f merged in, z2 does not close and the quotient outgrows 3n + 5 -- the oracle fails, the device reports 9.
    A table that holds a value twice is refused (code 1)."""
    import zkt_plonk_amd as z
    cv = F.BN254
    ctx = ctxs[cv.name]
    log_n, tau = 14, 0x2E80
    evals, (w,), vk, srs = _workload(z, ctx, cv, log_n, 1024, (4,), tau)
    pv = _Prover(z, ctx, cv, log_n, evals, vk, srs, tau)
    bl = field_elems(cv.fr.p, 1900, P.NUM_BLINDERS)
    plain = pv.want(w, bl)
    proofs = {}
    for pos in (0, 1023):
        wz = dict(w, table=np.insert(w["table"], pos, 0, axis=0))
        assert wz["table"].shape[0] == 1024
        proofs[pos] = pv.want(wz, bl)
        assert ctx.prove_prepared(pv.prep(wz, bl), pv.tr()) == proofs[pos]
    assert proofs[1023] == plain and proofs[0] != plain    # a 0 last is the padding's own zero key
    wz = dict(w, table=np.insert(w["table"], 512, 0, axis=0))
    with pytest.raises(ValueError, match="TooManyCoefficients"):
        pv.want(wz, bl)
    with pytest.raises(z.ZktError) as e:
        ctx.prove_prepared(pv.prep(wz, bl), pv.tr())
    assert e.value.code == 9, e.value
    twice = w["table"].copy()
    twice[700] = twice[20]
    with pytest.raises(z.ZktError) as e:
        ctx.prove_prepared(pv.prep(dict(w, table=twice), bl), pv.tr())
    assert e.value.code == 1 and "repeated" in str(e.value)
    assert ctx.prove_prepared(pv.prep(w, bl), pv.tr()) == plain
