"""Whole proofs under the key lengths callers really load.  The reference trims its committer key to 4 * circuit_bound()
coefficients (plonk-core/src/plonk.rs:79-85), a service loads a universal key longer still -- and much of the device path is
decided by the KEY's length, not the circuit's: the digit width and window count (msm.hip msm_setup), the launch regime
(msm.hpp MSM_DEFER_MAX / MSM_TAIL_INL_MAX, msm_batches_grouping), the layout of the Lagrange and wire-base tables (laid out
with the big key's plan, n + min(count - n, 8) bases long) and the size of every MSM work buffer.  A small circuit under a
long key reaches each combination in milliseconds: tests/key_length_cases.py lists the keys.  The oracle's bytes do not
depend on the key's length (tests/test_key_length_cases_host.py), so its setup and proofs are made once per curve from the
first n + 8 powers; every comparison is byte for byte."""
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import fields as F, plonk as P, coracle as K
from helpers import field_elems, run_sharded_ranks, sharded_exchange_bytes
import key_length_cases as KL
import wire_elim_cases as W

CURVES = [F.BN254, F.BLS12_381]
N, LOG_N = KL.N, KL.LOG_N
TAU = 0x4B65794C656E67746873          # one trapdoor for every key of this file
TOO_MANY_COEFFICIENTS = 5             # ZKT_ERR_TOO_MANY_COEFFICIENTS (include/zkt_plonk.h)
WIRE_ELIMINATION_MODES = (2, 0, 1)    # include/zkt_plonk.h zkt_ctx_set_wire_elimination: always, off, automatic (the default, last)


def _mont(cv, v):
    return K.fr_to_mont(cv, v) if len(v) else np.zeros((0, 4), dtype=np.uint64)


def _make_fixture(cv):
    """The circuit, its oracle setup under the first n + 8 powers, two oracle proofs (two blinder sets: the chained legs
    need a successor that differs), and everything the device is handed, in Montgomery words."""
    cs = P.synthetic_circuit(cv, 700, 32, seed=4242)
    assert cs.check_satisfied() and cs.circuit_bound() == N and cs.table and cs.pi
    srs = K.srs_mont(cv, TAU, N + 8)
    be = K.CBackend(cv, srs)
    pk, epk, vk = P.setup(be, [None] * (N + 8), cs, True)
    blinders = [field_elems(cv.fr.p, 0xB11D + k, P.NUM_BLINDERS) for k in range(2)]
    proofs = [P.prove(be, [None] * (N + 8), pk, epk, vk, cs, P.new_seeded_transcript(cv, vk), b) for b in blinders]
    pi_pos = sorted(cs.pi)
    pis = [cs.pi[k] for k in pi_pos]
    for pr in proofs:
        assert P.verify(cv, TAU, vk, pr, P.new_seeded_transcript(cv, vk), pis)
    # what lagrange.hip decides per wire for this wiring: over free variables where that shrinks the wire (route 2), else
    # over its distinct variables when those are fewer than 0.9 of the rows (route 1), else densely (0)
    routes2 = W.predicted_routes(cs, *W.eliminate(cv, cs))
    routes1 = [1 if len({v for v in ws if v != P.ZERO_VAR}) < W.MAX_FRAC * cs.n_gates else 0 for ws in (cs.w_l, cs.w_r, cs.w_o)]
    assert routes2 == [2, 2, 2] and routes1 == [1, 1, 0]
    return types.SimpleNamespace(
        cv=cv, cs=cs, srs=srs, vk=vk, pis=pis, blinders=blinders, proofs=proofs, want=[p.serialize(cv) for p in proofs],
        evals={k: _mont(cv, v) for k, v in P.setup_evals(be, cs).items()},
        wires=[_mont(cv, w) for w in cs.wire_evals(cs.n_gates)], values=_mont(cv, cs.values),
        idx=[W.to_idx(w) for w in (cs.w_l, cs.w_r, cs.w_o)], table=_mont(cv, cs.table), pi_pos=pi_pos, pi_vals=_mont(cv, pis),
        blinders_mont=[_mont(cv, b) for b in blinders], routes1=routes1, routes2=routes2)


@pytest.fixture(scope="module")
def fx():
    made = {}

    def get(cv):
        if cv.name not in made:
            made[cv.name] = _make_fixture(cv)
        return made[cv.name]

    return get


def _transcript(z, cv, vk):
    return z.seed_transcript(z.Transcript("merlin", "ZKT Plonk", fr_bits=cv.fr.bits, fq_bytes=cv.fq.limbs64 * 8), vk.n, vk.commits)


def _setup_commits_equal(z, cv, commits, vk):
    """GpuProver.setup's ten commitments against the oracle's VerifierKey"""
    for k, name in enumerate(z.PK_ORDER):
        xy, inf = commits[name]
        want = vk.commits[name]
        got = None if inf else K.points_from_mont(cv, np.asarray(xy).reshape(1, -1))[0]
        assert got == want, name


def _point(cv, xy, inf):
    return None if inf else K.points_from_mont(cv, np.asarray(xy).reshape(1, -1))[0]


ALL = [(cv.name, c.name) for cv in CURVES for c in KL.cases_for(cv.name)]


@pytest.mark.parametrize("cvname,key", ALL, ids=["%s-%s" % x for x in ALL])
def test_whole_proofs_under_every_key_length(cvname, key, fx):
    import zkt_plonk_amd as z
    cv = F.CURVES[cvname]
    f = fx(cv)
    case = KL.BY_NAME[key]
    count = case.count
    bits, windows = case.digits[cvname]
    want_bases = KL.lagrange_bases(count)
    tr = lambda: _transcript(z, cv, f.vk)
    ctx = z.Context(cv.name, 0)
    forks = []
    try:
        ctx.srs_generate(TAU, count)
        assert np.array_equal(ctx.srs_download(0, N + 8 if count >= N + 8 else count), f.srs[:min(count, N + 8)])
        assert ctx.msm_info() == dict(window_bits=bits, windows=windows, srs_count=count)
        # the ten VerifierKey commitments: MSMs of n scalars under the long key
        prover, commits = z.GpuProver.setup(ctx, LOG_N, f.evals)
        _setup_commits_equal(z, cv, commits, f.vk)
        # the witness in the composer's layout, resident in HBM (the form that reaches the wire-base tables), and as three
        # host evaluation vectors
        d_vars = ctx.alloc(f.values.nbytes)
        ctx.upload(d_vars, f.values)
        d_idx = []
        for w in f.idx:
            d_idx.append(ctx.alloc(w.nbytes))
            ctx.upload(d_idx[-1], w)
        dev = [ctx.prepare_vars_dev(d_vars, f.values.shape[0], d_idx[0], d_idx[1], d_idx[2], f.cs.n_gates, f.table, f.pi_pos,
                                    f.pi_vals, b) for b in f.blinders_mont]
        host = ctx.prepare_host(f.wires[0], f.wires[1], f.wires[2], f.table, f.pi_pos, f.pi_vals, f.blinders_mont[0])

        # Under n + 1 and n + 2 powers the reference refuses the proof (a polynomial with three blinders is longer than the
        # key: kzg10 TooManyCoefficients), and so must every route here; the legs are the same, the expected outcome the code.
        want = f.want if case.proves else [TOO_MANY_COEFFICIENTS] * 2
        info = dict(log_n=LOG_N, bases=want_bases)

        def attempt(c, prep, nxt=None):
            try:
                return c.prove_prepared(prep, tr(), nxt)
            except z.ZktError as err:
                return err.code

        def chained(c, what):
            assert attempt(c, dev[0], dev[1]) == want[0], (what, "announcing proof")
            assert attempt(c, dev[1]) == want[1], (what, "announced proof")

        forks.append(ctx.fork())                              # made before the first proof: builds its own tables
        got = attempt(ctx, dev[0])                            # the default route
        assert got == want[0], "default route, witness as variables in HBM"
        if case.proves:
            assert ctx.lagrange_info() == info
            assert P.verify(cv, TAU, f.vk, P.proof_deserialize(cv, got), P.new_seeded_transcript(cv, f.vk), f.pis)
        assert attempt(ctx, host) == want[0], "default route, host evaluation vectors"
        forks.append(ctx.fork())                              # made after it: reads the parent's tables
        for which, fk in zip(("fork made before the first proof", "fork made after the first proof"), forks):
            assert fk.msm_info() == ctx.msm_info(), which
            assert attempt(fk, dev[0]) == want[0], which
            assert not case.proves or fk.lagrange_info() == info, which
            chained(fk, which)
        while forks:
            forks.pop().close()
        # Every change of route below rebuilds the wire tables (a third of a second on BLS12-381, far more than a proof at
        # this size), so the legs are ordered to change it as seldom as they can: the tables the first proof built, the
        # coefficients, the tables over free variables (commitments, then proofs), the tables of modes 0 and 1, and last the
        # Lagrange switch, which drops them all.
        chained(ctx, "parent")
        # round 1 alone on each route of the wire commitments, against the oracle proof's a, b, c (two blinders a wire:
        # n + 2 coefficients, which a key of n + 1 powers cannot hold).  The wire tables need two blinder bases in the
        # second table as well; a shorter key leaves every wire on its coefficients.
        want_abc = [f.proofs[0].commits[k] for k in ("a", "b", "c")]
        for route, routed in ((1, f.routes1), (0, [0, 0, 0]), (2, f.routes2)):
            try:
                xy, inf, took = ctx.debug_commit_wires_dev(d_vars, f.values.shape[0], d_idx[0], d_idx[1], d_idx[2], f.cs.n_gates,
                                                           f.blinders_mont[0][:6], route, f.pi_pos)
            except z.ZktError as err:
                assert count < N + 2 and err.code == TOO_MANY_COEFFICIENTS, ("wire commitments, route", route, err)
                continue
            assert count >= N + 2, "committed wire polynomials longer than the key"
            assert [_point(cv, xy[k], inf[k]) for k in range(3)] == want_abc, ("wire commitments, route", route)
            assert took == routed, ("routes taken, route", route, took)
        for mode in WIRE_ELIMINATION_MODES:
            ctx.set_wire_elimination(mode)
            assert attempt(ctx, dev[0]) == want[0], ("set_wire_elimination", mode)
            if mode == 2:                                     # the tables over free variables under an announcement as well
                chained(ctx, "set_wire_elimination(2)")
            assert not case.proves or ctx.lagrange_info() == info
        ctx.set_lagrange(False)
        assert ctx.lagrange_info()["log_n"] == -1
        assert attempt(ctx, dev[0]) == want[0], "set_lagrange(False)"
        ctx.set_lagrange(True)
        assert attempt(ctx, dev[0]) == want[0], "set_lagrange(True) again"
        assert not case.proves or ctx.lagrange_info() == info
        assert ctx.msm_info() == dict(window_bits=bits, windows=windows, srs_count=count)
        for d in [d_vars] + d_idx:
            ctx.free(d)
    finally:
        for fk in forks:
            fk.close()
        ctx.close()


# ---- commitments of evaluation vectors ------------------------------------------------------------------------------------

def _evals_keys(n):
    return {"n+1": n + 1, "n+2": n + 2, "n+9": n + 9, "4n+1": 4 * n + 1, "2^17+65": (1 << 17) + 65}


@pytest.fixture(scope="module")
def evals_fx():
    """per (curve, log_n): a circuit of that domain (the call takes its domain from the loaded circuit), the vectors of
    tests/test_gpu_lagrange.py and the oracle's coefficient-form commitment of each with 0 .. 3 blinders"""
    from test_gpu_lagrange import _vectors, _oracle_commit
    made = {}

    def get(cv, log_n):
        if (cv.name, log_n) not in made:
            n = 1 << log_n
            cs = P.synthetic_circuit(cv, n - 3, 4, seed=log_n, n_public=2)
            assert cs.circuit_bound() == n
            srs = K.srs_mont(cv, TAU, n + 8)
            pk, epk, vk = P.setup(K.CBackend(cv, srs), [None] * (n + 8), cs, True)
            pkm = {k: _mont(cv, pk.polys[k]) for k in pk.polys}
            bl = field_elems(cv.fr.p, 4242, 3)
            vectors = _vectors(cv, log_n)
            want, length = {}, {}
            for name, ev in vectors.items():
                coeffs = K.fr_from_mont(cv, K.ntt_mont(cv, log_n, True, False, K.fr_to_mont(cv, ev)))
                while coeffs and coeffs[-1] == 0:
                    coeffs.pop()
                for k in range(4):
                    want[name, k] = _oracle_commit(cv, log_n, srs, ev, bl[:k])
                    length[name, k] = len(coeffs) + k      # coefficients of the blinded polynomial as kzg10 sees them
            made[cv.name, log_n] = types.SimpleNamespace(n=n, srs=srs, pkm=pkm, bl=bl, vectors=vectors, want=want, length=length)
        return made[cv.name, log_n]

    return get


@pytest.mark.parametrize("cv", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("key", KL.COMMIT_EVALS_KEYS)
def test_commit_evals_under_long_and_barely_long_enough_keys(cv, key, evals_fx):
    """zkt_commit_evals_dev on both paths, 0 .. 3 blinders, at log_n 3, 6 and 10 (n = the domain of each).  A key of n + 1 or
    n + 2 powers has fewer spare bases than a polynomial may have blinders: where the blinded polynomial is longer than the
    key the reference refuses (kzg10 TooManyCoefficients) and so must both paths, as tests/test_gpu_lagrange.py pins for a
    key without the bases a call needs; the device commits the fixed length n + k, so it may also refuse a vector whose
    coefficients were trimmed short enough to fit -- but it never returns another point than the oracle's."""
    import zkt_plonk_amd as z
    ctx = z.Context(cv.name, 0)
    try:
        for log_n in (3, 6, 10):
            e = evals_fx(cv, log_n)
            n = e.n
            count = _evals_keys(n)[key]
            if key != "2^17+65" or log_n == 3:        # the absolute key is generated once; the circuits change under it
                ctx.srs_generate(TAU, count)
                head = min(count, n + 8)
                assert np.array_equal(ctx.srs_download(0, head), e.srs[:head])
            assert ctx.msm_info()["srs_count"] == count
            z.GpuProver(ctx, log_n, e.pkm)
            spare = count - n
            d_ev = ctx.alloc(n * 32)
            for name, ev in e.vectors.items():
                ctx.upload(d_ev, K.fr_to_mont(cv, ev))
                for k in range(4):
                    bl = K.fr_to_mont(cv, e.bl[:k]) if k else None
                    for path in (0, 1):
                        what = (log_n, name, k, path)
                        if k <= spare:
                            out, inf = ctx.commit_evals_dev(d_ev, bl, path)
                            assert _point(cv, out, inf) == e.want[name, k], what
                            continue
                        try:
                            out, inf = ctx.commit_evals_dev(d_ev, bl, path)
                        except z.ZktError as err:
                            assert err.code == TOO_MANY_COEFFICIENTS, what
                            continue
                        assert e.length[name, k] <= count, ("committed a polynomial longer than the key", what)
                        assert _point(cv, out, inf) == e.want[name, k], what
            assert ctx.lagrange_info() == dict(log_n=log_n, bases=n + min(spare, 8))
            ctx.free(d_ev)
    finally:
        ctx.close()


# ---- the reference's own shape at the sizes where it changes regime ---------------------------------------------------------

# 4n + 1 powers: n = 2^14 -> 2^16 + 1 (14-bit digits, deferred), 2^15 -> 2^17 + 1 (17 / 16-bit digits, the ungrouped gap),
# 2^16 -> 2^18 + 1 (grouped, inlined tail additions)
REFERENCE_SHAPE = [("bn254", 14, (14, 19)), ("bn254", 15, (17, 15)), ("bn254", 16, (17, 15)), ("bls12_381", 15, (16, 16))]


@pytest.mark.parametrize("cvname,log_n,digits", REFERENCE_SHAPE, ids=["%s-2^%d" % x[:2] for x in REFERENCE_SHAPE])
def test_bench_workload_under_the_reference_key_of_4n_plus_1(cvname, log_n, digits):
    """bench.py's circuit proved under the key the reference would trim for it, against the CPU oracle's array prover on the
    first n + 8 powers."""
    import zkt_plonk_amd as z
    from oracle import fastplonk as FP
    from test_gpu_prove import _bench_workload, _check_srs_ends, _gpu_prove_arrays
    cv = F.CURVES[cvname]
    n = 1 << log_n
    tau = 0x5EED5EED1234567890ABCDEF % cv.fr.p
    ctx = z.Context(cv.name, 0)
    try:
        evals, w, vk = _bench_workload(z, ctx, cv, log_n, tau, key_count=4 * n + 1)
        assert ctx.msm_info() == dict(window_bits=digits[0], windows=digits[1], srs_count=4 * n + 1)
        srs = ctx.srs_download(0, n + 8)
        _check_srs_ends(cv, tau, srs)
        keys = FP.setup(cv, srs, log_n, evals, commitments=log_n <= 14)
        if log_n <= 14:
            assert keys.commits == vk.commits
        else:
            for name in ("q_c", "sigma3"):
                assert FP.commit(cv, srs, keys.pk[name]) == vk.commits[name], name
        blinders = field_elems(cv.fr.p, 4100 + log_n, P.NUM_BLINDERS)
        want = FP.prove(cv, srs, keys, w["a"], w["b"], w["c"], w["table"], w["pi"], P.new_seeded_transcript(cv, vk), blinders)
        got = _gpu_prove_arrays(z, ctx, cv, w, vk, blinders)
        assert got == want
        assert ctx.lagrange_info() == dict(log_n=log_n, bases=n + 8)
        assert _gpu_prove_arrays(z, ctx, cv, w, vk, blinders) == want         # once more on warm tables
        pis = [w["pi"][k] for k in w["pi_pos"]]
        assert P.verify(cv, tau, vk, P.proof_deserialize(cv, got), P.new_seeded_transcript(cv, vk), pis)
    finally:
        ctx.close()


# ---- the key file, whole ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cv", CURVES, ids=lambda c: c.name)
def test_prove_from_the_whole_reference_cli_key_file(cv, tmp_path):
    """tests/test_gpu_prove.py::test_prove_from_the_reference_cli_key_files with the committer key loaded as the reference
    wrote it: all 4n + 1 powers (max_powers = 0), not its first n + 8."""
    import zkt_plonk_amd as z
    from zkt_plonk_amd import _lib
    from oracle import keyfile as KF
    cs = P.synthetic_circuit(cv, 1500, 64, seed=404)
    n = cs.circuit_bound()
    tau = 0xF11E5
    srs_arr = K.srs_mont(cv, tau, 4 * n + 1)             # PC::trim keeps 4n + 1 powers (plonk.rs:79-85)
    be = K.CBackend(cv, srs_arr)
    pk, epk, vk = P.setup(be, [None] * (4 * n + 1), cs, True)
    blinders = field_elems(cv.fr.p, 61, P.NUM_BLINDERS)
    want = P.prove(be, [None] * (4 * n + 1), pk, epk, vk, cs, P.new_seeded_transcript(cv, vk), blinders).serialize(cv)
    (tmp_path / "ck").write_bytes(KF.committer_key_bytes(cv, K.points_from_mont(cv, srs_arr)))
    (tmp_path / "pk").write_bytes(KF.prover_key_bytes(cv, pk))
    (tmp_path / "vk").write_bytes(KF.verifier_key_bytes(cv, vk))
    ctx = z.Context(cv.name, 0)
    try:
        ctx.srs_load_file(str(tmp_path / "ck"), max_powers=0)
        assert ctx.msm_info()["srs_count"] == 4 * n + 1
        assert np.array_equal(ctx.srs_download(0, 4 * n + 1), srs_arr)
        ctx.circuit_load_file(str(tmp_path / "pk"), n.bit_length() - 1)
        n_, roots, commits, inf = _lib.keyfile_verifier_key(str(tmp_path / "vk"), cv.name)
        pts = {name: (None if inf[k] else K.points_from_mont(cv, commits[k:k + 1])[0]) for k, name in enumerate(z.PK_ORDER)}
        a, b, c = cs.wire_evals(cs.n_gates)
        pos = sorted(cs.pi)
        for rep in range(2):                              # the second proof on the tables the first one built
            tr = z.Transcript("merlin", "ZKT Plonk", fr_bits=cv.fr.bits, fq_bytes=cv.fq.limbs64 * 8)
            z.seed_transcript(tr, n_, pts)
            got = ctx.prove(K.fr_to_mont(cv, a), K.fr_to_mont(cv, b), K.fr_to_mont(cv, c), K.fr_to_mont(cv, cs.table), pos,
                            K.fr_to_mont(cv, [cs.pi[i] for i in pos]), K.fr_to_mont(cv, blinders), tr)
            assert got == want, rep
        assert ctx.lagrange_info() == dict(log_n=n.bit_length() - 1, bases=n + 8)
    finally:
        ctx.close()


# ---- the KZG seam: short polynomials in the non-deferred and in the grouped regime -------------------------------------------

@pytest.mark.parametrize("cv", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("count", KL.KZG_SEAM_COUNTS, ids=["2^16+65", "2^18+1"])
def test_kzg_seam_with_short_polynomials_under_a_long_key(cv, count):
    """zkt_kzg_commit_batch and zkt_kzg_open with the ragged lengths of tests/test_gpu_kzg_seam.py capped at n + 6 (what a
    proof at n = 2^10 commits), under a key whose regime a key of n + 8 powers never reaches."""
    import zkt_plonk_amd as z
    import test_gpu_kzg_seam as S
    top = N + 6
    want_srs = K.srs_mont(cv, TAU, N + 8)
    ctx = z.Context(cv.name, 0)
    try:
        ctx.srs_generate(TAU, count)
        assert ctx.msm_info()["srs_count"] == count
        srs = ctx.srs_download(0, N + 8)
        assert np.array_equal(srs, want_srs)
        for k in (1, 7, 32):
            rng = np.random.default_rng(300 + k)
            polys = [S._fr(cv, m, rng) for m in S._lens(k, top, rng)]
            for mont in (True, False):
                got = ctx.kzg_commit_batch(polys, montgomery=mont)
                d = S._upload_all(ctx, polys)
                try:
                    got_dev = ctx.kzg_commit_batch_dev(d, [p.shape[0] for p in polys], montgomery=mont)
                finally:
                    S._free_all(ctx, d)
                for j, p in enumerate(polys):
                    want = S._oracle_commit(cv, srs, p, mont)
                    assert S._same(got[j], want), "entry %d of %d (len %d, montgomery %s)" % (j, k, p.shape[0], mont)
                    assert S._same(got_dev[j], want), "_dev entry %d of %d (len %d, montgomery %s)" % (j, k, p.shape[0], mont)
        for k in (1, 10, 32):
            rng = np.random.default_rng(400 + k)
            lens = S._lens(k, top, rng) if k > 1 else [top]
            polys = [S._fr(cv, m, rng) for m in lens]
            ch = S._fr(cv, k, rng)
            if k > 2:
                ch[1] = 0
                ch[2] = ch[0]
            for name, zm in S._points(cv, rng):
                (w, inf), ev = ctx.kzg_open(polys, ch, zm)
                want_w, want_ev = S._oracle_open(cv, srs, polys, ch, zm)
                assert S._same((w, inf), want_w), "witness, k = %d, z = %s" % (k, name)
                assert np.array_equal(ev, want_ev), "evaluations, k = %d, z = %s" % (k, name)
            d = S._upload_all(ctx, polys)
            try:
                (w, inf), ev = ctx.kzg_open_dev(d, lens, ch, zm)
            finally:
                S._free_all(ctx, d)
            assert S._same((w, inf), want_w) and np.array_equal(ev, want_ev), "_dev, k = %d" % k
    finally:
        ctx.close()


# ---- one proof across ranks whose key slices lie above every polynomial -----------------------------------------------------

@pytest.mark.parametrize("cv", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("world", [2, 4])
def test_sharded_proof_under_the_reference_key_of_4n_plus_1(cv, world, fx):
    """The key of 4n + 1 powers cut into `world` slices: every polynomial of the proof (at most n + 6 coefficients) ends
    inside the first ranks' slices, so the upper ranks commit to nothing at all (prover.hip commit_begin) and still take
    part in every exchange.  Every rank's bytes are the oracle's; the exchanged bytes are the design's."""
    import zkt_plonk_amd as z
    from zkt_plonk_amd import parallel as par
    f = fx(cv)
    total = 4 * N + 1
    srs_arr = K.srs_mont(cv, TAU, total)
    assert np.array_equal(srs_arr[:N + 8], f.srs)
    assert par.shard_range(total, world - 1, world)[0] >= N + 8       # the last rank's slice starts above every polynomial
    jobs = [(f.wires[0], f.wires[1], f.wires[2], f.table, f.pi_pos, f.pi_vals, b) for b in f.blinders_mont]
    out = run_sharded_ranks(z, cv, N, srs_arr, {"evals": f.evals}, f.vk, jobs, world, key_total=total)
    xyzz = 4 * cv.fq.limbs64 * 8
    for r in range(world):
        proofs, (calls, sent), (setup_calls, setup_sent) = out[r]
        assert proofs == f.want, (world, r)
        assert (setup_calls, setup_sent) == (2, 10 * xyzz), (world, r)
        assert calls == 2 + 5 * len(jobs), (world, r)
        assert sent - setup_sent == sharded_exchange_bytes(cv, N, world, len(jobs)), (world, r)
