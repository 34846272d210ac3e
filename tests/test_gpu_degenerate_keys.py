"""GPU: committing, proving and verifying under the degenerate committer keys of tests/degenerate_keys.py -- keys under which
the key-derived tables (csrc/lagrange.hip, msm_table_finish) and the bucket accumulation meet equal bases, opposite bases
and bases at infinity, and honest proofs carry identity commitments.  Every comparison is bit for bit against the CPU
oracle (or against the coefficient route the oracle pins, for the wire routes); tests/test_degenerate_keys_oracle.py pins
the table itself.  tau = 0 is left out of the verifier legs (beta_h is then the G2 identity)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import plonk as P, coracle as K
from helpers import field_elems, rand_fr
import degenerate_keys as DK
import wire_elim_cases as W
import test_gpu_lagrange as TL
import test_gpu_wire_bases as WB
import test_gpu_wire_elimination as WE
import test_gpu_kzg_seam as KS

CURVES = DK.CURVES
CV_IDS = lambda c: c.name  # noqa: E731
by_case = pytest.mark.parametrize("case", DK.CASES, ids=DK.IDS)
by_curve = pytest.mark.parametrize("cv", CURVES, ids=CV_IDS)


@pytest.fixture(scope="module")
def ctxs():
    import zkt_plonk_amd as z
    c = {cv.name: z.Context(cv.name, 0) for cv in CURVES}
    yield c
    for x in c.values():
        x.close()


def _cv(name):
    return next(c for c in CURVES if c.name == name)


@functools.lru_cache(maxsize=None)
def _pk_polys(cv_name, gates, table, seed, n_public):
    """the prover key's polynomials of a synthetic circuit (they do not depend on the committer key) -> (cs, polys)"""
    import zkt_plonk_amd as z
    cv = _cv(cv_name)
    cs = P.synthetic_circuit(cv, gates, table, seed=seed, n_public=n_public)
    n = cs.circuit_bound()
    pk, _, _ = P.setup(K.CBackend(cv, K.srs_mont(cv, 0x1A6, n + 8)), [None] * (n + 8), cs, True)
    return cs, {k: K.fr_to_mont(cv, pk.polys[k]) if pk.polys[k] else np.zeros((0, 4), dtype=np.uint64) for k in z.PK_ORDER}


# ---- a. key generation --------------------------------------------------------------------------------------------
@by_case
@by_curve
def test_srs_generate_equals_the_oracles_powers(cv, case, ctxs):
    ctx = ctxs[cv.name]
    want = DK.key(cv, case)
    ctx.srs_generate(DK.tau_of(cv, case), DK.N + DK.SPARE)
    got = ctx.srs_download(0, DK.N + DK.SPARE)
    assert np.array_equal(got, want)
    assert DK.identity_bases(got) == case.identity_bases                 # an identity comes back as (0, 0)
    assert ctx.msm_info()["srs_count"] == DK.N + DK.SPARE


# ---- b. the Lagrange table ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lagrange_inputs(cv_name, log_n):
    """circuit polynomials, the evaluation vectors of tests/test_gpu_lagrange.py and their Montgomery forms, per size"""
    cv = _cv(cv_name)
    n = 1 << log_n
    cs, polys = _pk_polys(cv_name, n - 3, 4, log_n, 2)
    assert cs.circuit_bound() == n
    vecs = TL._vectors(cv, log_n)
    return polys, vecs, {name: K.fr_to_mont(cv, ev) for name, ev in vecs.items()}


def _check_commit_evals(ctx, cv, log_n, srs_arr):
    import zkt_plonk_amd as z
    n = 1 << log_n
    polys, vecs, vecs_mont = _lagrange_inputs(cv.name, log_n)
    ctx.srs_load(srs_arr)
    z.GpuProver(ctx, log_n, polys)
    d_ev = ctx.alloc(n * 32)
    try:
        bl_all = field_elems(cv.fr.p, 4242, 3)
        for name, ev in vecs.items():
            ctx.upload(d_ev, vecs_mont[name])
            for k in range(4):
                bl = bl_all[:k]
                want = TL._oracle_commit(cv, log_n, srs_arr, ev, bl)
                for path in (0, 1):
                    out, inf = ctx.commit_evals_dev(d_ev, K.fr_to_mont(cv, bl) if k else None, path)
                    got = None if inf else K.points_from_mont(cv, out)[0]
                    assert got == want, (name, k, path)
                    assert not inf or not out.any(), (name, k, path)
        info = ctx.lagrange_info()
        assert info["log_n"] == log_n and info["bases"] == n + 8
    finally:
        ctx.free(d_ev)


# 13: lagrange_build_t cuts the domain into min(n, 4096) segments, so k_lag_seg_sum and k_lag_prefix loop from 2^13 on
@by_case
@pytest.mark.parametrize("log_n", [3, 6, 11, 13])
@by_curve
def test_commit_evals_over_the_lagrange_table_of_a_degenerate_key(cv, log_n, case, ctxs):
    _check_commit_evals(ctxs[cv.name], cv, log_n, DK.key(cv, case, 1 << log_n))


# ---- c. wire routes -----------------------------------------------------------------------------------------------
class _KeyedSeam(WB._Seam):
    """tests/test_gpu_wire_bases.py's seam under a given key"""

    def __init__(self, cv, log_n, srs, seed=2):
        import zkt_plonk_amd as z
        self.cv, self.log_n, self.n = cv, log_n, 1 << log_n
        n = self.n
        cs, polys = _pk_polys(cv.name, n - 3, 4, seed, 2)
        assert cs.circuit_bound() == n
        self.srs = srs
        self.ctx = ctx = z.Context(cv.name, 0)
        ctx.srs_load(srs)
        z.GpuProver(ctx, log_n, polys)
        self.max_vars = 4 * n
        self.d_vars = ctx.alloc(self.max_vars * 32)
        self.d_idx = [ctx.alloc(4 * n) for _ in range(3)]
        self.d_ev = ctx.alloc(n * 32)
        self.blinders = K.fr_to_mont(cv, field_elems(cv.fr.p, 77 + log_n, 6))


class _KeyedElimSeam(WE._Seam):
    """tests/test_gpu_wire_elimination.py's seam (a satisfied circuit in device buffers) under a given key"""

    def __init__(self, cv, srs):
        import zkt_plonk_amd as z
        cs, polys = _pk_polys(cv.name, 1021, 4, 3, 2)                 # WE._synthetic(cv, 1021)
        self.cv, self.cs, self.n = cv, cs, cs.circuit_bound()
        assert self.n == DK.N
        self.log_n = DK.LOG_N
        self.ctx = ctx = z.Context(cv.name, 0)
        ctx.srs_load(srs)
        z.GpuProver(ctx, self.log_n, polys)
        self.n_vars, self.n_rows = len(cs.values), cs.n_gates
        self.d_vars = ctx.alloc(self.n_vars * 32)
        self.d_idx = [ctx.alloc(4 * self.n_rows) for _ in range(3)]
        self.blinders = K.fr_to_mont(cv, field_elems(cv.fr.p, 31 + self.log_n, 6))
        self.put(cs.values, (cs.w_l, cs.w_r, cs.w_o))


# The routes a key outside the domain takes.  tau = 0: every T_v is (count_v / n) G and every A_f a multiple of G, none of
# them the identity, so the tables are built -- over equal and proportional bases, with the identity as the second blinder
# base (V_1 = [0] G - [0] G).  w_2n: no T_v is the identity, as under an ordinary key.  (routes 1 / 2; what the rule of
# the wire-base section of lagrange.hip predicts, and what an MI355X took when these tests were written)
ROUTES_OUTSIDE_THE_DOMAIN = {"0": ([1, 1, 1], [2, 2, 2]), "w_2n": ([1, 1, 1], [2, 2, 2])}


@by_case
@by_curve
def test_wire_routes_equal_the_coefficient_route(cv, case):
    srs = DK.key(cv, case)
    # in the domain all T_v but those of one row are the identity: the documented fallback to the coefficients
    want1, want2 = ([0, 0, 0], [0, 0, 0]) if case.in_domain else ROUTES_OUTSIDE_THE_DOMAIN[case.name]
    s = _KeyedSeam(cv, DK.LOG_N, srs)
    try:
        n = s.n
        rng = np.random.default_rng(5)
        n_vars = 2 * n
        vals = WB._values(cv, n_vars, 900)
        for n_rows in (n, n - 9):
            wires = [WB._random_wiring(rng, n_rows, n_vars) for _ in range(3)]
            took = s.check(vals, wires, n_rows, "%s n_rows=%d" % (case.name, n_rows))     # routes 1 and 0 against path 0
            print("key %s %s n_rows=%d: route 1 took %s" % (case.name, cv.name, n_rows, took))
            assert took == want1, (case.name, n_rows, took)
    finally:
        s.close()
    e = _KeyedElimSeam(cv, srs)
    try:
        assert e.cs.check_satisfied() and W.predicted_routes(e.cs, *W.eliminate(cv, e.cs)) == [2, 2, 2]
        for what in ("first call", "tables reused"):
            took = e.check("%s, %s" % (case.name, what), None)                             # route 2 against route 0
            print("key %s %s %s: route 2 took %s" % (case.name, cv.name, what, took))
            assert took == want2, (case.name, what, took)
        # ... and the yardstick of this seam against the path-0 commitment of the gathered vectors
        xy, inf, _ = e.commit(0)
        full = np.concatenate([K.fr_to_mont(cv, e.cs.values), np.zeros((1, 4), np.uint64)])
        d_ev = e.ctx.alloc(e.n * 32)
        for k, w in enumerate((e.cs.w_l, e.cs.w_r, e.cs.w_o)):
            idx = W.to_idx(w)
            ev = np.zeros((e.n, 4), np.uint64)
            ev[:len(idx)] = full[np.where(idx == WB.ZERO, len(e.cs.values), idx)]
            e.ctx.upload(d_ev, ev)
            want_xy, want_inf = e.ctx.commit_evals_dev(d_ev, e.blinders[2 * k:2 * k + 2], 0)
            assert inf[k] == want_inf and np.array_equal(xy[k], want_xy), (case.name, "wire", k)
    finally:
        e.close()


# ---- d. whole proofs ----------------------------------------------------------------------------------------------
def _transcript(z, cv, vk):
    tr = z.Transcript("merlin", "ZKT Plonk", fr_bits=cv.fr.bits, fq_bytes=cv.fq.limbs64 * 8)
    z.seed_transcript(tr, vk.n, vk.commits)
    return tr


@by_case
@by_curve
def test_proofs_equal_the_oracles_and_verify(cv, case):
    import zkt_plonk_amd as z
    from zkt_plonk_amd import _lib
    from test_gpu_prove import _gpu_prove
    import verify_locate_cases as VC
    st = DK.statement(cv, case)
    cs = st.cs
    ctx = z.Context(cv.name, 0)
    try:
        got_on = _gpu_prove(z, ctx, cv, cs, st.pk, st.vk, st.srs, st.blinders)
        assert ctx.lagrange_info() == dict(log_n=DK.LOG_N, bases=DK.N + DK.SPARE)
        assert got_on == st.raw, "Lagrange route on"
        ctx.set_lagrange(False)
        assert _gpu_prove(z, ctx, cv, cs, st.pk, st.vk, st.srs, st.blinders) == st.raw, "Lagrange route off"
        ctx.set_lagrange(True)
        # the variables form: the wires over their base tables (mode 0) and over the free variables (mode 2)
        pi_pos = sorted(cs.pi)
        pi_vals = K.fr_to_mont(cv, [cs.pi[k] for k in pi_pos])
        for mode in (0, 2):
            ctx.set_wire_elimination(mode)
            for _ in range(2):                                   # the second proof reuses the tables the first one built
                got = ctx.prove_vars(K.fr_to_mont(cv, cs.values), W.to_idx(cs.w_l), W.to_idx(cs.w_r), W.to_idx(cs.w_o),
                                     K.fr_to_mont(cv, cs.table), pi_pos, pi_vals, K.fr_to_mont(cv, st.blinders),
                                     _transcript(z, cv, st.vk))
                assert got == st.raw, "variables form, wire elimination %d" % mode
        ctx.set_wire_elimination(1)
        assert DK.proof_identities(P.proof_deserialize(cv, got_on)) == case.proof_identities
        if case.name == "0":
            return
        # the device proof through the host verifier, then batches of it on the device
        h, beta_h = _lib.srs_generate_g2(cv.name, st.tau)
        it = DK.item(cv, st, got_on)
        assert _lib.verify(cv.name, *it[:7], h, beta_h, it[7])
        assert ctx.verify_batch_dev([DK.item(cv, st, got_on) for _ in range(3)], h, beta_h)
        good, bad = DK.entry(st, got_on), DK.entry(st, DK.flip_evaluation(got_on))
        entries = [good, bad, good, good]
        items = lambda: [DK.item(cv, st, e[2]) for e in entries]  # noqa: E731
        assert not ctx.verify_batch_dev(items(), h, beta_h)
        accepted, out_bad, n_checks = ctx.verify_batch_locate(items(), h, beta_h)
        assert not accepted and out_bad.tolist() == [False, True, False, False]
        assert 1 <= n_checks <= VC.bound(len(entries), 1)
        tree = ctx.debug_verify_batch_tree(items(), h, beta_h)
        VC.check_tree(cv, entries, tree)
    finally:
        ctx.close()


# ---- e. the fixed-base MSM at size --------------------------------------------------------------------------------
# 2^16 + 5 and 2^17 + 321: the two accumulation regimes tests/test_gpu_msm.py test_msm_skewed_digit_distributions names
@pytest.mark.parametrize("name", DK.NUMPY_KEYS)
@pytest.mark.parametrize("count", [(1 << 16) + 5, (1 << 17) + 321], ids=["2^16+5", "2^17+321"])
@by_curve
def test_msm_over_keys_of_equal_opposite_and_identity_bases(cv, count, name, ctxs):
    ctx = ctxs[cv.name]
    srs = DK.numpy_key(cv, name, count)
    ctx.srs_load(srs)
    assert ctx.msm_info()["srs_count"] == count
    rng = np.random.default_rng(count % 1000 + len(name))
    one = K.fr_to_mont(cv, [1])[0]
    rand = rand_fr(rng, count)
    mixed = rand_fr(rng, count)
    mixed[::3] = 0                                                       # a third zeros
    mixed[1::7] = one                                                    # a seventh ones
    equal = np.tile(K.fr_to_mont(cv, [0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF12345678 % cv.fr.p]), (count, 1))
    for what, sc in (("random", rand), ("zeros and ones", mixed), ("all equal", equal)):
        out, inf = ctx.msm(sc)
        want, winf = K.msm_mont(cv, srs, sc)
        assert inf == winf, (name, what)
        assert np.array_equal(out, want) if not winf else not out.any(), (name, what)
    if name == "-1":
        even = count - 1                                                 # G - G + G - ... an even number of times
        assert even % 2 == 0
        out, inf = ctx.msm(equal[:even])
        assert inf and not out.any()
        assert K.msm_mont(cv, srs[:even], equal[:even])[1]


# ---- f. the KZG seam ----------------------------------------------------------------------------------------------
@by_case
@by_curve
def test_kzg_commit_batch_and_open_equal_the_oracle(cv, case, ctxs):
    ctx = ctxs[cv.name]
    srs = DK.key(cv, case)
    ctx.srs_load(srs)
    count = srs.shape[0]
    rng = np.random.default_rng(300 + DK.IDS.index(case.name))
    polys = [KS._fr(cv, count, rng), KS._fr(cv, 1, rng), np.zeros((0, 4), dtype=np.uint64)]
    got = ctx.kzg_commit_batch(polys)
    for j, p in enumerate(polys):
        assert KS._same(got[j], KS._oracle_commit(cv, srs, p)), (case.name, "commitment", j)
    ch = KS._fr(cv, len(polys), rng)
    w = cv.fr.root_of_unity(DK.N)
    z_rand = int(rng.integers(2, 1 << 62)) * int(rng.integers(2, 1 << 62)) % cv.fr.p
    for what, zv in (("random", z_rand), ("w", w)):
        zm = K.fr_to_mont(cv, [zv])[0]
        (wit, inf), ev = ctx.kzg_open(polys, ch, zm)
        want_w, want_ev = KS._oracle_open(cv, srs, polys, ch, zm)
        assert KS._same((wit, inf), want_w), (case.name, "witness at z =", what)
        assert np.array_equal(ev, want_ev), (case.name, "evaluations at z =", what)
