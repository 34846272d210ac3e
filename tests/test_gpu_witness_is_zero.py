"""GPU: rule Z of the witness completion (zkt_witness_plan_create_ex with ZKT_WITNESS_RULE_IS_ZERO) against the Python
restatement (tests/is_zero_cases.py, pinned on the CPU by tests/test_is_zero_cases_oracle.py).  Every comparison is exact, on
the Montgomery words: completed maps, public inputs, kinds.  Before every completion each defined variable holds a distinct
non-zero pattern; everything the plan does not define comes back bit-identical."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import fields as F, plonk as P, coracle as K
from helpers import field_elems

import is_zero_cases as Z
import witness_plan_cases as W

BN, BLS = F.BN254, F.BLS12_381
CURVES = {"bn254": BN, "bls12_381": BLS}
CLEAN = (0, None)
NEVER = 1 << 31


class World:
    """Per module: one context per curve and the key polynomials of every case, each made once."""

    def __init__(self):
        import zkt_plonk_amd as z
        self.z = z
        self.ctx = {cv.name: z.Context(cv.name, 0) for cv in (BN, BLS)}
        self.loaded, self._polys, self._be = {}, {}, {}

    def close(self):
        for c in self.ctx.values():
            c.close()

    def backend(self, cv):
        if cv.name not in self._be:
            self._be[cv.name] = K.CBackend(cv, K.srs_mont(cv, 3, 2))
        return self._be[cv.name]

    def load(self, c):
        ctx = self.ctx[c.cv.name]
        if self.loaded.get(c.cv.name) != c.name:
            if c.name not in self._polys:
                be = self.backend(c.cv)
                ev = P.setup_evals(be, c.cs)
                self._polys[c.name] = [W.mont(c.cv, be.ifft(1 << c.log_n, ev[k])) for k in self.z.PK_ORDER]
            ctx.circuit_load(c.log_n, self._polys[c.name])
            self.loaded[c.cv.name] = c.name
        return ctx

    def plan(self, c, rules):
        return self.z.WitnessPlan(self.load(c), c.idx(0), c.idx(1), c.idx(2), c.n_vars, c.pi_pos, rules=rules)


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.close()


def run(ctx, plan, c, arr):
    """Completes the maps arr (batch, stride, 4) on the device -> (maps, pi (batch, n_pi, 4), status)"""
    batch, stride, n_pi = arr.shape[0], arr.shape[1], len(c.pi_pos)
    d, d_pi = ctx.alloc(max(arr.nbytes, 32)), ctx.alloc(max(batch * n_pi * 32, 32))
    try:
        ctx.upload(d, arr)
        plan.complete_dev(d, stride, batch, d_pi)
        status = plan.status(batch)
        out = ctx.download(d, arr.shape)
        pi = ctx.download(d_pi, (batch, n_pi, 4)) if n_pi else np.zeros((batch, 0, 4), dtype=np.uint64)
    finally:
        ctx.free(d)
        ctx.free(d_pi)
    return out, pi, status


def starts_and_wants(c, pl, witnesses, stride):
    """per distinct witness: (the uploaded map, the restatement's completed map, its public inputs) as Montgomery words"""
    out = []
    for k, values in enumerate(witnesses):
        start = Z.prefill(c, pl, values, stride, salt=k + 1)
        x, pi, bad = Z.complete(c, pl, start)
        assert bad == (0, W.NONE)
        out.append((W.mont(c.cv, start).reshape(-1, 4), W.mont(c.cv, x).reshape(-1, 4), W.mont(c.cv, pi).reshape(-1, 4)))
    return out


def check_batch(ctx, plan, c, pl, made, batch):
    """witness k of the batch is made[k % len(made)]: x = 0 and x != 0 stand side by side in one batch"""
    pick = [made[k % len(made)] for k in range(batch)]
    got, pi, st = run(ctx, plan, c, np.stack([m[0] for m in pick]))
    assert st == [CLEAN] * batch, c.name
    assert np.array_equal(got, np.stack([m[1] for m in pick])), c.name
    assert np.array_equal(pi, np.stack([m[2] for m in pick])), c.name
    keep = [v for v in range(got.shape[1]) if v >= c.n_vars or pl.kind[v] in (W.FREE, W.UNUSED)]
    assert np.array_equal(got[:, keep], np.stack([m[0] for m in pick])[:, keep]), c.name
    return got


def check_info(plan, c, pl):
    info = plan.info()
    assert (info["n_free"], info["n_out"], info["n_right"], info["n_unused"]) == (pl.n_free, pl.n_out, pl.n_right, pl.n_unused), c.name
    assert (info["depth"], info["max_level_rows"], info["n_pairs"]) == (pl.depth, pl.max_level_rows, pl.n_pairs), c.name
    assert plan.kinds().tolist() == pl.kind, c.name
    assert info["device_bytes"] >= 32 * len(pl.rows) + 16 * W.BATCH_MAX and info["device_bytes"] % 256 == 0


@pytest.mark.parametrize("log_n", [3, 4])
@pytest.mark.parametrize("cvname", sorted(CURVES))
def test_cases_with_and_without_the_bit(world, cvname, log_n):
    ctx = world.ctx[cvname]
    for case in Z.cases(CURVES[cvname], log_n):
        c = case.c
        pl = Z.plan(c, Z.RULE_IS_ZERO)
        plan = world.plan(c, Z.RULE_IS_ZERO)
        try:
            check_info(plan, c, pl)
            for v, k in case.kinds.items():
                assert plan.kinds()[v] == k, (c.name, v)
            if not case.near_miss:
                assert {Z.ZINV, Z.ZFLAG} <= set(plan.kinds().tolist()) and plan.info()["n_pairs"] > 0
            made = starts_and_wants(c, pl, case.witnesses, c.n_vars + 2)
            got = check_batch(ctx, plan, c, pl, made, len(made))
            for k, values in enumerate(case.witnesses):                  # the gadgets' own native assignments
                assert np.array_equal(got[k][:c.n_vars], W.mont(c.cv, values).reshape(-1, 4)), (c.name, k)
        finally:
            plan.close()
        # rules = 0 on the same circuit: as before, y is the caller's and comes back untouched
        pl0 = Z.plan(c, 0)
        plan = world.plan(c, 0)
        try:
            check_info(plan, c, pl0)
            assert plan.info()["n_pairs"] == 0 and max(plan.kinds().tolist()) <= W.RIGHT
            made = starts_and_wants(c, pl0, case.witnesses, c.n_vars)
            got = check_batch(ctx, plan, c, pl0, made, len(made))
            for v, k in case.kinds.items():
                if k == Z.ZINV:
                    assert pl0.kind[v] == W.FREE and all(np.array_equal(got[j][v], m[0][v]) for j, m in enumerate(made)), c.name
        finally:
            plan.close()


@pytest.mark.parametrize("cvname", sorted(CURVES))
def test_batches_of_1_3_and_256_on_the_wide_level(world, cvname):
    case = Z.wide_case(CURVES[cvname])
    c = case.c
    pl = Z.plan(c, Z.RULE_IS_ZERO)
    plan = world.plan(c, Z.RULE_IS_ZERO)
    try:
        check_info(plan, c, pl)
        assert plan.info()["n_pairs"] == Z.WIDE_PAIRS and plan.info()["launches"] == 1
        made = starts_and_wants(c, pl, case.witnesses, c.n_vars + 1)
        zs = [v for v, k in case.kinds.items() if k == Z.ZFLAG]
        assert any(len({bytes(m[1][v]) for m in made}) == 2 for v in zs)     # zero and non-zero across one batch
        for batch in (1, 3, W.BATCH_MAX):
            check_batch(world.ctx[cvname], plan, c, pl, made, batch)
    finally:
        plan.close()


def test_every_split_gives_the_same_map(world):
    """thresholds 1 (every level a launch of k_wp_wide), 2 and "never" (k_wp_narrow): the 300-pair level and the chained
    pairs' three levels through both kernels"""
    chained = next(k for k in Z.cases(BN, 3) if k.c.name.startswith("chained"))
    for case, launches in ((Z.wide_case(BN), {1: 1, 2: 1, NEVER: 1}), (chained, {1: 3, 2: 1, NEVER: 1})):
        c = case.c
        pl = Z.plan(c, Z.RULE_IS_ZERO)
        plan = world.plan(c, Z.RULE_IS_ZERO)
        try:
            made = starts_and_wants(c, pl, case.witnesses, c.n_vars)
            first = None
            for wide_min_rows in (1, 2, NEVER):
                plan.split(wide_min_rows)
                assert plan.info()["launches"] == launches[wide_min_rows] == W.launches(pl, wide_min_rows), c.name
                got = check_batch(world.ctx["bn254"], plan, c, pl, made, 3)
                first = got if first is None else first
                assert np.array_equal(got, first)
            plan.split(0)
        finally:
            plan.close()


def test_refusals_and_rules_0_is_the_plain_entry(world):
    z = world.z
    case = Z.cases(BN, 3)[0]
    c = case.c
    ctx = world.load(c)
    for rules in (2, 3, 1 << 31):
        with pytest.raises(z.ZktError) as e:
            ctx.witness_plan_create(c.idx(0), c.idx(1), c.idx(2), c.n_vars, c.pi_pos, rules=rules)
        assert e.value.code == 1
    fresh = z.Context("bn254", 0)
    try:
        with pytest.raises(z.ZktError) as e:
            fresh.witness_plan_create(c.idx(0), c.idx(1), c.idx(2), c.n_vars, c.pi_pos, rules=Z.RULE_IS_ZERO)
        assert e.value.code == 10
    finally:
        fresh.close()
    import ctypes
    L, vp = z.lib(), ctypes.c_void_p
    idx = [c.idx(k) for k in range(3)]
    h = vp()
    assert L.zkt_witness_plan_create_ex(ctx.handle, vp(idx[0].ctypes.data), vp(idx[1].ctypes.data), vp(idx[2].ctypes.data), c.n_rows,
                                        c.n_vars, 0, None, 0, 0, ctypes.byref(h)) == 0
    try:
        plain = world.plan(c, 0)
        try:
            assert ctx.witness_plan_kinds(h.value, c.n_vars).tolist() == plain.kinds().tolist()
            assert ctx.witness_plan_info(h.value) == plain.info()
        finally:
            plain.close()
    finally:
        ctx.witness_plan_free(h.value)


def test_end_to_end_prove_from_the_free_variables_of_a_comparison():
    """should_eq_with_output, a select on its flag and a second pair, at the size of the existing end-to-end test (2^15): upload
    the free variables only, complete, prove from the device map, verify."""
    import zkt_plonk_amd as z
    from zkt_plonk_amd import _lib
    cv, log_n = BN, 15
    cs = W._cs(cv, log_n)
    a, b = cs.assign_variable(0x1234567), cs.assign_variable(0x1234567)
    d, y, flag = Z.should_eq_with_output(cs, a, b)
    s = Z.conditional_select_one(cs, flag, a)
    y2, flag2 = Z.should_be_zero_with_output(cs, s)
    cs.set_variable_public(flag)
    cs.set_variable_public(flag2)
    c = W.Circuit.of(cs, log_n, name="e2e_eq")
    assert (c.values[flag], c.values[flag2]) == (1, 0) and cs.circuit_bound() == 1 << 15
    pl = Z.plan(c, Z.RULE_IS_ZERO)
    assert (pl.n_free, pl.n_pairs) == (2, 2)
    n, tau = 1 << log_n, 0x5EED6
    ctx = z.Context(cv.name, 0)
    plan = None
    try:
        ctx.srs_generate(tau, n + 8)
        be = K.CBackend(cv, K.srs_mont(cv, 3, 2))
        evals = {k: W.mont(cv, v) for k, v in P.setup_evals(be, cs).items()}
        prover, commits = z.GpuProver.setup(ctx, log_n, evals)
        vk_commits = {k: (None if inf else K.points_from_mont(cv, np.asarray(xy).reshape(1, -1))[0]) for k, (xy, inf) in commits.items()}
        plan = z.WitnessPlan(ctx, c.idx(0), c.idx(1), c.idx(2), c.n_vars, c.pi_pos, rules=Z.RULE_IS_ZERO)
        assert plan.info()["n_free"] == 2 and plan.info()["n_pairs"] == 2

        def dev(arr):
            p = ctx.alloc(max(arr.nbytes, 32))
            ctx.upload(p, arr)
            return p

        free_only = [v if pl.kind[k] == W.FREE else 0 for k, v in enumerate(c.values)]
        d_vars, d_pi = dev(W.mont(cv, Z.prefill(c, pl, free_only))), ctx.alloc(32 * len(c.pi_pos))
        d_idx = [dev(c.idx(k)) for k in range(3)]
        plan.complete_dev(d_vars, c.n_vars, 1, d_pi)
        pi_vals = ctx.download(d_pi, (len(c.pi_pos), 4))
        assert plan.status(1) == [CLEAN]
        assert W.unmont(cv, pi_vals) == [c.pi[i] for i in c.pi_pos] == [1, 0]
        assert W.unmont(cv, ctx.download(d_vars, (c.n_vars, 4))) == c.values
        table = W.mont(cv, cs.table)
        blinders = W.mont(cv, field_elems(cv.fr.p, 0xB11E, P.NUM_BLINDERS))
        made = ctx.prepare_vars_dev(d_vars, c.n_vars, d_idx[0], d_idx[1], d_idx[2], c.n_rows, table, c.pi_pos, pi_vals, blinders)
        assert ctx.check_witness(made, z.CHECK_WIRING).satisfied
        tr = lambda: z.seed_transcript(z.Transcript("merlin", "ZKT Plonk", fr_bits=cv.fr.bits, fq_bytes=cv.fq.limbs64 * 8), n, vk_commits)
        proof = ctx.prove_prepared(made, tr())
        roots = be.domain(n).elements()
        h, beta_h = _lib.srs_generate_g2(cv.name, tau)
        names = z.PK_ORDER
        assert _lib.verify(cv.name, n, np.stack([np.asarray(commits[k][0]).reshape(-1) for k in names]), [commits[k][1] for k in names],
                           W.mont(cv, [roots[i] for i in c.pi_pos]), pi_vals, proof, ctx.srs_download(0, 1)[0], h, beta_h, tr())
    finally:
        if plan is not None:
            plan.close()
        ctx.close()
