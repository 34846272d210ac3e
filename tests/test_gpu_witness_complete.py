"""GPU: zkt_witness_plan_* / zkt_witness_complete* against the Python restatement of the rule (tests/witness_plan_cases.py,
pinned on the CPU against the oracle's composer by tests/test_witness_plan_cases_oracle.py).  Every comparison is exact, on
the Montgomery words.  Before every completion each defined variable holds a distinct non-zero pattern; afterwards defined
variables equal the oracle's values and everything else -- free variables, variables on no wire, the padding up to the
stride -- is bit-identical to what was uploaded."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import fields as F, plonk as P, coracle as K
from helpers import field_elems

import witness_plan_cases as W

BN, BLS = F.BN254, F.BLS12_381
CURVES = {"bn254": BN, "bls12_381": BLS}
ERR_INVALID_ARGUMENT, ERR_NOT_LOADED = 1, 10
CLEAN = (0, None)


class World:
    """Per module: one context per curve and the key polynomials of every case, each made once."""

    def __init__(self):
        import zkt_plonk_amd as z
        self.z = z
        self.ctx = {cv.name: z.Context(cv.name, 0) for cv in (BN, BLS)}
        self.loaded = {}
        self._polys, self._evals, self._be = {}, {}, {}

    def close(self):
        for c in self.ctx.values():
            c.close()

    def backend(self, cv):
        if cv.name not in self._be:
            self._be[cv.name] = K.CBackend(cv, K.srs_mont(cv, 3, 2))
        return self._be[cv.name]

    def evals(self, c):
        if c.name not in self._evals:
            self._evals[c.name] = P.setup_evals(self.backend(c.cv), c.cs)
        return self._evals[c.name]

    def load(self, c, ctx=None):
        """the context of c's curve with c's key loaded (zkt_circuit_load from the oracle's polynomials: no SRS)"""
        own = ctx is None
        ctx = self.ctx[c.cv.name] if own else ctx
        if own and self.loaded.get(c.cv.name) == c.name:
            return ctx
        if c.name not in self._polys:
            be, ev = self.backend(c.cv), self.evals(c)
            self._polys[c.name] = [W.mont(c.cv, be.ifft(1 << c.log_n, ev[k])) for k in self.z.PK_ORDER]
        ctx.circuit_load(c.log_n, self._polys[c.name])
        if own:
            self.loaded[c.cv.name] = c.name
        return ctx

    def plan(self, c, ctx=None):
        ctx = self.load(c, ctx)
        return self.z.WitnessPlan(ctx, c.idx(0), c.idx(1), c.idx(2), c.n_vars, c.pi_pos)


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.close()


def run(ctx, plan, c, maps, stride=None, status_ctx=None):
    """Completes the integer maps (each `stride` long) on the device -> (maps (batch, stride, 4), pi (batch, n_pi, 4), status)"""
    stride = c.n_vars if stride is None else stride
    arr = np.stack([W.mont(c.cv, m).reshape(-1, 4) for m in maps]) if stride else np.zeros((len(maps), 0, 4), dtype=np.uint64)
    assert arr.shape == (len(maps), stride, 4)
    n_pi = len(c.pi_pos)
    d = ctx.alloc(max(arr.nbytes, 32))
    d_pi = ctx.alloc(max(len(maps) * n_pi * 32, 32))
    try:
        if arr.size:
            ctx.upload(d, arr)
        plan.complete_dev(d, stride, len(maps), d_pi, ctx=ctx)
        status = plan.status(len(maps), ctx=status_ctx or ctx)
        out = ctx.download(d, arr.shape) if arr.size else arr
        pi = ctx.download(d_pi, (len(maps), n_pi, 4)) if n_pi else np.zeros((len(maps), 0, 4), dtype=np.uint64)
    finally:
        ctx.free(d)
        ctx.free(d_pi)
    return out, pi, status


def expect(c, pl, start, stride=None):
    """the restatement's completion of `start` as Montgomery words, its public inputs and its status in the mirror's form"""
    x, pi, (n_bad, first) = W.complete(c, pl, start)
    return W.mont(c.cv, x).reshape(-1, 4), W.mont(c.cv, pi).reshape(-1, 4), (n_bad, None if first == W.NONE else first)


def check_one(ctx, plan, c, pl, values, stride=None, want_values=None):
    start = W.prefill(c, pl, values, stride)
    want, want_pi, want_st = expect(c, pl, start)
    got, pi, st = run(ctx, plan, c, [start], stride)
    assert st == [want_st], c.name
    assert np.array_equal(got[0], want), c.name
    assert np.array_equal(pi[0], want_pi), c.name
    # what the completion may not touch, said once more in its own words
    up = W.mont(c.cv, start).reshape(-1, 4)
    keep = [v for v in range(len(start)) if v >= c.n_vars or pl.kind[v] in (W.FREE, W.UNUSED)]
    assert np.array_equal(got[0][keep], up[keep]), c.name
    if want_values is not None:
        assert np.array_equal(got[0][:c.n_vars], W.mont(c.cv, want_values).reshape(-1, 4)), c.name
    return got, pi


def check_info(plan, c, pl, launches=None):
    info = plan.info()
    assert (info["n_free"], info["n_out"], info["n_right"], info["n_unused"]) == (pl.n_free, pl.n_out, pl.n_right, pl.n_unused), c.name
    assert (info["depth"], info["max_level_rows"]) == (pl.depth, pl.max_level_rows), c.name
    assert plan.kinds().tolist() == pl.kind, c.name
    assert info["device_bytes"] >= 32 * len(pl.rows) + 16 * W.BATCH_MAX and info["device_bytes"] % 256 == 0
    if launches is not None:
        assert info["launches"] == launches, c.name


@pytest.mark.parametrize("log_n", [3, 4])
@pytest.mark.parametrize("cvname", sorted(CURVES))
def test_handmade_circuits(world, cvname, log_n):
    for c, free, kinds, bad in W.handmade_cases(CURVES[cvname], log_n):
        pl = W.plan(c)
        plan = world.plan(c)
        try:
            check_info(plan, c, pl)
            for v, k in kinds.items():
                assert plan.kinds()[v] == k, (c.name, v)
            got, pi = check_one(world.ctx[cvname], plan, c, pl, W.handmade_values(c, free), stride=c.n_vars + 2)
            want_bad = (bad[0], None if bad[1] == W.NONE else bad[1])
            if want_bad != CLEAN:                                       # reported once, then the block reads clean
                assert plan.status(1) == [CLEAN]
        finally:
            plan.close()


@pytest.mark.parametrize("cvname,params", [("bn254", "synthetic"), ("bls12_381", "synthetic"), ("bn254", "shipped")])
def test_withdraw_circuit_from_its_free_variables(world, cvname, params):
    c = W.withdraw(cvname, params, 1)[0]
    pl = W.plan(c)
    plan = world.plan(c)
    try:
        check_info(plan, c, pl)
        got, pi = check_one(world.ctx[cvname], plan, c, pl, c.values, want_values=c.values)
        assert W.unmont(c.cv, pi[0]) == [c.pi[i] for i in c.pi_pos]
        # the host-pointer form, two witnesses
        start = W.prefill(c, pl, c.values)
        maps, pis, st = plan.complete(np.stack([W.mont(c.cv, start)] * 2))
        assert st == [CLEAN, CLEAN]
        for k in range(2):
            assert np.array_equal(maps[k], got[0]) and np.array_equal(pis[k], pi[0])
    finally:
        plan.close()


@pytest.mark.parametrize("cvname", sorted(CURVES))
def test_a_batch_with_one_unsolvable_witness(world, cvname):
    seeds = (1, 2, 3, 4)
    cs = [W.withdraw(cvname, "synthetic", s)[0] for s in seeds]
    c = cs[0]
    assert all(W.same_circuit(c, other) for other in cs[1:])
    pl = W.plan(c)
    stride = c.n_vars + 3
    starts = [W.prefill(c, pl, x.values, stride, salt=s) for x, s in zip(cs, seeds)]
    broken = W.prefill(c, pl, c.values, stride, salt=9)
    broken[W.secret_variable(c, pl)] = 0
    starts.insert(2, broken)
    plan = world.plan(c)
    try:
        ctx = world.ctx[cvname]
        got, pi, st = run(ctx, plan, c, starts, stride)
        wants = [expect(c, pl, s) for s in starts]
        bad_row = min(pl.def_row[v] for v in range(c.n_vars) if pl.kind[v] == W.RIGHT)
        assert st == [CLEAN, CLEAN, (1, bad_row), CLEAN, CLEAN]
        assert [w[2] for w in wants] == st
        for k, (want, want_pi, _) in enumerate(wants):
            assert np.array_equal(got[k], want), k
            assert np.array_equal(pi[k], want_pi), k
        for k, x in zip((0, 1, 3, 4), cs):
            assert np.array_equal(got[k][:c.n_vars], W.mont(c.cv, x.values).reshape(-1, 4)), k
        assert not np.array_equal(got[2][:c.n_vars], W.mont(c.cv, c.values).reshape(-1, 4))
        assert plan.status(5) == [CLEAN] * 5
    finally:
        plan.close()


def test_every_split_gives_the_same_map(world):
    c = W.withdraw("bn254", "synthetic", 1)[0]
    pl = W.plan(c)
    plan = world.plan(c)
    try:
        ctx = world.ctx["bn254"]
        first = None
        for wide_min_rows, launches in ((1, 1), (87, 2), (88, 1), (1 << 31, 1), (40, W.launches(pl, 40)), (20, W.launches(pl, 20))):
            assert launches == W.launches(pl, wide_min_rows)
            plan.split(wide_min_rows)
            assert plan.info()["launches"] == launches
            got, pi = check_one(ctx, plan, c, pl, c.values, want_values=c.values)
            first = got if first is None else first
            assert np.array_equal(got, first)
        assert W.launches(pl, 40) > 2 and 2 < W.launches(pl, 20) <= W.MAX_LAUNCHES       # runs between several wide levels
        plan.split(0)
    finally:
        plan.close()


def test_refusals_leave_a_plan_usable(world):
    z = world.z
    c = W.withdraw("bn254", "synthetic", 1)[0]
    pl = W.plan(c)
    plan = world.plan(c)
    ctx = world.ctx["bn254"]
    n = 1 << c.log_n
    idx = [c.idx(k) for k in range(3)]

    def refused(code, *a, **kw):
        with pytest.raises(z.ZktError) as e:
            ctx.witness_plan_create(*a, **kw)
        assert e.value.code == code, e.value

    try:
        fresh = z.Context("bn254", 0)
        try:
            with pytest.raises(z.ZktError) as e:
                fresh.witness_plan_create(idx[0], idx[1], idx[2], c.n_vars, c.pi_pos)
            assert e.value.code == ERR_NOT_LOADED
        finally:
            fresh.close()
        long = [np.concatenate([w, np.full(n + 1 - c.n_rows, W.ZERO, dtype=np.uint32)]) for w in idx]
        refused(ERR_INVALID_ARGUMENT, long[0], long[1], long[2], c.n_vars, c.pi_pos)                 # n_rows > n
        for k in range(3):
            bad = [w.copy() for w in idx]
            bad[k][c.n_rows // 2] = c.n_vars                                                         # neither < n_vars nor Zero
            refused(ERR_INVALID_ARGUMENT, bad[0], bad[1], bad[2], c.n_vars, c.pi_pos)
        refused(ERR_INVALID_ARGUMENT, idx[0], idx[1], idx[2], c.n_vars, c.pi_pos[:-1] + [n])         # a position >= n
        refused(ERR_INVALID_ARGUMENT, idx[0], idx[1], idx[2], c.n_vars, c.pi_pos[::-1])              # unsorted
        refused(ERR_INVALID_ARGUMENT, idx[0], idx[1], idx[2], c.n_vars, c.pi_pos[:1] * 2)            # repeated
        refused(ERR_INVALID_ARGUMENT, 0, 0, 0, c.n_vars, c.pi_pos, n_rows=c.n_rows)                  # NULL wiring, n_rows > 0
        # the completion's own refusals
        d = ctx.alloc(32 * c.n_vars)
        try:
            for args in ((d, c.n_vars - 1, 1), (d, c.n_vars, 0), (d, c.n_vars, W.BATCH_MAX + 1), (0, c.n_vars, 1)):
                with pytest.raises(z.ZktError) as e:
                    ctx.witness_complete_enqueue(plan.handle, *args)
                assert e.value.code == ERR_INVALID_ARGUMENT, args
        finally:
            ctx.free(d)
        other = world.ctx["bls12_381"]
        d = other.alloc(32 * c.n_vars)
        try:
            with pytest.raises(z.ZktError) as e:                                                     # a plan of another curve
                other.witness_complete_enqueue(plan.handle, d, c.n_vars, 1)
            assert e.value.code == ERR_INVALID_ARGUMENT
        finally:
            other.free(d)
        check_one(ctx, plan, c, pl, c.values, want_values=c.values)
    finally:
        plan.close()


def test_lifetime_reload_and_fork(world):
    from zkt_plonk_amd import _lib
    c = W.withdraw("bn254", "synthetic", 1)[0]
    small = W.handmade_cases(BN, 3)[0][0]
    pl = W.plan(c)
    ctx = world.ctx["bn254"]
    world.plan(c).close()                                   # the context's own scratch is grown here, once
    before = _lib.debug_live_allocations()
    plan = world.plan(c)
    during = _lib.debug_live_allocations()
    assert during[0] > before[0] and during[1] - before[1] == plan.info()["device_bytes"]
    check_one(ctx, plan, c, pl, c.values, want_values=c.values)
    plan.close()
    assert _lib.debug_live_allocations() == before
    plan = world.plan(c)
    try:
        world.load(small)                                   # another circuit in the context: the plan holds its own copies
        check_one(ctx, plan, c, pl, c.values, want_values=c.values)
        world.load(c)
        child = ctx.fork()                                  # a plan made on the parent completes on the fork
        try:
            check_one(child, plan, c, pl, c.values, want_values=c.values)
        finally:
            child.close()
    finally:
        plan.close()


def test_end_to_end_prove_from_the_free_variables(world):
    """(c): complete from the 85 free values, check the witness with its wiring, prove from the completed device map with
    the returned public inputs, compare with the proof from the oracle's map, verify."""
    z = world.z
    from zkt_plonk_amd import _lib
    cv = BN
    c, pub, cs = W.withdraw("bn254", "shipped", 1)
    pl = W.plan(c)
    n, tau = 1 << c.log_n, 0x5EED5
    ctx = z.Context(cv.name, 0)
    held = []
    try:
        ctx.srs_generate(tau, n + 8)
        evals = {k: W.mont(cv, v) for k, v in world.evals(c).items()}
        prover, commits = z.GpuProver.setup(ctx, c.log_n, evals)
        vk_commits = {k: (None if inf else K.points_from_mont(cv, np.asarray(xy).reshape(1, -1))[0]) for k, (xy, inf) in commits.items()}
        plan = z.WitnessPlan(ctx, c.idx(0), c.idx(1), c.idx(2), c.n_vars, c.pi_pos)
        held.append(plan)
        assert plan.info()["n_free"] == 85

        def dev(arr):
            d = ctx.alloc(max(arr.nbytes, 32))
            ctx.upload(d, arr)
            return d

        start = W.mont(cv, W.prefill(c, pl, c.values))
        d_vars, d_pi = dev(start), ctx.alloc(32 * len(c.pi_pos))
        d_idx = [dev(c.idx(k)) for k in range(3)]
        plan.complete_dev(d_vars, c.n_vars, 1, d_pi)
        pi_vals = ctx.download(d_pi, (len(c.pi_pos), 4))
        assert plan.status(1) == [CLEAN]
        assert W.unmont(cv, pi_vals) == [c.pi[i] for i in c.pi_pos]
        table = W.mont(cv, cs.table)
        blinders = W.mont(cv, field_elems(cv.fr.p, 0xB11D, P.NUM_BLINDERS))
        made = ctx.prepare_vars_dev(d_vars, c.n_vars, d_idx[0], d_idx[1], d_idx[2], c.n_rows, table, c.pi_pos, pi_vals, blinders)
        assert ctx.check_witness(made, z.CHECK_WIRING).satisfied
        tr = lambda: z.seed_transcript(z.Transcript("merlin", "ZKT Plonk", fr_bits=cv.fr.bits, fq_bytes=cv.fq.limbs64 * 8), n, vk_commits)
        proof = ctx.prove_prepared(made, tr())
        theirs = ctx.prepare_vars(W.mont(cv, c.values), c.idx(0), c.idx(1), c.idx(2), table, c.pi_pos,
                                  W.mont(cv, [c.pi[i] for i in c.pi_pos]), blinders)
        assert proof == ctx.prove_prepared(theirs, tr())
        roots = world.backend(cv).domain(n).elements()
        h, beta_h = _lib.srs_generate_g2(cv.name, tau)
        names = z.PK_ORDER
        assert _lib.verify(cv.name, n, np.stack([np.asarray(commits[k][0]).reshape(-1) for k in names]), [commits[k][1] for k in names],
                           W.mont(cv, [roots[i] for i in c.pi_pos]), pi_vals, proof, ctx.srs_download(0, 1)[0], h, beta_h, tr())
    finally:
        for p in held:
            p.close()
        ctx.close()
