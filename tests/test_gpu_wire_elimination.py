"""Wire commitments over the circuit's free variables (csrc/lagrange.hip "wire tables over free variables", csrc/wire_elim.hpp,
include/zkt_plonk.h "Commitments of evaluation vectors").  The yardstick is the coefficient route: route 0 of
zkt_debug_commit_wires_dev for single rounds, ctx.prove on host evaluation vectors for whole proofs.  On a witness that
satisfies the circuit every point and every proof must be bit-equal to it."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import fields as F, plonk as P, coracle as K
from helpers import field_elems
import wire_elim_cases as W
from test_gpu_wire_bases import withdraw, _setup, _transcript   # noqa: F401  (the 2^14 withdraw fixture and its helpers)


class _Seam:
    """The circuit `cs` loaded on a context with a key of n + 8 powers; its variable map and index vectors in device buffers
    whose addresses every call reuses."""

    def __init__(self, cv, cs):
        import zkt_plonk_amd as z
        self.cv, self.cs, self.n = cv, cs, cs.circuit_bound()
        n = self.n
        self.log_n = n.bit_length() - 1
        srs = K.srs_mont(cv, 0x5A17 + self.log_n, n + 8)
        pk, _, _ = P.setup(K.CBackend(cv, srs), [None] * (n + 8), cs, True)
        self.ctx = ctx = z.Context(cv.name, 0)
        ctx.srs_load(srs)
        z.GpuProver(ctx, self.log_n, {k: K.fr_to_mont(cv, pk.polys[k]) if pk.polys[k] else np.zeros((0, 4), dtype=np.uint64)
                                      for k in z.PK_ORDER})
        self.n_vars, self.n_rows = len(cs.values), cs.n_gates
        self.d_vars = ctx.alloc(self.n_vars * 32)
        self.d_idx = [ctx.alloc(4 * self.n_rows) for _ in range(3)]
        self.blinders = K.fr_to_mont(cv, field_elems(cv.fr.p, 31 + self.log_n, 6))
        self.put(cs.values, (cs.w_l, cs.w_r, cs.w_o))

    def close(self):
        self.ctx.close()

    def put(self, values, wires):
        self.ctx.upload(self.d_vars, K.fr_to_mont(self.cv, values))
        for d, w in zip(self.d_idx, wires):
            self.ctx.upload(d, W.to_idx(w))

    def commit(self, route, pi_pos=None):
        pos = sorted(self.cs.pi) if pi_pos is None else pi_pos
        return self.ctx.debug_commit_wires_dev(self.d_vars, self.n_vars, self.d_idx[0], self.d_idx[1], self.d_idx[2], self.n_rows,
                                               self.blinders, route, pos)

    def check(self, what, want_routes, pi_pos=None):
        """route 2 against route 0 on what the buffers hold now; returns the routes taken"""
        want = self.commit(0)
        got = self.commit(2, pi_pos)
        for k in range(3):
            assert got[1][k] == want[1][k] and np.array_equal(got[0][k], want[0][k]), (what, "wire", k)
        assert want[2] == [0, 0, 0]
        if want_routes is not None:
            assert got[2] == want_routes, (what, got[2])
        return got[2]


def _synthetic(cv, n_gates):
    cs = P.synthetic_circuit(cv, n_gates, 4, seed=3, n_public=2)
    assert cs.circuit_bound() == 1024
    return cs


def _small_withdraw(cv):
    from oracle import composer as OC
    import test_gpu_poseidon as TP
    return OC.withdraw_instance(cv, TP._gadget_params(cv, 4), inputs=1, height=2, seed=11)[0]


@pytest.mark.parametrize("cv", [F.BN254, F.BLS12_381], ids=lambda c: c.name)
@pytest.mark.parametrize("which", ["synthetic n_rows = n", "synthetic n_rows < n", "withdraw"])
def test_route_2_equals_the_coefficient_route(cv, which):
    cs = _small_withdraw(cv) if which == "withdraw" else _synthetic(cv, 1024 if which.endswith("= n") else 1021)
    assert cs.check_satisfied()
    predicted = W.predicted_routes(cs, *W.eliminate(cv, cs))
    assert predicted == [2, 2, 2]                          # every wire of these circuits shrinks
    s = _Seam(cv, cs)
    try:
        s.check(which, predicted)
        s.check(which + ", tables reused", predicted)
        # route 1 on the same buffers: the per-variable tables, which need no satisfying witness
        xy, inf, took = s.commit(1)
        want = s.commit(0)
        assert all(np.array_equal(xy[k], want[0][k]) for k in range(3)) and 2 not in took
    finally:
        s.close()


def _relabelled(cs, seed):
    """the same circuit with its variables renamed: other index vectors and another map, the same selectors, still satisfied"""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(len(cs.values)).tolist()
    values = [0] * len(cs.values)
    for old, new in enumerate(perm):
        values[new] = cs.values[old]
    wires = [[v if v == P.ZERO_VAR else perm[v] for v in ws] for ws in (cs.w_l, cs.w_r, cs.w_o)]
    return values, wires


def test_overwritten_wiring_and_other_public_input_positions_are_noticed():
    cv = F.BN254
    cs = _synthetic(cv, 1021)
    s = _Seam(cv, cs)
    try:
        assert s.check("first wiring", [2, 2, 2]) == [2, 2, 2]
        # the index vectors overwritten in place: this round falls back to the coefficients, the next has new tables
        values, wires = _relabelled(cs, 5)
        assert wires[2] != cs.w_o
        s.put(values, wires)
        assert s.check("stale tables", [0, 0, 0]) == [0, 0, 0]
        assert s.check("rebuilt tables", [2, 2, 2]) == [2, 2, 2]
        s.put(cs.values, (cs.w_l, cs.w_r, cs.w_o))
        s.check("back to the first wiring (stale again)", [0, 0, 0])
        s.check("rebuilt", [2, 2, 2])
        # A public input moved onto a linear row frees that row's output: its value is then whatever the proof's public
        # input makes it.  r = a defining row whose output stands on no other wire.
        kind, free, forms = W.eliminate(cv, cs)
        uses = {}
        for ws in (cs.w_l, cs.w_r, cs.w_o):
            for v in ws:
                uses[v] = uses.get(v, 0) + 1
        r = max(g for g in range(cs.n_gates) if cs.w_o[g] in forms and uses[cs.w_o[g]] == 1)
        v = cs.w_o[r]
        pos = sorted(set(cs.pi) | {r})
        assert W.eliminate(cv, cs, pi_pos=pos)[0][v] == W.FREE
        other = list(cs.values)
        other[v] = (other[v] + 12345) % cs.p
        s.put(other, (cs.w_l, cs.w_r, cs.w_o))
        s.check("public input on row %d" % r, [2, 2, 2], pos)      # tables of the old positions would give another point
        s.check("the same positions again", [2, 2, 2], pos)
        s.put(cs.values, (cs.w_l, cs.w_r, cs.w_o))
        s.check("the first positions", [2, 2, 2])
    finally:
        s.close()


def _dense(ctx, prep, tr):
    ctx.profile_enable(1)
    got = ctx.prove_prepared(prep, tr)
    dense = ctx.profile_get("msm_accumulate")[0]
    ctx.profile_enable(0)
    return got, dense


def test_withdraw_proofs_do_not_depend_on_the_route(withdraw):
    st, ctx = withdraw, withdraw["ctx"]
    ctx.set_wire_elimination(2)
    s = _setup(st, ctx)
    forks = [ctx.fork()]                           # made before the parent's first proof: builds its own tables
    try:
        tr = lambda: _transcript(st, s["vk"])
        want = [ctx.prove(*h, tr()) for h in s["hosts"]]
        assert want[0] != want[1] and len(want[0]) == 802
        got, dense = _dense(ctx, s["preps"][0], tr())
        assert got == want[0]
        assert dense == 6, "all three wires go over their free variables: six dense MSMs remain, not %d" % dense
        assert ctx.prove_prepared(s["preps"][1], tr()) == want[1]
        for i in range(4):                         # chained: the two witnesses alternate, every proof announces the next
            got = ctx.prove_prepared(s["preps"][i & 1], tr(), s["preps"][(i & 1) ^ 1])
            assert got == want[i & 1], "chained proof %d" % i
        assert ctx.prove_prepared(s["preps"][0], tr()) == want[0]      # drains the announcement
        forks.append(ctx.fork())                   # made after it: reads the parent's tables
        for f in forks:
            assert f.prove_prepared(s["preps"][1], tr()) == want[1]
            assert f.prove_prepared(s["preps"][0], tr(), s["preps"][1]) == want[0]
            assert f.prove_prepared(s["preps"][1], tr()) == want[1]
            got, dense = _dense(f, s["preps"][0], tr())
            assert got == want[0] and dense == 6, dense
    finally:
        for f in forks:
            f.close()
    try:                                           # (no fork reads the tables any more: the parent may rebuild them)
        ctx.set_wire_elimination(0)
        got, dense = _dense(ctx, s["preps"][0], tr())
        assert got == want[0] and dense == 7, dense
    finally:
        ctx.set_wire_elimination(1)


def test_an_unsatisfied_map_is_refused_alike(withdraw):
    """One Poseidon variable changed -- a free one (an s-box product) and a defined one (a running MDS sum): the proof is
    refused with the same status over free variables as with the route switched off."""
    import zkt_plonk_amd._lib as L
    st, ctx = withdraw, withdraw["ctx"]
    z, cv, cs, TP = st["z"], st["cv"], st["css"][0], st["TP"]
    s = _setup(st, ctx)
    g, d_idx = s["keep"]
    kind, free, forms = W.eliminate(cv, cs)
    base = cs.hash_calls[1][0]
    per = g.vars_per_hash
    bad_free = next(v for v in range(base + per // 2, base + per) if kind[v] == W.FREE)
    bad_defined = next(v for v in range(base + per // 2, base + per) if kind[v] == W.DEFINED and forms[v][0])
    blinders = K.fr_to_mont(cv, field_elems(cv.fr.p, 1415, P.NUM_BLINDERS))
    pi_pos = sorted(cs.pi)
    try:
        for bad in (bad_free, bad_defined):
            d_bad = TP._device_witness(ctx, cv, cs, g, corrupt=bad)
            prep = ctx.prepare_vars_dev(d_bad, len(cs.values), d_idx[0], d_idx[1], d_idx[2], cs.n_gates, K.fr_to_mont(cv, cs.table),
                                        pi_pos, K.fr_to_mont(cv, [cs.pi[k] for k in pi_pos]), blinders)
            codes = []
            for mode in (2, 0):
                ctx.set_wire_elimination(mode)
                with pytest.raises(L.ZktError) as e:
                    ctx.prove_prepared(prep, _transcript(st, s["vk"]))
                codes.append(e.value.code)
            assert codes == [9, 9], (bad, codes)          # ZKT_ERR_QUOTIENT_TOO_SHORT: the circuit is not satisfied
            ctx.free(d_bad)
    finally:
        ctx.set_wire_elimination(1)
