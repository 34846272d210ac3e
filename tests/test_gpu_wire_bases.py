"""Wire commitments over per-variable bases (csrc/lagrange.hip "wire base tables", include/zkt_plonk.h "Commitments of
evaluation vectors"): a wire's evaluation vector is a gather of the variable map, so its commitment needs one scalar per
distinct variable.  The yardstick is the coefficient route -- zkt_commit_evals_dev(path = 0, two blinders) on the evaluation
vector gathered with numpy, which tests/test_gpu_lagrange.py pins to the oracle -- and every point must be bit-equal to it."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import fields as F, plonk as P, coracle as K
from helpers import field_elems

ZERO = 0xFFFFFFFF


class _Seam:
    """A context with a key of n + 8 powers and a circuit of size n (any selectors), plus device buffers for a variable map and
    three index vectors that are reused (same addresses) by every call."""

    def __init__(self, cv, log_n, seed=1):
        import zkt_plonk_amd as z
        self.cv, self.log_n, self.n = cv, log_n, 1 << log_n
        n = self.n
        cs = P.synthetic_circuit(cv, n - 3, 4, seed=seed, n_public=2)
        assert cs.circuit_bound() == n
        self.srs = K.srs_mont(cv, 0x3B5 + log_n, n + 8)
        pk, _, _ = P.setup(K.CBackend(cv, self.srs), [None] * (n + 8), cs, True)
        self.ctx = ctx = z.Context(cv.name, 0)
        ctx.srs_load(self.srs)
        z.GpuProver(ctx, log_n, {k: K.fr_to_mont(cv, pk.polys[k]) if pk.polys[k] else np.zeros((0, 4), dtype=np.uint64)
                                 for k in z.PK_ORDER})
        self.max_vars = 4 * n
        self.d_vars = ctx.alloc(self.max_vars * 32)
        self.d_idx = [ctx.alloc(4 * n) for _ in range(3)]
        self.d_ev = ctx.alloc(n * 32)
        self.blinders = K.fr_to_mont(cv, field_elems(cv.fr.p, 77 + log_n, 6))

    def close(self):
        self.ctx.close()

    def put(self, values_mont, wires):
        self.ctx.upload(self.d_vars, values_mont)
        for d, w in zip(self.d_idx, wires):
            if len(w):
                self.ctx.upload(d, np.asarray(w, dtype=np.uint32))

    def commit(self, n_vars, n_rows, route=1):
        return self.ctx.debug_commit_wires_dev(self.d_vars, n_vars, self.d_idx[0], self.d_idx[1], self.d_idx[2], n_rows,
                                               self.blinders, route)

    def yardstick(self, values_mont, wires):
        """the three points through zkt_commit_evals_dev(path 0, k = 2) on the host-gathered evaluation vectors"""
        out = []
        full = np.concatenate([values_mont, np.zeros((1, 4), np.uint64)])
        for k, w in enumerate(wires):
            w = np.asarray(w, dtype=np.uint32)
            ev = np.zeros((self.n, 4), np.uint64)
            ev[:len(w)] = full[np.where(w == ZERO, len(values_mont), w)]
            self.ctx.upload(self.d_ev, ev)
            xy, inf = self.ctx.commit_evals_dev(self.d_ev, self.blinders[2 * k:2 * k + 2], 0)
            out.append((xy.copy(), inf))
        return out

    def check(self, values_mont, wires, n_rows, what, want_routes=None):
        self.put(values_mont, wires)
        want = self.yardstick(values_mont, wires)
        routed = None
        for route in (1, 0):
            xy, inf, took = self.commit(len(values_mont), n_rows, route)
            for k in range(3):
                assert inf[k] == want[k][1] and np.array_equal(xy[k], want[k][0]), (what, "route", route, "wire", k)
            if route == 0:
                assert took == [0, 0, 0], what
            else:
                routed = took
                if want_routes is not None:
                    assert took == want_routes, (what, took)
        return routed                                     # what the call with route = 1 reported


def _values(cv, n_vars, seed):
    return K.fr_to_mont(cv, field_elems(cv.fr.p, seed, n_vars))


def _random_wiring(rng, n_rows, n_vars):
    """indices with multiplicities 1 .. 9 and one variable on 300 rows; the upper half of the map appears on no wire"""
    pool = []
    v = 0
    while len(pool) < n_rows - 300:
        pool += [v] * int(rng.integers(1, 10))
        v += 1
    assert v + 1 < n_vars // 2
    pool = pool[:n_rows - 300] + [v] * 300
    return rng.permutation(np.array(pool, dtype=np.uint32))


@pytest.fixture(scope="module")
def seam():
    s = _Seam(F.BN254, 10)
    yield s
    s.close()


@pytest.mark.parametrize("cv", [F.BN254, F.BLS12_381], ids=lambda c: c.name)
def test_random_wirings_equal_the_coefficient_route(cv):
    s = _Seam(cv, 10, seed=2)
    try:
        n = s.n
        rng = np.random.default_rng(5)
        n_vars = 2 * n
        vals = _values(cv, n_vars, 900)
        for n_rows in (n, n - 9):
            wires = [_random_wiring(rng, n_rows, n_vars) for _ in range(3)]
            took = s.check(vals, wires, n_rows, "random n_rows=%d" % n_rows, [1, 1, 1])
            assert took == [1, 1, 1]
    finally:
        s.close()


def test_zero_rows_unused_variables_and_degenerate_wires(seam):
    s, cv, n = seam, seam.cv, seam.n
    rng = np.random.default_rng(6)
    n_vars = 3 * n
    vals = _values(cv, n_vars, 901)
    # Variable::Zero on a third of the rows (left), all Zero (right: an empty table; the blinded polynomial is trimmed to
    # nothing and goes through the coefficients), one variable on every row (output)
    n_rows = n - 9
    left = _random_wiring(rng, n_rows, n_vars)
    left[rng.permutation(n_rows)[:n_rows // 3]] = ZERO
    right = np.full(n_rows, ZERO, dtype=np.uint32)
    out = np.full(n_rows, 7, dtype=np.uint32)
    took = s.check(vals, [left, right, out], n_rows, "zero rows / all Zero / one variable")
    assert took[0] == 1 and took[2] == 1
    # the same with n_rows = n: one variable on all n rows is a constant vector (trimmed to one coefficient)
    left = _random_wiring(rng, n, n_vars)
    took = s.check(vals, [left, np.full(n, ZERO, dtype=np.uint32), np.full(n, 7, dtype=np.uint32)], n, "n_rows = n")
    assert took[0] == 1
    # a single variable in the whole map
    one = _values(cv, 1, 902)
    w = np.zeros(n - 9, dtype=np.uint32)
    wz = w.copy()
    wz[::3] = ZERO
    took = s.check(one, [w, wz, w], n - 9, "n_vars = 1")
    assert took == [1, 1, 1]


def test_all_distinct_variables_stay_on_the_dense_route(seam):
    s, cv, n = seam, seam.cv, seam.n
    rng = np.random.default_rng(8)
    n_vars = 2 * n
    vals = _values(cv, n_vars, 903)
    n_rows = n - 9
    distinct = rng.permutation(n_vars)[:n_rows].astype(np.uint32)
    shared = _random_wiring(rng, n_rows, n_vars)
    s.check(vals, [shared, distinct, shared[::-1].copy()], n_rows, "all distinct on the right wire", [1, 0, 1])


def test_an_index_outside_the_map_is_refused(seam):
    import zkt_plonk_amd._lib as L
    s, cv, n = seam, seam.cv, seam.n
    rng = np.random.default_rng(9)
    n_vars = n
    vals = _values(cv, n_vars, 904)
    n_rows = n - 9
    wires = [_random_wiring(rng, n_rows, 2 * n) % np.uint32(n_vars) for _ in range(3)]
    wires[1][17] = n_vars
    s.put(vals, wires)
    for route in (1, 0):
        with pytest.raises(L.ZktError) as e:
            s.commit(n_vars, n_rows, route)
        assert e.value.code == 1   # ZKT_ERR_INVALID_ARGUMENT


def test_index_vectors_overwritten_in_place_are_noticed(seam):
    s, cv, n = seam, seam.cv, seam.n
    rng = np.random.default_rng(10)
    n_vars = 2 * n
    vals = _values(cv, n_vars, 905)
    n_rows = n - 9
    first = [_random_wiring(rng, n_rows, n_vars) for _ in range(3)]
    assert s.check(vals, first, n_rows, "first wiring") == [1, 1, 1]
    second = [_random_wiring(rng, n_rows, n_vars) for _ in range(3)]
    s.put(vals, second)                                   # same device addresses, other contents
    want = s.yardstick(vals, second)
    xy, inf, took = s.commit(n_vars, n_rows, 1)
    for k in range(3):
        assert np.array_equal(xy[k], want[k][0]) and inf[k] == want[k][1], ("stale tables used for wire", k)
    assert took == [0, 0, 0]                              # committed again through the coefficients
    xy, inf, took = s.commit(n_vars, n_rows, 1)           # the tables were rebuilt for the new contents
    for k in range(3):
        assert np.array_equal(xy[k], want[k][0]) and inf[k] == want[k][1]
    assert took == [1, 1, 1]


def test_against_the_oracles_msm():
    """n = 2^8: the commitment of every wire against the oracle's own inverse transform, blinding and MSM."""
    from test_gpu_lagrange import _oracle_commit
    cv = F.BN254
    s = _Seam(cv, 8, seed=4)
    try:
        n = s.n
        rng = np.random.default_rng(11)
        n_vars = n
        ints = field_elems(cv.fr.p, 906, n_vars)
        vals = K.fr_to_mont(cv, ints)
        n_rows = n - 9
        wires = [rng.integers(0, 40 + 30 * k, size=n_rows).astype(np.uint32) for k in range(3)]
        wires[0][::5] = ZERO
        s.put(vals, wires)
        xy, inf, took = s.commit(n_vars, n_rows, 1)
        assert took == [1, 1, 1]
        bl = K.fr_from_mont(cv, s.blinders)
        for k in range(3):
            ev = [0 if v == ZERO else ints[v] for v in wires[k]] + [0] * (n - n_rows)
            want = _oracle_commit(cv, 8, s.srs, ev, bl[2 * k:2 * k + 2])
            got = None if inf[k] else K.points_from_mont(cv, xy[k])[0]
            assert got == want, k
    finally:
        s.close()


# ---- whole proofs: the withdraw circuit at 2^14, witness made on the device ---------------------------------------------
@pytest.fixture(scope="module")
def withdraw():
    import zkt_plonk_amd as z
    from oracle import composer as OC
    import test_gpu_poseidon as TP
    cv = F.BN254
    prm = TP._gadget_params(cv, 4)
    css = [OC.withdraw_instance(cv, prm, inputs=1, height=7, seed=sd)[0] for sd in (11, 12)]
    cs = css[0]
    assert (css[1].w_l, css[1].w_r, css[1].w_o) == (cs.w_l, cs.w_r, cs.w_o) and css[1].values != cs.values
    n = cs.circuit_bound()
    ctx = z.Context(cv.name, 0)
    ctx.srs_generate(0x5EED5EED1234567890ABCDEF % cv.fr.p, n + 8)
    evals = {k: K.fr_to_mont(cv, v) for k, v in P.setup_evals(K.CBackend(cv, K.srs_mont(cv, 3, 4)), cs).items()}
    st = dict(z=z, cv=cv, prm=prm, css=css, n=n, ctx=ctx, evals=evals, TP=TP)
    yield st
    ctx.close()


def _setup(st, ctx):
    """circuit, vk commitments, gadget, the two device witnesses, shared index vectors and prepared inputs on `ctx`"""
    z, cv, css, TP = st["z"], st["cv"], st["css"], st["TP"]
    cs = css[0]
    prover, commits = z.GpuProver.setup(ctx, 14, st["evals"])
    L = cv.fq.limbs64
    rinv = pow(1 << (64 * L), -1, cv.fq.p)
    vk = {}
    for name in z.PK_ORDER:
        xy, inf = commits[name]
        vk[name] = None if inf else tuple(sum(int(v) << (64 * i) for i, v in enumerate(h)) * rinv % cv.fq.p for h in (xy[:L], xy[L:]))
    g = TP._gadget(z, ctx, cv, st["prm"])
    to_idx = lambda ws: np.array([ZERO if v == P.ZERO_VAR else v for v in ws], dtype=np.uint32)
    d_idx = []
    for ws in (cs.w_l, cs.w_r, cs.w_o):
        d = ctx.alloc(4 * len(ws))
        ctx.upload(d, to_idx(ws))
        d_idx.append(d)
    blinders = K.fr_to_mont(cv, field_elems(cv.fr.p, 1415, P.NUM_BLINDERS))
    preps, hosts = [], []
    for c_ in css:
        d_vars = TP._device_witness(ctx, cv, c_, g)
        pi_pos = sorted(c_.pi)
        pi_vals = K.fr_to_mont(cv, [c_.pi[k] for k in pi_pos])
        table = K.fr_to_mont(cv, c_.table)
        preps.append(ctx.prepare_vars_dev(d_vars, len(c_.values), d_idx[0], d_idx[1], d_idx[2], c_.n_gates, table, pi_pos,
                                          pi_vals, blinders))
        a, b, c = c_.wire_evals(c_.n_gates)
        hosts.append((K.fr_to_mont(cv, a), K.fr_to_mont(cv, b), K.fr_to_mont(cv, c), table, pi_pos, pi_vals, blinders))
    return dict(vk=vk, preps=preps, hosts=hosts, keep=(g, d_idx))


def _transcript(st, vk):
    z, cv = st["z"], st["cv"]
    return z.seed_transcript(z.Transcript("merlin", "ZKT Plonk", fr_bits=cv.fr.bits, fq_bytes=8 * cv.fq.limbs64), st["n"], vk)


def test_proof_bytes_do_not_depend_on_the_wire_route(withdraw):
    st, ctx = withdraw, withdraw["ctx"]
    s = _setup(st, ctx)
    fork_before = ctx.fork()                       # made before the parent's first proof: builds its own tables
    try:
        tr = lambda: _transcript(st, s["vk"])
        # the same witnesses as three evaluation vectors (no variable map: the coefficient route)
        want = [ctx.prove(*h, tr()) for h in s["hosts"]]
        assert want[0] != want[1] and len(want[0]) == 802
        ctx.profile_enable(1)
        got = ctx.prove_prepared(s["preps"][0], tr())
        dense = ctx.profile_get("msm_accumulate")[0]
        ctx.profile_enable(0)
        assert got == want[0]
        assert dense == 7, "a and b are committed over their base tables: seven dense MSMs remain, not %d" % dense
        ctx.set_lagrange(False)
        assert ctx.prove_prepared(s["preps"][0], tr()) == want[0]
        ctx.set_lagrange(True)
        # chained: the two witnesses alternate, every proof announces the next
        for i in range(4):
            got = ctx.prove_prepared(s["preps"][i & 1], tr(), s["preps"][(i & 1) ^ 1])
            assert got == want[i & 1], "chained proof %d" % i
        assert ctx.prove_prepared(s["preps"][0], tr()) == want[0]      # drains the announcement
        # forks: one made before the parent's first proof, one after it (reads the parent's tables)
        fork_after = ctx.fork()
        try:
            for f in (fork_before, fork_after):
                assert f.prove_prepared(s["preps"][1], tr()) == want[1]
                assert f.prove_prepared(s["preps"][0], tr(), s["preps"][1]) == want[0]
                assert f.prove_prepared(s["preps"][1], tr()) == want[1]
        finally:
            fork_after.close()
    finally:
        fork_before.close()
