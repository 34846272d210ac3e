"""The withdraw circuit as a library component on the device (zkt_withdraw_*, zkt_note_leaves): rows, setup, the witness of
a batch of withdrawals and whole proofs, against the oracle's restatement of the reference composer (tests/withdraw_cases.py;
the host planner is pinned on the CPU by test_withdraw_layout_host.py) and against the existing setup path fed the oracle's
data."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import coracle as K, plonk as P
from helpers import field_elems

import withdraw_cases as WC

SENTINEL = 0x5E0715E15E0715E1       # every word of a map before the call


class World:
    """Per module: one context per curve, one circuit handle per shape, each made once."""

    def __init__(self):
        import zkt_plonk_amd as z
        self.z, self.ctx, self.circuits = z, {}, {}

    def context(self, cvname):
        if cvname not in self.ctx:
            self.ctx[cvname] = self.z.Context(cvname, 0)
        return self.ctx[cvname]

    def circuit(self, c):
        key = (c.cv.name, c.w, c.inputs, c.height, id(c.prm))
        if key not in self.circuits:
            self.circuits[key] = self.z.WithdrawCircuit(self.context(c.cv.name), c.words, c.inputs, c.height)
        return self.circuits[key]

    def close(self):
        for w in self.circuits.values():
            w.close()
        for c in self.ctx.values():
            c.close()


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.close()


class Map:
    """batch maps of `stride` scalars in HBM, every word the sentinel."""

    def __init__(self, ctx, batch, stride):
        self.ctx, self.batch, self.stride = ctx, batch, stride
        self.d = ctx.alloc(batch * stride * 32)
        ctx.upload(self.d, np.full((batch * stride, 4), SENTINEL, dtype=np.uint64))

    def words(self):
        return self.ctx.download(self.d, (self.batch, self.stride, 4))

    def free(self):
        self.ctx.free(self.d)


def _check_maps(cases, got, pi, status, stride):
    """Every variable equals cs.values, the padding still holds the sentinel, out_pi equals cs.pi in position order = the CLI's
    list, no path is reported."""
    for b, c in enumerate(cases):
        assert K.fr_from_mont(c.cv, got[b, :c.n_vars]) == c.cs.values, b
        assert (got[b, c.n_vars:] == np.uint64(SENTINEL)).all(), b
        assert K.fr_from_mont(c.cv, pi[b]) == [c.cs.pi[i] for i in c.pi_pos] == c.cli_pi, b
    assert status == [0] * len(cases)


def _run(world, cases, stride=None, siblings=True, root=True, tree=None):
    c0 = cases[0]
    w = world.circuit(c0)
    stride = c0.n_vars if stride is None else stride
    m = Map(w.ctx, len(cases), stride)
    try:
        pi, status = w.witness([WC.request_words(c.cv, c.req, siblings, root) for c in cases], m.d, stride, tree=tree)
        return m.words(), pi, status
    finally:
        m.free()


# ---- rows -----------------------------------------------------------------------------------------------------------------
ALL = [(s, False) for s in WC.SHAPES] + [(WC.SHIPPED, True)]
IDS = ["%s-x%d-%dx%d%s" % (s + ("-shipped" if sh else "",)) for s, sh in ALL]


@pytest.mark.parametrize("shape,shipped", ALL, ids=IDS)
def test_device_rows_equal_the_composer(world, shape, shipped):
    cvname, width, inputs, height = shape
    c = WC.case(cvname, width, inputs, height, shipped)
    w = world.circuit(c)
    info = w.info
    assert (info["inputs"], info["height"], info["width"]) == (inputs, height, width)
    assert info["n_gates"] == c.n_gates and info["n_vars"] == c.n_vars and info["n_pi"] == inputs + 4
    assert info["n_hashes"] == inputs * (3 + height) + 2 and info["vars_per_hash"] == c.prm.gates_per_hash
    assert (1 << info["log_n_min"]) >= c.n_gates > (1 << (info["log_n_min"] - 1))
    assert info["device_bytes"] >= 3 * 4 * c.n_gates
    assert w.pi_pos == c.pi_pos
    sel, wires = w.rows()
    for name, got, want in zip(("q_m", "q_l", "q_r", "q_o", "q_c", "q_lookup"), sel, c.selectors()):
        assert K.fr_from_mont(c.cv, got) == want, name
    for name, got, want in zip(("w_l", "w_r", "w_o"), wires, c.wires()):
        assert got.tolist() == want, name
    only_wires = w.rows(selectors=False)
    assert only_wires[0] is None and [a.tolist() for a in only_wires[1]] == c.wires()


def test_shapes_the_circuit_does_not_have_are_refused(world):
    z = world.z
    ctx = world.context("bn254")
    cv = WC.case("bn254", 4, 1, 1).cv
    good = WC.params_words(cv, WC.params("bn254", 4))
    for words, inputs, height in [(WC.params_words(cv, WC.params("bn254", 3)), 1, 1), (good, 0, 1), (good, 33, 1), (good, 1, 0), (good, 1, 65)]:
        with pytest.raises(z.ZktError) as e:
            ctx.withdraw_create(words, inputs, height)
        assert e.value.code == 1


# ---- setup ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def setups(world):
    """(case name) -> the ten commitments of zkt_circuit_setup_wiring fed the oracle composer's selectors, table mask and
    wiring; computed once, the SRS left loaded"""
    made = {}

    def get(c, tau=0x7E57):
        key = (c.cv.name, c.w, c.inputs, c.height)
        if key not in made:
            ctx = world.context(c.cv.name)
            n = c.cs.circuit_bound()
            log_n = n.bit_length() - 1
            ctx.srs_load(K.srs_mont(c.cv, tau, n + 8))
            ev = P.setup_evals(K.CBackend(c.cv, None), c.cs)
            evals = [None if k in ("sigma1", "sigma2", "sigma3") else K.fr_to_mont(c.cv, ev[k]) for k in world.z.PK_ORDER]
            wl, wr, wo = c.wires()
            made[key] = (log_n, tau, ctx.circuit_setup_wiring(log_n, evals, wl, wr, wo, c.n_vars))
        return made[key]
    return get


@pytest.mark.parametrize("shape", [WC.SHAPES[1], WC.SHAPES[4]], ids=[IDS[1], IDS[4]])
def test_setup_equals_the_setup_from_the_composers_data(world, setups, shape):
    c = WC.case(*shape)
    log_n, _, (want, want_inf) = setups(c)
    w = world.circuit(c)
    assert log_n == w.info["log_n_min"]
    got, got_inf = w.setup(log_n, WC.TABLE_SIZE)
    assert got_inf.tolist() == want_inf.tolist()
    assert np.array_equal(got, want)
    for bad_log_n, bad_table in ((log_n - 1, WC.TABLE_SIZE), (log_n, 1 << log_n)):
        with pytest.raises(world.z.ZktError) as e:
            w.setup(bad_log_n, bad_table)
        assert e.value.code == 1


# ---- witness --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", WC.SHAPES, ids=IDS[:len(WC.SHAPES)])
def test_witness_equals_the_composers_values(world, shape):
    c = WC.case(*shape)
    got, pi, status = _run(world, [c])
    _check_maps([c], got, pi, status, c.n_vars)


def test_a_batch_of_three_requests_with_padding(world):
    """Three different requests, stride = n_vars + 5: amount_out random, 0 (withdraw everything) and with bit 63 set (the
    amounts sum to 2^64 - 1); the padding keeps the sentinel."""
    cases = [WC.case("bn254", 4, 3, 2), WC.case("bn254", 4, 3, 2, seed=2, mode="all"), WC.case("bn254", 4, 3, 2, seed=3, mode="top")]
    assert sum(cases[1].req["amounts"]) == cases[1].req["withdraw_amount"]
    assert (sum(cases[2].req["amounts"]) - cases[2].req["withdraw_amount"]) >> 63 == 1
    stride = cases[0].n_vars + 5
    got, pi, status = _run(world, cases, stride)
    _check_maps(cases, got, pi, status, stride)
    again, pi2, _ = _run(world, cases[::-1], stride)                  # the kept index vectors serve a second call
    _check_maps(cases[::-1], again, pi2, status, stride)


def test_position_bits_of_both_values_and_a_single_input(world):
    c = WC.case("bn254", 5, 2, 2, seed=4, mode="bits")
    idx = [i for i, _ in c.req["poes"]]
    for level in range(2):
        assert {(i >> level) & 1 for i in idx} == {0, 1}
    got, pi, status = _run(world, [c])
    _check_maps([c], got, pi, status, c.n_vars)
    one = WC.case("bn254", 4, 1, 3, seed=5, mode="top")
    got, pi, status = _run(world, [one, WC.case("bn254", 4, 1, 3, seed=6, mode="all")])
    _check_maps([one, WC.case("bn254", 4, 1, 3, seed=6, mode="all")], got, pi, status, one.n_vars)


@pytest.mark.parametrize("shape", [WC.SHAPES[2], WC.SHAPES[4]], ids=[IDS[2], IDS[4]])
def test_siblings_from_a_device_tree_give_the_same_map(world, shape):
    """The caller's siblings and root, and siblings and root taken from a zkt_merkle_tree holding the same leaves (the spent
    notes and the decoys), produce identical maps."""
    cases = [WC.case(*shape), WC.case(*shape, seed=8)]
    w = world.circuit(cases[0])
    given, pi_given, st_given = _run(world, cases)
    _check_maps(cases, given, pi_given, st_given, cases[0].n_vars)
    for c in cases:
        tree = world.z.MerkleTree(w.ctx, w.poseidon_handle, c.height, 1 << c.height)
        try:
            tree.append(K.fr_to_mont(c.cv, c.req["leaves"]))
            assert K.fr_from_mont(c.cv, tree.root().reshape(1, 4)) == [c.req["root"]]
            got, pi, status = _run(world, [c], siblings=False, root=False, tree=tree)
            _check_maps([c], got, pi, status, c.n_vars)
            m = Map(w.ctx, 2, c.n_vars)                                 # one request of each kind in one call
            try:
                w.witness([WC.request_words(c.cv, c.req), WC.request_words(c.cv, c.req, siblings=False)], m.d, c.n_vars, tree=tree)
                mixed = m.words()
            finally:
                m.free()
            assert np.array_equal(mixed[0], got[0]) and np.array_equal(mixed[1], got[0])
        finally:
            tree.close()
    with pytest.raises(world.z.ZktError) as e:                        # no tree to take them from
        _run(world, [cases[0]], siblings=False)
    assert e.value.code == 1
    other = world.z.MerkleTree(w.ctx, w.poseidon_handle, cases[0].height + 1, 4)
    try:
        with pytest.raises(world.z.ZktError) as e:                    # a tree of another height
            _run(world, [cases[0]], siblings=False, tree=other)
        assert e.value.code == 1
    finally:
        other.close()


# ---- whole proof ----------------------------------------------------------------------------------------------------------
def _affine_commits(z, cv, commits, inf):
    return {k: (None if inf[i] else K.points_from_mont(cv, np.asarray(commits[i]).reshape(1, -1))[0]) for i, k in enumerate(z.PK_ORDER)}


@pytest.mark.parametrize("shape", [WC.SHAPES[1], WC.SHAPES[4]], ids=[IDS[1], IDS[4]])
def test_proof_from_the_device_map_equals_the_oracle_provers(world, shape):
    """zkt_withdraw_setup, zkt_withdraw_witness, zkt_prove on the device-made map: the oracle prover's bytes for the same
    blinders and table; zkt_verify accepts them with the CLI-order public inputs."""
    z = world.z
    from zkt_plonk_amd import _lib
    c = WC.case(*shape)
    cv, cs = c.cv, c.cs
    n, tau = cs.circuit_bound(), 0x5EED5
    srs = K.srs_mont(cv, tau, n + 8)
    be = K.CBackend(cv, srs)
    pk, epk, vk = P.setup(be, [None] * (n + 8), cs, True)
    blinders = field_elems(cv.fr.p, 0xB11D, P.NUM_BLINDERS)
    want = P.prove(be, [None] * (n + 8), pk, epk, vk, cs, P.new_seeded_transcript(cv, vk), blinders).serialize(cv)
    w = world.circuit(c)
    ctx = w.ctx
    ctx.srs_load(srs)
    log_n = n.bit_length() - 1
    commits, inf = w.setup(log_n, WC.TABLE_SIZE)
    pts = _affine_commits(z, cv, commits, inf)
    assert pts == {k: vk.commits[k] for k in z.PK_ORDER}
    m = Map(ctx, 1, c.n_vars)
    try:
        pi, status = w.witness([WC.request_words(cv, c.req)], m.d, c.n_vars)
        assert status == [0]
        prep = w.prepare(m.d, c.n_vars, 0, K.fr_to_mont(cv, cs.table), pi[0], K.fr_to_mont(cv, blinders))
        assert ctx.check_witness(prep, z.CHECK_WIRING).satisfied
        tr = lambda: z.seed_transcript(z.Transcript("merlin", "ZKT Plonk", fr_bits=cv.fr.bits, fq_bytes=cv.fq.limbs64 * 8), n, pts)
        proof = ctx.prove_prepared(prep, tr())
        assert proof == want
        roots = be.domain(n).elements()
        h, beta_h = _lib.srs_generate_g2(cv.name, tau)
        ok = lambda pub: _lib.verify(cv.name, n, commits, list(inf), K.fr_to_mont(cv, [roots[i] for i in c.pi_pos]), K.fr_to_mont(cv, pub), proof,
                                     ctx.srs_download(0, 1)[0], h, beta_h, tr())
        assert ok(c.cli_pi)
        assert not ok(c.cli_pi[:-1] + [c.cli_pi[-1] + 1])
    finally:
        m.free()


def test_a_wrong_sibling_is_reported_and_the_map_is_still_written(world):
    """A flipped sibling of note 1: bad_paths == 0b10, the map is the composer's for that (unsatisfiable) request, and
    zkt_circuit_check_witness names that note's equal_constrain row."""
    z = world.z
    c = WC.case(*WC.SHAPES[2])
    req = dict(c.req)
    idx, path = req["poes"][1]
    req["poes"] = [req["poes"][0], (idx, path[:-1] + [(path[-1] + 1) % c.prm.p])]
    twin = WC.synthesize(c.cv, c.prm, req)
    assert not twin.check_satisfied()
    note_rows = (3 + c.height) * c.prm.gates_per_hash + 7 * c.height + 4
    equal_row = 1 + 2 * note_rows - 2                                  # note 1's last row but one: equal_constrain(root, pub_root)
    assert (twin.q_l[equal_row], twin.q_r[equal_row], twin.q_o[equal_row]) == (1, c.prm.p - 1, 0)
    assert twin.w_r[equal_row] == 2 * c.inputs and twin.w_o[equal_row] == P.ZERO_VAR
    w = world.circuit(c)
    ctx = w.ctx
    n = c.cs.circuit_bound()
    ctx.srs_load(K.srs_mont(c.cv, 0x7E57, n + 8))
    w.setup(n.bit_length() - 1, WC.TABLE_SIZE)
    m = Map(ctx, 1, c.n_vars)
    try:
        pi, status = w.witness([WC.request_words(c.cv, req)], m.d, c.n_vars)
        assert status == [0b10]
        assert K.fr_from_mont(c.cv, m.words()[0]) == twin.values
        assert K.fr_from_mont(c.cv, pi[0]) == [twin.pi[i] for i in c.pi_pos]
        rep = ctx.check_witness(w.prepare(m.d, c.n_vars, 0, K.fr_to_mont(c.cv, twin.table), pi[0], None))
        assert not rep.satisfied and rep.n_arithmetic == 1 and rep.first_arithmetic == equal_row
    finally:
        m.free()


def test_refusals_leave_the_map_untouched(world):
    z = world.z
    c = WC.case(*WC.SHAPES[2])
    w = world.circuit(c)
    good = WC.request_words(c.cv, c.req)
    total = sum(c.req["amounts"])

    def bad(**kw):
        r = dict(good)
        r.update(kw)
        return r
    zero_secret = good["secrets"].copy()
    zero_secret[1] = 0
    index = good["leaf_indices"].copy()
    index[0] = 1 << c.height
    cases = [(bad(secrets=zero_secret), 6),                                               # ZKT_ERR_ZERO_DENOMINATOR
             (bad(withdraw_amount=total + 1), 1),
             (bad(amounts=np.array([1 << 63, 1 << 63], dtype=np.uint64), withdraw_amount=1), 1),
             (bad(leaf_indices=index), 1)]
    m = Map(w.ctx, 2, c.n_vars)
    try:
        for req, code in cases:
            for reqs in ([req], [good, req]):
                with pytest.raises(z.ZktError) as e:
                    w.ctx.withdraw_witness(w.handle, reqs, m.d, c.n_vars)
                assert e.value.code == code
        for reqs, stride in (([], c.n_vars), ([good], c.n_vars - 1), ([good] * 257, c.n_vars)):
            with pytest.raises(z.ZktError) as e:
                w.ctx.withdraw_witness(w.handle, reqs, m.d, stride)
            assert e.value.code == 1
        w.ctx.synchronize()
        assert (m.words() == np.uint64(SENTINEL)).all()
        pi, status = w.ctx.withdraw_witness(w.handle, [good], m.d, c.n_vars)          # the handle is as usable as before
        assert status == [0] and K.fr_from_mont(c.cv, pi[0]) == c.cli_pi
    finally:
        m.free()


# ---- deposit leaves -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 5])
def test_note_leaves_equal_the_native_hashes_and_feed_the_tree(world, m):
    c = WC.case(*WC.SHAPES[1])                                        # a tree of five notes
    assert len(c.req["notes"]) >= m
    w = world.circuit(c)
    ctx = w.ctx
    notes = c.req["notes"][:m]
    arrays = [K.fr_to_mont(c.cv, [nt[0] for nt in notes]), K.fr_to_mont(c.cv, [nt[1] for nt in notes]),
              np.array([nt[2] for nt in notes], dtype=np.uint64), np.zeros((m, 4), dtype=np.uint64)]
    d = [ctx.alloc(a.nbytes) for a in arrays]
    tree = world.z.MerkleTree(ctx, w.poseidon_handle, c.height, 1 << c.height)
    try:
        for p, a in zip(d, arrays):
            ctx.upload(p, a)
        ctx.note_leaves(w.poseidon_handle, d[0], d[1], d[2], m, d[3])
        want = [c.prm.native([nt[1], nt[2], c.prm.native([nt[0]])]) for nt in notes]
        assert K.fr_from_mont(c.cv, ctx.download(d[3], (m, 4))) == want == c.req["leaves"][:m]
        tree.append(d_leaves=d[3], m=m)
        from oracle import composer as OC
        native = OC.NativeMerkleTree(c.prm, c.height)
        for leaf in want:
            native.add_leaf(leaf)
        assert K.fr_from_mont(c.cv, tree.root().reshape(1, 4)) == [native.root]
    finally:
        tree.close()
        for p in d:
            ctx.free(p)


# ---- a caller's busy stream -----------------------------------------------------------------------------------------------
def test_enqueue_only_witness_then_prove_on_a_busy_stream(world):
    """zkt_withdraw_witness with neither output (enqueue only) returns while the caller's work on the stream is still
    pending, and zkt_prove follows directly on the map it left: the same proof as on the idle stream."""
    import torch
    import stream_rig as SR
    z = world.z
    c = WC.case(*WC.SHAPES[1])
    cv = c.cv
    ctx = z.Context(cv.name, 0)
    stream = torch.cuda.Stream()
    try:
        rig = SR.Rig(ctx, stream)
        n = c.cs.circuit_bound()
        log_n = n.bit_length() - 1
        ctx.srs_load(K.srs_mont(cv, 0x7E57, n + 8))
        w = z.WithdrawCircuit(ctx, c.words, c.inputs, c.height)
        commits, inf = w.setup(log_n, WC.TABLE_SIZE)
        pts = _affine_commits(z, cv, commits, inf)
        blinders = K.fr_to_mont(cv, field_elems(cv.fr.p, 0xB11D, P.NUM_BLINDERS))
        table = K.fr_to_mont(cv, c.cs.table)
        with torch.cuda.stream(stream):
            vars_t = torch.empty(c.n_vars * 4, dtype=torch.int64, device="cuda")
        reqs = [WC.request_words(cv, c.req)]
        pi_vals = K.fr_to_mont(cv, c.cli_pi)
        prep = w.prepare(vars_t.data_ptr(), c.n_vars, 0, table, pi_vals, blinders)
        tr = lambda: z.seed_transcript(z.Transcript("merlin", "ZKT Plonk", fr_bits=cv.fr.bits, fq_bytes=cv.fq.limbs64 * 8), n, pts)

        def body(mode, data):
            mode.begin()
            mode.enqueue("zkt_withdraw_witness", w.witness, reqs, vars_t.data_ptr(), c.n_vars, want_pi=False, want_status=False)
            proof = mode.blocking("zkt_prove", ctx.prove_prepared, prep, tr())
            return proof, SR.host(vars_t).reshape(-1, 4).copy()

        results = rig.three_ways(body, [], [], [], outs=[vars_t])
        first = ctx.prove_prepared(ctx.prepare_vars(K.fr_to_mont(cv, c.cs.values), *c.wires(), table, c.pi_pos, pi_vals, blinders), tr())
        SR.compare("zkt_withdraw_witness + zkt_prove", results, (first, K.fr_to_mont(cv, c.cs.values)), decoy_differs=False)
        assert rig.held_calls == 1
        w.close()
    finally:
        ctx.close()
