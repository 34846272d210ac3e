"""zkt_withdraw_prove: the CLI's ProveWithdraw for a batch of requests in one call, against the sequence of calls it replaces
(zkt_withdraw_witness, zkt_prove under a transcript seeded from the setup's commitments, zkt_verify, zkt_merkle_tree_append) and,
at one shape, against the oracle prover.  Requests come from tests/withdraw_cases.py: three per shape (seeds 1, 2, 3), each with
its own siblings and root, so the tree handed to the call only takes the new leaves.  The reference proofs of a shape are made
once and shared."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import composer as OC, coracle as K, plonk as P
from helpers import field_elems

import withdraw_cases as WC

SHAPES = [WC.SHAPES[1], WC.SHAPES[2], WC.SHAPES[4]]
IDS = ["%s-x%d-%dx%d" % s for s in SHAPES]
SENTINEL = 0x5E0715E15E0715E1
NONE = (1 << 64) - 1                # new_leaf_index of a request that added no leaf
TAU = 0x5EED5
ERR_INVALID_ARGUMENT, ERR_NOT_IN_TABLE = 1, 8


class Env:
    """One shape: three cases, the circuit set up on the curve's context, and the proofs of the assembled path."""

    def __init__(self, world, shape):
        z = world.z
        from zkt_plonk_amd import _lib
        self.z, self.shape = z, shape
        self.cases = [WC.case(*shape, seed=k) for k in (1, 2, 3)]
        c = self.cases[0]
        self.cv, self.n_vars, self.height = c.cv, c.n_vars, c.height
        assert all(x.req["ident_set"] == c.req["ident_set"] and x.n_vars == c.n_vars for x in self.cases)
        self.n = c.cs.circuit_bound()
        self.w = world.circuit(c)
        self.ctx = self.w.ctx
        self.set_mont = K.fr_to_mont(self.cv, c.req["ident_set"])
        self.table = K.fr_to_mont(self.cv, c.cs.table)
        self.blinders = np.stack([K.fr_to_mont(self.cv, field_elems(self.cv.fr.p, 0xB11D + b, P.NUM_BLINDERS)) for b in range(3)])
        self.reqs = [WC.request_words(x.cv, x.req) for x in self.cases]
        self.h, self.beta_h = _lib.srs_generate_g2(self.cv.name, TAU)
        self.ref = None

    def load(self, world):
        """The SRS and this shape's circuit on the context (another shape may have been there)."""
        if world.loaded.get(self.cv.name) is not self:
            self.srs = K.srs_mont(self.cv, TAU, self.n + 8)
            self.ctx.srs_load(self.srs)
            self.commits, self.inf = self.w.setup(self.n.bit_length() - 1, WC.TABLE_SIZE)
            self.pts = {k: (None if self.inf[i] else K.points_from_mont(self.cv, np.asarray(self.commits[i]).reshape(1, -1))[0])
                        for i, k in enumerate(self.z.PK_ORDER)}
            self.g = self.ctx.srs_download(0, 1)[0]
            world.loaded[self.cv.name] = self
            first = self.assembled(self.reqs[:1], self.table)      # the first proof after a load builds the domain's tables
            assert self.ref is None or first == self.ref[:1]
        if self.ref is None:
            self.ref = self.assembled(self.reqs, self.table)
        return self

    def transcript(self):
        z = self.z
        return z.seed_transcript(z.Transcript("merlin", "ZKT Plonk", fr_bits=self.cv.fr.bits, fq_bytes=self.cv.fq.limbs64 * 8), self.n, self.pts)

    def map(self, slots):
        d = self.ctx.alloc(slots * self.n_vars * 32)
        self.ctx.upload(d, np.full((slots * self.n_vars, 4), SENTINEL, dtype=np.uint64))
        return d

    def assembled(self, reqs, table):
        """The calls zkt_withdraw_prove replaces -> [proof bytes, or the code zkt_prove refused with, or None for a bad path]."""
        d = self.map(len(reqs))
        try:
            pi, status = self.w.witness(reqs, d, self.n_vars)
            out = []
            for b in range(len(reqs)):
                if status[b]:
                    out.append(None)
                    continue
                try:
                    out.append(self.ctx.prove_prepared(self.w.prepare(d, self.n_vars, b, table, pi[b], self.blinders[b]), self.transcript()))
                except self.z.ZktError as e:
                    out.append(e.code)
            return out
        finally:
            self.ctx.free(d)

    def tree(self, capacity=None):
        """A tree of the circuit's height that holds one leaf already where it has room for four."""
        t = self.z.MerkleTree(self.ctx, self.w.poseidon_handle, self.height, capacity or (1 << self.height))
        if capacity is None and (1 << self.height) >= 4:
            t.append(K.fr_to_mont(self.cv, [0xABCDEF]))
        return t

    def prove(self, reqs=None, slots=2, set_mont=None, tree=None, verify=True, append=False, beta_h=None, w=None, settled=True):
        """zkt_withdraw_prove over a fresh workspace of `slots` maps; whatever the call does -- prove, refuse a request, refuse
        the batch -- the library holds the device allocations afterwards that it held before (settled = False: the first proof
        after an SRS or a circuit was loaded, which builds that domain's tables)."""
        d = self.map(slots)
        reqs = self.reqs if reqs is None else reqs
        before = self.z._lib.debug_live_allocations()
        try:
            return (w or self.w).prove(reqs, d, slots, self.set_mont if set_mont is None else set_mont, self.blinders[:len(reqs)], tree=tree,
                                       verify_key=(self.g, self.h, self.beta_h if beta_h is None else beta_h) if verify else None, append=append)
        finally:
            assert not settled or self.z._lib.debug_live_allocations() == before
            self.ctx.free(d)

    def plain_proof_still_comes_out(self):
        """A plain zkt_prove on the same context afterwards gives its usual bytes."""
        assert self.assembled(self.reqs[:1], self.table) == self.ref[:1]


class World:
    def __init__(self):
        import zkt_plonk_amd as z
        self.z, self.ctx, self.circuits, self.envs, self.loaded = z, {}, {}, {}, {}

    def circuit(self, c):
        if c.cv.name not in self.ctx:
            self.ctx[c.cv.name] = self.z.Context(c.cv.name, 0)
        key = (c.cv.name, c.w, c.inputs, c.height)
        if key not in self.circuits:
            self.circuits[key] = self.z.WithdrawCircuit(self.ctx[c.cv.name], c.words, c.inputs, c.height)
        return self.circuits[key]

    def env(self, shape):
        if shape not in self.envs:
            self.envs[shape] = Env(self, shape)
        return self.envs[shape].load(self)

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


def _same_tree(env, t, leaves, prefilled):
    """t equals a second tree that got the same new leaves through zkt_merkle_tree_append: count, root, every layer."""
    t2 = env.tree()
    try:
        if leaves:
            assert t2.append(K.fr_to_mont(env.cv, leaves)) == prefilled
        assert t.count == t2.count == prefilled + len(leaves)
        assert np.array_equal(t.root(), t2.root())
        for L in range(env.height):
            assert np.array_equal(t.layer(L), t2.layer(L)), L
    finally:
        t2.close()


def _prefilled(env):
    return 1 if (1 << env.height) >= 4 else 0


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_one_call_equals_the_assembled_path(world, shape):
    """batch 3 in chunks of 2 maps (a chunk boundary inside the batch): every proof is the assembled path's for the same blinders
    and the deduplicated table -- at the first shape the oracle prover's as well --, out_pi is the CLI's list, all three verify,
    and the tree has the three new leaves at consecutive indices.  Chunks of 1 and of 3 maps give the same bytes.  A tree of
    height 1 holds two leaves, so at that shape the batch cannot be appended and the call runs with append = 0."""
    env = world.env(shape)
    z, cv = env.z, env.cv
    assert all(isinstance(p, bytes) and len(p) in (802, 1010) for p in env.ref)
    if shape == SHAPES[0]:
        be = K.CBackend(cv, env.srs)
        ck = [None] * (env.n + 8)
        for b, c in enumerate(env.cases):
            pk, epk, vk = P.setup(be, ck, c.cs, True)
            want = P.prove(be, ck, pk, epk, vk, c.cs, P.new_seeded_transcript(cv, vk), K.fr_from_mont(cv, env.blinders[b])).serialize(cv)
            assert env.ref[b] == want, b
    can_append = (1 << env.height) >= 3
    t = env.tree()
    before = z._lib.debug_live_allocations()
    try:
        proofs, pi, res = env.prove(slots=2, tree=t, append=can_append)
        assert z._lib.debug_live_allocations() == before
        assert proofs == env.ref
        for b, c in enumerate(env.cases):
            assert K.fr_from_mont(cv, pi[b]) == c.cli_pi, b
        first = _prefilled(env)
        assert res == [dict(code=0, bad_paths=0, verified=True, new_leaf_index=first + b if can_append else NONE) for b in range(3)]
        _same_tree(env, t, [c.cli_pi[-1] for c in env.cases] if can_append else [], first)
        if not can_append:            # what the small tree does hold: a batch of two
            p2, _, res2 = env.prove(reqs=env.reqs[:2], slots=1, tree=t, append=True)
            assert p2 == env.ref[:2] and res2 == [dict(code=0, bad_paths=0, verified=True, new_leaf_index=b) for b in range(2)]
            _same_tree(env, t, [c.cli_pi[-1] for c in env.cases[:2]], first)
        for slots in (1, 3):
            p2, pi2, res2 = env.prove(slots=slots, verify=False)
            assert p2 == env.ref and np.array_equal(pi2, pi), slots
            assert res2 == [dict(code=0, bad_paths=0, verified=False, new_leaf_index=NONE)] * 3
    finally:
        t.close()
    env.plain_proof_still_comes_out()


def _outside_the_set(c):
    """The case's request with the first spent note's identifier replaced by a value outside the set, the tree rebuilt around it:
    every path still ends in the root, only the lookup fails."""
    req = dict(c.req)
    spent = [i for i, _ in req["poes"]]
    x = 0x0DD1D
    assert x not in req["ident_set"]
    notes = [list(nt) for nt in req["notes"]]
    notes[spent[0]][1] = x
    tree = OC.NativeMerkleTree(c.prm, c.height)
    for secret, ident, amount, _ in notes:
        tree.add_leaf(c.prm.native([ident, amount, c.prm.native([secret])]))
    req.update(identifiers=[notes[i][1] for i in spent], poes=[(i, tree.merkle_path(i)) for i in spent], root=tree.root)
    return req


def _wrong_sibling(c):
    req = dict(c.req)
    idx, path = req["poes"][-1]
    req["poes"] = list(req["poes"][:-1]) + [(idx, path[:-1] + [(path[-1] + 1) % c.prm.p])]
    return req


@pytest.mark.parametrize("kind", ["outside_the_set", "wrong_sibling"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_a_bad_request_in_the_middle(world, shape, kind):
    """Request 1 with an identifier outside the set (zkt_prove refuses it: ZKT_ERR_NOT_IN_TABLE, and with it the announcement of
    request 2) or with a wrong sibling (bad_paths, not proved): requests 0 and 2 are proved with their usual bytes, verified and
    appended at consecutive indices; request 1 has its code, no proof and no leaf."""
    env = world.env(shape)
    c1 = env.cases[1]
    bad = _outside_the_set(c1) if kind == "outside_the_set" else _wrong_sibling(c1)
    reqs = [env.reqs[0], WC.request_words(env.cv, bad), env.reqs[2]]
    want1 = dict(code=ERR_NOT_IN_TABLE, bad_paths=0, verified=False, new_leaf_index=NONE) if kind == "outside_the_set" else \
        dict(code=ERR_INVALID_ARGUMENT, bad_paths=1 << (c1.inputs - 1), verified=False, new_leaf_index=NONE)
    first = _prefilled(env)
    can_append = (1 << env.height) >= 3          # room is asked for the whole batch up front: a tree of height 1 has none
    for slots in (2, 3):              # request 2 in the next chunk, and announced by request 1's proof
        t = env.tree()
        try:
            proofs, pi, res = env.prove(reqs=reqs, slots=slots, tree=t, append=can_append)
            assert proofs == [env.ref[0], b"", env.ref[2]], slots
            assert res == [dict(code=0, bad_paths=0, verified=True, new_leaf_index=first if can_append else NONE), want1,
                           dict(code=0, bad_paths=0, verified=True, new_leaf_index=first + 1 if can_append else NONE)], slots
            _same_tree(env, t, [env.cases[0].cli_pi[-1], env.cases[2].cli_pi[-1]] if can_append else [], first)
        finally:
            t.close()
    env.plain_proof_still_comes_out()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_identifiers_set_verification_and_append_rules(world, shape):
    """The set, the verification and the append rules at every shape.  Where the tree matters the batch is the whole one if a
    tree of the circuit's height has room for three leaves, else (height 1: two leaves) the first two requests."""
    env = world.env(shape)
    z, cv = env.z, env.cv
    ids = env.cases[0].req["ident_set"]
    # a repeated value is dropped, the first kept
    repeated = K.fr_to_mont(cv, ids[:3] + [ids[1]] + ids[3:] + [ids[0], ids[6]])
    proofs, _, res = env.prove(set_mont=repeated, verify=False)
    assert proofs == env.ref and all(r["code"] == 0 for r in res)
    # more distinct values than the table size the circuit was set up with
    with pytest.raises(z.ZktError) as e:
        env.prove(set_mont=K.fr_to_mont(cv, ids + list(range(1000, 1000 + WC.TABLE_SIZE + 1 - len(ids)))), verify=False)
    assert e.value.code == ERR_INVALID_ARGUMENT and "table size" in str(e.value)
    proofs, _, _ = env.prove(set_mont=K.fr_to_mont(cv, ids + list(range(1000, 1000 + WC.TABLE_SIZE - len(ids)))), verify=False, reqs=env.reqs[:1])
    assert len(proofs[0]) == len(env.ref[0]) and proofs[0] != env.ref[0]      # exactly the table size is taken: another table, another proof
    k = 3 if (1 << env.height) >= 3 else 2
    reqs, ref = env.reqs[:k], env.ref[:k]
    t = env.tree(capacity=min(4, 1 << env.height))          # empty, room for the batch
    try:
        root0 = t.root()
        # a wrong beta h: the pairing check rejects every proof, nothing is appended
        proofs, _, res = env.prove(reqs=reqs, tree=t, append=True, beta_h=env.h)
        assert proofs == ref and res == [dict(code=0, bad_paths=0, verified=False, new_leaf_index=NONE)] * k
        assert t.count == 0 and np.array_equal(t.root(), root0)
        # append = 0 leaves the tree untouched
        proofs, _, res = env.prove(reqs=reqs, tree=t, append=False)
        assert proofs == ref and res == [dict(code=0, bad_paths=0, verified=True, new_leaf_index=NONE)] * k
        assert t.count == 0 and np.array_equal(t.root(), root0)
    finally:
        t.close()
    # a tree without room for the batch is refused before anything is enqueued: maps and tree as they were
    t = env.tree(capacity=k - 1)
    d = env.map(2)
    try:
        with pytest.raises(z.ZktError) as e:
            env.w.prove(reqs, d, 2, env.set_mont, env.blinders[:k], tree=t, verify_key=(env.g, env.h, env.beta_h), append=True)
        assert e.value.code == ERR_INVALID_ARGUMENT and "room" in str(e.value)
        assert (env.ctx.download(d, (2 * env.n_vars, 4)) == np.uint64(SENTINEL)).all()
        assert t.count == 0
        # and a refusal zkt_withdraw_witness would make on the host, for a request of the SECOND chunk, fails the whole call
        zero_secret = dict(env.reqs[2], secrets=np.zeros_like(env.reqs[2]["secrets"]))
        with pytest.raises(z.ZktError) as e:
            env.w.prove(env.reqs[:2] + [zero_secret], d, 2, env.set_mont, env.blinders, append=False)
        assert e.value.code == 6 and (env.ctx.download(d, (2 * env.n_vars, 4)) == np.uint64(SENTINEL)).all()
    finally:
        env.ctx.free(d)
        t.close()
    env.plain_proof_still_comes_out()


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2]], ids=[IDS[0], IDS[2]])
def test_a_circuit_that_withdraw_setup_did_not_make(world, shape):
    """The start of a service over a data directory: the circuit comes from its ProverKey (zkt_circuit_load of the exported
    polynomials), a handle is created beside it, and zkt_withdraw_prove makes the commitments its transcripts are seeded from
    itself (zkt_circuit_commitments).  The same proof bytes, every proof verified; the second call makes nothing again and
    holds no more device memory than the first left; after the SRS is loaded again the commitments are made again; the table
    bound is zkt_prove's n - 1, as nobody told the library the table size."""
    env = world.env(shape)
    z, cv, ctx = env.z, env.cv, env.ctx
    ids = env.cases[0].req["ident_set"]
    world.loaded[cv.name] = None                     # the next test sets its circuit up again
    # the SRS loaded again under the circuit zkt_withdraw_setup made: the kept commitments belong to the old load
    ctx.srs_load(env.srs)
    proofs, _, res = env.prove(settled=False)
    assert proofs == env.ref and all(r["verified"] for r in res)
    # the circuit from its exported key, a fresh handle beside it
    ctx.circuit_load(env.n.bit_length() - 1, ctx.circuit_export())
    w2 = z.WithdrawCircuit(ctx, env.cases[0].words, env.cases[0].inputs, env.height)
    try:
        proofs, pi, res = env.prove(w=w2, settled=False)
        assert proofs == env.ref and all(r["verified"] and r["code"] == 0 for r in res)
        assert [K.fr_from_mont(cv, x) for x in pi] == [c.cli_pi for c in env.cases]
        held = z._lib.debug_live_allocations()
        proofs, _, res = env.prove(w=w2, slots=3)
        assert proofs == env.ref and all(r["verified"] for r in res) and z._lib.debug_live_allocations() == held
        # another key (a second tau) under the same circuit: commitments kept from the first key would seed other transcripts
        # than the verifier's, and nothing would verify
        from zkt_plonk_amd import _lib
        tau2 = TAU + 0x1234567
        ctx.srs_load(K.srs_mont(cv, tau2, env.n + 8))
        h2, beta_h2 = _lib.srs_generate_g2(cv.name, tau2)
        d = env.map(2)
        try:
            other, _, res = w2.prove(env.reqs, d, 2, env.set_mont, env.blinders, verify_key=(ctx.srs_download(0, 1)[0], h2, beta_h2))
        finally:
            ctx.free(d)
        assert all(r["code"] == 0 and r["verified"] for r in res) and all(a != b for a, b in zip(other, env.ref))
        ctx.srs_load(env.srs)
        proofs, _, res = env.prove(w=w2, slots=1, settled=False)
        assert proofs == env.ref and all(r["verified"] for r in res)
        # one value more than the setup's table size is no longer refused here: the bound is n - 1
        proofs, _, res = env.prove(w=w2, reqs=env.reqs[:1], verify=False,
                                   set_mont=K.fr_to_mont(cv, ids + list(range(1000, 1000 + WC.TABLE_SIZE + 1 - len(ids)))))
        assert res[0]["code"] in (0, 9)          # proved, or refused as a proof (the table no longer fits q_table): not as a batch
        with pytest.raises(z.ZktError) as e:
            env.prove(w=w2, reqs=env.reqs[:1], verify=False, set_mont=K.fr_to_mont(cv, list(range(1, env.n + 1))))
        assert e.value.code == ERR_INVALID_ARGUMENT and "table size" in str(e.value)
    finally:
        w2.close()
    env.plain_proof_still_comes_out()
