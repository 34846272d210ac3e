"""Forks of forks (zkt_ctx_fork, include/zkt_plonk.h): the tables several contexts read belong to none of them, so the
contexts of a chain root -> A -> B are destroyed in any order, the middle one first included, and the survivors go on
proving the oracle's bytes over the same tables; a context refuses to reload its key or circuit exactly while a context
forked from it reads them; and nothing is left allocated when the last context is gone (zkt_debug_live_allocations, which,
unlike the card's free memory, does not depend on other processes).

Two circuit bounds on both curves: n = 2048, the smallest at which the n-point class transforms are multi-pass plans, and
n = 16 (single-workgroup transforms); keys of n + 8 powers.  The root takes the quotient on classes and eliminates wire
variables wherever a table can be built, set before any fork, so every table group exists and is inherited.  The witness
lives on a context of its own, which no case closes before the end.  Every comparison is proof bytes against the oracle's."""
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import fields as F, plonk as P, coracle as K
from helpers import field_elems
import wire_elim_cases as W
from test_gpu_quotient_classes import SHAPE

CURVES = [F.BN254, F.BLS12_381]
BIG, SMALL = 2048, 16
# the order in which the three contexts of a chain are destroyed: the middle one first, the root first, the leaf first
ORDERS = [("A", "root", "B"), ("root", "A", "B"), ("B", "A", "root")]


def _mont(cv, v):
    return K.fr_to_mont(cv, v) if len(v) else np.zeros((0, 4), dtype=np.uint64)


def _make_fixture(cv, n):
    """The circuit, its oracle setup under n + 8 powers, two oracle proofs (two blinder sets: an announced successor has
    to differ), and everything the device is handed, in Montgomery words."""
    s = SHAPE[n]
    cs = P.synthetic_circuit(cv, s["gates"], s["table"], seed=n, n_public=s["n_public"], lookup_every=s["lookup_every"])
    assert cs.check_satisfied() and cs.circuit_bound() == n and cs.table and cs.pi
    srs = K.srs_mont(cv, 0xF0F0 + n, n + 8)
    be = K.CBackend(cv, srs)
    pk, epk, vk = P.setup(be, [None] * (n + 8), cs, True)
    blinders = [field_elems(cv.fr.p, 0xF02C + k, P.NUM_BLINDERS) for k in range(2)]
    want = [P.prove(be, [None] * (n + 8), pk, epk, vk, cs, P.new_seeded_transcript(cv, vk), b).serialize(cv) for b in blinders]
    assert want[0] != want[1]
    pi_pos = sorted(cs.pi)
    return types.SimpleNamespace(
        cv=cv, n=n, log_n=n.bit_length() - 1, cs=cs, srs=srs, vk=vk, want=want, pkm={k: _mont(cv, pk.polys[k]) for k in pk.polys},
        values=_mont(cv, cs.values), idx=[W.to_idx(w) for w in (cs.w_l, cs.w_r, cs.w_o)], table=_mont(cv, cs.table),
        pi_pos=pi_pos, pi_vals=_mont(cv, [cs.pi[k] for k in pi_pos]), blinders_mont=[_mont(cv, b) for b in blinders])


@pytest.fixture(scope="module")
def fx():
    made = {}

    def get(cv, n):
        if (cv.name, n) not in made:
            made[cv.name, n] = _make_fixture(cv, n)
        return made[cv.name, n]

    return get


def _live():
    from zkt_plonk_amd import _lib
    return _lib.debug_live_allocations()


class Rig:
    """The witnesses of one case on a context of their own, and the legs every case is made of."""

    def __init__(self, z, cv):
        self.z, self.cv = z, cv
        self.data = z.Context(cv.name, 0)
        self.dev = {}

    def witness(self, f):
        """f's variable map and index vectors in HBM -> its two prepared inputs"""
        d = self.data
        d_vars = d.alloc(f.values.nbytes)
        d.upload(d_vars, f.values)
        d_idx = []
        for w in f.idx:
            d_idx.append(d.alloc(w.nbytes))
            d.upload(d_idx[-1], w)
        self.dev[f.n] = [d.prepare_vars_dev(d_vars, f.values.shape[0], d_idx[0], d_idx[1], d_idx[2], f.cs.n_gates, f.table, f.pi_pos,
                                            f.pi_vals, b) for b in f.blinders_mont]

    def root(self, f):
        """a context with f's key and circuit on the routes that make every table group"""
        ctx = self.z.Context(self.cv.name, 0)
        ctx.set_quotient_route(1)
        ctx.set_wire_elimination(2)
        self.load(ctx, f)
        return ctx

    def load(self, ctx, f):
        ctx.srs_load(f.srs)
        self.z.GpuProver(ctx, f.log_n, f.pkm)

    def tr(self, f):
        z, cv = self.z, self.cv
        return z.seed_transcript(z.Transcript("merlin", "ZKT Plonk", fr_bits=cv.fr.bits, fq_bytes=cv.fq.limbs64 * 8), f.vk.n, f.vk.commits)

    def prove(self, ctx, f, what):
        """one proof -> the dense MSMs it took (profile scope msm_accumulate)"""
        ctx.profile_enable(1)
        got = ctx.prove_prepared(self.dev[f.n][0], self.tr(f))
        dense = ctx.profile_get("msm_accumulate")[0]
        ctx.profile_enable(0)
        assert got == f.want[0], what
        assert ctx.debug_quotient_top()[1], (what, "the proof did not take the classes route")
        return dense

    def chained(self, ctx, f, what):
        """two different proofs, the second announced by the first"""
        dev = self.dev[f.n]
        assert ctx.prove_prepared(dev[0], self.tr(f), dev[1]) == f.want[0], (what, "announcing proof")
        assert ctx.prove_prepared(dev[1], self.tr(f)) == f.want[1], (what, "announced proof")
        assert ctx.debug_quotient_top()[1], what

    def reads_the_sources_tables(self, src, fork, f, dense, what):
        """`fork` was made from `src` when src's tables existed: the same tables, the same wire routes"""
        assert fork.lagrange_info() == src.lagrange_info() and fork.lagrange_info()["log_n"] == f.log_n, what
        assert fork.msm_info() == src.msm_info(), what
        assert self.prove(fork, f, what) == dense, (what, "dense MSMs of a proof: other wire routes than the source's")

    def refuses_reload(self, ctx, f, what):
        z = self.z
        before = ctx.lagrange_info(), ctx.msm_info()
        with pytest.raises(z.ZktError):
            ctx.srs_load(f.srs)
        with pytest.raises(z.ZktError):
            z.GpuProver(ctx, f.log_n, f.pkm)
        assert (ctx.lagrange_info(), ctx.msm_info()) == before, (what, "a refused reload changed the context")

    def close_in(self, order, ctxs, after_close, reload=None):
        """destroys the chain in `order`; after every step the survivors prove: after_close[name](context).  When the leaf
        goes first, the middle context then reloads its key and circuit (nobody reads its tables any more)."""
        alive = dict(ctxs)
        for name in order:
            alive.pop(name).close()
            if name == "B" and "A" in alive and reload is not None:
                self.load(alive["A"], reload)
            for other, c in alive.items():
                after_close[other](c, "%s after %s closed (order %s)" % (other, name, " ".join(order)))


def _case(z, cv, body):
    """`body(rig)` between two readings of the live device allocations"""
    before = _live()
    rig = Rig(z, cv)
    try:
        body(rig)
    finally:
        rig.data.close()
    assert _live() == before, "device allocations (count, bytes) left behind"


@pytest.mark.parametrize("order", ORDERS, ids=["-".join(o) for o in ORDERS])
@pytest.mark.parametrize("cv", CURVES, ids=lambda c: c.name)
def test_middle_fork_owns_its_tables(cv, order, fx):
    """A is forked before the root's first proof: its proof builds a Lagrange table, class tables, wire tables and plans of
    its own, over the root's key table and circuit keys.  B, forked from A, reads all of them."""
    import zkt_plonk_amd as z
    f = fx(cv, BIG)

    def body(rig):
        rig.witness(f)
        ctxs = {}
        try:
            root = ctxs["root"] = rig.root(f)
            A = ctxs["A"] = root.fork()
            assert A.lagrange_info()["log_n"] == -1             # nothing to inherit yet
            dense = rig.prove(A, f, "A")
            B = ctxs["B"] = A.fork()
            rig.refuses_reload(A, f, "A while B reads its tables")
            rig.refuses_reload(root, f, "root while A and B read its key table and circuit keys")
            rig.reads_the_sources_tables(A, B, f, dense, "B")
            assert root.lagrange_info()["log_n"] == -1          # the root has still built nothing: B's tables are A's
            both = lambda c, what: rig.chained(c, f, what)
            rig.close_in(order, ctxs, dict(root=both, A=both, B=both), reload=f)
        finally:
            for c in ctxs.values():
                c.close()

    _case(z, cv, body)


@pytest.mark.parametrize("order", ORDERS, ids=["-".join(o) for o in ORDERS])
@pytest.mark.parametrize("cv", CURVES, ids=lambda c: c.name)
def test_middle_fork_reads_the_roots_tables(cv, order, fx):
    """The root proves first, so A inherits every table and B inherits them from A: all three read the root's."""
    import zkt_plonk_amd as z
    f = fx(cv, BIG)

    def body(rig):
        rig.witness(f)
        ctxs = {}
        try:
            root = ctxs["root"] = rig.root(f)
            dense = rig.prove(root, f, "root")
            A = ctxs["A"] = root.fork()
            B = ctxs["B"] = A.fork()
            rig.refuses_reload(A, f, "A while B reads through it")
            rig.refuses_reload(root, f, "root while A and B read its tables")
            rig.reads_the_sources_tables(A, B, f, dense, "B")
            both = lambda c, what: rig.chained(c, f, what)
            rig.close_in(order, ctxs, dict(root=both, A=both, B=both), reload=f)
        finally:
            for c in ctxs.values():
                c.close()

    _case(z, cv, body)


@pytest.mark.parametrize("order", ORDERS, ids=["-".join(o) for o in ORDERS])
@pytest.mark.parametrize("cv", CURVES, ids=lambda c: c.name)
def test_middle_fork_with_a_key_and_circuit_of_its_own(cv, order, fx):
    """A loads the n = 16 key and circuit while the root keeps n = 2048 (a fork may: it stops sharing those parts).  B,
    forked from A, proves the n = 16 proof on A's tables whether or not A is still there; the root goes on at n = 2048."""
    import zkt_plonk_amd as z
    big, small = fx(cv, BIG), fx(cv, SMALL)

    def body(rig):
        rig.witness(big)
        rig.witness(small)
        ctxs = {}
        try:
            root = ctxs["root"] = rig.root(big)
            rig.prove(root, big, "root")
            A = ctxs["A"] = root.fork()
            rig.load(A, small)                                   # not refused: nobody reads through A
            rig.load(root, big)                                  # nor is the root, whose only fork has let go of everything
            rig.prove(root, big, "root, reloaded")
            dense = rig.prove(A, small, "A")
            B = ctxs["B"] = A.fork()
            rig.refuses_reload(A, small, "A while B reads its tables")
            rig.reads_the_sources_tables(A, B, small, dense, "B")
            on_small = lambda c, what: rig.chained(c, small, what)
            on_big = lambda c, what: rig.chained(c, big, what)
            rig.close_in(order, ctxs, dict(root=on_big, A=on_small, B=on_small), reload=small)
        finally:
            for c in ctxs.values():
                c.close()

    _case(z, cv, body)
