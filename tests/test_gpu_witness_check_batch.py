"""GPU: zkt_circuit_check_witness_batch against zkt_circuit_check_witness.  The contract is equality: out[w] holds, byte for
byte, what the single call reports for witness w alone, given w's map, its public inputs, its table and the same flags.  The
single call is pinned against the Python restatement of its rules by tests/test_gpu_witness_check.py; here it is the reference,
computed once per distinct witness of a batch.  Where a defect has a known consequence the report is looked at as well, so that
the defects are known to be there."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import fields as F, plonk as P, coracle as K
from helpers import field_elems

import witness_cases as WC
import witness_plan_cases as W

BN, BLS = F.BN254, F.BLS12_381
ERR_INVALID_ARGUMENT, ERR_NOT_LOADED = 1, 10
WIRING = WC.CHECK_WIRING
TILE = 8                                   # CKB_TILE of csrc/check.hip
IDS = lambda v: v.name if hasattr(v, "name") else v


def mont(cv, vals):
    vals = list(vals)
    return K.fr_to_mont(cv, vals) if vals else np.zeros((0, 4), dtype=np.uint64)


class World:
    """Per module: circuits, key polynomials and contexts, each made once."""

    def __init__(self):
        import zkt_plonk_amd as z
        self.z = z
        self.ctx = {cv.name: z.Context(cv.name, 0) for cv in (BN, BLS)}
        self.loaded, self._cs, self._polys = {}, {}, {}

    def close(self):
        for c in self.ctx.values():
            c.close()

    def cs(self, cv, name):
        if (cv.name, name) not in self._cs:
            self._cs[cv.name, name] = (P.synthetic_circuit(cv, 700, 32, seed=4242) if name == "s700"        # n = 2^10: one workgroup
                                       else P.synthetic_circuit(cv, 8000, 32, seed=13))                    # n = 2^13: eight along the rows
        return self._cs[cv.name, name]

    def load(self, cv, name):
        ctx = self.ctx[cv.name]
        if self.loaded.get(cv.name) != name:
            cs = self.cs(cv, name)
            n = cs.circuit_bound()
            if (cv.name, name) not in self._polys:
                be = K.CBackend(cv, K.srs_mont(cv, 3, 2))
                ev = P.setup_evals(be, cs)
                self._polys[cv.name, name] = [mont(cv, be.ifft(n, ev[k])) for k in self.z.PK_ORDER]
            ctx.circuit_load(n.bit_length() - 1, self._polys[cv.name, name])
            self.loaded[cv.name] = name
        return ctx


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.close()


class Witness:
    """one witness of a batch: its map, its public inputs by the batch's positions, its table"""

    def __init__(self, values, pi, table):
        self.values, self.pi, self.table = list(values), list(pi), list(table)


def defects(cs, pos):
    """-> {name: Witness}; pos: the batch's public-input positions: the circuit's own, the last row before the padding and a
    padded row.  The last gate's variables stand on earlier rows too, so that row is broken alone through its public input."""
    p, g_last = cs.p, cs.n_gates - 1
    base = Witness(cs.values, [cs.pi.get(i, 0) for i in pos], cs.table)

    def changed(var=None, delta=1, pi_at=None, table=None):
        w = Witness(base.values, base.pi, base.table if table is None else table)
        if var is not None:
            w.values[var] = (w.values[var] + delta) % p
        if pi_at is not None:
            w.pi[pi_at] = (w.pi[pi_at] + 5) % p
        return w
    lk = WC.lookup_rows(cs)
    looked = cs.value_of(cs.w_o[lk[0]])
    assert cs.w_o[0] != P.ZERO_VAR and cs.w_o[g_last] != P.ZERO_VAR and pos[-1] >= cs.n_gates and looked != 0
    out = {"none": base,
           "row_0": changed(cs.w_o[0]),
           "last_row": changed(pi_at=pos.index(g_last)),
           "last_row_value": changed(cs.w_o[g_last]),
           "wrong_pi": changed(pi_at=1),
           "pi_on_padding": changed(pi_at=len(pos) - 1),
           "outside_table": changed(table=[t for t in cs.table if t != looked]),
           "outside_table_by_value": changed(cs.w_o[lk[0]], delta=0x1234567),
           "several": changed(cs.w_o[g_last], pi_at=0, table=[t for t in cs.table if t != looked])}
    out["several"].values[cs.w_o[0]] = (out["several"].values[cs.w_o[0]] + 9) % p
    return out


class Batch:
    """`batch` witnesses in HBM, witness k = kinds[k % len(kinds)], with the single call's report of each distinct one"""

    def __init__(self, ctx, cv, cs, witnesses, batch, pos, idx=None, pad=3):
        self.ctx, self.cv, self.held = ctx, cv, []
        self.batch, self.pos, self.n_vars, self.stride = batch, list(pos), len(cs.values), len(cs.values) + pad
        self.pick = [witnesses[k % len(witnesses)] for k in range(batch)]
        self.distinct = witnesses
        maps = np.zeros((batch, self.stride, 4), dtype=np.uint64)
        pis = np.zeros((batch, len(pos), 4), dtype=np.uint64)
        cache = {}
        for k, w in enumerate(self.pick):
            if id(w) not in cache:
                cache[id(w)] = (mont(cv, w.values), mont(cv, w.pi))
            maps[k, :self.n_vars], pis[k] = cache[id(w)]
            maps[k, self.n_vars:] = 0xA5A5A5A5 + k                       # the padding up to the stride is never read
        self.pis = pis
        self.d_vars, self.d_pi = self._dev(maps), self._dev(pis)
        self.idx = [np.ascontiguousarray(x, dtype=np.uint32) for x in (idx or WC.indices(cs))]
        self.n_rows = len(self.idx[0])
        self.d_idx = [self._dev(x) for x in self.idx]

    def _dev(self, arr):
        d = self.ctx.alloc(max(32, arr.nbytes))
        if arr.size:
            self.ctx.upload(d, arr)
        self.held.append(d)
        return d

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for d in self.held:
            self.ctx.free(d)

    def tables(self, variant):
        if variant == "none":
            return []
        if variant == "shared":
            return [mont(self.cv, self.pick[0].table)]
        return [mont(self.cv, w.table) for w in self.pick]

    def struct(self, variant="each", host_wiring=False, ctx=None, **over):
        w = self.idx if host_wiring else self.d_idx
        a = dict(d_variables=self.d_vars, stride=self.stride, batch=self.batch, n_vars=self.n_vars, pi_pos=self.pos, d_pi_vals=self.d_pi,
                 tables=self.tables(variant))
        a.update(over)
        return (ctx or self.ctx).witness_batch(a["d_variables"], a["stride"], a["batch"], a["n_vars"], w[0], w[1], w[2], a["pi_pos"],
                                               a["d_pi_vals"], a["tables"], n_rows=None if host_wiring else self.n_rows)

    def single(self, k, flags, variant="each", ctx=None):
        """the single call on witness k where it lies"""
        ctx = ctx or self.ctx
        w = self.pick[k]
        table = [] if variant == "none" else self.pick[0].table if variant == "shared" else w.table
        prep = ctx.prepare_vars_dev(self.d_vars + 32 * self.stride * k, self.n_vars, self.d_idx[0], self.d_idx[1], self.d_idx[2], self.n_rows,
                                    mont(self.cv, table), self.pos, self.pis[k], None)
        return ctx.check_witness(prep, flags)

    def check(self, flags=0, variant="each", host_wiring=False, ctx=None):
        got = (ctx or self.ctx).check_witness_batch(self.struct(variant, host_wiring, ctx), flags)
        assert len(got) == self.batch
        want = {}
        for k, w in enumerate(self.pick):
            if id(w) not in want:
                want[id(w)] = self.single(k, flags, variant, ctx)
            assert got[k].raw == want[id(w)].raw, (k, got[k], want[id(w)])
        return got


def positions(cs):
    return sorted(set(cs.pi) | {cs.n_gates - 1}) + [cs.circuit_bound() - 2]


@pytest.mark.parametrize("cv,name,batch", [(BN, "s8000", 1), (BN, "s8000", TILE - 1), (BN, "s8000", TILE), (BN, "s8000", TILE + 1),
                                           (BN, "s700", W.BATCH_MAX), (BLS, "s700", TILE + 1), (BLS, "s8000", 3)], ids=IDS)
def test_every_report_is_the_single_calls(world, cv, name, batch):
    cs = world.cs(cv, name)
    ctx = world.load(cv, name)
    pos = positions(cs)
    d = defects(cs, pos)
    order = ["row_0", "none", "last_row", "wrong_pi", "pi_on_padding", "outside_table", "several", "outside_table_by_value",
             "last_row_value"]
    with Batch(ctx, cv, cs, [d[k] for k in order], batch, pos) as b:
        got = b.check()
        by = {k: got[order.index(k)] for k in order if order.index(k) < batch}
        assert (by["row_0"].first_arithmetic, by["row_0"].satisfied) == (0, False)
        if batch >= TILE - 1:
            assert by["none"].satisfied
            assert by["last_row"].first_arithmetic == cs.n_gates - 1 and by["last_row"].n_arithmetic == 1
            assert (by["wrong_pi"].n_arithmetic, by["wrong_pi"].first_arithmetic) == (1, pos[1])
            assert (by["pi_on_padding"].n_arithmetic, by["pi_on_padding"].first_arithmetic) == (1, pos[-1]) and pos[-1] >= cs.n_gates
            assert by["outside_table"].n_lookup > 0 and by["outside_table"].n_arithmetic == 0
            assert by["several"].n_lookup > 0 and by["several"].n_arithmetic >= 3 and by["several"].first_arithmetic == 0
            if name == "s8000":                                          # first failing rows in different workgroups of the launch
                stride = 8 * 256
                assert cs.circuit_bound() == 1 << 13
                assert len({(r.first_arithmetic % stride) // 256 for r in got if r.first_arithmetic is not None}) >= 2
        if batch >= TILE:
            assert by["outside_table_by_value"].n_lookup == 1
        if batch > TILE:
            assert by["last_row_value"].n_arithmetic > 1 and 0 < by["last_row_value"].first_arithmetic < cs.n_gates - 1
        b.check(variant="shared")
        b.check(variant="none", host_wiring=True)


def test_wiring_is_checked_once_and_copied(world):
    cv = BN
    cs = world.cs(cv, "s8000")
    ctx = world.load(cv, "s8000")
    pos = positions(cs)
    d = defects(cs, pos)
    ws = [d["none"], d["row_0"], d["outside_table"]]
    with Batch(ctx, cv, cs, ws, 4, pos) as b:
        got = b.check(WIRING)
        assert [r.checked for r in got] == [7] * 4 and got[0].satisfied and all(r.n_wiring == 0 for r in got)
        b.check(WIRING, host_wiring=True)
    idx = [x.copy() for x in WC.indices(cs)]
    idx[0][5], idx[1][9] = idx[1][9], idx[0][5]                          # one swapped wire
    with Batch(ctx, cv, cs, ws, TILE + 1, pos, idx=idx) as b:
        got = b.check(WIRING)
        assert all(r.n_wiring == got[0].n_wiring > 0 and r.first_wiring == got[0].first_wiring and not r.satisfied for r in got)
        assert [r.n_wiring for r in b.check(0)] == [0] * (TILE + 1)


def _raw(z, ctx, st, flags, reports):
    return z.lib().zkt_circuit_check_witness_batch(ctx.handle, ctypes.byref(st.struct) if st is not None else None, flags, reports)


def test_refusals_write_no_report_and_leave_the_context_usable(world):
    from zkt_plonk_amd import _lib
    z, cv = world.z, BN
    cs = world.cs(cv, "s700")
    ctx = world.load(cv, "s700")
    pos = positions(cs)
    d = defects(cs, pos)
    n = cs.circuit_bound()
    reports = (_lib.WitnessReport * 3)()
    ctypes.memset(reports, 0xA5, ctypes.sizeof(reports))
    before = bytes(reports)
    with Batch(ctx, cv, cs, [d["none"], d["row_0"], d["wrong_pi"]], 3, pos) as b:
        two_tables = b.tables("each")[:2]
        bad_idx = [x.copy() for x in b.idx]
        bad_idx[2][3] = b.n_vars
        refused = [b.struct(batch=0), b.struct(batch=W.BATCH_MAX + 1), b.struct(stride=b.n_vars - 1), b.struct(tables=two_tables),
                   b.struct(d_pi_vals=0), b.struct(d_variables=0), b.struct(pi_pos=pos[:-1] + [n]),
                   b.struct(tables=[mont(cv, cs.table + cs.table[3:4])]),                     # a repeated table value
                   b.struct(tables=[mont(cv, list(range(1, n + 1)))]),                        # table_len >= n
                   ctx.witness_batch(b.d_vars, b.stride, 3, b.n_vars, bad_idx[0], bad_idx[1], bad_idx[2], pos, b.d_pi, [])]
        for st in refused:
            for flags in (0, WIRING):
                assert _raw(z, ctx, st, flags, reports) == ERR_INVALID_ARGUMENT
            assert bytes(reports) == before
            b.check()                                                    # a good call on the same context
        good = b.struct()
        for flags in (2, 4, WIRING | 8, -1):
            assert _raw(z, ctx, good, flags, reports) == ERR_INVALID_ARGUMENT
        assert _raw(z, ctx, None, 0, reports) == ERR_INVALID_ARGUMENT and _raw(z, ctx, good, 0, None) == ERR_INVALID_ARGUMENT
        fresh = z.Context(cv.name, 0)
        try:
            assert _raw(z, fresh, good, 0, reports) == ERR_NOT_LOADED
        finally:
            fresh.close()
        assert bytes(reports) == before
        assert _raw(z, ctx, good, WIRING, reports) == 0 and [r.satisfied for r in reports] == [1, 0, 0] and reports[2].checked == 7


def test_on_a_fork_and_repeated(world):
    cv = BN
    cs = world.cs(cv, "s8000")
    ctx = world.load(cv, "s8000")
    pos = positions(cs)
    d = defects(cs, pos)
    with Batch(ctx, cv, cs, [d["several"], d["none"], d["last_row"]], TILE + 2, pos) as b:
        ctx.profile_enable(True)
        first = [r.raw for r in b.check(WIRING)]
        assert ctx.profile_get("check_witness_batch")[0] == 1
        ctx.profile_enable(False)
        assert [r.raw for r in b.check(WIRING)] == first
        fork = ctx.fork()
        try:
            assert [r.raw for r in b.check(WIRING, ctx=fork)] == first
        finally:
            fork.close()


def test_under_a_communicator_locally(world):
    """a context with a communicator whose partner never shows up: the call is local, no collective is reached"""
    from zkt_plonk_amd import parallel as par
    z, cv = world.z, BN
    cs = world.cs(cv, "s700")
    plain = world.load(cv, "s700")
    pos = positions(cs)
    d = defects(cs, pos)
    ctx = z.Context(cv.name, 0)
    comm = par.LocalGroup(2).comm(0)
    try:
        ctx.set_comm(comm)
        ctx.circuit_load(10, world._polys[cv.name, "s700"])
        with Batch(ctx, cv, cs, [d["none"], d["several"], d["wrong_pi"]], TILE + 1, pos) as b:
            got = [r.raw for r in b.check(WIRING)]
        assert comm.calls == 0
        with Batch(plain, cv, cs, [d["none"], d["several"], d["wrong_pi"]], TILE + 1, pos) as b:
            assert [r.raw for r in b.check(WIRING)] == got
    finally:
        ctx.set_comm(None)
        ctx.close()


def test_behind_a_completion_on_the_same_stream(world):
    """complete four withdrawals from their free variables and judge them without a wait in between: the third one's secret is
    wrong, so its root comparison fails; the others are satisfied.  Every withdrawal looks its identifier up in its own set: one
    table each."""
    z, cv = world.z, BN
    cs_list = [W.withdraw("bn254", "synthetic", s) for s in (1, 2, 3, 4)]
    c, tables = cs_list[0][0], [mont(cv, x[2].table) for x in cs_list]
    assert all(W.same_circuit(c, x[0]) for x in cs_list[1:])
    pl = W.plan(c)
    ctx = world.ctx[cv.name]
    be = K.CBackend(cv, K.srs_mont(cv, 3, 2))
    ev = P.setup_evals(be, c.cs)
    ctx.circuit_load(c.log_n, [mont(cv, be.ifft(1 << c.log_n, ev[k])) for k in z.PK_ORDER])
    world.loaded[cv.name] = None
    starts = [W.prefill(c, pl, x[0].values, salt=k + 1) for k, x in enumerate(cs_list)]
    starts[2][W.secret_variable(c, pl)] += 1
    arr = np.stack([mont(cv, s) for s in starts])
    plan = z.WitnessPlan(ctx, c.idx(0), c.idx(1), c.idx(2), c.n_vars, c.pi_pos)
    held = [ctx.alloc(arr.nbytes), ctx.alloc(4 * len(c.pi_pos) * 32)] + [ctx.alloc(4 * c.n_rows) for _ in range(3)]
    try:
        d_vars, d_pi, d_idx = held[0], held[1], held[2:]
        ctx.upload(d_vars, arr)
        for k in range(3):
            ctx.upload(d_idx[k], c.idx(k))
        wb = ctx.witness_batch(d_vars, c.n_vars, 4, c.n_vars, d_idx[0], d_idx[1], d_idx[2], c.pi_pos, d_pi, tables, n_rows=c.n_rows)
        plan.complete_dev(d_vars, c.n_vars, 4, d_pi)
        got = ctx.check_witness_batch(wb, WIRING)                        # no wait, no status call in between
        assert [r.satisfied for r in got] == [True, True, False, True] and got[2].n_arithmetic >= 1 and got[2].n_wiring == 0
        assert plan.status(4) == [(0, None)] * 4
        pis = ctx.download(d_pi, (4, len(c.pi_pos), 4))
        for k in range(4):
            prep = ctx.prepare_vars_dev(d_vars + 32 * c.n_vars * k, c.n_vars, d_idx[0], d_idx[1], d_idx[2], c.n_rows, tables[k],
                                        c.pi_pos, pis[k], None)
            assert ctx.check_witness(prep, WIRING).raw == got[k].raw, k
    finally:
        plan.close()
        for d in held:
            ctx.free(d)


def test_an_announced_proof_keeps_its_bytes(world):
    """Between two proofs, the second announced with zkt_prove_set_next (its early rounds already issued), a batch is checked:
    both proofs' bytes are those of the same sequence without the check."""
    z, cv = world.z, BN
    cs = world.cs(cv, "s700")
    n, tau = cs.circuit_bound(), 0x7E58
    srs = K.srs_mont(cv, tau, n + 8)
    pk, _, vk = P.setup(K.CBackend(cv, srs), [None] * (n + 8), cs, False)
    ctx = world.ctx[cv.name]
    ctx.srs_load(srs)
    ctx.circuit_load(n.bit_length() - 1, [mont(cv, pk.polys[k]) for k in z.PK_ORDER])
    world.loaded[cv.name] = None
    pos = sorted(cs.pi)
    a, b_, c_ = cs.wire_evals(cs.n_gates)

    def prepared(seed):
        return ctx.prepare_host(mont(cv, a), mont(cv, b_), mont(cv, c_), mont(cv, cs.table), pos, mont(cv, [cs.pi[k] for k in pos]),
                                mont(cv, field_elems(cv.fr.p, seed, P.NUM_BLINDERS)))
    preps = [prepared(41), prepared(42)]
    tr = lambda: z.seed_transcript(z.Transcript("merlin", "ZKT Plonk", fr_bits=cv.fr.bits, fq_bytes=8 * cv.fq.limbs64), n, vk.commits)
    d = defects(cs, positions(cs))

    def sequence(with_check):
        first = ctx.prove_prepared(preps[0], tr(), preps[1])
        if with_check:
            with Batch(ctx, cv, cs, [d["several"], d["none"], d["row_0"]], TILE + 1, positions(cs)) as b:
                got = b.check(WIRING)
                assert not got[0].satisfied and got[1].satisfied
        return first, ctx.prove_prepared(preps[1], tr())

    plain = sequence(False)
    assert plain[0] != plain[1]
    assert sequence(True) == plain
