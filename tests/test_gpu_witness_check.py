"""zkt_circuit_check_witness on the device against the plain-Python restatement of its rules (tests/witness_cases.py,
pinned on the CPU by tests/test_witness_cases_oracle.py).  Every comparison is exact: the whole report equals the
restatement's.  Keys are loaded with zkt_circuit_load from the oracle's ProverKey polynomials; no SRS is involved except
where a proof is made."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import fields as F, plonk as P, coracle as K
from helpers import field_elems

import witness_cases as WC

BN, BLS = F.BN254, F.BLS12_381
ERR_INVALID_ARGUMENT, ERR_NOT_IN_TABLE, ERR_QUOTIENT_TOO_SHORT, ERR_NOT_LOADED = 1, 8, 9, 10
WIRING = WC.CHECK_WIRING
NO_FAILURE = dict(satisfied=True, n_arithmetic=0, first_arithmetic=None, residual=0, n_lookup=0, first_lookup=None, n_wiring=0,
                  first_wiring=None)


def _circuit(cv, name):
    if name == "tc":
        return P.test_circuit(cv, size=20)                          # n = 2^5
    if name == "s700":
        return P.synthetic_circuit(cv, 700, 32, seed=4242)          # n = 2^10, padded
    if name == "s1024":
        return P.synthetic_circuit(cv, 1024, 32, seed=1024)         # n = 2^10, no padding row
    return P.synthetic_circuit(cv, 8000, 32, seed=13)               # n = 2^13: several workgroups, the stride loop turns


def mont(cv, vals):
    vals = list(vals)
    return K.fr_to_mont(cv, vals) if vals else np.zeros((0, 4), dtype=np.uint64)


class World:
    """Per module: circuits, key polynomials and contexts, each made once.  A key is (curve, circuit name, variant); the
    variant names a change of the selectors made before the polynomials are taken."""

    def __init__(self):
        import zkt_plonk_amd as z
        self.z = z
        self.ctx = {cv.name: z.Context(cv.name, 0) for cv in (BN, BLS)}
        self.loaded = {}
        self._cs, self._evals, self._polys = {}, {}, {}

    def close(self):
        for c in self.ctx.values():
            c.close()

    def cs(self, cv, name):
        if (cv.name, name) not in self._cs:
            self._cs[cv.name, name] = _circuit(cv, name)
        return self._cs[cv.name, name]

    def backend(self, cv):
        return K.CBackend(cv, K.srs_mont(cv, 3, 2))

    def key_selectors(self, cv, name, variant):
        """The six selector vectors (padded to n) of the key `variant` of circuit `name`."""
        cs = self.cs(cv, name)
        n = cs.circuit_bound()
        sel = {k: list(v) + [0] * (n - cs.n_gates) for k, v in WC.selectors(cs).items()}
        for row, delta in VARIANTS[variant](cs):
            sel["q_c"][row] = (sel["q_c"][row] + delta) % cs.p
        return sel

    def load(self, cv, name, variant="plain"):
        ctx = self.ctx[cv.name]
        if self.loaded.get(cv.name) == (name, variant):
            return ctx
        cs = self.cs(cv, name)
        n = cs.circuit_bound()
        be = self.backend(cv)
        if (cv.name, name) not in self._evals:
            self._evals[cv.name, name] = P.setup_evals(be, cs)         # the vectors setup.rs transforms into the ProverKey
        if (cv.name, name, variant) not in self._polys:
            evals = dict(self._evals[cv.name, name])
            evals.update(self.key_selectors(cv, name, variant))
            self._polys[cv.name, name, variant] = [mont(cv, be.ifft(n, evals[k])) for k in self.z.PK_ORDER]
        ctx.circuit_load(n.bit_length() - 1, self._polys[cv.name, name, variant])
        self.loaded[cv.name] = (name, variant)
        return ctx


# key variants: rows of q_c shifted before the key is made -> [(row, delta)]
VARIANTS = {
    "plain": lambda cs: [],
    "plus_one_and_padding": lambda cs: [(WC.third_kind_rows(cs)[3], 1), (cs.circuit_bound() - 5, 7)],
    "minus_one": lambda cs: [(WC.third_kind_rows(cs)[3], -1)],
}


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.close()


class Forms:
    """The four ways a witness reaches the call: evaluation vectors or variables + wiring, host or device pointers."""

    def __init__(self, ctx, cv, a, b, c, table, pi, values=None, idx=None):
        self.ctx, self.held = ctx, []
        pos = sorted(pi)
        pv = mont(cv, [pi[k] for k in pos])
        tbl = mont(cv, table)
        wires = [mont(cv, x) for x in (a, b, c)]
        rows = wires[0].shape[0]
        self.eval_host = ctx.prepare_host(wires[0], wires[1], wires[2], tbl, pos, pv, None)
        d = [self._dev(x) for x in wires]
        self.eval_dev = ctx.prepare_dev(d[0], d[1], d[2], rows, tbl, pos, pv, None)
        self.vars_host = self.vars_dev = None
        if values is not None:
            vals = mont(cv, values)
            self.vars_host = ctx.prepare_vars(vals, idx[0], idx[1], idx[2], tbl, pos, pv, None)
            dv = self._dev(vals)
            di = [self._dev(np.ascontiguousarray(x, dtype=np.uint32)) for x in idx]
            self.vars_dev = ctx.prepare_vars_dev(dv, vals.shape[0], di[0], di[1], di[2], len(idx[0]), tbl, pos, pv, None)

    @classmethod
    def of(cls, ctx, cv, cs):
        a, b, c = cs.wire_evals(cs.n_gates)
        return cls(ctx, cv, a, b, c, cs.table, cs.pi, cs.values, WC.indices(cs))

    def _dev(self, arr):
        d = self.ctx.alloc(max(16, arr.nbytes))
        if arr.size:
            self.ctx.upload(d, arr)
        self.held.append(d)
        return d

    def all(self):
        return [f for f in (self.eval_host, self.eval_dev, self.vars_host, self.vars_dev) if f is not None]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for d in self.held:
            self.ctx.free(d)


def as_dict(cv, got):
    """a WitnessCheck in the restatement's terms (the residual back from Montgomery limbs)"""
    return dict(satisfied=got.satisfied, checked=got.checked, n_arithmetic=got.n_arithmetic, first_arithmetic=got.first_arithmetic,
                residual=K.fr_from_mont(cv, got.residual.reshape(1, 4))[0], n_lookup=got.n_lookup, first_lookup=got.first_lookup,
                n_wiring=got.n_wiring, first_wiring=got.first_wiring)


def check_forms(ctx, cv, forms, want, flags=0, which=None):
    reports = [ctx.check_witness(f, flags) for f in (which or forms.all())]
    for r in reports:
        assert as_dict(cv, r) == want
        assert r.raw == reports[0].raw
    return reports


def check_cs(world, cv, name, wit, variant="plain", flags=0):
    """The witness held by `wit` against key `variant` of circuit `name`, through all four forms (the two variables
    forms when the wiring is checked); -> the expected report."""
    ctx = world.load(cv, name, variant)
    base = world.cs(cv, name)
    a, b, c = wit.wire_evals(wit.n_gates)
    want = WC.expected_report(cv.fr.p, base.circuit_bound(), world.key_selectors(cv, name, variant), a, b, c, wit.table, wit.pi,
                              WC.indices(base) if flags & WIRING else None, WC.indices(wit) if flags & WIRING else None)
    with Forms.of(ctx, cv, wit) as f:
        check_forms(ctx, cv, f, want, flags, [f.vars_host, f.vars_dev] if flags & WIRING else None)
    return want


SIZES_BN = [(BN, "tc"), (BN, "s700"), (BN, "s1024"), (BN, "s8000")]
IDS = lambda v: v.name if hasattr(v, "name") else v


# ---- 1. satisfied ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cv,name", SIZES_BN + [(BLS, "s700")], ids=IDS)
def test_satisfied_witness_in_all_four_forms(cv, name, world):
    cs = world.cs(cv, name)
    assert cs.circuit_bound() == {"tc": 1 << 5, "s700": 1 << 10, "s1024": 1 << 10, "s8000": 1 << 13}[name]
    assert check_cs(world, cv, name, cs) == dict(NO_FAILURE, checked=3)
    assert any(int(x) == 0xFFFFFFFF for col in WC.indices(cs) for x in col)        # the wiring holds Variable::Zero entries
    assert check_cs(world, cv, name, cs, flags=WIRING) == dict(NO_FAILURE, checked=7)


# ---- 2. one variable's value changed --------------------------------------------------------------------------------
@pytest.mark.parametrize("cv,name", [(BN, "tc"), (BN, "s700"), (BN, "s8000"), (BLS, "s700")], ids=IDS)
def test_one_changed_value_breaks_several_rows(cv, name, world):
    cs = world.cs(cv, name)
    uses = {}
    for col in (cs.w_l, cs.w_r, cs.w_o):
        for g, v in enumerate(col):
            uses.setdefault(v, set()).add(g)
    var = max((v for v in uses if v != P.ZERO_VAR), key=lambda v: len(uses[v]))
    want = check_cs(world, cv, name, WC.with_value(cs, var, cs.values[var] + 3))
    assert want["n_arithmetic"] > 1 and want["first_arithmetic"] == min(uses[var]) and want["residual"] != 0


# ---- 3. / 4. failures at the edges, residuals of exactly 1 and p - 1 ------------------------------------------------
@pytest.mark.parametrize("name,row", [("s700", "first"), ("s700", "last_gate"), ("s1024", "last_gate"), ("s8000", "last_gate"),
                                      ("tc", "first")])
def test_single_failing_row_at_an_edge(name, row, world):
    """One row alone, through the evaluation form: its output value is off by one, so the equation gives q_o = -1."""
    cv = BN
    cs = world.cs(cv, name)
    ctx = world.load(cv, name)
    n = cs.circuit_bound()
    g = 0 if row == "first" else cs.n_gates - 1
    if name == "s1024":
        assert g == n - 1
    assert cs.q_o[g] == cv.fr.p - 1 and not cs.q_lookup[g]
    a, b, c = cs.wire_evals(cs.n_gates)
    c[g] = (c[g] + 1) % cv.fr.p
    want = WC.expected_report(cv.fr.p, n, WC.selectors(cs), a, b, c, cs.table, cs.pi)
    assert (want["n_arithmetic"], want["first_arithmetic"], want["residual"], want["n_lookup"]) == (1, g, cv.fr.p - 1, 0)
    with Forms(ctx, cv, a, b, c, cs.table, cs.pi) as f:
        check_forms(ctx, cv, f, want)


@pytest.mark.parametrize("cv,variant", [(BN, "plus_one_and_padding"), (BN, "minus_one"), (BLS, "minus_one")], ids=IDS)
def test_residuals_of_one_and_p_minus_one_and_a_padding_row(cv, variant, world):
    """q_c shifted by +-1 in the key at a row whose terms are all large: the sum there is 1 or p - 1, while every other
    such row still sums to a multiple of p and passes.  "plus_one_and_padding" also carries q_c = 7 in a padding row,
    where every wire is zero."""
    cs = world.cs(cv, "s700")
    rows = WC.third_kind_rows(cs)
    assert len(rows) > 100
    want = check_cs(world, cv, "s700", cs, variant)
    pad = variant == "plus_one_and_padding"
    assert (want["n_arithmetic"], want["first_arithmetic"], want["n_lookup"]) == (2 if pad else 1, rows[3], 0)
    assert want["residual"] == (1 if pad else cv.fr.p - 1)
    assert cs.circuit_bound() - 5 >= cs.n_gates


# ---- 5. random witness ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tc", "s700", "s8000"])
def test_random_witness_fails_nearly_everywhere(name, world):
    cs = world.cs(BN, name)
    want = check_cs(world, BN, name, WC.with_random_values(cs, 0xBAD))
    assert want["first_arithmetic"] == 0 and want["n_arithmetic"] >= cs.n_gates * 9 // 10
    assert want["n_lookup"] == len(WC.lookup_rows(cs)) and want["first_lookup"] == WC.lookup_rows(cs)[0]


# ---- 6. public inputs -----------------------------------------------------------------------------------------------
def test_wrong_and_moved_public_inputs(world):
    cv = BN
    cs = world.cs(cv, "s700")
    rows = sorted(cs.pi)
    want = check_cs(world, cv, "s700", WC.with_pi_value(cs, rows[2], cs.pi[rows[2]] + 5))
    assert (want["n_arithmetic"], want["first_arithmetic"], want["residual"]) == (1, rows[2], 5)
    free = next(g for g in range(100, cs.n_gates) if g not in cs.pi)
    want = check_cs(world, cv, "s700", WC.with_pi_moved(cs, rows[0], free))
    assert (want["n_arithmetic"], want["first_arithmetic"], want["residual"]) == (2, free, cs.pi[rows[0]])


# ---- 7. lookup ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cv", [BN, BLS], ids=IDS)
def test_value_removed_from_the_table(cv, world):
    cs = world.cs(cv, "s700")
    looked = [cs.value_of(cs.w_o[g]) for g in WC.lookup_rows(cs)]
    used = max(set(looked), key=looked.count)
    want = check_cs(world, cv, "s700", WC.with_table(cs, [t for t in cs.table if t != used]))
    hit = [g for g, v in zip(WC.lookup_rows(cs), looked) if v == used]
    assert want["n_arithmetic"] == 0 and (want["n_lookup"], want["first_lookup"]) == (len(hit), hit[0]) and len(hit) > 1


def test_tables_of_other_shapes(world):
    cv = BN
    cs = world.cs(cv, "s700")
    lk = WC.lookup_rows(cs)
    assert check_cs(world, cv, "s700", WC.with_table(cs, cs.table[::-1])) == dict(NO_FAILURE, checked=3)
    shuffled = list(cs.table)
    np.random.default_rng(5).shuffle(shuffled)
    assert check_cs(world, cv, "s700", WC.with_table(cs, shuffled)) == dict(NO_FAILURE, checked=3)
    only = cs.value_of(cs.w_o[lk[0]])
    one = check_cs(world, cv, "s700", WC.with_table(cs, [only]))                   # a table of length 1
    keep = [g for g in lk if cs.value_of(cs.w_o[g]) == only]
    assert one["n_lookup"] == len(lk) - len(keep) and 0 < len(keep) < len(lk)
    assert one["first_lookup"] == next(g for g in lk if g not in keep)
    none = check_cs(world, cv, "s700", WC.with_table(cs, []))
    assert (none["n_lookup"], none["first_lookup"], none["n_arithmetic"]) == (len(lk), lk[0], 0)


def test_looked_up_zero_passes_without_a_zero_in_the_table(world):
    cv = BN
    cs = world.cs(cv, "s700")
    ctx = world.load(cv, "s700")
    assert 0 not in cs.table
    g = WC.lookup_rows(cs)[2]
    a, b, c = cs.wire_evals(cs.n_gates)
    a[g] = c[g] = 0                                    # the row a - c = 0 still holds; it now looks up zero
    want = WC.expected_report(cv.fr.p, cs.circuit_bound(), WC.selectors(cs), a, b, c, cs.table, cs.pi)
    assert want == dict(NO_FAILURE, checked=3)
    with Forms(ctx, cv, a, b, c, cs.table, cs.pi) as f:
        check_forms(ctx, cv, f, want)
    with Forms(ctx, cv, a, b, c, [], cs.pi) as f:       # and with no table at all only that row passes
        check_forms(ctx, cv, f, WC.expected_report(cv.fr.p, cs.circuit_bound(), WC.selectors(cs), a, b, c, [], cs.pi))


# ---- 8. wiring ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tc", "s700", "s8000"])
def test_index_swapped_for_a_variable_of_equal_value(name, world):
    cv = BN
    cs = world.cs(cv, name)
    swapped, row = WC.with_equal_value_swap(cs)
    assert check_cs(world, cv, name, swapped) == dict(NO_FAILURE, checked=3)        # gates and lookups cannot see it
    want = check_cs(world, cv, name, swapped, flags=WIRING)
    assert want["n_arithmetic"] == 0 and want["n_lookup"] == 0 and not want["satisfied"]
    assert want["n_wiring"] > 1 and want["first_wiring"][1] <= row                 # the predecessors in both cycles


def test_wiring_check_needs_the_variables_form(world):
    cv = BN
    cs = world.cs(cv, "s700")
    ctx = world.load(cv, "s700")
    with Forms.of(ctx, cv, cs) as f:
        for prep in (f.eval_host, f.eval_dev):
            with pytest.raises(world.z.ZktError) as e:
                ctx.check_witness(prep, WIRING)
            assert e.value.code == ERR_INVALID_ARGUMENT


# ---- 9. errors and independence -------------------------------------------------------------------------------------
def _raw_call(z, ctx, prep, flags, report):
    return z.lib().zkt_circuit_check_witness(ctx.handle, ctypes.byref(prep.struct) if prep is not None else None, flags,
                                             ctypes.byref(report) if report is not None else None)


def test_errors_leave_the_report_alone(world):
    from zkt_plonk_amd import _lib
    z, cv = world.z, BN
    cs = world.cs(cv, "s700")
    n = cs.circuit_bound()
    marked = _lib.WitnessReport()
    ctypes.memset(ctypes.byref(marked), 0xA5, ctypes.sizeof(marked))
    before = bytes(marked)

    fresh = z.Context(cv.name, 0)
    try:
        with Forms.of(fresh, cv, cs) as f:
            assert _raw_call(z, fresh, f.eval_host, 0, marked) == ERR_NOT_LOADED and bytes(marked) == before
    finally:
        fresh.close()

    ctx = world.load(cv, "s700")
    with Forms.of(ctx, cv, cs) as f:
        assert _raw_call(z, ctx, f.eval_host, 0, None) == ERR_INVALID_ARGUMENT
        assert _raw_call(z, ctx, None, 0, marked) == ERR_INVALID_ARGUMENT
        for flags in (2, 4, WIRING | 8, -1):
            assert _raw_call(z, ctx, f.vars_host, flags, marked) == ERR_INVALID_ARGUMENT
        assert bytes(marked) == before
    idx = WC.indices(cs)
    a, b, c = cs.wire_evals(cs.n_gates)
    for col in range(3):                                  # an index one past the map, in each column, host and device
        bad = [x.copy() for x in idx]
        bad[col][cs.n_gates - 1 - col] = len(cs.values)
        with Forms(ctx, cv, a, b, c, cs.table, cs.pi, cs.values, bad) as f:
            for prep in (f.vars_host, f.vars_dev):
                for flags in (0, WIRING):
                    assert _raw_call(z, ctx, prep, flags, marked) == ERR_INVALID_ARGUMENT
                    assert "ZKT_VARIABLE_ZERO" in z.lib().zkt_last_error(ctx.handle).decode()
    long_rows = [0] * (n + 1)
    with Forms(ctx, cv, long_rows, long_rows, long_rows, cs.table, cs.pi) as f:           # n_rows > n
        assert _raw_call(z, ctx, f.eval_host, 0, marked) == ERR_INVALID_ARGUMENT
        assert _raw_call(z, ctx, f.eval_dev, 0, marked) == ERR_INVALID_ARGUMENT
    with Forms(ctx, cv, a, b, c, list(range(1, n + 1)), cs.pi) as f:                      # table_len >= n
        assert _raw_call(z, ctx, f.eval_host, 0, marked) == ERR_INVALID_ARGUMENT
    with Forms(ctx, cv, a, b, c, cs.table + cs.table[3:4], cs.pi) as f:                   # a repeated table value
        assert _raw_call(z, ctx, f.eval_host, 0, marked) == ERR_INVALID_ARGUMENT
    with Forms(ctx, cv, a, b, c, cs.table, {n: 1}) as f:                                  # a public input beyond the domain
        assert _raw_call(z, ctx, f.eval_host, 0, marked) == ERR_INVALID_ARGUMENT
    assert bytes(marked) == before
    with Forms.of(ctx, cv, cs) as f:                                                      # and the context still checks
        assert _raw_call(z, ctx, f.vars_dev, WIRING, marked) == 0 and marked.satisfied == 1 and marked.checked == 7


def test_same_report_every_time_and_on_a_fork(world):
    cv = BN
    cs = world.cs(cv, "s8000")
    ctx = world.load(cv, "s8000")
    bad = WC.with_random_values(WC.with_equal_value_swap(cs)[0], 7)
    want = WC.report_of_cs(bad, cs, wiring=True)
    assert want["n_arithmetic"] and want["n_lookup"] and want["n_wiring"]
    ctx.profile_enable(True)
    with Forms.of(ctx, cv, bad) as f:
        first = check_forms(ctx, cv, f, want, WIRING, [f.vars_dev, f.vars_host, f.vars_dev])[0]
    assert ctx.profile_get("check_witness")[0] == 3
    ctx.profile_enable(False)
    fork = ctx.fork()
    try:
        with Forms.of(fork, cv, bad) as f:
            assert check_forms(fork, cv, f, want, WIRING, [f.vars_dev, f.vars_host])[0].raw == first.raw
    finally:
        fork.close()


@pytest.fixture(scope="module")
def proving(world):
    """s700 on BN254 with an SRS: the oracle's setup (VerifierKey for the transcripts) and the loaded prover"""
    cv = BN
    cs = world.cs(cv, "s700")
    n = cs.circuit_bound()
    tau = 0x7E57
    srs = K.srs_mont(cv, tau, n + 8)
    pk, _, vk = P.setup(K.CBackend(cv, srs), [None] * (n + 8), cs, False)
    return dict(cs=cs, n=n, tau=tau, srs=srs, vk=vk, pk=[mont(cv, pk.polys[k]) for k in world.z.PK_ORDER])


def _transcript(z, cv, s):
    tr = z.Transcript("merlin", "ZKT Plonk", fr_bits=cv.fr.bits, fq_bytes=8 * cv.fq.limbs64)
    return z.seed_transcript(tr, s["n"], s["vk"].commits)


def _prepare(ctx, cv, cs, blinders):
    a, b, c = cs.wire_evals(cs.n_gates)
    pos = sorted(cs.pi)
    return ctx.prepare_host(mont(cv, a), mont(cv, b), mont(cv, c), mont(cv, cs.table), pos, mont(cv, [cs.pi[k] for k in pos]),
                            mont(cv, blinders))


def test_check_between_two_proofs_changes_neither(world, proving):
    """Between two proofs, the second announced with zkt_prove_set_next (its early rounds already issued), a bad witness
    is checked: both proofs' bytes are those of the same sequence without the check."""
    z, cv, s = world.z, BN, proving
    cs = s["cs"]
    ctx = world.ctx[cv.name]
    ctx.srs_load(s["srs"])
    ctx.circuit_load(s["n"].bit_length() - 1, s["pk"])
    world.loaded[cv.name] = None
    preps = [_prepare(ctx, cv, cs, field_elems(cv.fr.p, seed, P.NUM_BLINDERS)) for seed in (31, 32)]
    bad = WC.with_random_values(cs, 21)
    want = WC.report_of_cs(bad, cs, wiring=True)

    def sequence(with_check):
        first = ctx.prove_prepared(preps[0], _transcript(z, cv, s), preps[1])
        if with_check:
            with Forms.of(ctx, cv, bad) as f:
                check_forms(ctx, cv, f, want, WIRING, [f.vars_host, f.vars_dev])
                check_forms(ctx, cv, f, dict(want, checked=3, n_wiring=0, first_wiring=None), 0)
        return first, ctx.prove_prepared(preps[1], _transcript(z, cv, s))

    plain = sequence(False)
    assert plain[0] != plain[1] and len(plain[0]) == 802
    assert sequence(True) == plain


def test_the_check_and_the_prover_agree(world, proving):
    """What the check calls unsatisfied the prover refuses (ZKT_ERR_QUOTIENT_TOO_SHORT for a gate, ZKT_ERR_NOT_IN_TABLE
    for a lookup); what it calls satisfied proves and verifies."""
    z, cv, s = world.z, BN, proving
    cs = s["cs"]
    ctx = world.ctx[cv.name]
    ctx.srs_load(s["srs"])
    ctx.circuit_load(s["n"].bit_length() - 1, s["pk"])
    world.loaded[cv.name] = None
    blinders = field_elems(cv.fr.p, 33, P.NUM_BLINDERS)
    g = WC.third_kind_rows(cs)[5]
    used = cs.value_of(cs.w_o[WC.lookup_rows(cs)[0]])
    cases = [(cs, None), (WC.with_value(cs, cs.w_o[g], cs.values[cs.w_o[g]] + 1), ERR_QUOTIENT_TOO_SHORT),
             (WC.with_table(cs, [t for t in cs.table if t != used]), ERR_NOT_IN_TABLE)]
    for wit, code in cases:
        prep = _prepare(ctx, cv, wit, blinders)
        rep = ctx.check_witness(prep)
        assert as_dict(cv, rep) == WC.report_of_cs(wit, cs)
        if code is None:
            assert rep.satisfied
            proof = ctx.prove_prepared(prep, _transcript(z, cv, s))
            pis = [cs.pi[k] for k in sorted(cs.pi)]
            assert P.verify(cv, s["tau"], s["vk"], P.proof_deserialize(cv, proof), P.new_seeded_transcript(cv, s["vk"]), pis)
        else:
            assert not rep.satisfied and (rep.n_arithmetic > 0) == (code == ERR_QUOTIENT_TOO_SHORT)
            assert (rep.n_lookup > 0) == (code == ERR_NOT_IN_TABLE)
            with pytest.raises(z.ZktError) as e:
                ctx.prove_prepared(prep, _transcript(z, cv, s))
            assert e.value.code == code
