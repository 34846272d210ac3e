"""The fused streaming passes of rounds 3 and 5 and of the blinding (zkt_ctx_set_fused_passes, include/zkt_plonk.h) against
the launch sequence they replace (mode 2) and the CPU oracle, through the C ABI: the same proof bytes, the same refusals,
the same grand products and commitments.  Sizes: n + 8 coefficients straddle the 512-element workgroup of the division at
n = 512, the 1024-element scan block at n = 1024 and make a second level of block totals' prefixes at n = 2048; n = 8 and 16
are single workgroups everywhere, with blinders and slack filling most of a polynomial."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import fields as F, plonk as P, coracle as K
from helpers import field_elems

import forced_challenges as FC
import ntt_cases
import test_gpu_quotient_classes as QC
from test_gpu_lagrange import _oracle_commit

CURVES = [F.BN254, F.BLS12_381]
SIZES = [8, 16, 512, 1024, 2048]
SHAPE = {8: dict(gates=7, table=4, n_public=1, lookup_every=3), 16: dict(gates=14, table=8, n_public=2, lookup_every=5),
         512: dict(gates=500, table=32, n_public=5, lookup_every=16), 1024: dict(gates=1000, table=32, n_public=7, lookup_every=16),
         2048: dict(gates=2000, table=64, n_public=20, lookup_every=16), 4096: dict(gates=4000, table=64, n_public=3, lookup_every=16)}
FUSED, STEPWISE = 1, 2
CLASSES, WHOLE = 1, 2


def _synthetic(cv, n, value_seed):
    s = SHAPE[n]
    cs = P.synthetic_circuit(cv, s["gates"], s["table"], seed=n, n_public=s["n_public"], lookup_every=s["lookup_every"],
                             value_seed=value_seed)
    assert cs.check_satisfied() and cs.circuit_bound() == n
    return cs


def _short_selectors(cv, n):
    """Every one of the n rows is a gate with q_o = -1 and q_c = 5: those two key polynomials are constants (one coefficient,
    far below n), q_m and q_r are zero (no coefficient at all).  Lookups and a public input are among the rows."""
    table = [3 + 7 * i for i in range(4)]
    cs = P.ConstraintSystem(cv, table, 4)
    x = cs.assign_variable(11)
    while cs.n_gates < n - 1:
        g = cs.n_gates
        if g % 4 == 3:
            t = table[g % len(table)]
            cs.arith_constrain(cs.assign_variable(t - 5), P.ZERO_VAR, cs.assign_variable(t), q_l=1, q_o=-1, q_c=5, q_lookup=1)
        else:
            ql = 2 + g
            z = cs.assign_variable(ql * cs.value_of(x) + 5)
            cs.arith_constrain(x, P.ZERO_VAR, z, q_l=ql, q_o=-1, q_c=5)
            x = z
    cs.arith_constrain(P.ZERO_VAR, P.ZERO_VAR, x, q_o=-1, q_c=5, pi=cs.value_of(x) - 5)
    assert cs.n_gates == n and cs.check_satisfied() and cs.circuit_bound() == n
    return cs


_CASES = {}


def _case(cv, n, kind="synthetic"):
    key = (cv.name, n, kind)
    if key not in _CASES:
        css = [_short_selectors(cv, n)] if kind == "short" else [_synthetic(cv, n, 40 + k) for k in range(2)]
        _CASES[key] = QC.Case(cv, n, css)
    return _CASES[key]


@pytest.fixture(scope="module")
def ctxs():
    import zkt_plonk_amd as z
    c = {cv.name: z.Context(cv.name, 0) for cv in CURVES}
    yield c
    for x in c.values():
        x.close()


def _restore(ctx):
    ctx.set_fused_passes(0)
    ctx.set_quotient_route(0)


def _all_modes_and_routes(z, ctx, cs, seeds):
    """Witness 0 under seeds[0] alone, then the chain witness 0 -> witness 1 -> witness 0 with every successor announced,
    for both modes on both quotient routes: all the oracle's bytes (hence equal to each other)."""
    last = len(cs.css) - 1
    order = [(0, seeds[0]), (last, seeds[1]), (0, seeds[0])]
    for route in (CLASSES, WHOLE):
        ctx.set_quotient_route(route)
        got = {}
        for mode in (FUSED, STEPWISE):
            ctx.set_fused_passes(mode)
            got[mode] = [cs.prove(z, ctx, 0, seeds[0])]
            preps = [ctx.prepare_host(*cs.inputs(k, seed)) for k, seed in order]
            for i in range(len(order)):
                got[mode].append(ctx.prove_prepared(preps[i], cs.tr(z), preps[i + 1] if i + 1 < len(order) else None))
        want = [cs.want(0, seeds[0])] + [cs.want(k, seed) for k, seed in order]
        assert got[FUSED] == got[STEPWISE], route
        assert got[FUSED] == want, route


@pytest.mark.parametrize("cv,n", [(cv, n) for cv in CURVES for n in SIZES], ids=lambda v: getattr(v, "name", str(v)))
def test_proof_bytes(cv, n, ctxs):
    import zkt_plonk_amd as z
    ctx, cs = ctxs[cv.name], _case(cv, n)
    cs.load(z, ctx)
    try:
        _all_modes_and_routes(z, ctx, cs, (900, 931))
    finally:
        _restore(ctx)


@pytest.mark.parametrize("n", [16, 1024])
def test_key_polynomials_of_no_and_of_one_coefficient(n, ctxs):
    """q_m and q_r without a coefficient, q_o and q_c with one: ragged terms of the combination, some ending below every
    workgroup but the first."""
    import zkt_plonk_amd as z
    cv = F.BN254
    ctx, cs = ctxs[cv.name], _case(cv, n, "short")
    assert [len(cs.pk.polys[k]) for k in ("q_m", "q_r", "q_o", "q_c")] == [0, 0, 1, 1]
    cs.load(z, ctx)
    try:
        _all_modes_and_routes(z, ctx, cs, (905, 906))
    finally:
        _restore(ctx)


def test_forks_inherit_the_mode(ctxs):
    import zkt_plonk_amd as z
    cv = F.BN254
    ctx, cs = ctxs[cv.name], _case(cv, 16)
    cs.load(z, ctx)
    try:
        ctx.set_fused_passes(STEPWISE)
        with pytest.raises(z.ZktError):
            ctx.set_fused_passes(3)
        fork = ctx.fork()
        try:
            assert cs.prove(z, fork, 0, 900) == cs.want(0, 900)
            fork.set_fused_passes(FUSED)
            assert cs.prove(z, fork, 0, 900) == cs.want(0, 900)
        finally:
            fork.close()
    finally:
        _restore(ctx)


# ---- forced challenges -----------------------------------------------------------------------------------------------
REFUSED = ("xi_1", "beta_eq_gamma", "beta_eq_delta", "beta_eq_eps", "gamma_eq_delta", "gamma_eq_eps", "delta_eq_eps", "den_row0",
           "den_rown2", "lk_row0", "lk_rown2")


class Rig:
    def __init__(self, z, w, cases):
        self.w = w
        self.ctx = z.Context(w.cv.name, 0)
        self.prep = FC.load(z, self.ctx, w)
        self.cases = {name: (forced, exp) for name, forced, exp in cases}

    def run(self, name):
        """-> (rc, bytes, the table's expectation, the oracle's bytes or None)"""
        forced, exp = self.cases[name]
        rc, got = FC.prove_with(self.ctx, self.prep, FC.transcript(self.w, forced))
        return rc, got, exp


@pytest.fixture(scope="module")
def small():
    import zkt_plonk_amd as z
    rigs = {}
    for cv in CURVES:
        w = FC.world(cv, 100, 16, seed=8, tau=777, blinder_seed=1)
        assert w.n == 128
        rigs[cv.name] = Rig(z, w, FC.cases(cv, w.cs, w.pk, w.epk, w.n, w.trace))
    yield rigs
    for r in rigs.values():
        r.ctx.close()


@pytest.fixture(scope="module")
def big():
    import zkt_plonk_amd as z
    w = FC.world(F.BN254, 1500, 64, seed=1508, tau=0xB16 + 777, blinder_seed=2)
    assert w.n == 2048
    rig = Rig(z, w, FC.position_cases(F.BN254, w.cs, w.pk, w.epk, w.n, w.trace))
    yield rig
    rig.ctx.close()


def _xi_zero(rig):
    """xi = 0: both openings are at zero, the raw combination; r(xi) is its constant coefficient."""
    want, want_bytes, _ = FC.oracle_outcome(rig.w, rig.cases["xi_0"][0])
    assert want == FC.PROOF
    try:
        for route in (CLASSES, WHOLE):
            rig.ctx.set_quotient_route(route)
            for mode in (FUSED, STEPWISE):
                rig.ctx.set_fused_passes(mode)
                rc, got, exp = rig.run("xi_0")
                assert exp == FC.PROOF and rc == 0 and got == want_bytes, (route, mode, rc)
    finally:
        _restore(rig.ctx)


@pytest.mark.parametrize("cv", CURVES, ids=lambda c: c.name)
def test_xi_zero_on_both_routes(cv, small):
    _xi_zero(small[cv.name])


def test_xi_zero_on_several_blocks(big):
    _xi_zero(big)


@pytest.mark.parametrize("cv", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("name", REFUSED)
def test_refusals_at_forced_challenges(cv, name, small):
    """xi = 1, equal challenges and a zero denominator of either grand product keep their codes in the fused mode, and the
    next plain proof is the oracle's."""
    rig = small[cv.name]
    try:
        rig.ctx.set_quotient_route(CLASSES)
        rig.ctx.set_fused_passes(FUSED)
        rc, _, exp = rig.run(name)
        assert exp in (6, 7) and rc == exp, (name, rc, exp)
        rc, got = FC.prove_with(rig.ctx, rig.prep, FC.transcript(rig.w, {}))
        assert rc == 0 and got == rig.w.plain
    finally:
        _restore(rig.ctx)


def test_zero_denominator_in_the_second_scan_block(big):
    try:
        big.ctx.set_fused_passes(FUSED)
        for name in ("den_blk2", "den_rown2"):
            rc, _, exp = big.run(name)
            assert exp == 6 and rc == 6, (name, rc)
        rc, got, exp = big.run("den_rown1")       # row n - 1 is in no product
        want, want_bytes, _ = FC.oracle_outcome(big.w, big.cases["den_rown1"][0])
        assert exp == FC.PROOF and want == FC.PROOF and rc == 0 and got == want_bytes
    finally:
        _restore(big.ctx)


# ---- unsatisfied witnesses -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what,code", [("gate", 9), ("copy", 9), ("lookup", 8)])
@pytest.mark.parametrize("cv,n", [(cv, n) for cv in CURVES for n in (16, 2048)], ids=lambda v: getattr(v, "name", str(v)))
def test_unsatisfied_witness(cv, n, what, code, ctxs):
    """On the classes route r(xi), taken from the division's total in the fused mode, is what refuses a broken gate or copy
    constraint; the proof made right after equals a clean context's (the oracle's bytes)."""
    import zkt_plonk_amd as z
    ctx, cs = ctxs[cv.name], _case(cv, n)
    cs.load(z, ctx)
    wires = QC._broken(cs, what)
    try:
        ctx.set_fused_passes(FUSED)
        for route in (CLASSES, WHOLE):
            ctx.set_quotient_route(route)
            with pytest.raises(z.ZktError) as e:
                cs.prove(z, ctx, 0, 940, wires)
            assert e.value.code == code, (route, e.value.code)
            assert cs.prove(z, ctx, 0, 900) == cs.want(0, 900), route
    finally:
        _restore(ctx)


# ---- the grand products alone ----------------------------------------------------------------------------------------
def _per_block(p, seed, n):
    vals = field_elems(p, seed, (n + 1023) // 1024)
    return [vals[i // 1024] for i in range(n)]


@pytest.mark.parametrize("n", [8, 1024, 2048, 4096])
def test_grand_products_alone(n, ctxs):
    """zkt_debug_grand_products in the fused mode against K.z1_evals / K.z2_evals and the stepwise mode: random vectors;
    vectors whose every lookup ratio is 1 (z2 = 1 throughout); vectors constant on each 1024-block with another constant in
    every block, where a block prefix taken from the wrong block changes every element behind it."""
    import zkt_plonk_amd as z
    cv = F.BN254
    p = cv.fr.p
    log_n = n.bit_length() - 1
    ctx, cs = ctxs[cv.name], _case(cv, n)
    cs.load(z, ctx)
    m = lambda v: K.fr_to_mont(cv, v)
    sig = [m(s) for s in (cs.epk.sigma1, cs.epk.sigma2, cs.epk.sigma3)]
    ch = m(field_elems(p, 7100 + n, 4))
    vectors = {"random": [field_elems(p, 7200 + n + i, n) for i in range(7)],
               "ratios_1": [field_elems(p, 7300 + n + i, n) for i in range(3)] + [[0] * n] * 4,
               "per_block": [_per_block(p, 7400 + n + i, n) for i in range(7)]}
    try:
        for name, vec in vectors.items():
            v = [m(x) for x in vec]
            want1 = K.z1_evals(cv, log_n, ch[0], ch[1], v[0], v[1], v[2], *sig)
            want2 = K.z2_evals(cv, log_n, ch[2], ch[3], v[3], v[4], v[5], v[6])
            if name == "ratios_1":
                assert np.array_equal(want2, np.broadcast_to(m([1])[0], (n, 4)))
            for mode in (FUSED, STEPWISE):
                ctx.set_fused_passes(mode)
                z1, z2 = ctx.debug_grand_products(n, ch, v)
                assert np.array_equal(z1, want1), (name, mode)
                assert np.array_equal(z2, want2), (name, mode)
    finally:
        _restore(ctx)


# ---- blinding --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 4096])
def test_trimmed_lengths_and_blinders(n, ctxs):
    """zkt_commit_evals_dev with 0, 2 and 3 blinders on both paths: the coefficient path commits what the launch left in the
    polynomial (the blinders sit at its trimmed length), the Lagrange-basis path reads the length slot itself, so each point
    pins the length.  The low-degree vector of tests/ntt_cases.py (n = 4096) has n/4 + 3 coefficients: more than the 1024 top
    coefficients vanish and the workgroup walks down the polynomial itself."""
    import zkt_plonk_amd as z
    cv = F.BN254
    p = cv.fr.p
    log_n = n.bit_length() - 1
    ctx, cs = ctxs[cv.name], _case(cv, n)
    cs.load(z, ctx)
    vectors = {"random": field_elems(p, 8100 + n, n), "constant": [5] * n, "zero": [0] * n}
    if n == 4096:
        low = ntt_cases.make(cv, log_n, "ifft", "low_degree")
        assert low.expected[n // 4 + 2] != 0 and not any(low.expected[n // 4 + 3:])
        vectors["low_degree"] = low.input
    bl_all = field_elems(p, 8200, 3)
    d_ev = ctx.alloc(n * 32)
    try:
        for name, ev in vectors.items():
            ctx.upload(d_ev, K.fr_to_mont(cv, ev))
            for k in (0, 2, 3):
                bl = bl_all[:k]
                want = _oracle_commit(cv, log_n, cs.srs, ev, bl)
                for path in (0, 1):
                    got = {}
                    for mode in (FUSED, STEPWISE):
                        ctx.set_fused_passes(mode)
                        out, inf = ctx.commit_evals_dev(d_ev, K.fr_to_mont(cv, bl) if k else None, path)
                        got[mode] = None if inf else K.points_from_mont(cv, out)[0]
                    assert got[FUSED] == got[STEPWISE], (name, k, path)
                    assert got[FUSED] == want, (name, k, path)
    finally:
        ctx.free(d_ev)
        _restore(ctx)
