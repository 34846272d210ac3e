"""The device prover at forced Fiat-Shamir challenges (tests/forced_challenges.py): the branches of Prover::run that exist
only for special challenge values -- the refusals ZKT_ERR_ZERO_DENOMINATOR (6), ZKT_ERR_EQUAL_CHALLENGES (7),
ZKT_ERR_QUOTIENT_TOO_SHORT (9) at every exit, and the algebraic edge points the reference proves through -- which
challenges drawn from Merlin or Keccak never reach.  zkt_prove_with's callbacks drive the device with the same forced
transcript as the oracle, so every outcome is exact: the oracle's bytes, or the code the table names.  After a refusal
the context must go on producing the oracle's bytes, also when a successor was announced whose arrays are gone, and
without issuing any of that successor's early work."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import fields as F, coracle as K

import forced_challenges as FC

CURVES = [F.BN254, F.BLS12_381]
BIG_BLS = ("xi_wlast", "den_blk2")            # the two of the position-dependent cases that also run on BLS12-381
# one refusal of each exit of Prover::run: round 3, after the grand products, round 4's degree check (read in round 5),
# round 5 (behind the early round 1 of an announced successor)
EXITS = [("beta_eq_gamma", 7), ("den_row0", 6), ("alpha_0", 9), ("xi_1", 6)]


class Rig:
    """One circuit loaded on a context of its own, its cases, and the oracle's outcome per case (computed once)."""

    def __init__(self, z, w, cases):
        self.w = w
        self.ctx = z.Context(w.cv.name, 0)
        self.prep = FC.load(z, self.ctx, w)
        self.cases = {name: (forced, exp) for name, forced, exp in cases}
        self._oracle = {}

    def oracle(self, name):
        if name not in self._oracle:
            self._oracle[name] = FC.oracle_outcome(self.w, self.cases[name][0])
        return self._oracle[name]

    def plain(self, ctx=None, prep=None):
        return FC.prove_with(ctx or self.ctx, prep or self.prep, FC.transcript(self.w, {}))


@pytest.fixture(scope="module")
def small():
    """n = 128 on both curves: the circuit of test_prover_error_paths."""
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
    """n = 2048, the smallest n at which the scans of the grand products need a second 1024-element block, the evaluations a
    second 2048-coefficient segment (the polynomials have n + 8 coefficients) and the opening witness several 512-element
    workgroups."""
    import zkt_plonk_amd as z
    rigs = {}
    for cv in CURVES:
        w = FC.world(cv, 1500, 64, seed=1508, tau=0xB16 + 777, blinder_seed=2)
        assert w.n == 2048
        rigs[cv.name] = Rig(z, w, FC.position_cases(cv, w.cs, w.pk, w.epk, w.n, w.trace))
    yield rigs
    for r in rigs.values():
        r.ctx.close()


def _one_case(rig, name):
    w = rig.w
    forced, exp = rig.cases[name]
    want, want_bytes, want_drawn = rig.oracle(name)
    assert FC.matches(want, exp), (name, want, exp)               # pinned on the CPU too (test_forced_challenges_oracle.py)
    tr = FC.transcript(w, forced)
    rc, got = FC.prove_with(rig.ctx, rig.prep, tr)
    print("%s n=%d %s: device %s; table %s" % (w.cv.name, w.n, name, "proves, bytes %s" % ("equal" if got == want_bytes else "DIFFER")
                                                if rc == 0 else "refuses with %d" % rc, exp))
    if exp == FC.PROOF:
        assert rc == 0, (name, rc)
        assert got == want_bytes, name
        assert tr.drawn == want_drawn
        return
    assert rc != 0 and FC.matches(rc, exp), (name, rc, exp)
    # the challenges up to the refusal are the oracle's (the oracle may stop earlier or later within a round)
    common = set(tr.drawn) & set(want_drawn)
    assert {k: tr.drawn[k] for k in common} == {k: want_drawn[k] for k in common}
    rc, got = rig.plain()
    assert rc == 0 and got == w.plain, name


@pytest.mark.parametrize("cv", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("name", FC.NAMES)
def test_forced_challenge_cases(cv, name, small):
    """Every case of the table at n = 128: exactly the oracle's bytes, or exactly the expected code and then a plain Merlin
    proof on the same context that equals the oracle's."""
    _one_case(small[cv.name], name)


@pytest.mark.parametrize("cvname,name", [("bn254", nm) for nm in FC.POSITION_NAMES] + [("bls12_381", nm) for nm in BIG_BLS])
def test_position_dependent_cases_on_several_blocks(cvname, name, big):
    _one_case(big[cvname], name)


def _commitments_of_a_plain_proof(rig, ctx, prep):
    """-> (rc, bytes, dense commitments, Lagrange-basis commitments) of one plain proof (zkt_profile_get units)."""
    before = [ctx.profile_get(k)[0] for k in ("msm_main", "msm_lag_main")]
    rc, got = rig.plain(ctx, prep)
    return (rc, got) + tuple(ctx.profile_get(k)[0] - b for k, b in zip(("msm_main", "msm_lag_main"), before))


def _refuse_with_an_announcement_armed(rig, ctx, prep, name, code):
    """zkt_prove_set_next(successor); the forced proof fails with `code`; the successor's arrays are overwritten; then two
    plain proofs each equal the oracle's bytes and issue no more than a proof's own 13 dense commitments (early rounds of
    a stale successor would add 3 to 6) -- and, dense and Lagrange-basis alike, exactly as many as the same proof issued on
    this context before the refusal (its table polynomial cached, as it is afterwards)."""
    import zkt_plonk_amd as z
    w = rig.w
    L = z.lib()
    ctx.profile_enable(True)
    try:
        for rep in range(2):                     # the second one is the warm proof the later ones are compared with
            rc, got, dense, lag = _commitments_of_a_plain_proof(rig, ctx, prep)
            assert rc == 0 and got == w.plain
        doomed = FC.prepare(ctx, w)
        ctx.check(L.zkt_prove_set_next(ctx.handle, ctypes.byref(doomed.struct)))
        rc, _ = FC.prove_with(ctx, prep, FC.transcript(w, rig.cases[name][0]))
        assert rc == code, (name, rc)
        for arr in doomed._keep:
            if isinstance(arr, np.ndarray):
                arr[...] = 0xDEADBEEF            # whoever still reads these produces garbage
        for rep in range(2):
            rc, got, d, l = _commitments_of_a_plain_proof(rig, ctx, prep)
            print("%s %s after code %d, plain proof %d: rc %d, bytes %s, %d msm_main units (warm proof: %d), %d msm_lag_main (%d)"
                  % (w.cv.name, name, code, rep, rc, "equal" if got == w.plain else "DIFFER", d, dense, l, lag))
            assert rc == 0 and got == w.plain, (name, rep)
            assert d <= 13, (name, rep, d)
            assert (d, l) == (dense, lag), (name, rep)
    finally:
        ctx.profile_enable(False)
    del doomed


@pytest.mark.parametrize("cv", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("name,code", EXITS)
def test_refusal_with_an_announcement_armed(cv, name, code, small):
    rig = small[cv.name]
    _refuse_with_an_announcement_armed(rig, rig.ctx, rig.prep, name, code)


def test_refusals_on_a_forked_context(small):
    """The same sequences on a fork (its own streams and work buffers, the parent's tables); the parent proves the same
    bytes afterwards."""
    rig = small["bn254"]
    rc, got = rig.plain()                        # builds the Lagrange table the fork shares
    assert rc == 0 and got == rig.w.plain
    fork = rig.ctx.fork()
    try:
        prep = FC.prepare(fork, rig.w)
        for name, code in EXITS:
            _refuse_with_an_announcement_armed(rig, fork, prep, name, code)
        rc, got = rig.plain()
        assert rc == 0 and got == rig.w.plain
        rc, got = rig.plain(fork, prep)
        assert rc == 0 and got == rig.w.plain
    finally:
        fork.close()


def _grand_products_alone(rig, rows_refused):
    import zkt_plonk_amd as z
    w = rig.w
    cv, n = w.cv, w.n
    log_n = n.bit_length() - 1
    m = lambda v: K.fr_to_mont(cv, v)
    sig = [m(s) for s in (w.epk.sigma1, w.epk.sigma2, w.epk.sigma3)]
    for product in (1, 2):
        for k, row in enumerate(rows_refused):
            ch, vec = FC.grand_product_case(cv, w.epk, n, product, row, seed=len(rows_refused) * product + k)
            with pytest.raises(z.ZktError) as e:
                rig.ctx.debug_grand_products(n, m(list(ch)), [m(v) for v in vec])
            assert e.value.code == 6, (product, row)
        ch, vec = FC.grand_product_case(cv, w.epk, n, product, n - 1, seed=10 + product)
        c4, v = m(list(ch)), [m(x) for x in vec]
        z1, z2 = rig.ctx.debug_grand_products(n, c4, v)
        assert np.array_equal(z1, K.z1_evals(cv, log_n, c4[0], c4[1], v[0], v[1], v[2], *sig)), product
        assert np.array_equal(z2, K.z2_evals(cv, log_n, c4[2], c4[3], v[3], v[4], v[5], v[6])), product
    rc, got = rig.plain()
    assert rc == 0 and got == w.plain


@pytest.mark.parametrize("cv", CURVES, ids=lambda c: c.name)
def test_grand_products_alone_at_a_zero_denominator(cv, small):
    """zkt_debug_grand_products on arbitrary vectors: a denominator that vanishes at row 0 or n - 2 of either product is
    code 6; one at row n - 1, which no product includes, changes nothing (K.z1_evals / K.z2_evals)."""
    rig = small[cv.name]
    _grand_products_alone(rig, (0, rig.w.n - 2))


def test_grand_products_alone_at_a_zero_denominator_in_the_second_block(big):
    rig = big["bn254"]
    _grand_products_alone(rig, (FC.SECOND_BLOCK_ROW, rig.w.n - 2))
