"""The forced-challenge cases of tests/forced_challenges.py on the CPU oracle alone: every case's outcome equals the literal
the table gives, every proof among them survives a round trip through the wire format and is accepted by the oracle's
verifier under the same forced transcript, and the table holds enough of each kind that the GPU tests built on it
(tests/test_gpu_forced_challenges.py) cannot go vacuous."""
import numpy as np
import pytest

from oracle import fields as F, plonk as P, coracle as K

import forced_challenges as FC

CURVES = [F.BN254, F.BLS12_381]


@pytest.fixture(scope="module")
def worlds():
    return {cv.name: FC.world(cv, 100, 16, seed=8, tau=777, blinder_seed=1) for cv in CURVES}


@pytest.fixture(scope="module")
def outcomes(worlds):
    out = {}
    for cv in CURVES:
        w = worlds[cv.name]
        assert w.n == 128
        out[cv.name] = {name: (forced, exp) + FC.oracle_outcome(w, forced)
                        for name, forced, exp in FC.cases(cv, w.cs, w.pk, w.epk, w.n, w.trace)}
    return out


@pytest.mark.parametrize("cv", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("name", FC.NAMES)
def test_oracle_outcome_equals_the_table(cv, name, worlds, outcomes):
    w = worlds[cv.name]
    forced, exp, got, proof, drawn = outcomes[cv.name][name]
    assert FC.matches(got, exp), (name, got, exp)
    if got != FC.PROOF:
        return
    if name == "plain":
        assert proof == w.plain
    pis = [w.cs.pi[k] for k in sorted(w.cs.pi)]
    assert P.verify(cv, w.tau, w.vk, P.proof_deserialize(cv, proof), FC.transcript(w, forced), pis)
    # the same bytes under the unforced transcript are a proof for other challenges: rejected (the forcing took effect)
    if forced:
        assert not P.verify(cv, w.tau, w.vk, P.proof_deserialize(cv, proof), P.new_seeded_transcript(cv, w.vk), pis)


@pytest.mark.parametrize("cv", CURVES, ids=lambda c: c.name)
def test_the_table_cannot_go_vacuous(cv, outcomes):
    got = [o[2] for o in outcomes[cv.name].values()]
    assert sum(1 for g in got if g == FC.PROOF) >= 12
    for code in (6, 7, 9):
        assert code in got, code
    # all six pairs of equal challenges among beta, gamma, delta, epsilon
    pairs = set()
    for name, (forced, exp, g, _, drawn) in outcomes[cv.name].items():
        if g == 7:
            four = [drawn[k] for k in ("beta", "gamma", "delta", "epsilon")]
            eq = [(i, j) for i in range(4) for j in range(i + 1, 4) if four[i] == four[j]]
            assert len(eq) == 1, name
            pairs.add(eq[0])
    assert len(pairs) == 6


@pytest.mark.parametrize("cv", CURVES, ids=lambda c: c.name)
def test_forced_values_hit_what_they_aim_at(cv, worlds, outcomes):
    """The crafted challenges do what their names say: the named factor of the named row vanishes (and only rows up to
    n - 2 enter a product); xi cases sit on the domain; the forced transcript's state advances like the plain one's."""
    w = worlds[cv.name]
    p, n = cv.fr.p, w.n
    a = w.cs.wire_evals(n)[0]
    h1, h2 = w.trace.evals["h1"], w.trace.evals["h2"]
    for name, row in (("den_row0", 0), ("den_rown2", n - 2), ("den_rown1", n - 1)):
        d = outcomes[cv.name][name][4]
        assert (a[row] + d["beta"] * w.epk.sigma1[row] + d["gamma"]) % p == 0
    for name, row in (("lk_row0", 0), ("lk_rown2", n - 2), ("lk_rown1", n - 1)):
        d = outcomes[cv.name][name][4]
        assert (d["epsilon"] * (1 + d["delta"]) + h1[row] + d["delta"] * h2[row]) % p == 0
    for name in ("xi_w1", "xi_whalf", "xi_wlast"):
        xi = outcomes[cv.name][name][4]["xi"]
        assert pow(xi, n, p) == 1 and xi != 1
    assert outcomes[cv.name]["xi_wlast"][4]["xi"] * cv.fr.root_of_unity(n) % p == 1
    # unforced challenges before the forced one are the plain run's; the later ones differ (they depend on it)
    plain = outcomes[cv.name]["plain"][4]
    d = outcomes[cv.name]["alpha_1"][4]
    assert [d[k] for k in ("beta", "gamma", "delta", "epsilon")] == [plain[k] for k in ("beta", "gamma", "delta", "epsilon")]
    assert d["alpha"] == 1 and d["xi"] != plain["xi"]


@pytest.mark.parametrize("cv", CURVES, ids=lambda c: c.name)
def test_array_oracle_of_the_grand_products_at_a_zero_denominator(cv, worlds):
    """K.z1_evals / K.z2_evals, the references of the zkt_debug_grand_products test: a denominator that vanishes at row 0
    or n - 2 is refused, one at row n - 1 (which no product includes) gives the vectors of the big-integer restatement."""
    w = worlds[cv.name]
    n, log_n = w.n, w.n.bit_length() - 1
    dom = w.be.domain(n)
    m = lambda v: K.fr_to_mont(cv, v)
    sig = (w.epk.sigma1, w.epk.sigma2, w.epk.sigma3)

    def run(product, ch, vec):
        c4 = m(list(ch))
        if product == 1:
            return K.z1_evals(cv, log_n, c4[0], c4[1], m(vec[0]), m(vec[1]), m(vec[2]), *[m(s) for s in sig])
        return K.z2_evals(cv, log_n, c4[2], c4[3], m(vec[3]), m(vec[4]), m(vec[5]), m(vec[6]))

    for product in (1, 2):
        for k, row in enumerate((0, n - 2)):
            ch, vec = FC.grand_product_case(cv, w.epk, n, product, row, seed=2 * product + k)
            with pytest.raises(ZeroDivisionError):
                run(product, ch, vec)
        ch, vec = FC.grand_product_case(cv, w.epk, n, product, n - 1, seed=10 + product)
        if product == 1:
            want = P.compute_z1_evals(cv, dom, ch[0], ch[1], vec[0], vec[1], vec[2], *sig)
        else:
            want = P.compute_z2_evals(cv, dom, ch[2], ch[3], vec[3], vec[4], vec[5], vec[6])
        assert np.array_equal(run(product, ch, vec), m(want))


def test_position_dependent_cases_on_several_blocks():
    """The subset the GPU tests run at n = 2048 (two scan blocks): the oracle's outcomes equal the table there too."""
    cv = F.BN254
    w = FC.world(cv, 1500, 64, seed=1508, tau=0xB16 + 777, blinder_seed=2)
    assert w.n == 2048
    got = {name: (FC.oracle_outcome(w, forced)[0], exp) for name, forced, exp in FC.position_cases(cv, w.cs, w.pk, w.epk, w.n, w.trace)}
    assert tuple(got) == FC.POSITION_NAMES
    for name, (outcome, exp) in got.items():
        assert FC.matches(outcome, exp), (name, outcome, exp)
