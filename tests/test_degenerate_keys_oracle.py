"""No GPU: the case table of tests/degenerate_keys.py against the CPU oracle -- under every key the oracle's proof of the
fixed statement verifies under the trapdoor, round-trips through its own deserialiser, and the key and the commitments
hold exactly the identities the table says -- and the host verifier (zkt_verify, zkt_verify_batch, zkt_verify_prepare) on
those proofs, whose honest commitments and verifier keys hold identities.

tau = 0 is left out of every verifier leg: beta_h = [0] h is the G2 identity, and whether the pairing product takes that
is not what these tests are about."""
import numpy as np
import pytest

from oracle import plonk as P, coracle as K, curve as C
from zkt_plonk_amd import _lib
import degenerate_keys as DK

CURVE_IDS = lambda c: c.name  # noqa: E731


def test_the_table_names_each_key_once_and_says_what_it_forces():
    assert len(set(DK.IDS)) == len(DK.CASES) == 8
    assert [c.name for c in DK.CASES if c.name not in [v.name for v in DK.VERIFIER_CASES]] == ["0"]
    for c in DK.CASES:
        assert c.forces and set(c.proof_identities) <= set(P.Proof.COMMIT_ORDER) and set(c.vk_identities) <= set(P.PK_POLYS)


@pytest.mark.parametrize("cv", DK.CURVES, ids=CURVE_IDS)
def test_the_trapdoors_are_what_their_names_say(cv):
    p, n = cv.fr.p, DK.N
    w = cv.fr.root_of_unity(n)
    assert pow(w, n, p) == 1 and pow(w, n // 2, p) == p - 1
    tau = {c.name: DK.tau_of(cv, c) for c in DK.CASES}
    assert tau["0"] == 0 and tau["1"] == 1 and tau["-1"] == p - 1 and tau["w"] == w
    assert tau["w^(n-1)"] * w % p == 1 and tau["w^5"] == pow(w, 5, p)
    assert pow(tau["w_2n"], n, p) == p - 1                                     # tau^n = -1
    assert pow(tau["w^(n/4)"], 2, p) == p - 1                                  # order four
    for c in DK.CASES:
        assert c.in_domain == (pow(tau[c.name], n, p) == 1), c.name            # tau^n = 1: every blinder point is P - P
    assert len(set(tau.values())) == len(DK.CASES)


@pytest.mark.parametrize("cv", DK.CURVES, ids=CURVE_IDS)
def test_numpy_keys_are_the_powers(cv):
    for name in DK.NUMPY_KEYS:
        assert np.array_equal(DK.numpy_key(cv, name, 37), K.srs_mont(cv, DK.tau_of(cv, DK.BY_NAME[name]), 37)), name


@pytest.mark.parametrize("case", DK.CASES, ids=DK.IDS)
@pytest.mark.parametrize("cv", DK.CURVES, ids=CURVE_IDS)
def test_oracle_proves_and_verifies_and_the_identities_are_the_tables(cv, case):
    st = DK.statement(cv, case)
    assert DK.identity_bases(st.srs) == case.identity_bases
    assert st.srs.shape[0] == DK.N + DK.SPARE
    assert DK.proof_identities(st.proof) == case.proof_identities
    assert DK.vk_identities(st.vk) == case.vk_identities
    back = P.proof_deserialize(cv, st.raw)
    assert back.serialize(cv) == st.raw and DK.proof_identities(back) == case.proof_identities
    assert back.evaluations == st.proof.evaluations
    assert P.verify(cv, st.tau, st.vk, back, P.new_seeded_transcript(cv, st.vk), list(st.pis))
    bad = P.proof_deserialize(cv, DK.flip_evaluation(st.raw))
    assert not P.verify(cv, st.tau, st.vk, bad, P.new_seeded_transcript(cv, st.vk), list(st.pis))


@pytest.mark.parametrize("case", DK.VERIFIER_CASES, ids=[c.name for c in DK.VERIFIER_CASES])
@pytest.mark.parametrize("cv", DK.CURVES, ids=CURVE_IDS)
def test_host_verifier_takes_honest_proofs_with_identity_commitments(cv, case):
    st = DK.statement(cv, case)
    h, beta_h = _lib.srs_generate_g2(cv.name, st.tau)
    it = DK.item(cv, st)
    assert _lib.verify(cv.name, *it[:7], h, beta_h, it[7])
    assert _lib.verify_batch(cv.name, [DK.item(cv, st) for _ in range(3)], h, beta_h)
    # the two pairs, bit for bit against the oracle's restatement of proof.rs:285-503
    want = P.verify_prepare(cv, st.vk, P.proof_deserialize(cv, st.raw), P.new_seeded_transcript(cv, st.vk), list(st.pis))
    it = DK.item(cv, st)
    got, inf = _lib.verify_prepare(cv.name, *it[:7], it[7])
    pts = [None if inf[i] else K.points_from_mont(cv, got[i:i + 1])[0] for i in range(4)]
    assert [(pts[0], pts[1]), (pts[2], pts[3])] == want
    assert not got[np.asarray(inf, dtype=bool)].any()
    for L_, W_ in want:
        assert L_ == C.scalar_mul(cv, st.tau, W_)                              # e(L, h) == e(W, tau h)
    # one evaluation byte flipped: rejected alone and inside a batch
    flipped = DK.flip_evaluation(st.raw)
    it = DK.item(cv, st, flipped)
    assert not _lib.verify(cv.name, *it[:7], h, beta_h, it[7])
    assert not _lib.verify_batch(cv.name, [DK.item(cv, st), DK.item(cv, st, flipped), DK.item(cv, st)], h, beta_h)
