"""No GPU: the case table of tests/key_length_cases.py against the text of the sources it restates, and the fact the GPU
test rests on -- the oracle's proof bytes do not depend on how many powers the key holds beyond n + 8."""
import os
import re

import pytest

from oracle import fields as F, plonk as P, coracle as K
from helpers import field_elems
import key_length_cases as KL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zkt-plonk_amd", "csrc")


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _shifted(text, what):
    """`((size_t)1 << a) + b` right after `what` -> the integer"""
    m = re.search(re.escape(what) + r"\s*\(\(size_t\)1 << (\d+)\) \+ (\d+)", text)
    assert m, "cannot find `%s ((size_t)1 << a) + b` in the source" % what
    return (1 << int(m.group(1))) + int(m.group(2))


def test_regime_edges_sit_on_the_constants_of_the_sources():
    hpp, hip = _read("msm.hpp"), _read("msm.hip")
    assert _shifted(hpp, "constexpr size_t MSM_DEFER_MAX =") == KL.DEFER_MAX
    assert _shifted(hpp, "constexpr size_t MSM_TAIL_INL_MAX =") == KL.TAIL_INL_MAX
    # the grouping rule of msm_batches_grouping: deferred keys, and one band above them
    rule = re.search(r"return n <= MSM_DEFER_MAX \|\| \(n > (.*?) && n <= (.*?)\);", hip)
    assert rule, "msm_batches_grouping no longer reads `n <= MSM_DEFER_MAX || (n > lo && n <= hi)`"
    assert _shifted(rule.group(1), "") == KL.GROUP_LO and _shifted(rule.group(2), "") == KL.GROUP_HI
    assert "st->defer_tails = count <= MSM_DEFER_MAX;" in hip
    assert "c->msm->defer_tails || c->msm->count <= MSM_TAIL_INL_MAX" in hip
    counts = {c.count for c in KL.CASES}
    for edge in (KL.DEFER_MAX, KL.GROUP_LO, KL.GROUP_HI, KL.TAIL_INL_MAX):
        assert edge in counts and edge + 1 in counts, "both sides of the edge %d must be in the table" % edge
    for at in ((1 << 17) - 1, 1 << 17):
        assert at in counts


def test_the_table_is_consistent_with_the_rules_it_restates():
    names = [c.name for c in KL.CASES]
    assert len(set(names)) == len(names) and len({c.count for c in KL.CASES}) == len(names)
    n = KL.N
    for want in (n + 1, n + 2, n + 7, n + 9, 4 * n + 1, (1 << 19) + 1, (1 << 20) + 1, (1 << 21) + 1):
        assert any(c.count == want for c in KL.CASES), want
    for c in KL.CASES:
        assert c.count > n and c.why
        assert c.deferred == (c.count <= KL.DEFER_MAX), c.name
        assert c.grouped == (c.count <= KL.DEFER_MAX or KL.GROUP_LO < c.count <= KL.GROUP_HI), c.name
        assert c.inlined == (c.count <= KL.TAIL_INL_MAX), c.name
        assert set(c.digits) == ({"bn254"} if c.count > (1 << 21) else {"bn254", "bls12_381"}), c.name
        for curve, (bits, windows) in c.digits.items():
            total = KL.SCALAR_BITS[curve]
            # `windows` digits of `bits` or `bits - 1` bits cover the scalar exactly (msm_plan): bits = ceil(total / windows)
            assert windows * (bits - 1) < total <= windows * bits, (c.name, curve)
            assert windows * c.count < (1 << 31), (c.name, curve)      # 31-bit indices into the window table
    # the digit widths named in msm_setup's comments
    lg = lambda name: KL.BY_NAME[name].digits
    assert lg("2^17-1")["bn254"][0] == 14 and lg("2^17")["bn254"][0] == 17 and lg("2^17")["bls12_381"][0] == 16
    assert lg("2^19+1")["bls12_381"][0] == 18 and lg("2^20+1")["bls12_381"][0] == 19 and lg("2^21+1")["bn254"][0] == 19
    assert KL.lagrange_bases(n + 1) == n + 1 and KL.lagrange_bases(n + 7) == n + 7
    assert KL.lagrange_bases(n + 9) == n + 8 and KL.lagrange_bases(1 << 20) == n + 8


def test_scalar_bits_are_the_fields():
    assert KL.SCALAR_BITS == {cv.name: cv.fr.bits + 1 for cv in (F.BN254, F.BLS12_381)}


@pytest.mark.parametrize("cv", [F.BN254, F.BLS12_381], ids=lambda c: c.name)
def test_oracle_proof_bytes_do_not_depend_on_the_key_length(cv):
    """n + 8 against 4n + 1 powers (what the reference's PC::trim keeps) at n = 128: setup and proof are the same bytes,
    so one oracle proof under n + 8 powers is the reference for every key length of the GPU test."""
    cs = P.synthetic_circuit(cv, 100, 16, seed=8)
    n = cs.circuit_bound()
    assert n == 128
    long_key = K.srs_mont(cv, 777, 4 * n + 1)
    blinders = field_elems(cv.fr.p, 1, P.NUM_BLINDERS)
    got = []
    for count in (n + 8, 4 * n + 1):
        be = K.CBackend(cv, long_key[:count])
        pk, epk, vk = P.setup(be, [None] * count, cs, True)
        proof = P.prove(be, [None] * count, pk, epk, vk, cs, P.new_seeded_transcript(cv, vk), blinders)
        got.append((vk.commits, proof.serialize(cv)))
    assert got[0] == got[1]
    assert len(got[0][1]) == (802 if cv.name == "bn254" else 1010)
    # ... down to n + 3 powers, which the polynomials with three blinders need; below that kzg10 refuses the proof
    assert KL.MIN_PROVING_SPARE == 3
    assert [c.name for c in KL.CASES if not c.proves] == ["n+1", "n+2"]
    for spare in (3, 2):
        count = n + spare
        be = K.CBackend(cv, long_key[:count])
        pk, epk, vk = P.setup(be, [None] * count, cs, True)
        assert vk.commits == got[0][0]
        if spare >= KL.MIN_PROVING_SPARE:
            assert P.prove(be, [None] * count, pk, epk, vk, cs, P.new_seeded_transcript(cv, vk), blinders).serialize(cv) == got[0][1]
        else:
            with pytest.raises(ValueError, match="TooManyCoefficients"):
                P.prove(be, [None] * count, pk, epk, vk, cs, P.new_seeded_transcript(cv, vk), blinders)
