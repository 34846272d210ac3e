"""The structured transform inputs of ntt_cases.py against the C++ oracle (oracle/coracle.cpp orc_ntt), which the device
test (test_gpu_ntt_structured.py) compares with: the oracle reproduces every closed form, and every case that claims
exact zeros in its output has them -- so the device test does feed the kernels the zeros it is about."""
import numpy as np
import pytest

from oracle import fields as F, coracle as K
from oracle.ntt import Domain
import ntt_cases as NC

CURVES = [F.BN254, F.BLS12_381]


def _zero_rows(arr) -> int:
    return int((~np.asarray(arr).any(axis=1)).sum())


@pytest.mark.parametrize("cv", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("log_n", [4, 11, 14])
def test_oracle_reproduces_closed_forms_and_zero_counts(cv, log_n):
    n = 1 << log_n
    closed = zero_claims = 0
    for name, inv, cos in NC.VARIANTS:
        for cname in NC.ALL_CASES:
            case = NC.make(cv, log_n, name, cname)
            if case is None:
                assert cname == "periodic_32" and n < 32
                continue
            assert len(case.input) <= n and all(0 <= v < cv.fr.p for v in case.input), (name, cname)
            out = K.ntt_mont(cv, log_n, inv, cos, K.fr_to_mont(cv, case.input))
            if case.expected is not None:
                assert len(case.expected) == n
                assert np.array_equal(out, K.fr_to_mont(cv, case.expected)), (cv.name, log_n, name, cname)
                closed += 1
            if case.zeros is not None:
                # Montgomery words of zero are zero words: a residue 0 stored as p would not count
                assert _zero_rows(out) == case.zeros, (cv.name, log_n, name, cname)
                assert case.expected is None or sum(1 for v in case.expected if v == 0) == case.zeros
                zero_claims += 1
    # every variant of zeros, delta and geometric; three of four of the constant, alternating and periodic cases; low_degree inverse
    assert closed >= 4 * 12 + 3 * 6 + 2 and zero_claims >= 4 * 6 + 3 * 6 + 2


@pytest.mark.parametrize("cv", CURVES, ids=lambda c: c.name)
def test_the_reduced_list_is_part_of_the_full_one_and_keeps_its_zeros(cv):
    assert set(NC.LARGE_CASES) <= set(NC.ALL_CASES)
    assert NC.case_names(NC.LARGE_FROM - 1) == NC.ALL_CASES and NC.case_names(NC.LARGE_FROM) == NC.LARGE_CASES
    claims = [NC.make(cv, 6, "ifft", c).zeros for c in NC.LARGE_CASES]
    assert sum(z is not None for z in claims) >= 5          # constant, alternating, two geometric, low degree
    assert [NC.default_split(k) for k in (10, 11, 14, 16, 17, 18, 25)] == [[], [6, 5], [7, 7], [8, 8], [6, 6, 5], [6, 6, 6], [9, 8, 8]]


@pytest.mark.parametrize("cv", CURVES, ids=lambda c: c.name)
def test_low_degree_inputs_are_evaluations_by_the_definition(cv):
    """The one input built with the oracle's forward transform, pinned to Horner evaluation at 2^4."""
    f, log_n = cv.fr, 4
    d = Domain(f, 1 << log_n)
    for variant, shift in (("ifft", 1), ("coset_ifft", f.generator)):
        case = NC.make(cv, log_n, variant, "low_degree")
        coeffs = case.expected[:(1 << log_n) // 4 + 3]
        assert all(coeffs) and case.expected[len(coeffs):] == [0] * case.zeros
        for i, v in enumerate(case.input):
            x, acc = shift * d.element(i) % f.p, 0
            for c in reversed(coeffs):
                acc = (acc * x + c) % f.p
            assert acc == v
