"""The C++ oracle's combine_split (oracle/coracle.cpp orc_combine_split), which the device split is checked against, pinned
to the big-integer restatement of lookup/multiset.rs:103-146 (oracle/plonk.py) at the shapes of test_gpu_lookup.py."""
import numpy as np
import pytest

from oracle import fields as F, plonk as P, coracle as K
import lookup_cases as LC


def _ints(arr):
    return [int.from_bytes(r.tobytes(), "little") for r in np.asarray(arr, dtype=np.uint64).reshape(-1, 4)]


@pytest.mark.parametrize("cv", [F.BN254, F.BLS12_381], ids=lambda c: c.name)
def test_combine_split_known_answer(cv):
    # multiset.rs:95-102: t = {2, 4, 1, 3}, f = {2, 3, 3, 2} -> s = {2, 2, 2, 4, 1, 3, 3, 3}, h1 = {2, 2, 1, 3}, h2 = {2, 4, 3, 3}
    t, f = [2, 4, 1, 3], [2, 3, 3, 2]
    assert P.combine_split(t, f) == ([2, 2, 1, 3], [2, 4, 3, 3])
    h1, h2 = K.combine_split(K.fr_to_mont(cv, t), K.fr_to_mont(cv, f))
    assert K.fr_from_mont(cv, h1) == [2, 2, 1, 3] and K.fr_from_mont(cv, h2) == [2, 4, 3, 3]


@pytest.mark.parametrize("log_n", [12, 13, 14])
def test_combine_split_oracle_on_device_test_shapes(log_n):
    """Every key count of the device test up to n (1 .. 8193 and n), 0 absent / first / middle / last, five f patterns."""
    n = 1 << log_n
    rng = np.random.default_rng(0x5917 + log_n)
    seen = 0
    for label, table, fs in LC.cases(rng, n):
        t = LC.pad(table, n)
        for kind, f in fs:
            h1, h2 = K.combine_split(t, f)
            assert h1.shape[0] == n and h2.shape[0] == n, (label, kind)
            w1, w2 = P.combine_split(_ints(t), _ints(f))
            assert _ints(h1) == w1 and _ints(h2) == w2, (label, kind)
            seen += 1
    assert seen >= 5 * (4 * len(LC.key_counts(n)) - 3)
    # a looked-up value outside the table, first or last in f
    table = LC.make_table(rng, 1025, "middle")
    bad = LC.random_values(rng, 1, avoid=table)
    for at in (0, n - 1):
        f = LC.make_f(rng, n, LC.padded_keys(table), "uniform")
        f[at] = bad[0]
        with pytest.raises(KeyError):
            K.combine_split(LC.pad(table, n), f)
        with pytest.raises(KeyError):
            P.combine_split(_ints(LC.pad(table, n)), _ints(f))
