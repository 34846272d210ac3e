"""Committer-key lengths under which a small circuit (n = 2^10) is proved in tests/test_gpu_key_lengths.py, with what
csrc/msm.hip decides from the KEY's length alone: the digit width and window count of msm_setup (scalars of Fr::BITS + 1
bits: 255 on BN254, 256 on BLS12-381) and the launch regime (msm.hpp MSM_DEFER_MAX / MSM_TAIL_INL_MAX, msm.hip
msm_batches_grouping).  Everything here is written out by hand from those rules, not computed by them:
tests/test_key_length_cases_host.py checks that the edges still sit on the constants of the sources, the GPU test that
zkt_msm_info reports these digits.  Plain module: no GPU, no library."""
from collections import namedtuple

LOG_N = 10
N = 1 << LOG_N

# the regime edges as the sources have them today (checked against their text by the host test)
DEFER_MAX = (1 << 16) + 64        # msm.hpp MSM_DEFER_MAX: tails deferred (and commitments grouped) up to here
GROUP_LO = (1 << 17) + 64         # msm.hip msm_batches_grouping: grouped again above this ...
GROUP_HI = (1 << 18) + 64         # ... up to this
TAIL_INL_MAX = (1 << 18) + 64     # msm.hpp MSM_TAIL_INL_MAX: the bucket reduction's additions inline their products up to here

SCALAR_BITS = {"bn254": 255, "bls12_381": 256}

# The longest polynomials of a proof are the blinded z1 / z2 / h1 (three blinders: n + 3 coefficients); kzg10 refuses a
# polynomial longer than the key (TooManyCoefficients), so a whole proof needs n + 3 powers.  The oracle says the same
# (host test).  Under a shorter key the device must refuse as the reference does.
MIN_PROVING_SPARE = 3


# count: powers in the key; digits: {curve: (window_bits, windows)}; deferred / grouped / inlined: the launch regime
class Case(namedtuple("Case", "name count why digits deferred grouped inlined")):
    @property
    def proves(self):
        return self.count >= N + MIN_PROVING_SPARE


_D8 = {"bn254": (8, 32), "bls12_381": (8, 32)}          # lg 10: digits of lg - 2 = 8 bits, the floor
_D10 = {"bn254": (10, 26), "bls12_381": (10, 26)}       # lg 12
_D14 = {"bn254": (14, 19), "bls12_381": (14, 19)}       # lg 16
_D17 = {"bn254": (17, 15), "bls12_381": (16, 16)}       # lg 17 and 18: BN254 fifteen windows of 17, BLS12-381 sixteen of 16
_D19 = {"bn254": (17, 15), "bls12_381": (18, 15)}       # lg 19
_D20 = {"bn254": (17, 15), "bls12_381": (19, 14)}       # lg 20
_D21 = {"bn254": (19, 14)}                              # lg 21: lg - 2 = 19 bits, 2^18 buckets, wide pairs

CASES = [
    Case("n+1", N + 1, "one spare base: the second table holds a single blinder point; no wire commitment fits, the proof is refused", _D8, True, True, True),
    Case("n+2", N + 2, "two spare bases: the least the wire tables need; round 1 fits, round 2 (three blinders) is refused", _D8, True, True, True),
    Case("n+7", N + 7, "one below the clamp of the second table's spare bases", _D8, True, True, True),
    Case("n+9", N + 9, "one above the clamp: the second table keeps 8 of 9 spare bases", _D8, True, True, True),
    Case("4n+1", 4 * N + 1, "the reference's own key (PC::trim to 4 * circuit_bound)", _D10, True, True, True),
    Case("2^16+64", (1 << 16) + 64, "last key with deferred tails", _D14, True, True, True),
    Case("2^16+65", (1 << 16) + 65, "first key without: 14-bit digits, tails not deferred, not grouped", _D14, False, False, True),
    Case("2^17-1", (1 << 17) - 1, "last key on 14-bit digits", _D14, False, False, True),
    Case("2^17", 1 << 17, "first key on BN254's 17-bit and BLS12-381's 16-bit digits", _D17, False, False, True),
    Case("2^17+64", (1 << 17) + 64, "last key of the ungrouped gap", _D17, False, False, True),
    Case("2^17+65", (1 << 17) + 65, "first key whose rounds are grouped again", _D17, False, True, True),
    Case("2^18+1", (1 << 18) + 1, "grouped batches of short MSMs under a 2^18 key", _D17, False, True, True),
    Case("2^18+64", (1 << 18) + 64, "last grouped key, last with inlined tail additions", _D17, False, True, True),
    Case("2^18+65", (1 << 18) + 65, "first key with neither", _D17, False, False, False),
    Case("2^19+1", (1 << 19) + 1, "BLS12-381 on 18-bit digits", _D19, False, False, False),
    Case("2^20+1", (1 << 20) + 1, "BLS12-381 on 19-bit digits; BN254's headline digits over a short MSM", _D20, False, False, False),
    Case("2^21+1", (1 << 21) + 1, "BN254 only: 19-bit digits, pairs of the wide format", _D21, False, False, False),
]

BY_NAME = {c.name: c for c in CASES}


def cases_for(curve_name):
    return [c for c in CASES if curve_name in c.digits]


def lagrange_bases(count, n=N):
    """bases of the second (Lagrange-prefix) table under a key of `count` powers: n + min(count - n, 8)"""
    return n + min(count - n, 8)


# the keys under which commitments of evaluation vectors and the KZG seam are run
COMMIT_EVALS_KEYS = ("n+1", "n+2", "n+9", "4n+1", "2^17+65")      # `n` here is the domain of each log_n, see the test
KZG_SEAM_COUNTS = ((1 << 16) + 65, (1 << 18) + 1)
