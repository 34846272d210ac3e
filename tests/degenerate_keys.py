"""Degenerate committer keys: the powers of a trapdoor tau under which the key-derived tables meet the exceptional cases of
the group law (equal bases, opposite bases, bases at infinity), and the honest proofs and verifier keys under them carry
commitments that are the identity.  zkt_srs_load takes every one of them, the reference proves and verifies under them,
and a wrong exceptional branch shows only here.  tests/test_degenerate_keys_oracle.py pins this table on the CPU,
tests/test_gpu_degenerate_keys.py drives the device code with it.

The fixed statement of the table's last two columns: P.synthetic_circuit(cv, 900, 64, seed=12) (n = 1024), a key of n + 8
powers, blinders field_elems(p, 555, NUM_BLINDERS).  Both columns came out the same on BN254 and BLS12-381.

With w the generator of the size-n domain: tau = w^k makes [L_i(tau)] G the identity for every i but k, so the prefix sums
S_1 .. S_k of the Lagrange table are the identity and the rest are all the same point n G (the table keeps 1/n in the
scalars), every blinder point V_j = [tau^(n+j)] G - [tau^j] G is P + (-P), and T_v of a wire is the identity for every
variable that does not stand on row k.  Plain module: no GPU, no library beyond the CPU oracle."""
import functools
from collections import namedtuple

import numpy as np

from oracle import fields as F, curve as C, plonk as P, coracle as K
from helpers import field_elems

CURVES = [F.BN254, F.BLS12_381]
LOG_N = 10
N = 1 << LOG_N
SPARE = 8                      # the keys hold n + 8 powers
GATES, TABLE, SEED, BLINDER_SEED = 900, 64, 12, 555

# tau(cv, n) -> the trapdoor; forces: the exceptional branches the key is there to drive; identity_bases: bases at infinity
# in an (n + 8)-power key; proof_identities / vk_identities: the commitments of the fixed statement that are the identity
Case = namedtuple("Case", "name tau forces identity_bases proof_identities vk_identities in_domain")


def _w(cv, n):
    return cv.fr.root_of_unity(n)


CASES = [
    Case("0", lambda cv, n: 0,
         "k_srs_generate produces identities; the first MSM table is one base and n + 7 identities (k_srs_windows, k_srs_to_fx, "
         "k_msm_accumulate skip them); k_lag_level's u + v and u - v with v the identity on every level, every [L_i] G equal "
         "(k_lag_seg_sum / k_lag_prefix add P + P, then 2P + P ...); V_j the identity for j > 0 and -G for j = 0; every T_v "
         "a multiple of G: a wire table full of equal bases",
         N + SPARE - 1, (), (), False),
    Case("1", lambda cv, n: 1,
         "all bases equal G: every bucket addition of k_msm_accumulate is P + P; k_lag_level's u == v on every butterfly "
         "that is not identity + identity (xyzz_add's doubling branch for u + v, its identity branch for u - v, then the "
         "`!xyzz_is_identity(d)` skip); [L_0] G = n G is the only Lagrange point, so the prefix table is n G throughout "
         "(k_lag_seg_sum / k_lag_prefix add identities); V_j = G - G (xyzz_add_mixed's P == -Q)",
         0, (), ("q_l", "q_r", "q_c", "q_lookup", "q_table"), True),
    Case("-1", lambda cv, n: cv.fr.p - 1,
         "bases G, -G, G, ...: bucket additions are P + P or P + (-P); k_lag_level's u == v on every level but the last "
         "and u == -v (u + v the identity, u - v a doubling) on the last; identity prefix sums S_1 .. S_(n/2) stored into "
         "table2 by xyzz_to_affine; V_j = P - P",
         0, ("t", "h1", "h2"), ("q_m", "q_lookup"), True),
    Case("w", lambda cv, n: _w(cv, n),
         "tau in the domain with no two key bases equal: [L_1] G = n G is the only Lagrange point that is not the identity, "
         "which k_lag_level reaches through scalar multiplications that end at the identity; one identity prefix sum, "
         "then n G; V_j = P - P",
         0, (), ("q_m", "q_c", "q_lookup", "q_table"), True),
    Case("w^(n-1)", lambda cv, n: pow(_w(cv, n), n - 1, cv.fr.p),
         "tau on the last (padding) row: S_1 .. S_(n-1) are the identity, the whole second table but one sum and the "
         "window multiples of identities (msm_table_finish); six honest proof commitments are the identity",
         0, ("a", "b", "c", "t", "h1", "h2"), ("q_m", "q_l", "q_r", "q_o", "q_c", "q_lookup"), True),
    Case("w^5", lambda cv, n: pow(_w(cv, n), 5, cv.fr.p),
         "tau on an early row of the domain: five identity prefix sums, the first segment of k_lag_prefix at 2^13 changes "
         "from the identity to n G inside its loop",
         0, (), ("q_m", "q_lookup", "q_table"), True),
    Case("w_2n", lambda cv, n: cv.fr.root_of_unity(2 * n),
         "tau^n = -1: V_j = [-tau^j] G - [tau^j] G is P + P (xyzz_add_mixed's doubling branch); the key's second half is "
         "minus its first half",
         0, (), (), False),
    Case("w^(n/4)", lambda cv, n: pow(_w(cv, n), n // 4, cv.fr.p),
         "tau of order four: the key is G, [i] G, -G, -[i] G repeated, so buckets and the top levels of k_lag_level see "
         "both P + P and P + (-P); n/4 identity prefix sums",
         0, ("t", "h1", "h2"), ("q_m", "q_c", "q_lookup"), True),
]
BY_NAME = {c.name: c for c in CASES}
IDS = [c.name for c in CASES]
VERIFIER_CASES = [c for c in CASES if c.name != "0"]      # tau = 0: beta_h is the G2 identity, left out of every verifier leg


def tau_of(cv, case, n=N):
    return case.tau(cv, n) % cv.fr.p


def key(cv, case, n=N, spare=SPARE):
    """the (n + spare)-power key of `case` for a domain of size n, Montgomery limbs, identities as (0, 0)"""
    return _key(cv.name, case.name, n, spare).copy()


@functools.lru_cache(maxsize=None)
def _key(cv_name, case_name, n, spare):
    cv = next(c for c in CURVES if c.name == cv_name)
    return K.srs_mont(cv, tau_of(cv, BY_NAME[case_name], n), n + spare)


def identity_bases(srs):
    return int((~srs.any(axis=1)).sum())


def numpy_key(cv, name, count):
    """The keys of tau = 0, 1 and -1 written out without a scalar multiplication: G then identities, G repeated, G and -G
    alternating."""
    G = C.generator(cv)
    g, minus_g = K.points_to_mont(cv, [G, (G[0], cv.fq.p - G[1])])
    out = np.zeros((count, g.shape[0]), dtype=np.uint64)
    if name == "0":
        out[0] = g
    elif name == "1":
        out[:] = g
    elif name == "-1":
        out[0::2] = g
        out[1::2] = minus_g
    else:
        raise KeyError(name)
    return out


NUMPY_KEYS = ("0", "1", "-1")

Statement = namedtuple("Statement", "cs n tau srs pk epk vk blinders proof raw pis")


@functools.lru_cache(maxsize=None)
def _statement(cv_name, case_name):
    cv = next(c for c in CURVES if c.name == cv_name)
    case = BY_NAME[case_name]
    cs = P.synthetic_circuit(cv, GATES, TABLE, seed=SEED)
    n = cs.circuit_bound()
    assert n == N
    srs = _key(cv_name, case_name, n, SPARE)
    be = K.CBackend(cv, srs)
    pk, epk, vk = P.setup(be, [None] * (n + SPARE), cs, True)
    blinders = field_elems(cv.fr.p, BLINDER_SEED, P.NUM_BLINDERS)
    proof = P.prove(be, [None] * (n + SPARE), pk, epk, vk, cs, P.new_seeded_transcript(cv, vk), blinders)
    return Statement(cs, n, tau_of(cv, case, n), srs, pk, epk, vk, blinders, proof, proof.serialize(cv),
                     tuple(cs.pi[k] for k in sorted(cs.pi)))


def statement(cv, case):
    """The fixed circuit set up and proved by the CPU oracle under the key of `case`, once per (curve, case)."""
    return _statement(cv.name, case.name)


def proof_identities(proof):
    return tuple(k for k in P.Proof.COMMIT_ORDER if proof.commits[k] is None)


def vk_identities(vk):
    return tuple(k for k in P.PK_POLYS if vk.commits[k] is None)


def entry(st, raw=None):
    """the statement as an entry of tests/test_gpu_verify_batch.py's batches: (vk, public inputs, proof bytes, transcript kind)"""
    return (st.vk, st.pis, st.raw if raw is None else raw, "merlin")


def item(cv, st, raw=None):
    """the verifier's inputs for the statement: (n, vk commitments, flags, pi roots, public inputs, proof, G, transcript)"""
    import zkt_plonk_amd as z
    tr = z.Transcript("merlin", "ZKT Plonk", fr_bits=cv.fr.bits, fq_bytes=cv.fq.limbs64 * 8)
    z.seed_transcript(tr, st.vk.n, st.vk.commits)
    return (st.vk.n, K.points_to_mont(cv, [st.vk.commits[k] for k in z.PK_ORDER]), [st.vk.commits[k] is None for k in z.PK_ORDER],
            K.fr_to_mont(cv, st.vk.pi_roots), K.fr_to_mont(cv, list(st.pis)), st.raw if raw is None else raw, st.srs[0], tr)


def flip_evaluation(raw):
    bad = bytearray(raw)
    bad[-40] ^= 1
    return bytes(bad)
