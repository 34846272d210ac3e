"""The table of "proofs" for the batch verifier's term stage (zkt_ctx_set_verify_terms, zkt_debug_verify_terms,
zkt_debug_verify_terms_host): tests/test_verify_terms_host.py and tests/test_gpu_verify_terms.py walk it.

The stage replays the transcript and computes scalars; it does no group arithmetic and never checks validity.  So most
rows are fabricated: 13 commitments that are small multiples of g, compressed by the oracle, 12 random canonical
evaluations, random public inputs and roots, ten small multiples of g as the verifier key.  A row is
    Row(name, entry, forced)    entry = (n, key points by PK_ORDER name, pi_roots, public inputs, proof bytes, kind)
with forced = None or the seven integers (beta, gamma, delta, epsilon, alpha, xi, eta) that replace the transcript's
answers.  ROWS(cv) are the unforced rows, FORCED(cv) the forced ones, two_refusals(cv) the batch with two refused proofs."""
import functools
import hashlib
import json
import os
import random
from collections import namedtuple

import numpy as np

from oracle import curve as C, coracle as K

Row = namedtuple("Row", "name entry forced")
CHALLENGES = ("beta", "gamma", "delta", "epsilon", "alpha", "xi", "eta")
OK, ZERO_DENOMINATOR, EQUAL_CHALLENGES = 0, 6, 7
SRC_COUNT = 24


def _nb(cv):
    return (cv.fq.bits + 2 + 7) // 8


@functools.lru_cache(maxsize=None)
def _multiples(cv, count=40):
    g = C.generator(cv)
    out, p = [], None
    for _ in range(count):
        p = C.add(cv, p, g)
        out.append(p)
    return out


def fabricated(cv, seed, n, n_pi, kind="merlin", identity=(), roots=None):
    """One fabricated entry.  identity: which of the 13 commitments are the identity; roots: the public-input roots, or
    None for random ones."""
    rnd = random.Random(1000 * seed + n_pi)
    p = cv.fr.p
    mult = _multiples(cv)
    raw = bytearray()
    for k in range(13):
        raw += bytes(_nb(cv) - 1) + b"\x40" if k in identity else C.point_serialize_compressed(cv, mult[rnd.randrange(len(mult))])
        if k >= 11:
            raw += b"\x00"                                   # Option::None
    for _ in range(12):
        raw += rnd.randrange(p).to_bytes(32, "little")
    import zkt_plonk_amd as z
    key = {name: (None if (seed + i) % 11 == 0 else mult[rnd.randrange(len(mult))]) for i, name in enumerate(z.PK_ORDER)}
    roots = tuple(rnd.randrange(p) for _ in range(n_pi)) if roots is None else tuple(roots)
    assert len(roots) == n_pi
    return (n, key, roots, tuple(rnd.randrange(p) for _ in range(n_pi)), bytes(raw), kind)


def real(cv):
    """The three oracle proofs of tests/test_gpu_verify_batch.py as entries."""
    from test_gpu_verify_batch import _made
    return [(vk.n, vk.commits, tuple(vk.pi_roots), tuple(pis), raw, kind) for vk, pis, raw, kind in _made(cv)[0]]


@functools.lru_cache(maxsize=None)
def ROWS(cv):
    """Unforced rows: every n_pi in 0 .. 12 and 40 (whatever the sponge position after seeding, some row crosses a STROBE
    block edge inside a scalar; n_pi = 0 is an empty message and no inversion), n in {1, 2^4, 2^8, 2^TWO_ADICITY}, an
    identity commitment under both transcript kinds, both kinds mixed on BN254, and the three real proofs."""
    eth = "ethereum" if cv.name == "bn254" else "merlin"
    sizes = [1, 1 << 4, 1 << 8, 1 << cv.fr.two_adicity]
    rows = []
    for j, n_pi in enumerate(list(range(13)) + [40]):
        kind = eth if j % 3 == 1 else "merlin"
        rows.append(Row("pi%d_n%d_%s" % (n_pi, sizes[j % 4].bit_length() - 1, kind), fabricated(cv, 10 + j, sizes[j % 4], n_pi, kind), None))
    rows.append(Row("identity_h1_merlin", fabricated(cv, 40, 1 << 4, 3, "merlin", identity=(4,)), None))
    rows.append(Row("identity_a_qhi_%s" % eth, fabricated(cv, 41, 1 << 8, 2, eth, identity=(0, 10)), None))
    rows.append(Row("identity_all_merlin", fabricated(cv, 42, 1 << 4, 1, "merlin", identity=tuple(range(13))), None))
    rows += [Row("real%d" % i, e, None) for i, e in enumerate(real(cv))]
    return tuple(rows)


def _plain_forced(cv, seed):
    rnd = random.Random(7000 + seed)
    vals = [rnd.randrange(2, cv.fr.p) for _ in range(7)]
    assert len(set(vals[:4])) == 4
    return vals


def _forced_entry(cv, seed, kind="merlin"):
    """n = 16 with public inputs on the domain points w^1, w^2, w^5"""
    w = cv.fr.root_of_unity(16)
    return fabricated(cv, seed, 16, 3, kind, roots=[pow(w, k, cv.fr.p) for k in (1, 2, 5)])


@functools.lru_cache(maxsize=None)
def FORCED(cv):
    """(rows, expected statuses): each of the six equal pairs, xi = 1, xi on a public-input root, xi on the domain but on
    no root (proved: zh = 0), xi = 0, alpha = 0, eta in {0, 1}, and a plain row."""
    p = cv.fr.p
    w = cv.fr.root_of_unity(16)
    eth = "ethereum" if cv.name == "bn254" else "merlin"
    rows, want = [], []

    def put(name, expected, kind="merlin", **over):
        f = _plain_forced(cv, len(rows))
        for k, v in over.items():
            f[CHALLENGES.index(k)] = f[CHALLENGES.index(v)] if isinstance(v, str) else v % p
        rows.append(Row(name, _forced_entry(cv, 60 + len(rows), kind), tuple(f)))
        want.append(expected)

    put("plain", OK)
    for a, b in (("beta", "gamma"), ("beta", "delta"), ("beta", "epsilon"), ("gamma", "delta"), ("gamma", "epsilon"), ("delta", "epsilon")):
        put("%s_eq_%s" % (a, b), EQUAL_CHALLENGES, eth if a == "gamma" else "merlin", **{b: a})
    put("xi_1", ZERO_DENOMINATOR, xi=1)
    put("xi_root", ZERO_DENOMINATOR, eth, xi=pow(w, 2, p))
    put("xi_domain", OK, xi=pow(w, 3, p))
    put("xi_0", OK, eth, xi=0)
    put("alpha_0", OK, alpha=0)
    put("eta_0", OK, eta=0)
    put("eta_1", OK, eth, eta=1)
    return tuple(rows), tuple(want)


@functools.lru_cache(maxsize=None)
def two_refusals(cv):
    """Twelve forced rows: a zero denominator at index 5, equal challenges at index 9, nothing refused below 5."""
    rows = []
    for i in range(12):
        f = _plain_forced(cv, 100 + i)
        if i == 5:
            f[5] = 1
        if i == 9:
            f[1] = f[0]
        rows.append(Row("two_refusals_%d" % i, _forced_entry(cv, 80 + i), tuple(f)))
    want = [OK] * 12
    want[5], want[9] = ZERO_DENOMINATOR, EQUAL_CHALLENGES
    return tuple(rows), tuple(want)


def with_root_on_xi(cv, row):
    """The row with its first public-input root moved onto the xi its own transcript draws.  The roots are not hashed, so xi
    stays where it is and the proof is refused for a zero denominator with nothing forced: a refusal the batch calls
    themselves can be given."""
    from zkt_plonk_amd import _lib
    xi = K.fr_from_mont(cv, _lib.debug_verify_terms_host(cv.name, [item(cv, row)], None, None, 0)[0][0])[5]
    n, key, roots, pis, raw, kind = row.entry
    return Row(row.name + "_root_on_xi", (n, key, (xi,) + tuple(roots[1:]), pis, raw, kind), None)


@functools.lru_cache(maxsize=None)
def two_natural_refusals(cv):
    """Twelve unforced rows, proofs 5 and 9 refused for a zero denominator, nothing refused below 5.  (Equal challenges
    cannot be had without forcing: they would be a collision of the transcript's hash.)"""
    rows = cycle(ROWS(cv), 12)
    rows[5], rows[9] = with_root_on_xi(cv, rows[5]), with_root_on_xi(cv, rows[9])
    return tuple(rows)


def cycle(rows, count):
    return [rows[i % len(rows)] for i in range(count)]


# ---- rows -> the arguments of the entry points ---------------------------------------------------------------------
_ARRAYS = {}


def item(cv, row):
    """One row as an element of `items` (zkt_plonk_amd._lib.verify_batch), with a freshly seeded transcript."""
    import zkt_plonk_amd as z
    n, key, roots, pis, raw, kind = row.entry
    tr = z.Transcript(kind, "ZKT Plonk", fr_bits=cv.fr.bits, fq_bytes=cv.fq.limbs64 * 8)
    z.seed_transcript(tr, n, key)
    k = (cv.name, row.name)
    if k not in _ARRAYS:
        _ARRAYS[k] = (K.points_to_mont(cv, [key[name] for name in z.PK_ORDER]), [key[name] is None for name in z.PK_ORDER],
                      K.fr_to_mont(cv, list(roots)) if roots else np.zeros((0, 4), dtype=np.uint64),
                      K.fr_to_mont(cv, list(pis)) if pis else np.zeros((0, 4), dtype=np.uint64),
                      K.points_to_mont(cv, [C.generator(cv)])[0])
    commits, inf, r, v, g = _ARRAYS[k]
    return (n, commits, inf, r, v, raw, g, tr)


def items(cv, rows):
    return [item(cv, r) for r in rows]


def forced_array(cv, rows):
    """None when no row is forced, else (count, 7, 4) Montgomery words"""
    if all(r.forced is None for r in rows):
        return None
    assert all(r.forced is not None for r in rows)
    return K.fr_to_mont(cv, [v for r in rows for v in r.forced]).reshape(len(rows), 7, 4)


def rho_array(cv, count, seed=5):
    """2 * count coefficients of 128 bits, the first one 1, as canonical words (what the batch verifier draws)"""
    rnd = random.Random(seed)
    vals = [1] + [rnd.randrange(1 << 128) for _ in range(2 * count - 1)]
    return np.array([[(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)] for v in vals], dtype=np.uint64)


def probes(its):
    """a challenge drawn from every transcript of `its`: where each handle was left"""
    return [it[7].challenge_scalar("probe") for it in its]


def same(a, b):
    """two results of debug_verify_terms* are equal, integer for integer"""
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- the results pinned in tests/golden/verify_terms_pinned.json (tests/golden/make_golden_verify_terms.py) ----------
PINNED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "verify_terms_pinned.json")


def pinned_batches(cv):
    """(name, rows, rho) of every pinned batch, with the coefficients the other tests give it"""
    rows, forced = list(ROWS(cv)), list(FORCED(cv)[0])
    return (("rows", rows, rho_array(cv, len(rows))), ("forced", forced, rho_array(cv, len(forced), seed=6)),
            ("two_refusals", list(two_refusals(cv)[0]), None), ("two_natural_refusals", list(two_natural_refusals(cv)), None))


def digests(result, left):
    """per proof the SHA-256 over its status, seven challenges, r0, 24 sums and the handle's probe after the call"""
    ch, r0, acc, status = result
    words = lambda a: np.ascontiguousarray(a, dtype="<u8").tobytes()  # noqa: E731
    return [hashlib.sha256(int(status[i]).to_bytes(4, "little", signed=True) + words(ch[i]) + words(r0[i]) + words(acc[i]) +
                           left[i].to_bytes(32, "little")).hexdigest() for i in range(len(left))]


@functools.lru_cache(maxsize=None)
def pinned():
    return json.load(open(PINNED))
