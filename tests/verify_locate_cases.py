"""Batches for zkt_verify_batch_locate (tests/test_verify_locate_host.py, tests/test_gpu_verify_locate.py): the three
oracle proofs of tests/test_gpu_verify_batch.py cycled to a count, some of them made bad in a well-formed way (the host
verifier takes every one of them through zkt_verify_prepare without an error and rejects it), and the tree such a batch
must give, put together from the host verifier's own pairs."""
import functools

import numpy as np

from test_gpu_verify_batch import _made, _item, _items, _cycle  # noqa: F401


def _nb(cv):
    return (cv.fq.bits + 2 + 7) // 8


def _commitment_at(cv, k):
    """byte offset of commitment k in a proof (a one-byte Option follows commitments 11 and 12)"""
    return k * _nb(cv) + (1 if k == 12 else 0)


def _with_identities(cv, proof, which):
    raw = bytearray(proof)
    for k in which:
        at = _commitment_at(cv, k)
        raw[at:at + _nb(cv)] = bytes(_nb(cv) - 1) + b"\x40"
    return bytes(raw)


def flipped(cv, e):
    """a flipped evaluation byte"""
    raw = bytearray(e[2])
    raw[-40] ^= 1
    return e[:2] + (bytes(raw),) + e[3:]


def pi_plus_one(cv, e):
    """a public input plus one"""
    return (e[0], ((e[1][0] + 1) % cv.fr.p,) + e[1][1:]) + e[2:]


def h1_identity(cv, e):
    """the identity encoding at h1"""
    return e[:2] + (_with_identities(cv, e[2], [4]),) + e[3:]


def witnesses_identity(cv, e):
    """the identity encoding at both opening witnesses: Q_i is the identity"""
    return e[:2] + (_with_identities(cv, e[2], [11, 12]),) + e[3:]


def all_identity(cv, e):
    """the identity encoding at all 13 commitments"""
    return e[:2] + (_with_identities(cv, e[2], range(13)),) + e[3:]


KINDS = [flipped, pi_plus_one, h1_identity, witnesses_identity, all_identity]


def swapped(a, b):
    """two proofs swapped between their statements"""
    return a[:2] + b[2:], b[:2] + a[2:]


def batch(cv, count, bad):
    """`count` entries, those at the positions `bad` made bad: one kind after the other, and two neighbours of a set of
    even size swapped between their statements in place of the last two kinds."""
    made = _made(cv)[0]
    entries = _cycle(made, count)
    bad = sorted(bad)
    singles = bad
    if len(bad) >= 2 and len(bad) % 2 == 0:
        i, j = bad[-2:]
        entries[i], entries[j] = swapped(entries[i], entries[j])
        singles = bad[:-2]
    for n, i in enumerate(singles):
        entries[i] = KINDS[(n + count) % len(KINDS)](cv, entries[i])
    return entries


def mixed_batch(cv, count):
    """Every kind of bad proof that fits into `count` entries, the identity cases first -> (entries, bad positions)."""
    made = _made(cv)[0]
    entries = _cycle(made, count)
    bad = set()
    for i, kind in enumerate([all_identity, witnesses_identity, h1_identity, flipped, pi_plus_one]):
        if i < count:
            entries[i] = kind(cv, entries[i])
            bad.add(i)
    if count >= 8:
        entries[6], entries[7] = swapped(entries[6], entries[7])
        bad |= {6, 7}
    return entries, bad


_VERDICTS = {}
_PAIRS = {}


def _key(cv, e, extra=()):
    return (cv.name, id(e[0]), e[1], e[2], e[3]) + tuple(extra)


def verdict(cv, e, beta_h):
    """zkt_verify on one entry"""
    from zkt_plonk_amd import _lib
    h = _made(cv)[2]
    k = _key(cv, e, (beta_h.tobytes(),))
    if k not in _VERDICTS:
        it = _item(cv, e)
        _VERDICTS[k] = _lib.verify(cv.name, *it[:7], h, beta_h, it[7])
    return _VERDICTS[k]


def pairs(cv, e):
    """zkt_verify_prepare's (L1, W1, L2, W2) and flags for one entry"""
    from zkt_plonk_amd import _lib
    k = _key(cv, e)
    if k not in _PAIRS:
        it = _item(cv, e)
        _PAIRS[k] = _lib.verify_prepare(cv.name, *it[:7], it[7])
    return _PAIRS[k]


def levels(count):
    sizes = [count]
    while sizes[-1] > 1:
        sizes.append((sizes[-1] + 1) // 2)
    return sizes


def bound(count, n_bad):
    """the most pairing checks a call may make"""
    return 1 + 2 * n_bad * max(count - 1, 0).bit_length()


def check_tree(cv, entries, tree):
    """Every leaf is the host MSM over that proof's zkt_verify_prepare pairs with the returned rho, every inner node the host
    sum of its children, an unpaired node its child, and the flags say which nodes are the identity."""
    from zkt_plonk_amd import _lib
    nodes, inf, rho = tree
    count = len(entries)
    sizes = levels(count)
    assert nodes.shape[:2] == (2, sum(sizes)) and inf.shape == (2, sum(sizes)) and rho.shape == (2 * count, 4)
    assert rho[0].tolist() == [1, 0, 0, 0] and not rho[:, 2:].any()
    for i, e in enumerate(entries):
        pr, _ = pairs(cv, e)
        for half, idx in ((0, [0, 2]), (1, [1, 3])):
            want, want_inf = _lib.g1_msm_host(cv.name, pr[idx], rho[2 * i:2 * i + 2], montgomery=False)
            assert np.array_equal(nodes[half, i], want), (i, half)
            assert bool(inf[half, i]) == bool(want_inf), (i, half)
    at = 0
    for l in range(len(sizes) - 1):
        up = at + sizes[l]
        for m in range(sizes[l + 1]):
            for half in range(2):
                kids = nodes[half, at + 2 * m:min(at + 2 * m + 2, up)]
                want, want_inf = _lib.g1_sum_host(cv.name, kids)
                assert np.array_equal(nodes[half, up + m], want), (l, m, half)
                assert bool(inf[half, up + m]) == bool(want_inf), (l, m, half)
        at = up
    assert not nodes[inf].any()                         # an identity node comes back as (0, 0)


@functools.lru_cache(maxsize=None)
def host_reference(cv, count):
    """The mixed batch of `count` proofs through the host entry, once -> (entries, bad, (accepted, out_bad, n_checks, tree))"""
    from zkt_plonk_amd import _lib
    made, srs, h, beta_h, wrong = _made(cv)
    entries, bad = mixed_batch(cv, count)
    return entries, bad, _lib.debug_verify_locate_host(cv.name, _items(cv, entries), h, beta_h)
