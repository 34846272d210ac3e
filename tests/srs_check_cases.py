"""Inputs of the zkt_g1_check / zkt_srs_check tests (tests/test_srs_check_host.py, tests/test_gpu_srs_check.py): uncompressed
G1 points that are not plain points, each with the status the rules of include/zkt_plonk.h give it -- worked out here with
Python integers and oracle.curve, never by the library -- and test keys with their challenge sums."""
import functools

import numpy as np

from oracle import fields as F, coracle as K, curve as C

CURVES = [F.BN254, F.BLS12_381]
VALID, IDENTITY, NOT_CANONICAL, BOTH_FLAGS, NOT_ON_CURVE, NOT_IN_SUBGROUP = range(6)
TAU = 0x7A57E5EED
N_KEY = 257
SEED_A = bytes(range(1, 33))
SEED_B = bytes((7 * i + 3) & 0xFF for i in range(32))


def _times_r(cv, P):
    """r P (oracle.curve.scalar_mul reduces its scalar mod r, so r - 1 times and once more)"""
    return C.add(cv, C.scalar_mul(cv, cv.fr.p - 1, P), P)


def oracle_status(cv, x_raw, y_raw):
    """The status of the point whose limbs hold the integers x_raw, y_raw (Montgomery form when canonical)."""
    q = cv.fq.p
    if x_raw >= q or y_raw >= q:
        return NOT_CANONICAL
    if x_raw == 0 and y_raw == 0:
        return IDENTITY
    P = (cv.fq.from_mont(x_raw), cv.fq.from_mont(y_raw))
    if not C.is_on_curve(cv, P):
        return NOT_ON_CURVE
    if cv.name == "bls12_381" and _times_r(cv, P) is not None:
        return NOT_IN_SUBGROUP
    return VALID


def raw(cv, P):
    """(x, y) canonical -> the integers its Montgomery limbs hold"""
    return (cv.fq.to_mont(P[0]), cv.fq.to_mont(P[1]))


def rows(cv, raws):
    """[(x_raw, y_raw)] -> (n, 2 * limbs) uint64"""
    L = cv.fq.limbs64
    if not raws:
        return np.zeros((0, 2 * L), dtype=np.uint64)
    return K.ints_to_limbs([v for xy in raws for v in xy], L).reshape(len(raws), 2 * L)


@functools.lru_cache(maxsize=None)
def good(cv):
    """P_i = (i + 1) G for i < 130, then their negations -> [(x_raw, y_raw)]; the limbs are those of coracle.points_to_mont."""
    G = C.generator(cv)
    pts, P = [], G
    for _ in range(130):
        pts.append(P)
        P = C.add(cv, P, G)
    pts += [C.neg(cv, p) for p in pts]
    out = [raw(cv, p) for p in pts]
    assert np.array_equal(rows(cv, out), K.points_to_mont(cv, pts))
    return out


def _off_subgroup(cv, count):
    """curve points outside G1, found as tests/test_gpu_g1_decompress.py::_bad finds them"""
    q, nb = cv.fq.p, (cv.fq.bits + 2 + 7) // 8
    rng = np.random.default_rng(381)
    out = []
    while len(out) < count:
        x = int.from_bytes(rng.bytes(nb), "little") % q
        y = C.sqrt_mod((x * x * x + cv.b) % q, q)
        if y is None:
            continue
        assert C.is_on_curve(cv, (x, y)) and _times_r(cv, (x, y)) is not None
        out.append((x, q - y if len(out) else y))
    return out


@functools.lru_cache(maxsize=None)
def bad(cv):
    """The points that are not valid -> [(name, (x_raw, y_raw), status)]; the status is oracle_status's, and the one the
    case was built for."""
    q = cv.fq.p
    pts = good(cv)
    (x5, y5), (x9, y9) = pts[5], pts[9]
    P7 = (cv.fq.from_mont(pts[7][0]), cv.fq.from_mont(pts[7][1]))
    assert x5 + q < 1 << (64 * cv.fq.limbs64) and y5 + q < 1 << (64 * cv.fq.limbs64)      # both fit the limb width
    x = 2
    while True:                                                   # a point of y^2 = x^3 + b + 1
        y = C.sqrt_mod((x * x * x + cv.b + 1) % q, q)
        if y:
            break
        x += 1
    other_b = (x, y)
    assert not C.is_on_curve(cv, other_b) and not C.is_on_curve(cv, (P7[0], (P7[1] + 1) % q))
    out = [
        ("identity", (0, 0), IDENTITY),
        ("x + q", (x5 + q, y5), NOT_CANONICAL),
        ("y + q", (x5, y5 + q), NOT_CANONICAL),
        ("x = q", (q, y9), NOT_CANONICAL),
        ("y + 1", raw(cv, (P7[0], (P7[1] + 1) % q)), NOT_ON_CURVE),
        ("another b", raw(cv, other_b), NOT_ON_CURVE),
        ("x + q and y off the curve", (x9 + q, raw(cv, (P7[0], (P7[1] + 1) % q))[1]), NOT_CANONICAL),
    ]
    if cv.name == "bls12_381":
        out += [("outside G1 #%d" % k, raw(cv, P), NOT_IN_SUBGROUP) for k, P in enumerate(_off_subgroup(cv, 2))]
    for name, xy, st in out:
        assert oracle_status(cv, *xy) == st, name
    return out


def by_status(cv):
    """one bad point per status that can occur -> {status: (x_raw, y_raw)}"""
    out = {}
    for _, xy, st in bad(cv):
        out.setdefault(st, xy)
    return out


def spots(n):
    """the first and last index and both sides of every wave boundary below 512"""
    return sorted({p for p in [0, n - 1] + [w * 64 + d for w in range(1, 8) for d in (-1, 0, 1)] if 0 <= p < n})


def scattered(cv, n, rot=0):
    """n points: the valid ones in turn, the bad ones at spots(n), rotated by `rot` -> ((n, 2 limbs) uint64, status (n,))"""
    g, b = good(cv), bad(cv)
    raws = [g[i % len(g)] for i in range(n)]
    status = [VALID] * n
    for j, p in enumerate(spots(n)):
        _, xy, st = b[(j + rot) % len(b)]
        raws[p], status[p] = xy, st
    return rows(cv, raws), np.array(status, dtype=np.uint8)


# ---- keys -------------------------------------------------------------------------------------------------------------
def rho_of(cv, seed):
    return int.from_bytes(seed, "little") % cv.fr.p


@functools.lru_cache(maxsize=None)
def key_points(cv, tau=TAU, count=N_KEY):
    return C.srs_powers(cv, tau, count)


@functools.lru_cache(maxsize=None)
def key(cv, tau=TAU, count=N_KEY):
    """oracle.curve.srs_powers as Montgomery limbs (read-only: callers copy before editing)"""
    k = K.points_to_mont(cv, key_points(cv, tau, count))
    k.setflags(write=False)
    return k


@functools.lru_cache(maxsize=None)
def long_key(cv, count):
    """The same key continued past N_KEY by coracle.srs_mont (srs_powers walks every power in Python: seconds per
    thousand); the two agree on the N_KEY powers both make."""
    k = K.srs_mont(cv, TAU, count)
    assert np.array_equal(k[:N_KEY], key(cv))
    k.setflags(write=False)
    return k


def challenge_sum(cv, pts_mont, rho):
    """S = sum_i rho^i P_i by coracle's Pippenger -> (xy limbs, is_infinity)"""
    n = pts_mont.shape[0]
    pw, p = [], 1
    for _ in range(n):
        pw.append(p)
        p = p * rho % cv.fr.p
    return K.msm_mont(cv, pts_mont, K.fr_to_mont(cv, pw), True)


def double_point(cv, pts_mont, k):
    """a copy with P_k replaced by 2 P_k"""
    out = pts_mont.copy()
    P = K.points_from_mont(cv, pts_mont[k:k + 1])[0]
    out[k] = K.points_to_mont(cv, [C.double(cv, P)])[0]
    return out
