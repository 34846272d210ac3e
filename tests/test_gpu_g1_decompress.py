"""GPU: zkt_g1_decompress / zkt_g1_decompress_dev, checked deserialisation of compressed arkworks G1 points on the device,
against the CPU oracle (oracle.curve.point_deserialize_compressed, coracle.points_to_mont): exact limbs, exact statuses."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import fields as F, coracle as K, curve as C

CURVES = [F.BN254, F.BLS12_381]
LENGTHS = [0, 1, 63, 64, 65, 520, 4097]       # one lane, a full wave, one past it, several workgroups (13 * 40), a ragged tail
VALID, IDENTITY, NOT_CANONICAL, BOTH_FLAGS, NOT_ON_CURVE, NOT_IN_SUBGROUP = range(6)


@pytest.fixture(scope="module")
def ctxs():
    import zkt_plonk_amd as z
    c = {cv.name: z.Context(cv.name, 0) for cv in CURVES}
    yield c
    for x in c.values():
        x.close()


def _times_r(cv, P):
    """r P (oracle.curve.scalar_mul reduces its scalar mod r, so r - 1 times and once more)"""
    return C.add(cv, C.scalar_mul(cv, cv.fr.p - 1, P), P)


def _nb(cv):
    return (cv.fq.bits + 2 + 7) // 8


def _raw(cv, x, flags=0):
    b = bytearray(int(x).to_bytes(_nb(cv), "little"))
    b[-1] |= flags
    return bytes(b)


@functools.lru_cache(maxsize=None)
def _good(cv):
    """Valid encodings: P_(i+1) = P_i + G for 2100 steps, then the negations.  -> (list of bytes, list of points)"""
    G = C.generator(cv)
    pts, P = [], G
    for _ in range(2100):
        pts.append(P)
        P = C.add(cv, P, G)
    pts += [C.neg(cv, p) for p in pts]
    enc = [C.point_serialize_compressed(cv, p) for p in pts]
    signs = {e[-1] & 0x80 for e in enc[:2100]}
    assert signs == {0, 0x80}, "both root signs must occur among the P_i"
    assert all(C.point_deserialize_compressed(cv, e) == p for e, p in zip(enc[:50], pts[:50]))
    return enc, pts


@functools.lru_cache(maxsize=None)
def _bad(cv):
    """The encodings that are not plain points -> list of (bytes, expected status)"""
    q, nb = cv.fq.p, _nb(cv)
    out = [
        (_raw(cv, 0, 0x40), IDENTITY),                                   # the identity as arkworks writes it
        (_raw(cv, 0x1234567, 0x40), IDENTITY),                           # infinity over a non-zero canonical x: ignored
        (_raw(cv, q + 5, 0x40), NOT_CANONICAL),                          # infinity over x >= q
        (_raw(cv, q), NOT_CANONICAL),
        (_raw(cv, (1 << (8 * nb - 2)) - 1), NOT_CANONICAL),
        (_raw(cv, C.generator(cv)[0], 0xC0), BOTH_FLAGS),
        (_raw(cv, q + 5, 0xC0), BOTH_FLAGS),                             # the flags are judged before x
    ]
    x = 1
    while True:                                                          # the first x whose x^3 + b is a non-residue
        rhs = (x * x * x + cv.b) % q
        if rhs and pow(rhs, (q - 1) // 2, q) != 1:
            break
        x += 1
    out.append((_raw(cv, x), NOT_ON_CURVE))
    out.append((_raw(cv, x, 0x80), NOT_ON_CURVE))
    if cv.name == "bls12_381":
        rng = np.random.default_rng(381)
        found = 0
        while found < 2:
            x = int.from_bytes(rng.bytes(nb), "little") % q
            y = C.sqrt_mod((x * x * x + cv.b) % q, q)
            if y is None:
                continue
            assert C.is_on_curve(cv, (x, y)) and _times_r(cv, (x, y)) is not None   # r P != 0: outside G1
            out.append((_raw(cv, x, 0x80 if found else 0), NOT_IN_SUBGROUP))
            found += 1
    return out


def _cases(cv, n):
    """n encodings: valid points, with the others scattered at the first, last and wave-boundary positions.
    -> (bytes, expected status (n,), expected points (n, 2 limbs))"""
    enc, pts = _good(cv)
    bad = _bad(cv)
    items = [(enc[i % len(enc)], VALID, pts[i % len(enc)]) for i in range(n)]
    spots = sorted({p for p in [0, n - 1] + [w * 64 + d for w in range(1, 8) for d in (-1, 0)] if 0 <= p < n})
    for j, p in enumerate(spots):
        data, st = bad[(j + n) % len(bad)]
        items[p] = (data, st, None)
    status = np.array([st for _, st, _ in items], dtype=np.uint8)
    want = K.points_to_mont(cv, [pt for _, _, pt in items]) if n else np.zeros((0, 2 * cv.fq.limbs64), np.uint64)
    return b"".join(d for d, _, _ in items), status, want


@pytest.mark.parametrize("cv", CURVES, ids=lambda c: c.name)
def test_every_kind_of_encoding_gets_its_status(ctxs, cv):
    """Each special encoding on its own, then all of them in one call: status and point ((0,0) unless valid)."""
    ctx = ctxs[cv.name]
    bad = _bad(cv)
    enc, pts = _good(cv)
    for data, st in bad:
        out, got = ctx.g1_decompress(data)
        assert got.tolist() == [st] and not out.any(), (data.hex(), st)
    out, got = ctx.g1_decompress(b"".join(d for d, _ in bad) + enc[0] + enc[2100])
    assert got.tolist() == [st for _, st in bad] + [VALID, VALID]
    assert not out[:len(bad)].any()
    assert np.array_equal(out[len(bad):], K.points_to_mont(cv, [pts[0], pts[2100]]))
    want = sorted({st for _, st in bad})
    assert want == ([1, 2, 3, 4, 5] if cv.name == "bls12_381" else [1, 2, 3, 4])


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("cv", CURVES, ids=lambda c: c.name)
def test_decompress_matches_the_oracle(ctxs, cv, n):
    ctx = ctxs[cv.name]
    data, status, want = _cases(cv, n)
    if n == 65:                                   # the device form, in place of the host form
        nb, words = _nb(cv), 2 * cv.fq.limbs64
        d_in, d_out, d_st = ctx.alloc(n * nb), ctx.alloc(n * words * 8), ctx.alloc(n)
        try:
            ctx.upload(d_in, np.frombuffer(data, dtype=np.uint8))
            ctx.g1_decompress_dev(d_in, n, d_out, d_st)
            ctx.synchronize()
            out = ctx.download(d_out, (n, words))
            got = ctx.download(d_st, (n,), dtype=np.uint8)
        finally:
            for p in (d_in, d_out, d_st):
                ctx.free(p)
    else:
        out, got = ctx.g1_decompress(data)
    assert out.shape == want.shape and got.shape == status.shape
    assert np.array_equal(got, status), np.nonzero(got != status)[0][:8]
    assert np.array_equal(out, want), np.nonzero((out != want).any(axis=1))[0][:8]


def test_limits_and_errors(ctxs):
    import zkt_plonk_amd as z
    from zkt_plonk_amd import _lib
    ctx = ctxs["bn254"]
    L = z.lib()
    buf = (ctypes.c_uint8 * 64)()
    out = np.zeros(16, dtype=np.uint64)
    st = (ctypes.c_uint8 * 2)()
    u = out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    # the count is judged before any memory is touched
    assert L.zkt_g1_decompress(ctx.handle, buf, _lib.G1_DECOMPRESS_MAX + 1, u, st) == 1
    assert b"ZKT_G1_DECOMPRESS_MAX" in L.zkt_last_error(ctx.handle)
    assert L.zkt_g1_decompress_dev(ctx.handle, None, _lib.G1_DECOMPRESS_MAX + 1, None, None) == 1
    assert L.zkt_g1_decompress(ctx.handle, None, 0, None, None) == 0          # n = 0: ZKT_OK, nothing touched
    assert L.zkt_g1_decompress_dev(ctx.handle, None, 0, None, None) == 0
    assert L.zkt_g1_decompress(None, buf, 1, u, st) == 1
    assert L.zkt_g1_decompress(ctx.handle, None, 1, u, st) == 1
    assert L.zkt_g1_decompress(ctx.handle, buf, 1, None, st) == 1
    assert L.zkt_g1_decompress(ctx.handle, buf, 1, u, None) == 1
    with pytest.raises(ValueError):
        ctx.g1_decompress(b"\0" * 33)
    d = ctx.alloc(256)
    try:
        with pytest.raises(z.ZktError):                                        # a misaligned device buffer is refused
            ctx.g1_decompress_dev(d + 4, 1, d + 64, d + 200)
    finally:
        ctx.free(d)
    # the context still works afterwards
    enc, pts = _good(F.BN254)
    out2, got = ctx.g1_decompress(enc[1])
    assert got.tolist() == [VALID] and np.array_equal(out2, K.points_to_mont(F.BN254, [pts[1]]))
