"""Host arithmetic of the quotient on three classes of the 4n coset (csrc/quotient_classes.hpp through
zkt_debug_quotient_classes_host; no device): the constants of the 3 x 3 combination and the six top coefficients u formed
from windows of 14 coefficients, against the oracle's polynomial arithmetic (oracle/ntt.py) at n = 8 and 16, where the
degree bounds behind the windows are tight."""
import random

import numpy as np
import pytest

from oracle import coracle as K, fields as F
from oracle.ntt import Domain, trim
from zkt_plonk_amd import _lib

CURVES = [F.BN254, F.BLS12_381]
K1, K2 = 7, 13


def _mul(f, a, b):
    d = Domain(f, 1 << (len(a) + len(b)).bit_length())
    ea, eb = d.fft(a), d.fft(b)
    return d.ifft([x * y % f.p for x, y in zip(ea, eb)])[:len(a) + len(b) - 1]


def _add(f, *ps):
    out = [0] * max(len(q) for q in ps)
    for q in ps:
        for i, v in enumerate(q):
            out[i] = (out[i] + v) % f.p
    return out


def _scale(f, a, s):
    return [v * s % f.p for v in a]


def _shifted(f, a, w):   # a(wX)
    return [v * pow(w, i, f.p) % f.p for i, v in enumerate(a)]


def _window(n, a):
    a = list(a) + [0] * (n + 8 - len(a))
    return a[n - 6:n + 8]


def _consts(cv, log_n):
    z = np.zeros((10, 14, 4), dtype=np.uint64)
    _, consts = _lib.quotient_classes_host(cv.name, log_n, z, np.zeros((3, 4), dtype=np.uint64))
    c = K.fr_from_mont(cv, consts)
    return c[0:4], [c[4 + 3 * k:7 + 3 * k] for k in range(3)], c[13:16]


@pytest.mark.parametrize("log_n", [3, 4])
@pytest.mark.parametrize("cv", CURVES, ids=lambda c: c.name)
def test_constants(cv, log_n):
    f, n = cv.fr, 1 << log_n
    p = f.p
    gamma, vinv, g3 = _consts(cv, log_n)
    d4 = Domain(f, 4 * n)
    for j in range(4):   # X^n on the class of the coset point g w_4n^j
        assert gamma[j] == pow(f.generator * d4.element(j) % p, n, p)
        assert gamma[j] == pow(f.generator * d4.element(j + 4 * 3) % p, n, p)
    for k in range(3):   # vinv times the Vandermonde matrix (gamma_j^m) is the identity
        for m in range(3):
            assert sum(vinv[k][j] * pow(gamma[j], m, p) for j in range(3)) % p == (1 if k == m else 0)
    assert g3 == [pow(gamma[3], e, p) for e in (1, 2, 3)]
    # Z3 = (X^n - gamma_0)(X^n - gamma_1)(X^n - gamma_2) in Y = X^n
    z3 = [1]
    for j in range(3):
        z3 = _add(f, [0] + z3, _scale(f, z3, -gamma[j] % p))
    assert z3 == [g3[2], g3[1], g3[0], 1]
    # a polynomial of 3n + 6 coefficients from its remainders modulo X^n - gamma_j and its six top coefficients
    rng = random.Random(log_n)
    t = [rng.randrange(p) for _ in range(3 * n + 6)]
    E = [[sum(t[i + m * n] * pow(gamma[j], m, p) for m in range(4) if i + m * n < len(t)) % p for i in range(n)] for j in range(3)]
    u = t[3 * n:]
    got = [0] * (4 * n)
    for i in range(n):
        T = [sum(vinv[k][j] * E[j][i] for j in range(3)) % p for k in range(3)]
        ui = u[i] if i < 6 else 0
        got[i] = (T[0] + ui * g3[2]) % p
        got[n + i] = (T[1] + ui * g3[1]) % p
        got[2 * n + i] = (T[2] + ui * g3[0]) % p
        got[3 * n + i] = ui
    assert got == t + [0] * (n - 6)


@pytest.mark.parametrize("trimmed", [False, True], ids=["dense", "b-trimmed"])
@pytest.mark.parametrize("log_n", [3, 4])
@pytest.mark.parametrize("cv", CURVES, ids=lambda c: c.name)
def test_top_coefficients(cv, log_n, trimmed):
    f, n = cv.fr, 1 << log_n
    p = f.p
    rng = random.Random(100 * log_n + trimmed)
    rnd = lambda k: [rng.randrange(p) for _ in range(k)]
    # degrees as the prover has them: wires n + 1, z1 z2 h1 n + 2, h2 n + 1, keys and t n - 1
    a, b, c = rnd(n + 2), rnd(n + 2), rnd(n + 2)
    if trimmed:
        b = rnd(3)   # a constant wire: its polynomial is trimmed and its blinders sit low
    z1, z2, h1, h2, t = rnd(n + 3), rnd(n + 3), rnd(n + 3), rnd(n + 2), rnd(n)
    s1, s2, s3, ql = rnd(n), rnd(n), rnd(n), rnd(n)
    qm, qlft, qr, qo, qc, qt, pi, l1 = (rnd(n) for _ in range(8))
    alpha, beta, gamma, delta, eps = rnd(5)
    w = Domain(f, n).element(1)
    mul = lambda *ps: _mul(f, ps[0], mul(*ps[1:])) if len(ps) > 1 else ps[0]
    opd = (1 + delta) % p
    eopd = eps * opd % p
    # the numerator of quotient_poly.rs:98-224, term by term
    gate = _add(f, mul(a, b, qm), mul(a, qlft), mul(b, qr), mul(c, qo), qc, pi)
    p1 = mul(z1, _add(f, a, [gamma, beta]), _add(f, b, [gamma, beta * K1 % p]), _add(f, c, [gamma, beta * K2 % p]))
    p2 = mul(_shifted(f, z1, w), _add(f, a, _scale(f, s1, beta), [gamma]), _add(f, b, _scale(f, s2, beta), [gamma]),
             _add(f, c, _scale(f, s3, beta), [gamma]))
    k1 = mul(z2, _add(f, [eps], mul(c, ql)), _add(f, [eopd], t, _scale(f, _shifted(f, t, w), delta)))
    k2 = mul(_shifted(f, z2, w), _add(f, [eopd], h1, _scale(f, h2, delta)), _add(f, [eopd], h2, _scale(f, _shifted(f, h1, w), delta)))
    one_less = lambda z: _add(f, z, [p - 1])
    num = _add(f, gate, _scale(f, p1, alpha), _scale(f, p2, -alpha % p), _scale(f, k1, pow(alpha, 3, p) * opd % p),
               _scale(f, k2, -pow(alpha, 3, p) % p), _scale(f, mul(one_less(z1), l1), pow(alpha, 2, p)),
               _scale(f, mul(one_less(z2), l1), pow(alpha, 4, p)), _scale(f, mul(t, qt), pow(alpha, 5, p)))
    num = num + [0] * (4 * n + 6 - len(num))
    assert len(trim(num)) <= 4 * n + 6
    want = num[4 * n:4 * n + 6]
    windows = K.fr_to_mont(cv, sum((_window(n, q) for q in (a, b, c, z1, z2, t, s1, s2, s3, ql)), [])).reshape(10, 14, 4)
    u, _ = _lib.quotient_classes_host(cv.name, log_n, windows, K.fr_to_mont(cv, [alpha, beta, delta]))
    assert K.fr_from_mont(cv, u) == want
    if not trimmed:
        assert want[5] != 0   # the bound is tight: degree 4n + 5
