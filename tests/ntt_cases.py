"""Structured inputs of the four transforms (fft, ifft, coset_fft, coset_ifft) at the values where the pass kernels' lazy
reduction can go wrong: exact zeros (a difference u - v with u == v is carried as 4p through a Shoup product), operands
at the top of their range (p - 1, values within 8 of p), and outputs that are zero everywhere but one place or over a
long run -- what the prover's inverse transform of a low-degree evaluation vector produces.  Shared by the CPU check of
the oracle (test_ntt_cases_oracle.py) and the device test (test_gpu_ntt_structured.py).

Every generator takes (cv, log_n, variant) and returns a Case: the input as canonical integers, the expected output in
closed form where one exists (never taken from the oracle's transform of that input), and the number of output entries
the case claims to be exactly zero.  w is the domain's root, g the coset generator, R1 * S1 = n the default first-pass
split of the device transform."""
from collections import namedtuple

import numpy as np

from oracle import coracle as K

VARIANTS = (("fft", 0, 0), ("ifft", 1, 0), ("coset_fft", 0, 1), ("coset_ifft", 1, 1))
FORWARD = ("fft", "coset_fft")

Case = namedtuple("Case", "input expected zeros")   # expected: n integers or None; zeros: a count or None


def default_split(log_n: int):
    """The device's pass radices (csrc/ntt.hip split_log_n): none up to 2^10, two passes up to 2^16, three above."""
    if log_n <= 10:
        return []
    p = 2 if log_n <= 16 else 3
    return [log_n // p + (1 if i < log_n % p else 0) for i in range(p)]


def first_pass(log_n: int):
    """(R1, S1); sizes the single-workgroup kernel serves are given the balanced two-way split."""
    sp = default_split(log_n)
    log_r1 = sp[0] if sp else (log_n + 1) // 2
    return 1 << log_r1, 1 << (log_n - log_r1)


def _powers(base: int, count: int, p: int, scale: int = 1):
    out, x = [], scale % p
    for _ in range(count):
        out.append(x)
        x = x * base % p
    return out


def _characters(cv, log_n, variant, terms):
    """Output of x_j = sum a w^(j e) over terms (a, e): n a at -e (fft), a at e (ifft), a g^-e at e (coset_ifft)."""
    f, n = cv.fr, 1 << log_n
    if variant == "coset_fft":
        return None
    out = [0] * n
    for a, e in terms:
        e %= n
        if variant == "fft":
            out[-e % n] = (out[-e % n] + n * a) % f.p
        elif variant == "ifft":
            out[e] = (out[e] + a) % f.p
        else:
            out[e] = (out[e] + a * pow(f.inv(f.generator), e, f.p)) % f.p
    return out


def _constant(c):
    def gen(cv, log_n, variant):
        n, v = 1 << log_n, c % cv.fr.p
        exp = _characters(cv, log_n, variant, [(v, 0)]) if v else [0] * n
        return Case([v] * n, exp, None if exp is None else (n - 1 if v else n))
    return gen


def _plus_minus_one(cv, log_n, variant):
    n, p = 1 << log_n, cv.fr.p
    exp = _characters(cv, log_n, variant, [(1, n // 2)])             # (-1)^j = w^(j n/2)
    return Case([1, p - 1] * (n // 2), exp, None if exp is None else n - 1)


def _zero_max(cv, log_n, variant):
    n, p = 1 << log_n, cv.fr.p
    half = cv.fr.inv(2)
    exp = _characters(cv, log_n, variant, [(p - half, 0), (half, n // 2)])   # -(1 - (-1)^j) / 2
    return Case([0, p - 1] * (n // 2), exp, None if exp is None else n - 2)


def _delta(which):
    def gen(cv, log_n, variant):
        f, n = cv.fr, 1 << log_n
        s1 = first_pass(log_n)[1]
        j = {"0": 0, "1": 1, "S1-1": s1 - 1, "S1": s1, "n/2": n // 2, "n-1": n - 1}[which]
        x = [0] * n
        x[j] = 1
        w, g = f.root_of_unity(n), f.generator
        if variant == "fft":                       # w^(jk)
            exp = _powers(pow(w, j, f.p), n, f.p)
        elif variant == "coset_fft":               # g^j w^(jk)
            exp = _powers(pow(w, j, f.p), n, f.p, pow(g, j, f.p))
        elif variant == "ifft":                    # w^(-jk) / n
            exp = _powers(pow(f.inv(w), j, f.p), n, f.p, f.inv(n))
        else:                                      # g^-k w^(-jk) / n
            exp = _powers(pow(f.inv(w), j, f.p) * f.inv(g) % f.p, n, f.p, f.inv(n))
        return Case(x, exp, None)
    return gen


def _geometric(which):
    def gen(cv, log_n, variant):
        f, n = cv.fr, 1 << log_n
        r1 = first_pass(log_n)[0]
        k = {"0": 0, "1": 1, "R1": r1 % n, "n/2+1": (n // 2 + 1) % n, "n-1": n - 1}[which]
        w, g = f.root_of_unity(n), f.generator
        wk = pow(w, k, f.p)
        if variant == "fft":                       # w^(-jk): n at k
            x, val = _powers(f.inv(wk), n, f.p), n % f.p
        elif variant == "coset_fft":               # (g w^k)^-j: n at k
            x, val = _powers(f.inv(g * wk % f.p), n, f.p), n % f.p
        elif variant == "ifft":                    # w^(jk): 1 at k
            x, val = _powers(wk, n, f.p), 1
        else:                                      # g^k w^(jk): 1 at k
            x, val = _powers(wk, n, f.p, pow(g, k, f.p)), 1
        exp = [0] * n
        exp[k] = val
        return Case(x, exp, n - 1)
    return gen


def _random_ints(seed, count, p):
    rng = np.random.default_rng(seed)
    return [int.from_bytes(rng.bytes(40), "little") % p for _ in range(count)]


def _low_degree(cv, log_n, variant):
    """n/4 + 3 random coefficients (the prover's n + 3 on 4n).  The inverse variants are handed their evaluations on the
    domain / the coset (computed with the oracle's FORWARD transform) and must return the coefficients and 3n/4 - 3 exact
    zeros; the forward variants are handed the coefficients as a ragged input."""
    n, p = 1 << log_n, cv.fr.p
    coeffs = _random_ints(0x10DE6 + log_n, n // 4 + 3, p)
    if variant in FORWARD:
        return Case(coeffs, None, None)
    evals = K.fr_from_mont(cv, K.ntt_mont(cv, log_n, 0, variant == "coset_ifft", K.fr_to_mont(cv, coeffs)))
    return Case(evals, coeffs + [0] * (n - len(coeffs)), n - len(coeffs))


def _periodic(which):
    def gen(cv, log_n, variant):
        f, n = cv.fr, 1 << log_n
        r1 = first_pass(log_n)[0]
        m = {"2": 2, "32": 32, "R1": r1}[which]
        if m > n:
            return None
        y = _random_ints(0x9E410D + m, m, f.p)
        x = y * (n // m)
        if variant == "coset_fft":
            return Case(x, None, None)
        # x_j = y_(j mod m): the transform lives on the multiples of n/m, where it is the m-point transform of y
        wm = f.root_of_unity(m) if variant == "fft" else f.inv(f.root_of_unity(m))
        wpow = _powers(wm, m, f.p)
        scale = (n // m) % f.p if variant == "fft" else f.inv(m)
        exp = [0] * n
        ginv = f.inv(f.generator)
        for t in range(m):
            v = sum(y[r] * wpow[r * t % m] for r in range(m)) % f.p * scale % f.p
            if variant == "coset_ifft":
                v = v * pow(ginv, t * (n // m), f.p) % f.p
            exp[t * (n // m)] = v
        return Case(x, exp, n - m)
    return gen


def _near_p(cv, log_n, variant):
    n, p = 1 << log_n, cv.fr.p
    pick = np.random.default_rng(0x2EA59 + log_n).integers(0, 16, size=n)
    return Case([int(v) if v < 8 else p - 16 + int(v) for v in pick], None, None)


GENERATORS = {
    "zeros": _constant(0),
    "ones": _constant(1),
    "all_p_minus_1": _constant(-1),
    "plus_minus_one": _plus_minus_one,
    "zero_max": _zero_max,
    "low_degree": _low_degree,
    "near_p": _near_p,
}
GENERATORS.update({"delta_" + j: _delta(j) for j in ("0", "1", "S1-1", "S1", "n/2", "n-1")})
GENERATORS.update({"geometric_" + k: _geometric(k) for k in ("0", "1", "R1", "n/2+1", "n-1")})
GENERATORS.update({"periodic_" + m: _periodic(m) for m in ("2", "32", "R1")})

ALL_CASES = tuple(GENERATORS)
# 2^17 and above: the host's big-integer lists dominate the time, so a part of the list only
LARGE_CASES = ("all_p_minus_1", "plus_minus_one", "delta_S1", "geometric_R1", "geometric_n/2+1", "low_degree", "near_p")
LARGE_FROM = 17


def case_names(log_n: int):
    return LARGE_CASES if log_n >= LARGE_FROM else ALL_CASES


def make(cv, log_n: int, variant: str, name: str):
    """The named Case; None only from a periodic case whose period is longer than n."""
    return GENERATORS[name](cv, log_n, variant)
