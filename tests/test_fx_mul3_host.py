"""CPU: fx_mul3_inl (csrc/fx.hpp), the three-product Montgomery sum behind the closing pass of the classes route, at its
stated bounds against Python big integers, beside tests/test_fx_contracts_host.py.  zkt_host_fx_op carries four operands per
record and its list of operations is closed, so the function runs in a small host program of its own (tests/fx_mul3_host.hip,
compiled for the host only), fed through standard input.

Contract (fx.hpp): limbs < 2^29, a b + c d + e f < R' p  ->  normalised limbs, value < 2p, value = sum / R' mod p.
The column bound (3 L operand products, L reduction products and a carry under 2^64) does not depend on the values: with
every limb of every operand at 2^29 - 1 the result is still the exact (sum + m p) / R' with m < R'."""
import importlib.util
import math
import os
import random
import subprocess

import pytest

from oracle import fields as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 29
FIELDS = [(0, F.BN254.fr, 8), (1, F.BLS12_381.fr, 8), (2, F.BN254.fq, 8), (3, F.BLS12_381.fq, 12)]   # id, field, 32-bit words


def _limbs_count(words):
    return (32 * words + 28) // 29


def _split(v, L):
    """normalised limbs of v < 2^(29 L + 3): the top limb keeps the excess"""
    out = [(v >> (B * i)) & ((1 << B) - 1) for i in range(L - 1)]
    top = v >> (B * (L - 1))
    assert top < (1 << 32)
    return out + [top]


def _value(limbs):
    return sum(int(x) << (B * i) for i, x in enumerate(limbs))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    spec = importlib.util.spec_from_file_location("zkt_build", os.path.join(ROOT, "zkt-plonk_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    exe = str(tmp_path_factory.mktemp("fx_mul3") / "fx_mul3_host")
    r = subprocess.run([b.CLANG, "-x", "hip", "--cuda-host-only", "-I/opt/rocm/include", "-O1", "-std=c++17", "-Wno-psabi",
                        os.path.join(ROOT, "tests", "fx_mul3_host.hip"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]

    def run(fid, L, records):
        text = "".join("%d %s\n" % (fid, " ".join(str(x) for op in rec for x in op)) for rec in records)
        r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        rows = [[int(x) for x in line.split()] for line in r.stdout.splitlines()]
        assert len(rows) == len(records) and all(len(row) == L for row in rows)
        return rows
    return run


def _operands(p, L, rnd):
    """Six-tuples of values with a b + c d + e f < R' p: canonical ones and their edges, every product at a third of the
    bound, one product taking nearly all of it, lazily reduced operands (8p times 8p fits three times over for these
    fields only where 192 p < R': checked, not assumed)."""
    Rp = 1 << (B * L)
    bound = Rp * p
    third = math.isqrt(bound // 3)
    top = min(math.isqrt(bound) - 1, Rp - 1)
    out = [(0,) * 6, (p - 1,) * 6, (1, 1, 0, 0, 0, 0), (0, 0, 0, 0, p - 1, p - 1), (third,) * 6, (top, top, 0, 0, 0, 0),
           (0, 0, top, top, 0, 0), (0, 0, 0, 0, top, top), (top, top, 1, p - 1, 0, 5)]
    if 3 * 64 * p < Rp:
        out.append((8 * p - 1,) * 6)
    for _ in range(200):
        out.append(tuple(rnd.randrange(p) for _ in range(6)))
    for _ in range(100):
        out.append(tuple(rnd.randrange(third + 1) for _ in range(6)))
    for t in out:
        assert t[0] * t[1] + t[2] * t[3] + t[4] * t[5] < bound and max(t) < Rp
    return out


@pytest.mark.parametrize("fid,f,words", FIELDS, ids=lambda x: getattr(x, "name", str(x)))
def test_three_products_share_one_reduction_within_the_stated_bound(fid, f, words, driver):
    p, L = f.p, _limbs_count(words)
    Rp = 1 << (B * L)
    rnd = random.Random("fx_mul3/%d" % fid)
    tuples = _operands(p, L, rnd)
    rows = driver(fid, L, [[_split(v, L) for v in t] for t in tuples])
    rinv = pow(Rp, -1, p)
    for t, row in zip(tuples, rows):
        s = t[0] * t[1] + t[2] * t[3] + t[4] * t[5]
        got = _value(row)
        assert all(x < (1 << B) for x in row[:-1]), t
        assert got < 2 * p, (t, got)
        assert got % p == s * rinv % p, t


@pytest.mark.parametrize("fid,f,words", FIELDS, ids=lambda x: getattr(x, "name", str(x)))
def test_a_column_of_full_limbs_stays_below_64_bits(fid, f, words, driver):
    """Every limb at 2^29 - 1 (and random full-width limbs): the values are far outside a b + c d + e f < R' p, so the result
    is not below 2p, but every column sum is at its largest: had one wrapped, (sum + m p) / R' would not come out exact."""
    p, L = f.p, _limbs_count(words)
    Rp = 1 << (B * L)
    full = [(1 << B) - 1] * L
    rnd = random.Random("fx_mul3 columns/%d" % fid)
    recs = [[full] * 6]
    for _ in range(50):
        recs.append([[rnd.randrange(1 << B) | (1 << (B - 1)) for _ in range(L)] for _ in range(6)])
    rows = driver(fid, L, recs)
    rinv = pow(Rp, -1, p)
    for rec, row in zip(recs, rows):
        v = [_value(op) for op in rec]
        s = v[0] * v[1] + v[2] * v[3] + v[4] * v[5]
        got = _value(row)
        assert got % p == s * rinv % p
        assert s // Rp <= got < s // Rp + p + 1          # (s + m p) / R' with 0 <= m < R'
