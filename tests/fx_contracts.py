"""Contracts of the limb arithmetic in zkt-plonk_amd/csrc/fx.hpp and ecx.hpp, as plain Python big integers.

One row per routine (and per call site whose margin is tight): the bound each operand must meet, as a value bound and
a bound on limbs 0 .. L-2, the bound the result meets, and the line the contract comes from.  The generators build
operands that sit on those bounds: the largest values, the representation with every low limb at its bound, small
residues lifted by the largest multiple of p, random values with limbs pushed up by borrowing, plain random values.
The checks compare the result with the big-integer value and its bounds.  Shared by tests/test_fx_contracts_host.py
(the host build of the routines) and tests/test_gpu_fx_contracts.py (the device build).

Limb layout (L limbs of B bits, R' = 2^(B L) = 2^(32 N + SH)) comes from the library, zkt_debug_fx_layout.

Template instantiations under csrc/ without a row of their own:
    fx_unpack_s<P, 0 / SH>       -- the body of fx_unpack / fx_unpack_shift (rows UNPACK, UNPACK_SHIFT)
    fx_mul_raw, fx_mont_chain*, fx_mont_column, fx_mad_rows*, fx_mad0
                                 -- the bodies of the products (rows MUL .. MUL_SHOUP run them on the device)
    fx_zero, fx_one, fx_const_to_ark, fx_const_from_ark
                                 -- constants, reached through FROM_ARK / TO_ARK and the curve rows
    fx_neg_p_inverse             -- host-only table setup, checked by the MUL_LOW row's caller in tests/test_field_host.py
    fx_load_limbs, fx_shl_sh, fx_shfl, xx_shfl_down, xx_identity, xx_load*, xx_store*
                                 -- memory moves and cross-lane shuffles, no arithmetic
"""
from __future__ import annotations

import random
from dataclasses import dataclass, field
from math import isqrt
from typing import Callable, List, Optional, Sequence

from oracle import curve as C
from oracle import fields as F

# (curve id, which (0 Fr, 1 Fq), field)
FIELDS = [(0, 0, F.BN254_FR), (0, 1, F.BN254_FQ), (1, 0, F.BLS12_381_FR), (1, 1, F.BLS12_381_FQ)]
CURVES = [(0, F.BN254), (1, F.BLS12_381)]


@dataclass
class Fd:
    """A field in limb form."""
    f: F.PrimeField
    which: int
    L: int
    B: int
    SH: int

    @property
    def p(self) -> int:
        return self.f.p

    @property
    def N(self) -> int:              # 32-bit words of the packed form
        return self.f.limbs64 * 2

    @property
    def Rp(self) -> int:             # R' = 2^(B L)
        return 1 << (self.B * self.L)

    @property
    def W(self) -> int:              # words of one fx record (a, b, c, d)
        return 4 * self.L

    def limbs(self, v: int) -> List[int]:
        """normalised limbs of v (the top limb keeps the excess)"""
        m = (1 << self.B) - 1
        out = [(v >> (self.B * i)) & m for i in range(self.L - 1)]
        out.append(v >> (self.B * (self.L - 1)))
        return out

    def value(self, limbs: Sequence[int]) -> int:
        return sum(int(x) << (self.B * i) for i, x in enumerate(limbs))

    def words(self, v: int) -> List[int]:
        return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(self.N)]

    def wvalue(self, words: Sequence[int]) -> int:
        return sum(int(x) << (32 * i) for i, x in enumerate(words[: self.N]))


def p_(k):
    """value < k p (k may be a fraction given as a (num, den) pair)"""
    if isinstance(k, tuple):
        return lambda fd: -(-k[0] * fd.p // k[1])
    return lambda fd: k * fd.p


def le_p(k):
    """value <= k p"""
    return lambda fd: k * fd.p + 1


@dataclass
class Spec:
    """one operand: value < v(fd); limbs 0 .. L-2 < lim(fd); top limb < top(fd); packed: N-word integer, not limbs"""
    v: Callable[[Fd], int]
    lim: Callable[[Fd], int] = lambda fd: 1 << fd.B
    top: Callable[[Fd], int] = lambda fd: 1 << 32
    packed: bool = False


@dataclass
class Out:
    """the result: kind 'exact' (value == expected), 'mod' (value = expected mod p), 'bool' (word 0 = expected);
    value < v(fd); limbs 0 .. L-2 < lim(fd); all_limbs: the top limb < lim too; packed: N words"""
    kind: str
    v: Optional[Callable[[Fd], int]] = None
    lim: Callable[[Fd], int] = lambda fd: 1 << fd.B
    all_limbs: bool = False
    packed: bool = False


@dataclass
class Row:
    name: str
    op: str                 # zkt_fx_op name without the ZKT_FX_ prefix
    src: str                # where the contract is stated
    ins: List[Spec]
    out: Out
    only: Callable[[Fd], bool] = field(default=lambda fd: True)   # fields the row applies to


def _rp_sqrt(fd: Fd) -> int:                 # a, b below this: a b < R' p
    return isqrt(fd.Rp * fd.p)


def _rp_sqrt_half(fd: Fd) -> int:            # a, b, c, d below this: a b + c d < R' p
    return isqrt(fd.Rp * fd.p // 2)


N29 = lambda fd: 1 << fd.B                   # noqa: E731  (a normalised limb)
LAZY3 = lambda fd: 3 << fd.B                 # noqa: E731  fx_sub_lazy's result limbs: < 2^29 + 2^30
NTT_SHOUP_LIMB = lambda fd: int(2 ** 31.33) + 1   # noqa: E731  ntt.hip:88 "limbs < 2^31.33", taken inclusive
SCALAR = lambda fd: fd.which == 0           # noqa: E731
L9 = lambda fd: fd.L <= 9                   # noqa: E731

ROWS: List[Row] = [
    # ---- conversions
    Row("unpack", "UNPACK", "fx.hpp:183", [Spec(lambda fd: 1 << (32 * fd.N), packed=True)], Out("exact", all_limbs=True)),
    Row("unpack_shift", "UNPACK_SHIFT", "fx.hpp:183", [Spec(lambda fd: 1 << (32 * fd.N), packed=True)],
        Out("exact", all_limbs=True)),
    Row("pack", "PACK", "fx.hpp:209", [Spec(lambda fd: 1 << (32 * fd.N))], Out("exact", packed=True)),
    Row("from_ark", "FROM_ARK", "fx.hpp:871", [Spec(p_(1), packed=True)], Out("mod", p_(2))),
    Row("to_ark", "TO_ARK", "fx.hpp:875", [Spec(p_(8))], Out("mod", p_(1), packed=True)),
    Row("normalize", "NORMALIZE", "fx.hpp:227",
        [Spec(lambda fd: (1 << 32) - 16 << (fd.B * (fd.L - 1)), lim=lambda fd: (1 << 32) - 16, top=lambda fd: (1 << 32) - 16)],
        Out("exact")),
    # ---- additive
    Row("add", "ADD", "fx.hpp:243", [Spec(lambda fd: fd.Rp // 2)] * 2, Out("exact")),
    Row("dbl", "DBL", "fx.hpp:336", [Spec(lambda fd: fd.Rp // 2)], Out("exact")),
    Row("sub_1", "SUB_1", "fx.hpp:259", [Spec(p_(16)), Spec(le_p(1))], Out("exact")),
    Row("sub_2", "SUB_2", "fx.hpp:259 / poly.hip:414 (a = d8 < 16p)", [Spec(p_(16)), Spec(le_p(2))], Out("exact")),
    Row("sub_4", "SUB_4", "fx.hpp:259", [Spec(p_(16)), Spec(le_p(4))], Out("exact")),
    Row("sub_8", "SUB_8", "fx.hpp:259", [Spec(p_(16)), Spec(le_p(8))], Out("exact")),
    Row("sub2_6", "SUB2_6", "fx.hpp:318 / ecx.hpp:114 (b + 2c <= 6p)", [Spec(p_(16)), Spec(le_p(2)), Spec(le_p(2))],
        Out("exact")),
    Row("add_lazy", "ADD_LAZY", "fx.hpp:293", [Spec(p_(8))] * 2, Out("exact", lim=lambda fd: 1 << 30, all_limbs=True)),
    Row("add_lazy_2", "ADD_LAZY", "fx.hpp:293 (second level: limbs < 2^31)", [Spec(p_(16), lim=lambda fd: 1 << 30)] * 2,
        Out("exact", lim=lambda fd: 1 << 31, all_limbs=True)),
    Row("sub_lazy_3", "SUB_LAZY_3", "fx.hpp:277", [Spec(p_(8)), Spec(le_p(2))], Out("exact", lim=LAZY3, all_limbs=True)),
    Row("sub_lazy_4", "SUB_LAZY_4", "fx.hpp:277 / ntt.hip:87", [Spec(p_(8)), Spec(le_p(3))],
        Out("exact", lim=LAZY3, all_limbs=True)),
    Row("sub_lazy_5", "SUB_LAZY_5", "fx.hpp:277 / ecx.hpp:119", [Spec(p_(8)), Spec(le_p(4))],
        Out("exact", lim=LAZY3, all_limbs=True)),
    Row("sub_lazy_9", "SUB_LAZY_9", "fx.hpp:277 / ecx.hpp:119", [Spec(p_(8)), Spec(le_p(8))],
        Out("exact", lim=LAZY3, all_limbs=True)),
    Row("sub_lazy_wide_8_30", "SUB_LAZY_WIDE_8_30", "fx.hpp:302 / ntt.hip:88",
        [Spec(p_(8), lim=lambda fd: 1 << 30), Spec(le_p(7), lim=lambda fd: (1 << 30) + 1)],
        Out("exact", lim=lambda fd: 5 << 29, all_limbs=True)),
    # ---- products
    Row("mul_8p", "MUL", "fx.hpp:340", [Spec(p_(8))] * 2, Out("mod", p_(2))),
    Row("mul_rp", "MUL", "fx.hpp:340 (a b < R' p)", [Spec(_rp_sqrt)] * 2, Out("mod", p_(2))),
    Row("mul_lazy", "MUL", "fx.hpp:280 (one operand with limbs < 3 * 2^29)", [Spec(p_(7), lim=LAZY3), Spec(p_(8))],
        Out("mod", p_(2))),
    Row("mul_inl_8p", "MUL_INL", "fx.hpp:340", [Spec(p_(8))] * 2, Out("mod", p_(2))),
    Row("mul_inl_rp", "MUL_INL", "fx.hpp:340 (a b < R' p)", [Spec(_rp_sqrt)] * 2, Out("mod", p_(2))),
    Row("mul_inl_lazy", "MUL_INL", "fx.hpp:280 (one operand with limbs < 3 * 2^29)", [Spec(p_(8)), Spec(p_(7), lim=LAZY3)],
        Out("mod", p_(2))),
    Row("sqr_8p", "SQR", "fx.hpp:340", [Spec(p_(8))], Out("mod", p_(2))),
    Row("sqr_rp", "SQR", "fx.hpp:340 (a a < R' p)", [Spec(_rp_sqrt)], Out("mod", p_(2))),
    Row("sqr_inl_8p", "SQR_INL", "fx.hpp:515", [Spec(p_(8))], Out("mod", p_(2))),
    Row("sqr_inl_rp", "SQR_INL", "fx.hpp:515 (a a < R' p)", [Spec(_rp_sqrt)], Out("mod", p_(2))),
    Row("mul2_inl_rp", "MUL2_INL", "fx.hpp:556 (a b + c d < R' p)", [Spec(_rp_sqrt_half)] * 4, Out("mod", p_(2))),
    Row("mul_shoup", "MUL_SHOUP", "fx.hpp:688 (limbs <= 2^31.33, value < 2^(29 L))",
        [Spec(lambda fd: fd.Rp, lim=NTT_SHOUP_LIMB), Spec(p_(1)), Spec(p_(1))], Out("mod", p_(3), all_limbs=True), only=L9),
    Row("mul_low", "MUL_LOW", "fx.hpp:765", [Spec(lambda fd: fd.Rp, top=N29)] * 2, Out("exact", all_limbs=True)),
    # ---- reductions and tests
    Row("reduce_small", "REDUCE_SMALL", "fx.hpp:625", [Spec(p_(64))], Out("mod", p_(2))),
    Row("reduce_lazy", "REDUCE_LAZY", "fx.hpp:781 (limbs up to 2^31)", [Spec(p_(64), lim=lambda fd: 1 << 31)],
        Out("mod", p_(3)), only=lambda fd: fd.limbs(fd.p)[-1] >= 1 << 16),
    Row("cond_sub_p", "COND_SUB_P", "fx.hpp:649", [Spec(p_(2))], Out("mod", p_(1))),
    Row("canon", "CANON", "fx.hpp:669", [Spec(p_(64))], Out("mod", p_(1))),
    Row("is_zero_canon", "IS_ZERO_CANON", "fx.hpp:673", [Spec(p_(1))], Out("bool")),
    Row("is_zero_lt2p", "IS_ZERO_LT2P", "ecx.hpp:35", [Spec(p_(2))], Out("bool")),
    # ---- call-site envelopes: the worst case each tight call site claims
    Row("quotient_p12", "MUL2_INL", "poly.hip:418-419 (2p * 28p + 3p * 4p < R' p)",
        [Spec(p_(2)), Spec(p_(28)), Spec(p_(3), lim=LAZY3), Spec(p_(4))], Out("mod", p_(2)), only=SCALAR),
    Row("quotient_k12", "MUL2_INL", "poly.hip:431-432 (2p * 4p + 3p * 4p)",
        [Spec(p_(2)), Spec(p_(4)), Spec(p_(3), lim=LAZY3), Spec(p_(4))], Out("mod", p_(2)), only=SCALAR),
    Row("quotient_p1", "MUL", "poly.hip:414 (2p * 20p)", [Spec(p_(2)), Spec(p_(20))], Out("mod", p_(2)), only=SCALAR),
    Row("lincomb", "MUL2_INL", "poly.hip:83 (canonical terms and scalars)", [Spec(p_(1))] * 4, Out("mod", p_(2)),
        only=SCALAR),
    Row("poseidon_mds", "MUL2_INL", "poseidon.hip:105 (state < 5.72p, matrix entry < p)",
        [Spec(p_((572, 100))), Spec(p_(1)), Spec(p_((572, 100))), Spec(p_(1))], Out("mod", p_(2)), only=SCALAR),
    Row("poseidon_sbox", "MUL", "poseidon.hip:33 (state < 5.72p squared)", [Spec(p_((572, 100)))] * 2, Out("mod", p_(2)),
        only=SCALAR),
    Row("ecx_y3_lazy", "MUL2_INL", "ecx.hpp:113-119 (6p * 11p + 2p * 5p, lazy limbs < 3 * 2^29, L = 9)",
        [Spec(p_(6)), Spec(p_(11), lim=LAZY3), Spec(p_(2)), Spec(p_(5), lim=LAZY3)], Out("mod", p_(2)),
        only=lambda fd: fd.which == 1 and fd.L <= 9),
    Row("ecx_y3_norm", "MUL2_INL", "ecx.hpp:121 (6p * 10p + 2p * 4p, normalised, L = 14)",
        [Spec(p_(6)), Spec(p_(10)), Spec(p_(2)), Spec(p_(4))], Out("mod", p_(2)), only=lambda fd: fd.which == 1 and fd.L > 9),
    Row("ntt_twiddle_l0", "MUL_SHOUP", "ntt.hip:87 (fx_sub_lazy<4>: < 7p, limbs < 3 * 2^29)",
        [Spec(p_(7), lim=LAZY3), Spec(p_(1)), Spec(p_(1))], Out("mod", p_(3), all_limbs=True), only=lambda fd: SCALAR(fd) and L9(fd)),
    Row("ntt_twiddle", "MUL_SHOUP", "ntt.hip:88 (fx_sub_lazy_wide<8, 30>: < 15p, limbs < 2^31.33)",
        [Spec(p_(15), lim=NTT_SHOUP_LIMB), Spec(p_(1)), Spec(p_(1))], Out("mod", p_(3), all_limbs=True),
        only=lambda fd: SCALAR(fd) and L9(fd)),
]


# ---- operand generators ---------------------------------------------------------------------------------------------
def _fits(fd: Fd, s: Spec, limbs: Sequence[int]) -> bool:
    V, lim, top = s.v(fd), s.lim(fd), s.top(fd)
    return (all(0 <= x < lim for x in limbs[:-1]) and 0 <= limbs[-1] < min(top, 1 << 32)
            and fd.value(limbs) < V)


def borrow(fd: Fd, v: int, lim: int) -> List[int]:
    """limbs of v with every low limb pushed as close to lim as the value above it allows"""
    l = fd.limbs(v)
    unit = 1 << fd.B
    for _ in range(fd.L):
        changed = False
        for i in range(fd.L - 2, -1, -1):
            # take k units from limb i + 1 into limb i
            k = min(l[i + 1], (lim - 1 - l[i]) // unit)
            if k > 0:
                l[i + 1] -= k
                l[i] += k * unit
                changed = True
        if not changed:
            break
    return l


def max_limbs(fd: Fd, s: Spec) -> Optional[List[int]]:
    """low limbs at their bound, the rest in the top limb, the value still under the bound"""
    low = [s.lim(fd) - 1] * (fd.L - 1)
    base = fd.value(low + [0])
    V = s.v(fd)
    if base >= V:
        return None
    t = (V - 1 - base) >> (fd.B * (fd.L - 1))
    t = min(t, s.top(fd) - 1, (1 << 32) - 1)
    return low + [t]


def residues(fd: Fd) -> List[int]:
    p = fd.p
    return [0, 1, 2, p - 1, p - 2, fd.Rp % p, pow(fd.Rp, 2, p), p // 2, (1 << fd.SH) % p, 1 << (fd.f.bits - 1)]


def operand_values(fd: Fd, s: Spec, rnd: random.Random, n_random: int) -> List[List[int]]:
    """limb lists (or packed integers as one-element lists) on the bounds of s"""
    V = s.v(fd)
    out: List[List[int]] = []
    if s.packed:
        vals = [V - 1 - k for k in range(4)] + [r for r in residues(fd) if r < V]
        vals += [rnd.randrange(V) for _ in range(n_random)]
        return [[v] for v in vals]
    cands: List[List[int]] = []
    for k in range(4):                                           # the largest values
        cands.append(fd.limbs(V - 1 - k))
        cands.append(borrow(fd, V - 1 - k, s.lim(fd)))
    m = max_limbs(fd, s)
    if m is not None:
        cands.append(m)
        for j in range(fd.L - 1):                                # one low limb off its maximum
            mm = list(m)
            mm[j] -= 1 + rnd.randrange(3)
            cands.append(mm)
    p = fd.p
    for r in residues(fd):                                       # the same residue lifted by the largest k (and by 1, 2)
        kmax = (V - 1 - r) // p
        for k in sorted({kmax, max(kmax - 1, 0), 0, min(1, kmax), min(2, kmax)}):
            v = r + k * p
            cands.append(fd.limbs(v))
            cands.append(borrow(fd, v, s.lim(fd)))
    for _ in range(n_random):                                    # random, limbs pushed up; plain random
        v = rnd.randrange(V)
        cands.append(borrow(fd, v, s.lim(fd)))
        cands.append(fd.limbs(rnd.randrange(V)))
    for c in cands:
        if _fits(fd, s, c):
            out.append(c)
    return out


def records(fd: Fd, row: Row, rnd: random.Random, n: int) -> List[List[List[int]]]:
    """at least n operand tuples for row: every generated value of every operand appears, against random partners,
    and also against the largest value of every other operand"""
    pools = [operand_values(fd, s, rnd, max(8, n // 8)) for s in row.ins]
    out = []
    for i in range(max(n, max(len(p) for p in pools))):
        out.append([pool[i] if i < len(pool) else pool[rnd.randrange(len(pool))] for pool in pools])
    for j, pool in enumerate(pools):
        for k in range(min(len(pool), 24)):
            out.append([pools[t][0] if t != j else pool[k] for t in range(len(pools))])
    return out


def pack_fx(fd: Fd, row: Row, tuples) -> List[List[int]]:
    """(n, 4 L) u32 words"""
    res = []
    for tup in tuples:
        w = [0] * fd.W
        for j, (s, v) in enumerate(zip(row.ins, tup)):
            src = fd.words(v[0]) if s.packed else v
            w[j * fd.L: j * fd.L + len(src)] = src
        res.append(w)
    return res


# ---- expected results -----------------------------------------------------------------------------------------------
def expected(fd: Fd, op: str, vals: List[int]) -> int:
    p, Rp, Ri = fd.p, fd.Rp, pow(fd.Rp, -1, fd.p)
    a = vals[0]
    b, c, d = (vals + [0, 0, 0])[1:4]
    if op == "UNPACK" or op == "PACK" or op == "NORMALIZE":
        return a
    if op == "UNPACK_SHIFT":
        return a << fd.SH
    if op == "FROM_ARK":
        return a * (1 << fd.SH) % p
    if op == "TO_ARK":
        return a * pow(1 << fd.SH, -1, p) % p
    if op in ("ADD", "ADD_LAZY"):
        return a + b
    if op == "DBL":
        return 2 * a
    if op.startswith("SUB_LAZY_WIDE_"):
        return a + int(op.split("_")[3]) * p - b
    if op.startswith("SUB_LAZY_") or op.startswith("SUB_"):
        return a + int(op.rsplit("_", 1)[1]) * p - b
    if op == "SUB2_6":
        return a + 6 * p - b - 2 * c
    if op in ("MUL", "MUL_INL"):
        return a * b * Ri % p
    if op in ("SQR", "SQR_INL"):
        return a * a * Ri % p
    if op == "MUL2_INL":
        return (a * b + c * d) * Ri % p
    if op == "MUL_SHOUP":
        return a * b % p
    if op == "MUL_LOW":
        return a * b % Rp
    if op in ("REDUCE_SMALL", "REDUCE_LAZY", "COND_SUB_P", "CANON"):
        return a % p
    if op == "IS_ZERO_CANON":
        return int(a == 0)
    if op == "IS_ZERO_LT2P":
        return int(a % p == 0)
    raise KeyError(op)


def shoup_operands(fd: Fd, tup):
    """MUL_SHOUP: the second operand is w (canonical), the third its quotient floor(w R' / p)"""
    w = fd.value(tup[1]) % fd.p
    return [tup[0], fd.limbs(w), fd.limbs(w * fd.Rp // fd.p)]


def build(fd: Fd, row: Row, rnd: random.Random, n: int):
    """(tuples of operand values, u32 records) for row on fd"""
    tuples = records(fd, row, rnd, n)
    if row.op == "MUL_SHOUP":
        tuples = [shoup_operands(fd, t) for t in tuples]
    return tuples, pack_fx(fd, row, tuples)


def check(fd: Fd, row: Row, tuples, out) -> None:
    """assert that each result row of out (n, 4 L) meets row's contract"""
    for i, (tup, o) in enumerate(zip(tuples, out)):
        vals = [v[0] if s.packed else fd.value(v) for s, v in zip(row.ins, tup)]
        want = expected(fd, row.op, vals)
        o = [int(x) for x in o]
        where = "%s %s record %d: inputs %s" % (fd.f.name, row.name, i, [hex(v) for v in vals])
        if row.out.kind == "bool":
            assert o[0] == want, "%s: predicate %d, want %d" % (where, o[0], want)
            continue
        if row.out.packed:
            got = fd.wvalue(o)
        else:
            limbs = o[: fd.L]
            got = fd.value(limbs)
            lim = row.out.lim(fd)
            checked = limbs if row.out.all_limbs else limbs[:-1]
            bad = [j for j, x in enumerate(checked) if x >= lim]
            assert not bad, "%s: limbs %s not below %#x: %s" % (where, bad, lim, [hex(x) for x in limbs])
        if row.out.kind == "exact":
            assert got == want, "%s: value %#x, want %#x" % (where, got, want)
        else:
            assert got % fd.p == want, "%s: residue %#x, want %#x" % (where, got % fd.p, want)
        if row.out.v is not None:
            bound = row.out.v(fd)
            assert got < bound, "%s: value %#x not below %s (%.3f p)" % (where, got, row.src, got / fd.p)


# ---- curve records --------------------------------------------------------------------------------------------------
XYZZ_BOUNDS = (8, 4, 2, 2)      # ecx.hpp:6: X < 8p, Y < 4p, ZZ < 2p, ZZZ < 2p, limbs normalised
CURVE_OPS = ["ADD_MIXED", "ADD_MIXED_INL", "ADD", "ADD_INL", "DOUBLE", "DOUBLE_AFFINE"]
CURVE_SRC = {"ADD_MIXED": "ecx.hpp:87", "ADD_MIXED_INL": "ecx.hpp:87 (INL)", "ADD": "ecx.hpp:134", "ADD_INL": "ecx.hpp:134 (INL)",
             "DOUBLE": "ecx.hpp:65", "DOUBLE_AFFINE": "ecx.hpp:47"}


def curve_points(cv: F.Curve, rnd: random.Random, n: int) -> List[C.Point]:
    P = C.scalar_mul(cv, rnd.randrange(1, cv.fr.p), C.generator(cv))
    G = C.generator(cv)
    pts = [P]
    for _ in range(n - 1):
        pts.append(C.add(cv, pts[-1], G))
    return pts


def _lift(fd: Fd, r: int, kmax: int, mode: int, rnd: random.Random) -> List[int]:
    """r (canonical) + k p below kmax p: k the largest (mode 0), random (1) or 0 (2)"""
    k = [kmax - 1, rnd.randrange(kmax), 0][mode]
    return fd.limbs(r + k * fd.p)


def xyzz_point(fd: Fd, P: C.Point, rnd: random.Random, mode: int) -> List[int]:
    """4 L + 1 words: P in XYZZ form, R' Montgomery, random Z, each coordinate lifted towards its bound"""
    L = fd.L
    if P is None:
        return [0] * (4 * L) + [1]
    p, Rp = fd.p, fd.Rp
    z = rnd.randrange(1, p)
    zz, zzz = z * z % p, z * z * z % p
    coords = [P[0] * zz % p, P[1] * zzz % p, zz, zzz]
    words = []
    for v, kb in zip(coords, XYZZ_BOUNDS):
        words += _lift(fd, v * Rp % p, kb, mode if mode < 3 else rnd.randrange(3), rnd)
    return words + [0]


def affine_point(fd: Fd, P: C.Point) -> List[int]:
    """canonical affine coordinates in R' form in the x, y slots"""
    L = fd.L
    return fd.limbs(P[0] * fd.Rp % fd.p) + fd.limbs(P[1] * fd.Rp % fd.p) + [0] * (2 * L) + [0]


def curve_records(cv: F.Curve, fd: Fd, op: str, rnd: random.Random, n: int):
    """(expected affine results, (n, 2 (4 L + 1)) records) for op, with the exceptional pairs included"""
    pts = curve_points(cv, rnd, max(8, n // 8))
    want, recs = [], []
    for i in range(n):
        P = pts[i % len(pts)]
        Q = pts[(i * 7 + 3) % len(pts)]
        kind = i % 8
        mode = (i // 8) % 4
        if op in ("ADD_MIXED", "ADD_MIXED_INL"):
            # kind 0: P + P (doubling path), 1: P + (-P), 2: identity + Q, else a general pair
            if kind == 0:
                Q = P
            elif kind == 1:
                Q = C.neg(cv, P)
            Pin = None if kind == 2 else P
            recs.append(xyzz_point(fd, Pin, rnd, mode) + affine_point(fd, Q))
            want.append(C.add(cv, Pin, Q))
        elif op in ("ADD", "ADD_INL"):
            # kind 0: P + P with different Z, 1: P + (-P), 2: identity + Q, 3: P + identity
            if kind == 0:
                Q = P
            elif kind == 1:
                Q = C.neg(cv, P)
            Pin = None if kind == 2 else P
            Qin = None if kind == 3 else Q
            recs.append(xyzz_point(fd, Pin, rnd, mode) + xyzz_point(fd, Qin, rnd, (mode + 1) % 4))
            want.append(C.add(cv, Pin, Qin))
        elif op == "DOUBLE":
            Pin = None if kind == 2 else P
            recs.append(xyzz_point(fd, Pin, rnd, mode) + [0] * (4 * fd.L + 1))
            want.append(C.add(cv, Pin, Pin))
        else:   # DOUBLE_AFFINE
            recs.append(affine_point(fd, P) + [0] * (4 * fd.L + 1))
            want.append(C.add(cv, P, P))
    return want, recs


def check_curve(cv: F.Curve, fd: Fd, op: str, want, out) -> None:
    p, L = fd.p, fd.L
    for i, (w, o) in enumerate(zip(want, out)):
        o = [int(x) for x in o]
        where = "%s %s (%s) record %d" % (cv.name, op, CURVE_SRC[op], i)
        if w is None:
            assert o[4 * L] == 1, "%s: want the identity" % where
            continue
        assert o[4 * L] == 0, "%s: got the identity" % where
        X, Y, ZZ, ZZZ = [o[j * L:(j + 1) * L] for j in range(4)]
        for name, limbs, kb in zip(("X", "Y", "ZZ", "ZZZ"), (X, Y, ZZ, ZZZ), XYZZ_BOUNDS):
            assert all(x < 1 << fd.B for x in limbs[:-1]), "%s: %s limbs not normalised: %s" % (where, name, limbs)
            v = fd.value(limbs)
            assert v < kb * p, "%s: %s = %.3f p, bound %d p (ecx.hpp:6)" % (where, name, v / p, kb)
        x, y, zz, zzz = (fd.value(c) % p for c in (X, Y, ZZ, ZZZ))
        assert zz != 0 and zzz != 0, "%s: ZZ or ZZZ is zero" % where
        # ZZ^3 = ZZZ^2 for the true Z; in R' form (ZZ R')^3 = (ZZZ R')^2 R'
        assert pow(zz, 3, p) == zzz * zzz * fd.Rp % p, "%s: ZZ^3 != ZZZ^2" % where
        got = (x * pow(zz, -1, p) % p, y * pow(zzz, -1, p) % p)
        assert got == w, "%s: affine %s, want %s" % (where, got, w)
