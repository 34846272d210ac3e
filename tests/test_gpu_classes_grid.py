"""The classes route of round 4 with the class in the grid, its closing pass and round 3's totals in one launch (modes 0 / 1 of
zkt_ctx_set_fused_passes) against the launch sequence they replace (mode 2), through set_quotient_route(CLASSES): the same
proof bytes and the same 4n coefficients left in the quotient vector, element by element.

Sizes: n = 8 and 16 (k_ntt_small; the folded head is the whole input at 8 and half of it at 16), 128, 2048 (the first size on
k_ntt_pass, two passes, two scan blocks) on both curves, and n = 2^17 (the first three-pass size) on BN254.  Every proof
transforms batches of three polynomials (a b c; f h1 h2) and of two (z1 z2), and its three E_j in place in the inverse
direction.  The oracle's proofs are those of tests/test_gpu_quotient_classes.py, made once per (curve, n) and shared."""
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import fields as F, plonk as P, coracle as K
from helpers import field_elems

import test_gpu_quotient_classes as QC

CURVES = [F.BN254, F.BLS12_381]
SIZES = [8, 16, 128, 2048]
FUSED, STEPWISE = 1, 2
CLASSES, WHOLE = 1, 2
K1, K2 = 7, 13

params = pytest.mark.parametrize("cv,n", [(cv, n) for cv in CURVES for n in SIZES], ids=lambda v: getattr(v, "name", str(v)))


@pytest.fixture(scope="module")
def ctxs():
    import zkt_plonk_amd as z
    c = {cv.name: z.Context(cv.name, 0) for cv in CURVES}
    yield c
    for x in c.values():
        x.close()


def _restore(ctx):
    ctx.set_fused_passes(0)
    ctx.set_quotient_route(0)


def _proof_and_quotient(ctx, n, prove):
    got = prove()
    q = ctx.debug_quotient_coeffs(4 * n)
    assert ctx.debug_quotient_top()[1], "the proof did not take the classes route"
    return got, q


@params
def test_stepwise_and_fused_leave_the_same_bytes_and_quotient(cv, n, ctxs):
    import zkt_plonk_amd as z
    ctx, cs = ctxs[cv.name], QC._case(cv, n)
    cs.load(z, ctx)
    try:
        ctx.set_quotient_route(CLASSES)
        out = {}
        for mode in (STEPWISE, FUSED):
            ctx.set_fused_passes(mode)
            out[mode] = _proof_and_quotient(ctx, n, lambda: cs.prove(z, ctx, 0, 900))
        assert out[FUSED][0] == out[STEPWISE][0]
        assert np.array_equal(out[FUSED][1], out[STEPWISE][1])
        assert out[FUSED][0] == cs.want(0, 900)
        assert out[FUSED][1][3 * n + 5].any() and not out[FUSED][1][3 * n + 6:].any()
    finally:
        _restore(ctx)


@params
def test_after_a_whole_coset_proof_of_another_witness(cv, n, ctxs):
    """The whole-coset route leaves another witness's 4n coefficients in the quotient vector and blinders in the chunks'
    slack (the low chunk's sits at n + 2): the classes route right behind it must leave exactly the whole route's
    coefficients of its own witness, zeros above 3n + 5 included, and the oracle's bytes."""
    import zkt_plonk_amd as z
    ctx, cs = ctxs[cv.name], QC._case(cv, n)
    cs.load(z, ctx)
    try:
        ctx.set_quotient_route(WHOLE)
        ctx.set_fused_passes(STEPWISE)
        assert cs.prove(z, ctx, 0, 900) == cs.want(0, 900)
        q_whole = ctx.debug_quotient_coeffs(4 * n)
        for mode in (STEPWISE, FUSED):
            ctx.set_fused_passes(mode)
            ctx.set_quotient_route(WHOLE)
            assert cs.prove(z, ctx, 1, 931) == cs.want(1, 931), mode
            assert not np.array_equal(ctx.debug_quotient_coeffs(4 * n), q_whole)
            ctx.set_quotient_route(CLASSES)
            got, q = _proof_and_quotient(ctx, n, lambda: cs.prove(z, ctx, 0, 900))
            assert got == cs.want(0, 900), mode
            assert np.array_equal(q, q_whole), mode
    finally:
        _restore(ctx)


_ZERO_BLINDERS = {}


def _zero_blinder_proof(cs):
    key = (cs.cv.name, cs.n)
    if key not in _ZERO_BLINDERS:
        _ZERO_BLINDERS[key] = P.prove(cs.be, [None] * (cs.n + 8), cs.pk, cs.epk, cs.vk, cs.css[0], P.new_seeded_transcript(cs.cv, cs.vk),
                                      [0] * P.NUM_BLINDERS).serialize(cs.cv)
    return _ZERO_BLINDERS[key]


@params
def test_chunk_seams_and_trimmed_lengths(cv, n, ctxs):
    """The seams t[n + 1] | t[n + 2] and t[2n + 3] | t[2n + 4] of the three chunks and their trimmed lengths: the constant-b
    witness of tests/test_gpu_quotient_classes.py, and a witness with every blinder zero (the quotient then ends below
    3n + 6, the chunks' blinders are zero and the high chunk is trimmed shorter), in both modes against the oracle."""
    import zkt_plonk_amd as z
    ctx = ctxs[cv.name]
    try:
        cb = QC._case(cv, n, "constant_b")
        cb.load(z, ctx)
        ctx.set_quotient_route(CLASSES)
        out = {}
        for mode in (STEPWISE, FUSED):
            ctx.set_fused_passes(mode)
            out[mode] = _proof_and_quotient(ctx, n, lambda: cb.prove(z, ctx, 0, 910))
            assert out[mode][0] == cb.want(0, 910), mode
        assert np.array_equal(out[FUSED][1], out[STEPWISE][1])

        cs = QC._case(cv, n)
        cs.load(z, ctx)
        ctx.set_quotient_route(CLASSES)
        inputs = cs.inputs(0, 900)[:-1] + (K.fr_to_mont(cv, [0] * P.NUM_BLINDERS),)
        want = _zero_blinder_proof(cs)
        for mode in (STEPWISE, FUSED):
            ctx.set_fused_passes(mode)
            out[mode] = _proof_and_quotient(ctx, n, lambda: ctx.prove(*inputs, cs.tr(z)))
            assert out[mode][0] == want, mode
        assert np.array_equal(out[FUSED][1], out[STEPWISE][1])
        assert not out[FUSED][1][3 * n:].any()
    finally:
        _restore(ctx)


@pytest.mark.parametrize("cv", CURVES, ids=lambda c: c.name)
def test_a_fork_and_an_announced_successor(cv, ctxs):
    """n = 2048: a forked context (it shares the parent's class tables and plans) and a chain whose successors are announced
    (zkt_prove_set_next: rounds 1 and 2 of the next proof, their class transforms included, are issued ahead)."""
    import zkt_plonk_amd as z
    n = 2048
    ctx, cs = ctxs[cv.name], QC._case(cv, n)
    cs.load(z, ctx)
    try:
        ctx.set_quotient_route(CLASSES)
        ctx.set_fused_passes(FUSED)
        assert cs.prove(z, ctx, 0, 900) == cs.want(0, 900)
        q0 = ctx.debug_quotient_coeffs(4 * n)
        fork = ctx.fork()
        try:
            got, q = _proof_and_quotient(fork, n, lambda: cs.prove(z, fork, 0, 900))
            assert got == cs.want(0, 900) and np.array_equal(q, q0)
        finally:
            fork.close()
        order = [(0, 900), (1, 931), (0, 900)]
        preps = [ctx.prepare_host(*cs.inputs(k, seed)) for k, seed in order]
        for i, (k, seed) in enumerate(order):
            nxt = preps[i + 1] if i + 1 < len(order) else None
            got, q = _proof_and_quotient(ctx, n, lambda: ctx.prove_prepared(preps[i], cs.tr(z), nxt))
            assert got == cs.want(k, seed), i
        assert np.array_equal(q, q0)
    finally:
        _restore(ctx)


# ---- n = 2^17: three passes --------------------------------------------------------------------------------------------
def _to_limbs(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(len(vals), 4).copy()


def _mont(ctx, p, vals):
    """canonical integers -> Montgomery words on the device (x * R^2 / R)"""
    arr = _to_limbs(vals)
    return ctx.debug_fr_mul(arr, np.tile(_to_limbs([pow(1 << 256, 2, p)]), (len(vals), 1)))


def _chain_circuit(p, gen, log_n, table_size=64, n_public=3):
    """2^log_n - 8 rows: products, sums and linear gates chained by copy constraints (the output of one row is the left wire of
    the next), a lookup every sixteenth row, public inputs at the end; the evaluations of the selectors and of the
    permutation as proof_system::setup takes them."""
    rnd = random.Random(0xC1A55 + log_n)
    n = 1 << log_n
    gates = n - 8
    table = rnd.sample(range(1, 1 << 62), table_size - 1)
    w = pow(gen, (p - 1) >> log_n, p)
    roots = [1] * n
    for i in range(1, n):
        roots[i] = roots[i - 1] * w % p
    a, b, c = [0] * n, [0] * n, [0] * n
    q_m, q_l, q_r, q_o, q_c, q_lk = ([0] * n for _ in range(6))
    s1, s2, s3 = list(roots), [K1 * x % p for x in roots], [K2 * x % p for x in roots]
    pi = {}
    prev = None
    for i in range(gates - n_public):
        q_o[i] = p - 1
        if i % 16 == 15:
            a[i] = c[i] = table[rnd.randrange(len(table))]
            q_l[i] = q_lk[i] = 1
        else:
            if prev is None:
                a[i] = rnd.randrange(p)
            else:
                a[i] = c[prev]
                s3[prev] = roots[i]                 # one cycle {Output(prev), Left(i)}
                s1[i] = K2 * roots[prev] % p
            b[i] = rnd.randrange(p)
            if i % 3 == 0:
                c[i] = a[i] * b[i] % p
                q_m[i] = 1
            elif i % 3 == 1:
                c[i] = (a[i] + b[i]) % p
                q_l[i] = q_r[i] = 1
            else:
                q_l[i], q_r[i], q_c[i] = rnd.randrange(p), rnd.randrange(p), rnd.randrange(p)
                c[i] = (q_l[i] * a[i] + q_r[i] * b[i] + q_c[i]) % p
        prev = i
    for i in range(gates - n_public, gates):
        c[i] = pi[i] = rnd.randrange(p)
        q_o[i] = p - 1
    sel = dict(q_m=q_m, q_l=q_l, q_r=q_r, q_o=q_o, q_c=q_c, sigma1=s1, sigma2=s2, sigma3=s3, q_lookup=q_lk,
               q_table=[0] * table_size + [1] * (n - table_size))
    return dict(gates=gates, a=a, b=b, c=c, sel=sel, table=table, pi=pi)


def test_three_pass_transforms_at_2_17():
    """BN254, n = 2^17: each class transform is three launches of k_ntt_pass with the raw planes of nine (or six, or three)
    transforms between them.  The circuit is set up on the device; mode 2 is the reference."""
    import zkt_plonk_amd as z
    cv, log_n = F.BN254, 17
    n, p = 1 << log_n, cv.fr.p
    circ = _chain_circuit(p, cv.fr.generator, log_n)
    ctx = z.Context(cv.name, 0)
    try:
        ctx.srs_generate(0x5EED17 % p, n + 8)
        _, commits = z.GpuProver.setup(ctx, log_n, {name: _mont(ctx, p, circ["sel"][name]) for name in z.PK_ORDER})
        L = cv.fq.limbs64
        rinv = pow(1 << (64 * L), -1, cv.fq.p)
        vk = {name: None if inf else (sum(int(v) << (64 * i) for i, v in enumerate(xy[:L])) * rinv % cv.fq.p,
                                      sum(int(v) << (64 * i) for i, v in enumerate(xy[L:])) * rinv % cv.fq.p)
              for name, (xy, inf) in commits.items()}
        g = circ["gates"]
        pos = sorted(circ["pi"])
        inputs = (_mont(ctx, p, circ["a"][:g]), _mont(ctx, p, circ["b"][:g]), _mont(ctx, p, circ["c"][:g]), _mont(ctx, p, circ["table"]),
                  pos, _mont(ctx, p, [circ["pi"][i] for i in pos]), _mont(ctx, p, field_elems(p, 1717, P.NUM_BLINDERS)))

        def prove():
            tr = z.Transcript("merlin", "ZKT Plonk", fr_bits=cv.fr.bits, fq_bytes=cv.fq.limbs64 * 8)
            return ctx.prove(*inputs, z.seed_transcript(tr, n, vk))
        ctx.set_quotient_route(CLASSES)
        out = {}
        for mode in (STEPWISE, FUSED):
            ctx.set_fused_passes(mode)
            out[mode] = _proof_and_quotient(ctx, n, prove)
        assert out[FUSED][0] == out[STEPWISE][0]
        assert np.array_equal(out[FUSED][1], out[STEPWISE][1])
        assert out[FUSED][1][3 * n + 5].any() and not out[FUSED][1][3 * n + 6:].any()
    finally:
        ctx.close()
