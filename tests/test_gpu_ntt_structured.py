"""GPU parity of the NTT where test_gpu_ntt.py's uniformly random inputs do not reach: structured inputs whose outputs hold
exact zeros and operands at the top of their range (ntt_cases.py), every pass radix 2^5 .. 2^9 as first, middle and last
pass (zkt_debug_ntt_split), batches of ragged transforms in one launch per pass (zkt_debug_ntt_batch) and the out-of-place
device entry (zkt_ntt_dev).  Whole outputs, bit for bit, against the CPU oracle: these are exact field elements."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import fields as F, coracle as K
from helpers import rand_fr
import ntt_cases as NC

CURVES = [F.BN254, F.BLS12_381]
VARIANTS = list(NC.VARIANTS)
INVALID_ARGUMENT = 1


@pytest.fixture(scope="module")
def ctxs():
    import zkt_plonk_amd as z
    c = {cv.name: z.Context(cv.name, 0) for cv in CURVES}
    yield c
    for x in c.values():
        x.close()


def _zero_rows(arr) -> int:
    return int((~arr.any(axis=1)).sum())


# the single-workgroup kernel and the splits [6,5], [7,7], [8,8], [6,6,5], [6,6,6]
@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: v[0])
@pytest.mark.parametrize("log_n", [10, 11, 14, 16, 17, 18])
@pytest.mark.parametrize("cv", CURVES, ids=lambda c: c.name)
def test_structured_inputs(cv, log_n, variant, ctxs):
    name, inv, cos = variant
    ran = 0
    for cname in NC.case_names(log_n):
        case = NC.make(cv, log_n, name, cname)
        if case is None:
            continue
        x = K.fr_to_mont(cv, case.input)
        got = ctxs[cv.name].ntt(log_n, x, inverse=bool(inv), coset=bool(cos))
        assert np.array_equal(got, K.ntt_mont(cv, log_n, inv, cos, x)), (cv.name, log_n, name, cname)
        if case.expected is not None:
            assert np.array_equal(got, K.fr_to_mont(cv, case.expected)), (cv.name, log_n, name, cname, "closed form")
        if case.zeros is not None:       # a zero residue leaves the kernel as the word 0, never as p
            assert _zero_rows(got) == case.zeros, (cv.name, log_n, name, cname)
        ran += 1
    assert ran == len(NC.case_names(log_n))


# [R,5,5], [5,R,5], [5,5,R] and the two-pass [R,5], [5,R] for R = 5 .. 9, and [9,9]: every radix as first, middle and last pass
SPLITS = {
    11: [[5, 6], [6, 5]],
    12: [[7, 5], [5, 7]],
    13: [[8, 5], [5, 8]],
    14: [[9, 5], [5, 9]],
    15: [[5, 5, 5]],
    16: [[6, 5, 5], [5, 6, 5], [5, 5, 6]],
    17: [[7, 5, 5], [5, 7, 5], [5, 5, 7]],
    18: [[8, 5, 5], [5, 8, 5], [5, 5, 8], [9, 9]],
    19: [[9, 5, 5], [5, 9, 5], [5, 5, 9]],
}


@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: v[0])
@pytest.mark.parametrize("log_n", sorted(SPLITS))
@pytest.mark.parametrize("cv", CURVES, ids=lambda c: c.name)
def test_every_radix_in_every_position(cv, log_n, variant, ctxs):
    """The policy reaches radix 2^9 only from 2^25, 2^5 only as a last pass and 2^8 never as a middle pass below 2^23; the
    pass kernels take any split whose tiles fit.  Every forced split, and the policy's own on the same context before and
    after, gives the oracle's output."""
    name, inv, cos = variant
    ctx = ctxs[cv.name]
    n = 1 << log_n
    rng = np.random.default_rng(0x5917 + log_n)
    full = rand_fr(rng, n)
    inputs = [("random", full), ("random n/4+8", full[:n // 4 + 8])]
    inputs += [(c, K.fr_to_mont(cv, NC.make(cv, log_n, name, c).input)) for c in ("all_p_minus_1", "geometric_n/2+1")]
    want = [K.ntt_mont(cv, log_n, inv, cos, x) for _, x in inputs]
    try:
        for split in [[]] + SPLITS[log_n] + [[]]:
            assert sum(split) in (0, log_n)
            ctx.debug_ntt_split(split)
            for (label, x), w in zip(inputs, want):
                got = ctx.ntt(log_n, x, inverse=bool(inv), coset=bool(cos))
                assert np.array_equal(got, w), (cv.name, log_n, name, split or "policy", label)
    finally:
        ctx.debug_ntt_split([])


@pytest.mark.parametrize("cv", CURVES, ids=lambda c: c.name)
def test_forced_split_refusals(cv, ctxs):
    """(No split of two or three radices 2^5 .. 2^9 breaks a tile constraint -- log_s >= 10 - LOG_R before the last pass,
    log_r1 >= 10 - LOG_R on it -- so that refusal cannot be provoked through the entry.)"""
    import zkt_plonk_amd as z
    ctx = ctxs[cv.name]
    x = rand_fr(np.random.default_rng(5), 1 << 12)
    want12 = K.ntt_mont(cv, 12, 0, 0, x)
    try:
        for bad in ([6], [5, 5, 5, 5], [4, 8], [10, 5], [5, 5, 10], [6, 3, 6], [5, -1]):
            with pytest.raises(z.ZktError) as e:
                ctx.debug_ntt_split(bad)
            assert e.value.code == INVALID_ARGUMENT, bad
        assert np.array_equal(ctx.ntt(12, x), want12)              # a refused override leaves the policy in place
        ctx.debug_ntt_split([5, 6])                                # fits 2^11 only
        with pytest.raises(z.ZktError) as e:
            ctx.ntt(12, x)                                         # although a policy plan for 2^12 exists
        assert e.value.code == INVALID_ARGUMENT
        with pytest.raises(z.ZktError) as e:
            ctx.ntt(17, x)
        assert e.value.code == INVALID_ARGUMENT
        assert np.array_equal(ctx.ntt(11, x[:2048]), K.ntt_mont(cv, 11, 0, 0, x[:2048]))
        assert np.array_equal(ctx.ntt(10, x[:1024]), K.ntt_mont(cv, 10, 0, 0, x[:1024]))   # up to 2^10: no passes to split
        ctx.debug_ntt_split([])
        assert np.array_equal(ctx.ntt(12, x), want12)
        fork = ctx.fork()
        try:
            with pytest.raises(z.ZktError) as e:
                fork.debug_ntt_split([7, 5])
            assert e.value.code == INVALID_ARGUMENT
            assert np.array_equal(fork.ntt(12, x), want12)
        finally:
            fork.close()
    finally:
        ctx.debug_ntt_split([])


def _batch_lengths(n):
    return [[n, n // 4 + 8, 1, n - 3],          # all four differ
            [n - 3, 0, n, n // 4 + 8]]          # an empty polynomial in the middle


# the single-workgroup loop, two passes, three passes
@pytest.mark.parametrize("log_n", [9, 11, 14, 17])
@pytest.mark.parametrize("cv", CURVES, ids=lambda c: c.name)
def test_batched_transforms(cv, log_n, ctxs):
    """gridDim.y selects the polynomial, each with its own in_len: every output of a batch is the single transform of its
    own input.  The input buffers hold n elements, random beyond in_len, so a length taken from another polynomial shows."""
    import zkt_plonk_amd as z
    ctx = ctxs[cv.name]
    n = 1 << log_n
    rng = np.random.default_rng(0xBA7C + log_n)
    pool = [rand_fr(rng, n) for _ in range(4)]
    d_in = [ctx.alloc(n * 32) for _ in range(4)]
    d_out = [ctx.alloc(n * 32) for _ in range(4)]
    want = {}

    def expected(y, length, inv, cos):
        key = (y, length, inv, cos)
        if key not in want:
            x = pool[y][:length]
            want[key] = K.ntt_mont(cv, log_n, inv, cos, x) if length else np.zeros((n, 4), dtype=np.uint64)
            assert np.array_equal(ctx.ntt(log_n, x, inverse=bool(inv), coset=bool(cos)), want[key])
        return want[key]

    try:
        variants = VARIANTS if log_n == 11 else [v for v in VARIANTS if v[0] in ("coset_fft", "ifft")]   # the prover's batches
        for name, inv, cos in variants:
            for lens in _batch_lengths(n):
                for nb in (1, 2, 3, 4):
                    for in_place in (False, True):
                        for y in range(nb):
                            ctx.upload(d_in[y], pool[y])
                        outs = d_in[:nb] if in_place else d_out[:nb]
                        ctx.debug_ntt_batch(log_n, d_in[:nb], lens[:nb], outs, inverse=bool(inv), coset=bool(cos))
                        for y in range(nb):
                            got = ctx.download(outs[y], (n, 4))
                            assert np.array_equal(got, expected(y, lens[y], inv, cos)), (cv.name, log_n, name, lens[:nb], y, in_place)
        for nb in (0, 5):
            with pytest.raises(z.ZktError) as e:
                ctx.debug_ntt_batch(log_n, (d_in + d_in)[:5], [n] * 5, (d_out + d_out)[:5], nb=nb)
            assert e.value.code == INVALID_ARGUMENT
    finally:
        for d in d_in + d_out:
            ctx.free(d)


@pytest.mark.parametrize("log_n", [8, 12, 17])
@pytest.mark.parametrize("cv", CURVES, ids=lambda c: c.name)
def test_ntt_dev_out_of_place(cv, log_n, ctxs):
    """zkt_ntt_dev from an input buffer of exactly in_len elements into another buffer: the input is left as it was and
    nothing is written past the n outputs; then the same transform in place."""
    import zkt_plonk_amd as z
    ctx = ctxs[cv.name]
    n = 1 << log_n
    rng = np.random.default_rng(0x00B + log_n)
    pattern = np.full((64, 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    for in_len in (n // 4 + 8, n):
        x = rand_fr(rng, in_len)
        d_in, d_out, d_io = ctx.alloc(in_len * 32), ctx.alloc((n + 64) * 32), ctx.alloc(n * 32)
        try:
            for name, inv, cos in VARIANTS:
                want = K.ntt_mont(cv, log_n, inv, cos, x)
                ctx.upload(d_in, x)
                ctx.upload(d_out, np.vstack([np.repeat(pattern[:1], n, axis=0), pattern]))
                ctx.ntt_dev(log_n, d_in, in_len, d_out, inverse=bool(inv), coset=bool(cos))
                out = ctx.download(d_out, (n + 64, 4))
                assert np.array_equal(out[:n], want), (cv.name, log_n, in_len, name)
                assert np.array_equal(out[n:], pattern), (cv.name, log_n, in_len, name, "written past n")
                assert np.array_equal(ctx.download(d_in, (in_len, 4)), x), (cv.name, log_n, in_len, name, "input changed")
                # in place, the buffer's tail beyond in_len holding the pattern
                ctx.upload(d_io, np.vstack([x, np.repeat(pattern[:1], n - in_len, axis=0)]))
                ctx.ntt_dev(log_n, d_io, in_len, d_io, inverse=bool(inv), coset=bool(cos))
                assert np.array_equal(ctx.download(d_io, (n, 4)), want), (cv.name, log_n, in_len, name, "in place")
            with pytest.raises(z.ZktError) as e:
                ctx.ntt_dev(log_n, d_in, in_len, 0)
            assert e.value.code == INVALID_ARGUMENT
        finally:
            for d in (d_in, d_out, d_io):
                ctx.free(d)
