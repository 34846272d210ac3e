"""GPU: zkt_verify_batch_prepare_dev / zkt_verify_batch_dev, a batch of proofs under one SRS verified with the
decompressions and the two combinations on the device, against the host verifier (zkt_verify, zkt_verify_batch,
zkt_verify_prepare + zkt_g1_msm_host) on proofs of the CPU oracle: circuits of 150 / 90 / 150 gates, one SRS, Merlin
transcripts and the Ethereum transcript on BN254."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import fields as F, plonk as P, coracle as K, curve as C, pairing as PR
from helpers import field_elems

CURVES = [F.BN254, F.BLS12_381]
TAU = 0x1234567ABCDEF


def g2_mont(cv, pts):
    """G2 affine points ((x0, x1), (y0, y1)) -> (n, 4 * limbs) Montgomery limbs."""
    L = cv.fq.limbs64
    flat = []
    for q in pts:
        flat.extend([q[0][0], q[0][1], q[1][0], q[1][1]])
    a = K.ints_to_limbs(flat, L)
    out = np.empty_like(a)
    assert K.lib().orc_fq_convert(cv.curve_id, 1, K._p(a), a.shape[0], K._p(out)) == 0
    return out.reshape(len(pts), 4 * L)


@functools.lru_cache(maxsize=None)
def _made(cv):
    """Three oracle proofs (two circuit shapes, three statements) under one SRS -> (entries, srs, h, beta_h, wrong beta_h);
    an entry is (vk, public inputs, proof bytes, transcript kind)."""
    T = PR.Tower(cv)
    H = PR.G2_GENERATORS[cv.name]
    h, beta_h, wrong = g2_mont(cv, [H])[0], g2_mont(cv, [T.g2_mul(TAU, H)])[0], g2_mont(cv, [T.g2_mul(TAU + 1, H)])[0]
    specs = [(150, 16, 77, 3, "merlin"), (90, 8, 78, 2, "ethereum" if cv.name == "bn254" else "merlin"), (150, 16, 79, 3, "merlin")]
    made, srs = [], None
    for gates, tbl, seed, n_public, kind in specs:
        cs = P.synthetic_circuit(cv, gates, tbl, seed=seed, n_public=n_public)
        n = cs.circuit_bound()
        if srs is None:
            srs = K.srs_mont(cv, TAU, n + 8)            # the first circuit is the largest: one key for all
        be = K.CBackend(cv, srs[:n + 8])
        pk, epk, vk = P.setup(be, [None] * (n + 8), cs, True)
        proof = P.prove(be, [None] * (n + 8), pk, epk, vk, cs, P.new_seeded_transcript(cv, vk, kind),
                        field_elems(cv.fr.p, seed, P.NUM_BLINDERS)).serialize(cv)
        made.append((vk, tuple(cs.pi[k] for k in sorted(cs.pi)), proof, kind))
    return made, srs, h, beta_h, wrong


_VK_ARRAYS = {}


def _vk_arrays(cv, vk, shared):
    """The verifier key's arrays: ONE set per key when shared, a fresh copy per call otherwise."""
    import zkt_plonk_amd as z
    if shared and id(vk) in _VK_ARRAYS:
        return _VK_ARRAYS[id(vk)]
    arrs = (K.points_to_mont(cv, [vk.commits[k] for k in z.PK_ORDER]), [vk.commits[k] is None for k in z.PK_ORDER],
            K.fr_to_mont(cv, vk.pi_roots))
    if shared:
        _VK_ARRAYS[id(vk)] = arrs
    return arrs


def _item(cv, entry, shared=True):
    import zkt_plonk_amd as z
    vk, pis, raw, kind = entry
    srs = _made(cv)[1]
    tr = z.Transcript(kind, "ZKT Plonk", fr_bits=cv.fr.bits, fq_bytes=cv.fq.limbs64 * 8)
    z.seed_transcript(tr, vk.n, vk.commits)
    commits, inf, roots = _vk_arrays(cv, vk, shared)
    return (vk.n, commits, inf, roots, K.fr_to_mont(cv, list(pis)), raw, srs[0] if shared else srs[0].copy(), tr)


def _items(cv, entries, shared=True):
    return [_item(cv, e, shared) for e in entries]


def _cycle(made, count):
    return [made[i % len(made)] for i in range(count)]


@pytest.fixture(scope="module")
def ctxs():
    """One context per curve with no key and no circuit: the call needs neither."""
    import zkt_plonk_amd as z
    c = {cv.name: z.Context(cv.name, 0) for cv in CURVES}
    yield c
    for x in c.values():
        x.close()


@pytest.mark.parametrize("cv", CURVES, ids=lambda c: c.name)
def test_accepts_what_the_host_accepts_and_rejects_the_rest(ctxs, cv):
    from zkt_plonk_amd import _lib
    ctx = ctxs[cv.name]
    made, srs, h, beta_h, wrong = _made(cv)
    for it in _items(cv, made):                  # per-proof zkt_verify: the verdict every batch below must share
        assert _lib.verify(cv.name, *it[:7], h, beta_h, it[7])
    big = _cycle(made, 67)                       # crosses the wave and workgroup boundaries of the 13 * count launch
    for entries in (made, made[:1], big):
        assert ctx.verify_batch_dev(_items(cv, entries), h, beta_h)
        assert _lib.verify_batch(cv.name, _items(cv, entries), h, beta_h)
    assert not ctx.verify_batch_dev(_items(cv, made), h, wrong)                    # another trapdoor
    for k in (0, 33, 66):                                                          # a flipped evaluation byte in proof k
        vk, pis, proof, kind = big[k]
        bad = bytearray(proof)
        bad[-40] ^= 1
        assert not ctx.verify_batch_dev(_items(cv, big[:k] + [(vk, pis, bytes(bad), kind)] + big[k + 1:]), h, beta_h)
    vk, pis, proof, kind = made[1]
    assert not ctx.verify_batch_dev(_items(cv, [made[0], (vk, ((pis[0] + 1) % cv.fr.p,) + pis[1:], proof, kind), made[2]]), h, beta_h)
    # two proofs of the same shape swapped between their statements
    assert not ctx.verify_batch_dev(_items(cv, [made[0][:2] + made[2][2:], made[1], made[2][:2] + made[0][2:]]), h, beta_h)
    assert ctx.verify_batch_dev(_items(cv, made), h, beta_h)                       # and the context still accepts


def _times_r(cv, P):
    """r P (oracle.curve.scalar_mul reduces its scalar mod r, so r - 1 times and once more)"""
    return C.add(cv, C.scalar_mul(cv, cv.fr.p - 1, P), P)


def _off_curve_x(cv):
    q, x = cv.fq.p, 1
    while True:
        rhs = (x * x * x + cv.b) % q
        if rhs and pow(rhs, (q - 1) // 2, q) != 1:
            return x
        x += 1


@pytest.mark.parametrize("cv", CURVES, ids=lambda c: c.name)
def test_errors(ctxs, cv):
    import zkt_plonk_amd as z
    from zkt_plonk_amd import _lib
    ctx = ctxs[cv.name]
    made, srs, h, beta_h, wrong = _made(cv)
    nb = (cv.fq.bits + 2 + 7) // 8

    def with_proof(k, raw):
        return made[:k] + [made[k][:2] + (raw,) + made[k][3:]] + made[k + 1:]

    with pytest.raises(z.ZktError) as e:                                           # truncated bytes
        ctx.verify_batch_dev(_items(cv, with_proof(2, made[2][2][:-1])), h, beta_h)
    assert e.value.code == 1 and "proof 2" in str(e.value)
    with pytest.raises(z.ZktError) as e:                                           # the b commitment of proof 1: x off the curve
        raw = bytearray(made[1][2])
        raw[nb:2 * nb] = _off_curve_x(cv).to_bytes(nb, "little")
        ctx.verify_batch_dev(_items(cv, with_proof(1, bytes(raw))), h, beta_h)
    assert e.value.code == 1 and "proof 1" in str(e.value) and "commitment 1" in str(e.value) and "curve" in str(e.value)
    if cv.name == "bls12_381":
        rng = np.random.default_rng(5)
        q = cv.fq.p
        while True:
            x = int.from_bytes(rng.bytes(nb), "little") % q
            y = C.sqrt_mod((x * x * x + cv.b) % q, q)
            if y is not None and _times_r(cv, (x, y)) is not None:
                break
        with pytest.raises(z.ZktError) as e:                                       # on the curve, outside the subgroup
            raw = bytearray(made[2][2])
            raw[6 * nb:7 * nb] = x.to_bytes(nb, "little")
            ctx.verify_batch_dev(_items(cv, with_proof(2, bytes(raw))), h, beta_h)
        assert e.value.code == 1 and "proof 2" in str(e.value) and "commitment 6" in str(e.value) and "subgroup" in str(e.value)
    with pytest.raises(z.ZktError) as e:
        ctx.verify_batch_dev([], h, beta_h)
    assert e.value.code == 1
    with pytest.raises(z.ZktError) as e:
        ctx.verify_batch_prepare_dev([], h, beta_h)
    assert e.value.code == 1
    # a count above the cap is refused before any item is read
    L = z.lib()
    ins, trs, k, hh, bh, keep = _lib._verify_batch_args(ctx.curve, _items(cv, made[:1]), h, beta_h)
    ok = ctypes.c_int(7)
    u = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    assert L.zkt_verify_batch_dev(ctx.handle, ins, trs, _lib.VERIFY_BATCH_DEV_MAX + 1, u(hh), u(bh), ctypes.byref(ok)) == 1
    assert b"ZKT_VERIFY_BATCH_DEV_MAX" in L.zkt_last_error(ctx.handle) and ok.value == 7
    assert ctx.verify_batch_dev(_items(cv, made), h, beta_h)                       # none of it sticks


def _host_fold(cv, entries, rho, h, beta_h):
    """sum_j rho_j L_j and sum_j rho_j W_j from zkt_verify_prepare's pairs, on the host."""
    from zkt_plonk_amd import _lib
    Ls, Ws = [], []
    for e in entries:
        it = _item(cv, e)
        pairs, _ = _lib.verify_prepare(cv.name, *it[:7], it[7])
        Ls += [pairs[0], pairs[2]]
        Ws += [pairs[1], pairs[3]]
    return (_lib.g1_msm_host(cv.name, np.stack(Ls), rho, montgomery=False),
            _lib.g1_msm_host(cv.name, np.stack(Ws), rho, montgomery=False))


@pytest.mark.parametrize("count", [3, 67])
@pytest.mark.parametrize("cv", CURVES, ids=lambda c: c.name)
def test_fold_is_bit_exact_and_merging_goes_by_content(ctxs, cv, count):
    ctx = ctxs[cv.name]
    made, srs, h, beta_h, wrong = _made(cv)
    entries = _cycle(made, count)
    ab, inf, rho = ctx.verify_batch_prepare_dev(_items(cv, entries), h, beta_h)
    assert rho.shape == (2 * count, 4)
    assert rho[0].tolist() == [1, 0, 0, 0]
    assert not rho[:, 2:].any()                                                    # 128-bit coefficients
    assert len({tuple(r) for r in rho.tolist()}) == 2 * count                      # pairwise distinct
    (a_want, a_inf), (b_want, b_inf) = _host_fold(cv, entries, rho, h, beta_h)
    assert np.array_equal(ab[0], a_want) and np.array_equal(ab[1], b_want)
    assert inf.tolist() == [a_inf, b_inf] == [False, False]
    # one shared verifier-key array per circuit, or a separate copy per item: the same bases, scalars and coefficients
    ab2, inf2, rho2 = ctx.verify_batch_prepare_dev(_items(cv, entries, shared=False), h, beta_h)
    assert np.array_equal(ab, ab2) and np.array_equal(rho, rho2) and inf.tolist() == inf2.tolist()
    # the coefficients depend on every input: another beta h, other coefficients
    _, _, rho3 = ctx.verify_batch_prepare_dev(_items(cv, entries), h, wrong)
    assert not np.array_equal(rho[1:], rho3[1:]) and rho3[0].tolist() == [1, 0, 0, 0]


def _small_proof_setup(cv):
    cs = P.test_circuit(cv)
    n = cs.circuit_bound()
    srs = K.srs_mont(cv, 0x5EED, n + 8)
    be = K.CBackend(cv, srs)
    pk, epk, vk = P.setup(be, [None] * (n + 8), cs, True)
    blinders = [[(i + 1 + 100 * k) * 0x9E3779B97F4A7C15 % cv.fr.p for i in range(P.NUM_BLINDERS)] for k in range(2)]
    want = [P.prove(be, [None] * (n + 8), pk, epk, vk, cs, P.new_seeded_transcript(cv, vk), b).serialize(cv) for b in blinders]
    return cs, n, srs, pk, vk, blinders, want


def test_an_announced_proof_keeps_its_bytes():
    """Prove, announce the next proof (zkt_prove_set_next), verify a batch on the same context, run the announced proof:
    its bytes are those of the proof made with nothing in between.  Once more on a forked context."""
    import zkt_plonk_amd as z
    cv = F.BN254
    made, _, h, beta_h, wrong = _made(cv)
    cs, n, srs, pk, vk, blinders, want = _small_proof_setup(cv)
    ctx = z.Context(cv.name, 0)
    try:
        ctx.srs_load(srs)
        z.GpuProver(ctx, n.bit_length() - 1, {k: K.fr_to_mont(cv, pk.polys[k]) for k in z.PK_ORDER})
        a, b, c = cs.wire_evals(cs.n_gates)
        wires = [K.fr_to_mont(cv, w) for w in (a, b, c)]
        table = K.fr_to_mont(cv, cs.table)
        pi_pos = sorted(cs.pi)
        pi_vals = K.fr_to_mont(cv, [cs.pi[k] for k in pi_pos])

        def tr():
            return z.seed_transcript(z.Transcript("merlin", "ZKT Plonk"), vk.n, vk.commits)

        def round_trip(c):
            d = []
            for w in wires:
                d.append(c.alloc(w.nbytes))
                c.upload(d[-1], w)
            try:
                preps = [c.prepare_dev(d[0], d[1], d[2], cs.n_gates, table, pi_pos, pi_vals, K.fr_to_mont(cv, x)) for x in blinders]
                assert c.prove_prepared(preps[0], tr(), preps[1]) == want[0]        # proof 1 is announced
                assert c.verify_batch_dev(_items(cv, made), h, beta_h)
                assert not c.verify_batch_dev(_items(cv, made), h, wrong)
                assert c.prove_prepared(preps[1], tr()) == want[1]
            finally:
                for x in d:
                    c.free(x)

        round_trip(ctx)
        fork = ctx.fork()
        try:
            z.GpuProver(fork, n.bit_length() - 1)
            round_trip(fork)
        finally:
            fork.close()
        round_trip(ctx)                                                             # and the parent is none the worse
        assert ctx.msm_info()["srs_count"] == n + 8                                 # under the key it was given
    finally:
        ctx.close()
