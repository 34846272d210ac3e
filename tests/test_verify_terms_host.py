"""CPU: the batch verifier's term stage as the kernel computes it (csrc/verify_terms.hpp on the core's transcript state,
zkt_debug_verify_terms_host route 1) against the host route (route 0: the same replay through the handle's own calls, which
the verifier tests hold to the oracle and tests/test_verify_terms_pinned.py to what it returned before the two shared code): statuses, the seven challenges, r0 and the 24 sums, integer for
integer, over the table of tests/verify_terms_cases.py on both curves, and where every transcript handle is left.  The
STROBE-128 and Keccak-256 of the shared file against the known answers of tests/test_transcript_host.py and against the
handles' own calls on random traffic."""
import os
import random
import re

import numpy as np
import pytest

from oracle import fields as F, plonk as P, curve as C, coracle as K

import verify_terms_cases as TC

CURVES = [F.BN254, F.BLS12_381]
IDS = lambda c: c.name  # noqa: E731
HERE = os.path.dirname(os.path.abspath(__file__))


def _both_routes(cv, rows, rho):
    """-> (route 0's result, route 1's) after checking that they and the handles' probes are equal"""
    from zkt_plonk_amd import _lib
    forced = TC.forced_array(cv, rows)
    out, left = [], []
    for route in (0, 1):
        its = TC.items(cv, rows)
        out.append(_lib.debug_verify_terms_host(cv.name, its, rho, forced, route))
        left.append(TC.probes(its))
    for name, a, b in zip(("challenges", "r0", "sums", "status"), out[0], out[1]):
        assert np.array_equal(a, b), name
    assert left[0] == left[1]
    return out[0]


@pytest.mark.parametrize("cv", CURVES, ids=IDS)
def test_the_shared_code_equals_the_host_code_on_every_row(cv):
    rows = list(TC.ROWS(cv))
    ch, r0, acc, status = _both_routes(cv, rows, TC.rho_array(cv, len(rows)))
    assert not status.any()
    assert ch.reshape(len(rows), -1).any(axis=1).all() and acc.reshape(len(rows), -1).any(axis=1).all()
    # one row at a time and without coefficients (all ones): the same challenges, whatever the batch around a proof
    for i in (0, 1, 13, len(rows) - 1):
        one = _both_routes(cv, rows[i:i + 1], None)
        assert np.array_equal(one[0][0], ch[i]) and np.array_equal(one[1][0], r0[i])


@pytest.mark.parametrize("cv", CURVES, ids=IDS)
def test_forced_challenges_refusals_and_edge_points(cv):
    rows, want = TC.FORCED(cv)
    ch, r0, acc, status = _both_routes(cv, list(rows), TC.rho_array(cv, len(rows), seed=6))
    assert status.tolist() == list(want)
    forced = TC.forced_array(cv, rows)
    for i, (row, st) in enumerate(zip(rows, want)):
        drawn = {TC.OK: 7, TC.ZERO_DENOMINATOR: 6, TC.EQUAL_CHALLENGES: 4}[st]
        assert np.array_equal(ch[i, :drawn], forced[i, :drawn]), row.name       # the forced values are what was used ...
        assert not ch[i, drawn:].any(), row.name                                 # ... as far as the proof got
        assert acc[i].any() == (st == TC.OK) and (st == TC.OK or not r0[i].any()), row.name


@pytest.mark.parametrize("cv", CURVES, ids=IDS)
def test_a_batch_with_two_refused_proofs(cv):
    rows, want = TC.two_refusals(cv)
    status = _both_routes(cv, list(rows), None)[3]
    assert status.tolist() == list(want)
    assert np.flatnonzero(status).tolist() == [5, 9]


def _oracle_challenges(cv, vk, pis, raw, kind):
    """the seven challenges of one proof from oracle/transcript.py, replayed in Python"""
    tr = P.new_seeded_transcript(cv, vk, kind)
    nb = TC._nb(cv)
    pts, pos = [], 0
    for k in range(13):
        pts.append(C.point_deserialize_compressed(cv, raw[pos:pos + nb]))
        pos += nb + (1 if k >= 11 else 0)
    evs = [int.from_bytes(raw[pos + 32 * i:pos + 32 * i + 32], "little") for i in range(12)]
    out = []
    tr.append_scalars("pi", list(pis))
    for name, pt in zip(("a", "b", "c", "t", "h1", "h2"), pts[:6]):
        tr.append_commitment(name + "_commit", pt)
    out += [tr.challenge_scalar(c) for c in ("beta", "gamma", "delta", "epsilon")]
    for name, pt in zip(("z1", "z2"), pts[6:8]):
        tr.append_commitment(name + "_commit", pt)
    out.append(tr.challenge_scalar("alpha"))
    for name, pt in zip(("q_lo", "q_mid", "q_hi"), pts[8:11]):
        tr.append_commitment(name + "_commit", pt)
    out.append(tr.challenge_scalar("xi"))
    for name, v in zip(("a_eval", "b_eval", "c_eval", "sigma1_eval", "sigma2_eval", "z1_next_eval", "q_lookup_eval", "t_eval",
                        "t_next_eval", "z2_next_eval", "h1_next_eval", "h2_eval"), evs):
        tr.append_scalar(name, v)
    out.append(tr.challenge_scalar("eta"))
    return out


@pytest.mark.parametrize("cv", CURVES, ids=IDS)
def test_the_real_proofs_draw_the_oracles_challenges(cv):
    from zkt_plonk_amd import _lib
    from test_gpu_verify_batch import _made
    rows = [r for r in TC.ROWS(cv) if r.name.startswith("real")]
    assert len(rows) == 3
    ch = _lib.debug_verify_terms_host(cv.name, TC.items(cv, rows), None, None, 1)[0]
    for i, (vk, pis, raw, kind) in enumerate(_made(cv)[0]):
        assert K.fr_from_mont(cv, ch[i]) == _oracle_challenges(cv, vk, pis, raw, kind), i


def _known_answers():
    """the hexadecimal answers of tests/test_transcript_host.py, in its order: merlin's vector, then the three of the
    Ethereum transcript"""
    found = re.findall(r'"([0-9a-f]{64})"', open(os.path.join(HERE, "test_transcript_host.py")).read())
    assert len(found) == 4
    return found


def test_strobe_and_keccak256_of_the_shared_code_give_the_known_answers():
    import zkt_plonk_amd as z
    from zkt_plonk_amd._lib import debug_verify_terms_transcript as shared
    merlin, e1, e2, e3 = _known_answers()
    t = z.Transcript("merlin", "test protocol")
    shared(t, 0, b"some label", b"some data")
    assert shared(t, 2, b"challenge", bits=264).hex() == merlin                 # 264 bits: 32 bytes of prf
    # gadgets/src/transcript.rs:101-127; the u64 is appended by the handle, the shared code has no such call
    e = z.Transcript("ethereum", "test")
    e.append_u64("a", 1)
    assert shared(e, 2, b"a", bits=254)[::-1].hex() == e1
    shared(e, 0, b"b", (2).to_bytes(32, "little"))
    assert shared(e, 2, b"b", bits=254)[::-1].hex() == e2
    shared(e, 1, b"c", (3).to_bytes(32, "little") + (4).to_bytes(32, "little"))
    assert shared(e, 2, b"c", bits=254)[::-1].hex() == e3


def test_random_traffic_through_the_shared_code_matches_the_handles_own_calls():
    import zkt_plonk_amd as z
    from zkt_plonk_amd._lib import debug_verify_terms_transcript as shared
    rnd = random.Random(11)
    for cv in CURVES:
        nb = cv.fq.limbs64 * 8
        G = C.generator(cv)
        for kind in ["merlin"] + (["ethereum"] if cv.name == "bn254" else []):
            mine, ref = (z.Transcript(kind, "ZKT Plonk", fr_bits=cv.fr.bits, fq_bytes=nb) for _ in range(2))
            for step in range(300):                          # far more than one sponge block of traffic
                op = rnd.randrange(3)
                if op == 0:
                    v = rnd.randrange(cv.fr.p)
                    shared(mine, 0, b"a_eval", v.to_bytes(32, "little")); ref.append_scalar("a_eval", v)
                elif op == 1:
                    pt = C.scalar_mul(cv, rnd.randrange(1, 1 << 20), G)
                    data = pt[0].to_bytes(nb, "little") + pt[1].to_bytes(nb, "little")
                    shared(mine, 1, b"t_commit", data); ref.append_commitment("t_commit", pt)
                else:
                    got = int.from_bytes(shared(mine, 2, b"beta", bits=cv.fr.bits), "little")
                    assert got == ref.challenge_scalar("beta"), (cv.name, kind, step)
            assert mine.challenge_scalar("eta") == ref.challenge_scalar("eta")


def test_arguments_are_checked():
    import ctypes
    from zkt_plonk_amd import _lib
    cv = F.BN254
    rows = list(TC.ROWS(cv))[:2]
    with pytest.raises(_lib.ZktError) as e:
        _lib.debug_verify_terms_host(cv.name, TC.items(cv, rows), None, None, 2)       # route 2 needs a context
    assert e.value.code == 1
    bad = rows[0]._replace(entry=rows[0].entry[:4] + (rows[0].entry[4][:-1],) + rows[0].entry[5:])
    with pytest.raises(_lib.ZktError) as e:
        _lib.debug_verify_terms_host(cv.name, TC.items(cv, [bad]), None, None, 1)      # a truncated proof
    assert e.value.code == 1
