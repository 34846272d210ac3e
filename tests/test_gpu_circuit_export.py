"""GPU: the keys that device setup makes, handed back -- zkt_circuit_export (ProverKey), zkt_circuit_commitments / _check_vk_file
(VerifierKey), zkt_circuit_export_epk / _write_epk_file (ExtendedProverKey), zkt_circuit_save_files / zkt_srs_save_file (the
files of the reference CLI's `Compile`, bin/src/main.rs:105-111) -- against the oracle's setup (oracle/plonk.py) and its
key-file writers (oracle/keyfile.py).  Every proving case uses n >= 2^7."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import fields as F, plonk as P, coracle as K, keyfile as KF
from helpers import field_elems
import sigma_cases as SC

CURVES = [F.BN254, F.BLS12_381]
SEL7 = ("q_m", "q_l", "q_r", "q_o", "q_c", "q_lookup", "q_table")


@pytest.fixture(scope="module")
def ctxs():
    import zkt_plonk_amd as z
    c = {cv.name: z.Context(cv.name, 0) for cv in CURVES}
    yield c
    for x in c.values():
        x.close()


_ORACLE = {}


def _oracle(cv, log_n):
    """The oracle's setup of one circuit per (curve, size), computed once and left unchanged: log_n = 3 has 7 rows (no power
    of two) and five all-zero selectors, whose commitments are the identity."""
    key = (cv.name, log_n)
    if key not in _ORACLE:
        cs = {3: lambda: P.synthetic_circuit(cv, 5, 2, seed=1), 6: lambda: P.synthetic_circuit(cv, 40, 8, seed=6),
              7: lambda: P.synthetic_circuit(cv, 100, 16, seed=7)}[log_n]()
        n = cs.circuit_bound()
        assert n == 1 << log_n
        srs = K.srs_mont(cv, 0xC0DE + log_n, n + 8)
        be = K.CBackend(cv, srs)
        pk, epk, vk = P.setup(be, [None] * (n + 8), cs, True)
        evals = P.setup_evals(be, cs)
        s = dict(cv=cv, cs=cs, n=n, log_n=log_n, srs=srs, be=be, pk=pk, epk=epk, vk=vk,
                 evals7={k: K.fr_to_mont(cv, evals[k]) for k in SEL7},
                 idx=[SC.to_index(w, P.ZERO_VAR) for w in (cs.w_l, cs.w_r, cs.w_o)])
        if log_n >= 7:
            blinders = field_elems(cv.fr.p, 91, P.NUM_BLINDERS)
            a, b, c = cs.wire_evals(cs.n_gates)
            pos = sorted(cs.pi)
            s.update(proof=P.prove(be, [None] * (n + 8), pk, epk, vk, cs, P.new_seeded_transcript(cv, vk), blinders).serialize(cv),
                     wires=[K.fr_to_mont(cv, x) for x in (a, b, c)], table=K.fr_to_mont(cv, cs.table), pos=pos,
                     pi_vals=K.fr_to_mont(cv, [cs.pi[i] for i in pos]), blinders=K.fr_to_mont(cv, blinders))
        _ORACLE[key] = s
    return _ORACLE[key]


def _mont(cv, vals):
    return K.fr_to_mont(cv, vals) if len(vals) else np.zeros((0, 4), dtype=np.uint64)


def _setup_wiring(ctx, s):
    ctx.srs_load(s["srs"])
    evals = [s["evals7"].get(k) for k in P.PK_POLYS]
    return ctx.circuit_setup_wiring(s["log_n"], evals, s["idx"][0], s["idx"][1], s["idx"][2], len(s["cs"].values))


def _commit_points(cv, commits, inf):
    return [None if inf[k] else K.points_from_mont(cv, commits[k:k + 1])[0] for k in range(10)]


def _transcript(z, cv, n, commits):
    tr = z.Transcript("merlin", "ZKT Plonk", fr_bits=cv.fr.bits, fq_bytes=cv.fq.limbs64 * 8)
    return z.seed_transcript(tr, n, commits)


def _prove(z, ctx, s, commits=None):
    tr = _transcript(z, s["cv"], s["n"], s["vk"].commits if commits is None else commits)
    return ctx.prove(s["wires"][0], s["wires"][1], s["wires"][2], s["table"], s["pos"], s["pi_vals"], s["blinders"], tr)


@pytest.mark.parametrize("cv", CURVES, ids=lambda c: c.name)
def test_export_trims_at_every_edge(cv, ctxs):
    """zkt_circuit_load at log_n = 10 of hand-made polynomials, zero-padded to n: zkt_circuit_export returns their true lengths
    (DensePolynomial::from_coefficients_vec) and values, with and without a download."""
    from zkt_plonk_amd import _lib
    ctx = ctxs[cv.name]
    n = 1 << 10
    for load, lengths in enumerate(((0, 1, 2, 63, 64, 65, 255, 256, 257, 1023), (1024, 0, 1023, 1, 257, 2, 256, 65, 64, 63))):
        polys = []
        for k, ln in enumerate(lengths):
            vals = field_elems(cv.fr.p, 1000 * load + k, ln) if ln else []
            if ln:
                vals[-1] = vals[-1] or 1                    # the leading coefficient is what the length hangs on
            if ln > 4:
                vals[ln - 2] = vals[ln // 2] = vals[0] = 0  # zeros that are not trailing stay
            polys.append(vals)
        padded = [np.concatenate([_mont(cv, v), np.zeros((n - len(v), 4), dtype=np.uint64)]) for v in polys]
        ctx.circuit_load(10, padded)
        live = _lib.debug_live_allocations()
        assert ctx.circuit_export(lengths_only=True) == list(lengths)
        got = ctx.circuit_export()
        assert _lib.debug_live_allocations() == live
        for k, ln in enumerate(lengths):
            assert got[k].shape == (ln, 4), (load, k)
            assert K.fr_from_mont(cv, got[k]) == polys[k] if ln else got[k].size == 0, (load, k)


@pytest.mark.parametrize("log_n", [3, 7])
@pytest.mark.parametrize("cv", CURVES, ids=lambda c: c.name)
def test_export_after_setup_from_the_wiring_is_the_oracles_prover_key(cv, log_n, ctxs):
    s = _oracle(cv, log_n)
    assert log_n != 3 or s["cs"].n_gates & (s["cs"].n_gates - 1)
    ctx = ctxs[cv.name]
    _setup_wiring(ctx, s)
    got = ctx.circuit_export()
    for k, name in enumerate(P.PK_POLYS):
        assert K.fr_from_mont(cv, got[k]) == list(s["pk"].polys[name]) if len(got[k]) else len(s["pk"].polys[name]) == 0, name
    assert ctx.circuit_export(lengths_only=True) == [len(s["pk"].polys[k]) for k in P.PK_POLYS]


@pytest.mark.parametrize("log_n", [3, 7])
@pytest.mark.parametrize("cv", CURVES, ids=lambda c: c.name)
def test_commitments_of_a_loaded_prover_key(cv, log_n, ctxs):
    """zkt_circuit_commitments after zkt_circuit_load of the exported polynomials: what setup returned, and the oracle's
    VerifierKey; the all-zero selectors of the log_n = 3 circuit commit to the identity."""
    from zkt_plonk_amd import _lib
    s = _oracle(cv, log_n)
    ctx = ctxs[cv.name]
    from_setup, inf_setup = _setup_wiring(ctx, s)
    polys = ctx.circuit_export()
    ctx.circuit_load(log_n, polys)
    live = _lib.debug_live_allocations()
    commits, inf = ctx.circuit_commitments()
    assert _lib.debug_live_allocations() == live
    assert np.array_equal(commits, from_setup) and list(inf) == list(inf_setup)
    want = [s["vk"].commits[k] for k in P.PK_POLYS]
    assert _commit_points(cv, commits, inf) == want
    assert (log_n == 3) == (None in want)
    for k in range(10):
        assert not inf[k] or not commits[k].any()
    if log_n == 7:                                          # the key need only reach the longest polynomial
        longest = max(len(p) for p in polys)
        ctx.srs_load(s["srs"][:longest])
        again, inf2 = ctx.circuit_commitments()
        assert np.array_equal(again, commits) and list(inf2) == list(inf)
        ctx.srs_load(s["srs"][:longest - 1])
        with pytest.raises(_lib.ZktError) as e:
            ctx.circuit_commitments()
        assert e.value.code == 5, "ZKT_ERR_TOO_MANY_COEFFICIENTS"


@pytest.mark.parametrize("log_n", [3, 6])
@pytest.mark.parametrize("cv", CURVES, ids=lambda c: c.name)
def test_extended_prover_key_vectors_and_file(cv, log_n, ctxs, tmp_path):
    from zkt_plonk_amd import _lib
    s = _oracle(cv, log_n)
    n = s["n"]
    ctx = ctxs[cv.name]
    _setup_wiring(ctx, s)
    vecs = KF.extended_prover_key_vectors(s["epk"])
    live = _lib.debug_live_allocations()
    lens, none = ctx.circuit_export_epk()
    assert none is None and lens == [len(vecs[k]) for k in KF.EPK_ORDER]
    for i, name in enumerate(KF.EPK_ORDER):
        lens, got = ctx.circuit_export_epk(i)
        assert K.fr_from_mont(cv, got) == [v % cv.fr.p for v in vecs[name]], name
        with pytest.raises(_lib.ZktError) as e:             # room for one element too few
            ctx.circuit_export_epk(i, cap=lens[i] - 1)
        assert e.value.code == 1
    f = tmp_path / "epk.bin"
    ctx.write_epk_file(str(f))
    assert _lib.debug_live_allocations() == live
    assert [p.name for p in tmp_path.iterdir()] == ["epk.bin"], "a temporary file stayed"
    assert f.read_bytes() == KF.extended_prover_key_bytes(cv, s["epk"])
    assert ctx.check_epk_file(str(f)) is None
    with pytest.raises(_lib.ZktError) as e:
        ctx.write_epk_file(str(tmp_path / "missing" / "epk.bin"))
    assert "missing" in str(e.value)
    assert _lib.debug_live_allocations() == live


@pytest.mark.parametrize("cv", CURVES, ids=lambda c: c.name)
def test_compile_on_one_context_prove_from_the_files_on_another(cv, ctxs, tmp_path):
    """`Compile` (bin/src/main.rs:105-111) on context A, a prover started from its files on a fresh context B: the same proof
    bytes as A's and the oracle's, accepted by zkt_verify under the file's VerifierKey; zkt_circuit_check_vk_file finds the
    file's key to be B's own, and names the commitment that a flipped byte damages."""
    import zkt_plonk_amd as z
    from zkt_plonk_amd import _lib
    from oracle import pairing as PR
    from test_pairing_host import g2_mont
    s = _oracle(cv, 7)
    n, cs = s["n"], s["cs"]
    A = ctxs[cv.name]
    _setup_wiring(A, s)
    ck, pk, vk = (str(tmp_path / x) for x in ("ck", "pk", "vk"))
    A.circuit_save_files(pk, vk, None, s["pos"])
    A.srs_save_file(ck)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["ck", "pk", "vk"]
    assert open(ck, "rb").read() == KF.committer_key_bytes(cv, K.points_from_mont(cv, s["srs"]))
    assert open(pk, "rb").read() == KF.prover_key_bytes(cv, s["pk"])
    assert open(vk, "rb").read() == KF.verifier_key_bytes(cv, s["vk"])
    A.srs_save_file(ck, n + 1)                              # a prefix of the key
    assert open(ck, "rb").read() == KF.committer_key_bytes(cv, K.points_from_mont(cv, s["srs"][:n + 1]))
    A.srs_save_file(ck)
    for bad in ([5, 5], [6, 5], [n], [0, n + 3]):           # positions: ascending, distinct, below n -- else nothing is written
        with pytest.raises(_lib.ZktError) as e:
            A.circuit_save_files(str(tmp_path / "pk2"), str(tmp_path / "vk2"), None, bad)
        assert e.value.code == 1
    assert sorted(p.name for p in tmp_path.iterdir()) == ["ck", "pk", "vk"]
    proof_a = _prove(z, A, s)
    assert proof_a == s["proof"]
    B = z.Context(cv.name, 0)
    try:
        B.srs_load_file(ck)
        B.circuit_load_file(pk, 7)
        n_, roots, commits, inf = _lib.keyfile_verifier_key(vk, cv.name)
        assert n_ == n and K.fr_from_mont(cv, roots) == s["vk"].pi_roots
        pts = dict(zip(z.PK_ORDER, _commit_points(cv, commits, inf)))
        assert _prove(z, B, s, pts) == proof_a
        tau = 0xC0DE + 7
        H = PR.G2_GENERATORS[cv.name]
        ok = _lib.verify(cv.name, n_, commits, list(inf), roots, s["pi_vals"], proof_a, s["srs"][0], g2_mont(cv, [H])[0],
                         g2_mont(cv, [PR.Tower(cv).g2_mul(tau, H)])[0], _transcript(z, cv, n_, pts))
        assert ok
        assert B.check_vk_file(vk) is None
        blob = bytearray(open(vk, "rb").read())
        nb = 8 * cv.fq.limbs64
        first = 16 + 32 * len(s["pos"])
        for k in (0, 4, 9):
            b = bytearray(blob)
            b[first + k * 2 * nb + 3] ^= 1                  # a byte of commitment k's x
            (tmp_path / "vk_bad").write_bytes(bytes(b))
            assert B.check_vk_file(str(tmp_path / "vk_bad")) == k
        b = bytearray(blob)
        b[1] ^= 1                                           # another n
        (tmp_path / "vk_bad").write_bytes(bytes(b))
        assert B.check_vk_file(str(tmp_path / "vk_bad")) == 10
        assert _prove(z, B, s, pts) == proof_a
    finally:
        B.close()


@pytest.mark.parametrize("cv", CURVES, ids=lambda c: c.name)
def test_exports_leave_the_prover_and_the_allocations_as_they_were(cv, ctxs, tmp_path):
    """A proof before and a proof after export, commitments, export_epk and write_epk_file are byte-equal; a fork's exports are
    its parent's; with a next proof announced the three work-buffer calls are refused and export is served."""
    import ctypes
    import zkt_plonk_amd as z
    from zkt_plonk_amd import _lib
    s = _oracle(cv, 7)
    ctx = ctxs[cv.name]
    from_setup, inf_setup = _setup_wiring(ctx, s)
    before = _prove(z, ctx, s)
    assert before == s["proof"]
    live = _lib.debug_live_allocations()
    polys = ctx.circuit_export()
    assert _lib.debug_live_allocations() == live
    commits, inf = ctx.circuit_commitments()
    assert _lib.debug_live_allocations() == live
    epk = [ctx.circuit_export_epk(i)[1] for i in range(17)]
    assert _lib.debug_live_allocations() == live
    ctx.write_epk_file(str(tmp_path / "epk"))
    assert _lib.debug_live_allocations() == live
    assert ctx.check_vk_file(_vk_file(cv, s, tmp_path)) is None
    assert _lib.debug_live_allocations() == live
    assert np.array_equal(commits, from_setup) and list(inf) == list(inf_setup)
    assert _prove(z, ctx, s) == before
    fork = ctx.fork()
    try:
        for k, p in enumerate(fork.circuit_export()):
            assert np.array_equal(p, polys[k])
        fc, fi = fork.circuit_commitments()
        assert np.array_equal(fc, commits) and list(fi) == list(inf)
        for i in (0, 5, 9, 14, 15, 16):
            assert np.array_equal(fork.circuit_export_epk(i)[1], epk[i]), i
        fork.write_epk_file(str(tmp_path / "epk_fork"))
        assert (tmp_path / "epk_fork").read_bytes() == (tmp_path / "epk").read_bytes()
        assert _prove(z, fork, s) == before
    finally:
        fork.close()
    assert _lib.debug_live_allocations() == live
    # a successor announced and its early rounds issued behind a proof: the calls are served (the early work is redone)
    prep = ctx.prepare_host(s["wires"][0], s["wires"][1], s["wires"][2], s["table"], s["pos"], s["pi_vals"], s["blinders"])
    tr = lambda: _transcript(z, cv, s["n"], s["vk"].commits)
    assert ctx.prove_prepared(prep, tr(), next_prep=prep) == before
    c2, i2 = ctx.circuit_commitments()
    assert np.array_equal(c2, commits) and np.array_equal(ctx.circuit_export_epk(16)[1], epk[16])
    assert ctx.prove_prepared(prep, tr()) == before
    # a next proof announced (zkt_prove_set_next) and not yet begun: the work buffers are spoken for
    ctx.check(ctx._L.zkt_prove_set_next(ctx.handle, ctypes.byref(prep.struct)))
    for refused in (ctx.circuit_commitments, lambda: ctx.circuit_export_epk(0), lambda: ctx.write_epk_file(str(tmp_path / "no")),
                    lambda: ctx.check_vk_file(str(tmp_path / "vk")), lambda: ctx.circuit_save_files(None, str(tmp_path / "no"))):
        with pytest.raises(_lib.ZktError) as e:
            refused()
        assert e.value.code == 1 and "announced" in str(e.value)
    assert not (tmp_path / "no").exists()
    for k, p in enumerate(ctx.circuit_export()):
        assert np.array_equal(p, polys[k])
    ctx.circuit_save_files(str(tmp_path / "pk_only"))       # the ProverKey alone needs no work buffer either
    assert (tmp_path / "pk_only").read_bytes() == KF.prover_key_bytes(cv, s["pk"])
    assert ctx.prove_prepared(prep, tr()) == before         # (withdraws the announcement)
    assert _lib.debug_live_allocations() == live


def _vk_file(cv, s, tmp_path):
    f = tmp_path / "vk"
    f.write_bytes(KF.verifier_key_bytes(cv, s["vk"]))
    return str(f)
