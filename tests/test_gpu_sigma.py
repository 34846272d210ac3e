"""zkt_circuit_sigma_dev / zkt_circuit_setup_wiring: the sigma evaluations made on the device from the wiring
(permutation/mod.rs:76-177) against the CPU oracle, element for element, and the setup that is fed by them against the
oracle's VerifierKey and proof bytes.  The expected values of the raw cases come from tests/sigma_cases.py, which
tests/test_sigma_rule_host.py pins against the oracle."""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import fields as F, plonk as P, coracle as K
from helpers import field_elems

import sigma_cases as SC

CURVES = [F.BN254, F.BLS12_381]
SEL7 = ("q_m", "q_l", "q_r", "q_o", "q_c", "q_lookup", "q_table")
ERR_INVALID_ARGUMENT, ERR_INVALID_DOMAIN_SIZE = 1, 2


@pytest.fixture(scope="module")
def ctxs():
    import zkt_plonk_amd as z
    c = {cv.name: z.Context(cv.name, 0) for cv in CURVES}
    yield c
    for x in c.values():
        x.close()


class DevWiring:
    """three uint32 index vectors resident in HBM"""

    def __init__(self, ctx, cols):
        self.ctx, self.ptrs = ctx, []
        self.rows = len(cols[0])
        for x in cols:
            x = np.ascontiguousarray(x, dtype=np.uint32)
            d = ctx.alloc(max(4, x.nbytes))
            if x.size:
                ctx.upload(d, x)
            self.ptrs.append(d)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for d in self.ptrs:
            self.ctx.free(d)


def _sigma(ctx, log_n, cols, n_vars):
    with DevWiring(ctx, cols) as dw:
        return ctx.circuit_sigma(log_n, dw.ptrs[0], dw.ptrs[1], dw.ptrs[2], dw.rows, n_vars)


def _indices(cs):
    return [SC.to_index(w, P.ZERO_VAR) for w in (cs.w_l, cs.w_r, cs.w_o)]


# ---- 1. oracle circuits ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cv", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("which", ["test_circuit", "synthetic"])
def test_sigma_of_oracle_circuits(cv, which, ctxs):
    cs = P.test_circuit(cv, size=20) if which == "test_circuit" else P.synthetic_circuit(cv, 700, 32, seed=4242)
    n = cs.circuit_bound()
    assert n == (1 << 5 if which == "test_circuit" else 1 << 10)
    evals = P.setup_evals(K.CBackend(cv, K.srs_mont(cv, 3, 2)), cs)
    got = _sigma(ctxs[cv.name], n.bit_length() - 1, _indices(cs), len(cs.values))
    for j, name in enumerate(("sigma1", "sigma2", "sigma3")):
        assert np.array_equal(got[j], K.fr_to_mont(cv, evals[name])), name


# ---- 2. raw index vectors -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def raw():
    """name -> (case, expected three (n, 4) Montgomery arrays), computed once"""
    cv = F.BN254
    out = {}
    for name, case in SC.raw_cases().items():
        w, log_n = case["w"], case["log_n"]
        vals = SC.sigma_values(cv.fr.p, log_n, SC.sigma_targets(w[:, 0], w[:, 1], w[:, 2], 1 << log_n),
                               cv.fr.root_of_unity(1 << log_n))
        out[name] = (case, [K.fr_to_mont(cv, v) for v in vals])
    return out


@pytest.mark.parametrize("name", sorted(SC.raw_cases()))
def test_sigma_of_raw_index_vectors(name, raw, ctxs):
    case, want = raw[name]
    w = case["w"]
    got = _sigma(ctxs["bn254"], case["log_n"], [w[:, 0], w[:, 1], w[:, 2]], case["n_vars"])
    for j in range(3):
        bad = np.flatnonzero((got[j] != want[j]).any(axis=1))
        assert bad.size == 0, "sigma%d differs at %d rows, first %d" % (j + 1, bad.size, bad[0])


# ---- 3. determinism -------------------------------------------------------------------------------------------------
def test_sigma_is_the_same_every_time_and_on_a_fork(raw, ctxs):
    case, want = raw["b_long_runs_odd_rows"]
    w = case["w"]
    ctx = ctxs["bn254"]
    cols = [w[:, 0], w[:, 1], w[:, 2]]
    first = _sigma(ctx, case["log_n"], cols, case["n_vars"])
    again = _sigma(ctx, case["log_n"], cols, case["n_vars"])
    fork = ctx.fork()
    try:
        forked = _sigma(fork, case["log_n"], cols, case["n_vars"])
    finally:
        fork.close()
    for j in range(3):
        assert first[j].tobytes() == again[j].tobytes() == forked[j].tobytes() == want[j].tobytes()


# ---- 5. whole setup (before 4 and 6, which reuse its fixture) ---------------------------------------------------------
@pytest.fixture(scope="module")
def setups():
    """per curve: the oracle's setup and one proof of synthetic_circuit(cv, 700, 32, seed=4242), computed once"""
    out = {}
    for cv in CURVES:
        cs = P.synthetic_circuit(cv, 700, 32, seed=4242)
        n = cs.circuit_bound()
        srs_arr = K.srs_mont(cv, 0x7E57, n + 8)
        be = K.CBackend(cv, srs_arr)
        pk, epk, vk = P.setup(be, [None] * (n + 8), cs, True)
        evals = P.setup_evals(be, cs)
        blinders = field_elems(cv.fr.p, 31, P.NUM_BLINDERS)
        want = P.prove(be, [None] * (n + 8), pk, epk, vk, cs, P.new_seeded_transcript(cv, vk), blinders).serialize(cv)
        a, b, c = cs.wire_evals(cs.n_gates)
        out[cv.name] = dict(cs=cs, n=n, log_n=n.bit_length() - 1, srs=srs_arr, vk=vk, proof=want,
                            evals7={k: K.fr_to_mont(cv, evals[k]) for k in SEL7},
                            evals10={k: K.fr_to_mont(cv, v) for k, v in evals.items()},
                            wires=[K.fr_to_mont(cv, x) for x in (a, b, c)], table=K.fr_to_mont(cv, cs.table),
                            pi={i: K.fr_to_mont(cv, [v])[0] for i, v in cs.pi.items()}, blinders=K.fr_to_mont(cv, blinders))
    return out


def _affine(cv, xy):
    L = cv.fq.limbs64
    rinv = pow(1 << (64 * L), -1, cv.fq.p)
    return (sum(int(v) << (64 * i) for i, v in enumerate(xy[:L])) * rinv % cv.fq.p,
            sum(int(v) << (64 * i) for i, v in enumerate(xy[L:])) * rinv % cv.fq.p)


def _transcript(z, cv, s):
    tr = z.Transcript("merlin", "ZKT Plonk", fr_bits=cv.fr.bits, fq_bytes=8 * cv.fq.limbs64)
    return z.seed_transcript(tr, s["n"], s["vk"].commits)


def _prove(z, cv, prover, s):
    return prover.prove(s["wires"][0], s["wires"][1], s["wires"][2], s["table"], s["pi"], s["blinders"], _transcript(z, cv, s))


@pytest.mark.parametrize("cv", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("wiring", ["host", "device"])
def test_setup_from_the_wiring(cv, wiring, ctxs, setups):
    """zkt_circuit_setup_wiring = proof_system::setup from selectors, table mask and wiring: the oracle's ten VerifierKey
    commitments, and the proof that follows equals the oracle's bytes."""
    import zkt_plonk_amd as z
    ctx, s = ctxs[cv.name], setups[cv.name]
    cs = s["cs"]
    ctx.srs_load(s["srs"])
    idx = _indices(cs)
    if wiring == "host":
        prover, commits = z.GpuProver.setup_wiring(ctx, s["log_n"], s["evals7"], idx[0], idx[1], idx[2], len(cs.values))
    else:
        with DevWiring(ctx, idx) as dw:
            prover, commits = z.GpuProver.setup_wiring(ctx, s["log_n"], s["evals7"], dw.ptrs[0], dw.ptrs[1], dw.ptrs[2],
                                                       len(cs.values), n_rows=dw.rows)
    for name in z.PK_ORDER:
        xy, inf = commits[name]
        want = s["vk"].commits[name]
        if want is None:
            assert inf, name
        else:
            assert not inf and _affine(cv, xy) == want, name
    assert _prove(z, cv, prover, s) == s["proof"]


def test_setup_from_the_wiring_of_the_withdraw_layout(ctxs):
    """The bench's circuit at its smallest shape (n = 2^14): the ten commitments of zkt_circuit_setup_wiring equal those of
    zkt_circuit_setup fed with the host-made vectors (argsort + 3 n Python integers)."""
    import zkt_plonk_amd as z
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import withdraw_workload as WW
    cv = F.BN254
    ctx = ctxs[cv.name]
    log_n = min(WW.SHAPES)
    width, inputs, height = WW.SHAPES[log_n]
    hs = WW.reference_hasher(cv.fr.p, width)
    lay = WW.layout(hs, WW.make_instance(hs, inputs, height, seed=0x5EED))
    sel = WW.setup_vectors(lay, log_n, cv.fr.generator)
    evals = {name: K.fr_to_mont(cv, sel[name]) for name in z.PK_ORDER}
    ctx.srs_generate(0x5EED5EED, (1 << log_n) + 8)
    _, want = z.GpuProver.setup(ctx, log_n, evals)
    idx = [np.asarray(w, dtype=np.uint32) for w in lay.w]
    assert any((x == WW.ZERO).any() for x in idx) and lay.n_gates < 1 << log_n
    _, got = z.GpuProver.setup_wiring(ctx, log_n, {k: evals[k] for k in SEL7}, idx[0], idx[1], idx[2], len(lay.values))
    for name in z.PK_ORDER:
        assert got[name][1] == want[name][1] and np.array_equal(got[name][0], want[name][0]), name


# ---- 4. errors ------------------------------------------------------------------------------------------------------
def test_sigma_dev_errors(ctxs):
    import zkt_plonk_amd as z
    ctx = ctxs["bn254"]
    w = SC.raw_cases()["a_below_one_wave"]["w"]
    cols = [w[:, 0].copy(), w[:, 1].copy(), w[:, 2].copy()]
    cols[1][2] = 4                                            # == n_vars: one past the last variable
    with pytest.raises(z.ZktError) as e:
        _sigma(ctx, 3, cols, 4)
    assert e.value.code == ERR_INVALID_ARGUMENT and "ZKT_VARIABLE_ZERO" in str(e.value)
    nine = [np.zeros(9, dtype=np.uint32)] * 3
    with pytest.raises(z.ZktError) as e:                      # n_rows = n + 1
        _sigma(ctx, 3, nine, 4)
    assert e.value.code == ERR_INVALID_ARGUMENT
    for log_n in (-1, 26):
        with pytest.raises(z.ZktError) as e:
            _sigma(ctx, log_n, [w[:, 0], w[:, 1], w[:, 2]], 4)
        assert e.value.code == ERR_INVALID_DOMAIN_SIZE


def test_setup_wiring_errors_leave_no_stale_circuit(ctxs, setups):
    """Every refused call gives its code, and a context that had a circuit loaded reports afterwards what it reports
    after a failing zkt_circuit_setup: an error, never a proof of the previous circuit."""
    import zkt_plonk_amd as z
    cv = F.BN254
    ctx, s = ctxs[cv.name], setups[cv.name]
    cs, log_n, n = s["cs"], s["log_n"], s["n"]
    idx = _indices(cs)
    n_vars = len(cs.values)
    ctx.srs_load(s["srs"])

    def load():
        prover, _ = z.GpuProver.setup(ctx, log_n, s["evals10"])
        assert _prove(z, cv, prover, s) == s["proof"]
        return prover

    def code_of(fn):
        with pytest.raises(z.ZktError) as e:
            fn()
        return e.value.code

    # what the existing entry does: a vector longer than n is refused, and the circuit loaded before is gone
    prover = load()
    too_long = dict(s["evals10"], q_m=np.zeros((n + 1, 4), dtype=np.uint64))
    assert code_of(lambda: z.GpuProver.setup(ctx, log_n, too_long)) == ERR_INVALID_ARGUMENT
    after_failed_setup = code_of(lambda: _prove(z, cv, prover, s))

    bad_index = [x.copy() for x in idx]
    bad_index[2][17] = n_vars
    over = [np.zeros(n + 1, dtype=np.uint32)] * 3
    with_sigma = [None if k.startswith("sigma") else s["evals7"][k] for k in z.PK_ORDER]
    with_sigma[6] = s["evals10"]["sigma2"]
    refused = [lambda: z.GpuProver.setup_wiring(ctx, log_n, s["evals7"], bad_index[0], bad_index[1], bad_index[2], n_vars),
               lambda: z.GpuProver.setup_wiring(ctx, log_n, s["evals7"], over[0], over[1], over[2], n_vars),
               lambda: ctx.circuit_setup_wiring(log_n, with_sigma, idx[0], idx[1], idx[2], n_vars)]
    for fn in refused:
        prover = load()
        assert code_of(fn) == ERR_INVALID_ARGUMENT
        assert code_of(lambda: _prove(z, cv, prover, s)) == after_failed_setup
    # and the context is still good for a setup
    prover, _ = z.GpuProver.setup_wiring(ctx, log_n, s["evals7"], idx[0], idx[1], idx[2], n_vars)
    assert _prove(z, cv, prover, s) == s["proof"]


# ---- 6. side effects ------------------------------------------------------------------------------------------------
def test_sigma_dev_between_two_proofs_changes_nothing(ctxs, setups, raw):
    """zkt_circuit_sigma_dev between two proofs of a loaded circuit, the second one announced (its early rounds are
    already issued): the second proof's bytes are those of the same sequence without the call."""
    import zkt_plonk_amd as z
    cv = F.BN254
    ctx, s = ctxs[cv.name], setups[cv.name]
    ctx.srs_load(s["srs"])
    z.GpuProver.setup(ctx, s["log_n"], s["evals10"])
    pi_pos = sorted(s["pi"])
    pi_vals = np.stack([s["pi"][k] for k in pi_pos])
    bl2 = K.fr_to_mont(cv, field_elems(cv.fr.p, 32, P.NUM_BLINDERS))
    preps = [ctx.prepare_host(s["wires"][0], s["wires"][1], s["wires"][2], s["table"], pi_pos, pi_vals, bl)
             for bl in (s["blinders"], bl2)]
    case, want_sigma = raw["e_third_digit"]
    w = case["w"]

    def sequence(with_call):
        first = ctx.prove_prepared(preps[0], _transcript(z, cv, s), preps[1])
        if with_call:
            got = _sigma(ctx, case["log_n"], [w[:, 0], w[:, 1], w[:, 2]], case["n_vars"])
            assert all(np.array_equal(g, x) for g, x in zip(got, want_sigma))
        return first, ctx.prove_prepared(preps[1], _transcript(z, cv, s))

    plain = sequence(False)
    assert plain[0] == s["proof"]
    assert sequence(True) == plain
