"""Every entry point that takes device pointers or runs on the context's stream (tests/stream_cases.py), on a stream the
CALLER owns and keeps busy: WHEN the library reads and writes relative to the caller's work, not what it computes.

Each case runs three times through tests/stream_rig.py: on the idle stream over a decoy input (valid data with another
answer; everything lazy is allocated here), on the idle stream over the real input, and on the held stream -- a bounded
spin, a marker event, the caller's kernels that write the real input over the decoy, then the library call with nothing
in between, then a caller kernel that reads the outputs.  held == idle == the CPU oracle, exactly: this is field and curve
arithmetic.  An enqueue-only entry must have returned while the marker was pending, a synchronising one must have been
entered while it was: asserted, never skipped.

Known limitation: with few hardware queues a racing side stream can share a queue with the held stream and be serialised
behind it, so the test can miss a race on some runs.  It can never report one that is not there."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import fields as F, plonk as P, coracle as K, composer as OC, poseidon as OP
from helpers import field_elems, rand_fr

import merkle_path_cases as MC
import merkle_tree_cases as TC
import ntt_cases as NC
import witness_cases as WC

CURVES = [F.BN254, F.BLS12_381]
IDS = lambda v: getattr(v, "name", str(v))
N_KEY = (1 << 12) + 5            # powers of the key the MSM and KZG cases run over
TAU = 0x57EA7
CLASSES, WHOLE = 1, 2
CHAIN = [(0, 900), (0, 901), (1, 931)]        # (witness, blinder seed) of test_gpu_quotient_classes: its oracle proofs are shared


class World:
    """Per module: per curve one context on a torch stream for the key-only entries, one for the circuit entries, one on
    the default stream; the spin is calibrated once."""

    def __init__(self):
        import torch
        import zkt_plonk_amd as z
        import stream_rig as R
        self.z, self.R, self.torch = z, R, torch
        self.rigs, self.srs_, self.key_loaded, self.t0 = {}, {}, set(), time.perf_counter()
        self.first = None

    def rig(self, cv, role="key"):
        if (cv.name, role) not in self.rigs:
            ctx = self.z.Context(cv.name, 0)
            rig = self.R.Rig(ctx, None if role == "default" else self.torch.cuda.Stream())
            if self.first is None:
                rig.calibrate()
                self.first = rig
            else:
                rig.share_calibration(self.first)
            self.rigs[cv.name, role] = rig
        return self.rigs[cv.name, role]

    def srs(self, cv):
        if cv.name not in self.srs_:
            self.srs_[cv.name] = K.srs_mont(cv, TAU, N_KEY)
        return self.srs_[cv.name]

    def keyed(self, cv):
        rig = self.rig(cv)
        if cv.name not in self.key_loaded:
            rig.ctx.srs_load(self.srs(cv))
            self.key_loaded.add(cv.name)
        return rig

    def circuit(self, cv, n=128, role="circuit"):
        """The n-row circuit of test_gpu_quotient_classes loaded on the circuit context -> (rig, case)."""
        import test_gpu_quotient_classes as QC
        rig, case = self.rig(cv, role), QC._case(cv, n)
        if getattr(rig, "loaded", None) != n:
            case.load(self.z, rig.ctx)
            rig.loaded = n
        return rig, case

    def close(self):
        slow = max((r.slowest for r in self.rigs.values()), key=lambda s: s[1], default=("", 0.0))
        held = sum(r.held_calls for r in self.rigs.values())
        if self.first is not None:
            hold = max(r.hold_ms() for r in self.rigs.values())
            print("\ncaller-stream rig: %.0f spin cycles per ms; slowest warmed enqueue-only call %s %.3f ms; hold %.1f ms; "
                  "%d holds; module wall time %.1f s" % (self.first.cycles_per_ms, slow[0], slow[1] * 1e3, hold, held,
                                                         time.perf_counter() - self.t0))
        for r in self.rigs.values():
            r.ctx.close()


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.close()


# ---- transforms ---------------------------------------------------------------------------------------------------------
MULTI_PASS = next(k for k in range(10, 20) if len(NC.default_split(k)) > 1)     # the smallest size of more than one pass
NTT_FORMS = [("forward", 0, 0, 0, False), ("inverse_coset", 1, 1, 0, False), ("in_place", 0, 1, 0, True), ("short_input", 1, 0, 3, False)]


@pytest.mark.parametrize("log_n", [10, MULTI_PASS])
@pytest.mark.parametrize("cv", CURVES, ids=IDS)
def test_ntt_dev(world, cv, log_n):
    rig, R = world.rig(cv), world.R
    ctx, n = rig.ctx, 1 << log_n
    assert MULTI_PASS == 11
    rng = np.random.default_rng(10 + log_n)
    real, decoy = rand_fr(rng, n), rand_fr(rng, n)
    d_in, d_out = R.dev(decoy), R.dev(np.zeros((n, 4), np.uint64))
    for name, inv, cos, short, in_place in NTT_FORMS:
        in_len, dst = n - short, d_in if in_place else d_out

        def body(m, data):
            m.begin([(d_in, data[0])])
            m.enqueue("zkt_ntt_dev", ctx.ntt_dev, log_n, d_in.data_ptr(), in_len, dst.data_ptr(), inverse=bool(inv), coset=bool(cos))
            return m.consume(dst)

        res = rig.three_ways(body, [d_in], [R.dev(decoy)], [R.dev(real)], [] if in_place else [d_out])
        R.compare("zkt_ntt_dev %s 2^%d" % (name, log_n), res, K.ntt_mont(cv, log_n, inv, cos, real[:in_len]))


@pytest.mark.parametrize("log_n", [10, MULTI_PASS])
@pytest.mark.parametrize("cv", CURVES, ids=IDS)
def test_debug_ntt_batch(world, cv, log_n):
    rig, R = world.rig(cv), world.R
    ctx, n = rig.ctx, 1 << log_n
    rng = np.random.default_rng(20 + log_n)
    lens = [n, n - 3, n // 2]
    real, decoy = [rand_fr(rng, n) for _ in lens], [rand_fr(rng, n) for _ in lens]
    d_in = [R.dev(x) for x in decoy]
    d_out = [d_in[0]] + [R.dev(np.zeros((n, 4), np.uint64)) for _ in lens[1:]]           # polynomial 0 in place

    def body(m, data):
        m.begin(list(zip(d_in, data)))
        m.enqueue("zkt_debug_ntt_batch", ctx.debug_ntt_batch, log_n, [t.data_ptr() for t in d_in], lens, [t.data_ptr() for t in d_out],
                  inverse=False, coset=True)
        return [m.consume(t) for t in d_out]

    res = rig.three_ways(body, d_in, [R.dev(x) for x in decoy], [R.dev(x) for x in real], d_out[1:])
    R.compare("zkt_debug_ntt_batch 2^%d" % log_n, res, [K.ntt_mont(cv, log_n, 0, 1, x[:k]) for x, k in zip(real, lens)])


# ---- the key and the MSMs -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cv", CURVES, ids=IDS)
def test_srs_load_dev_and_msm_dev(world, cv):
    """A key of 2^12 + 5 points that the caller's kernel produces on the held stream, read back through zkt_srs_download;
    then one MSM over all of it."""
    rig, R = world.rig(cv), world.R
    ctx, srs = rig.ctx, world.srs(cv)
    other = K.srs_mont(cv, TAU + 1, N_KEY)
    d_key = R.dev(other)

    def load(m, data):
        m.begin([(d_key, data[0])])
        m.blocking("zkt_srs_load_dev", ctx.srs_load_dev, d_key.data_ptr(), N_KEY)
        return ctx.srs_download(0, N_KEY)

    R.compare("zkt_srs_load_dev", rig.three_ways(load, [d_key], [R.dev(other)], [R.dev(srs)]), srs)
    world.key_loaded.add(cv.name)
    rng = np.random.default_rng(31)
    real, decoy = rand_fr(rng, N_KEY), rand_fr(rng, N_KEY)
    d_sc = R.dev(decoy)

    def msm(m, data):
        m.begin([(d_sc, data[0])])
        return m.blocking("zkt_msm_g1_dev", ctx.msm_dev, d_sc.data_ptr(), N_KEY)

    want, inf = K.msm_mont(cv, srs, real)
    assert not inf
    R.compare("zkt_msm_g1_dev", rig.three_ways(msm, [d_sc], [R.dev(decoy)], [R.dev(real)]), want)


@pytest.mark.parametrize("cv", CURVES, ids=IDS)
def test_msm_enqueue_dev_reuses_a_slot(world, cv):
    """Four enqueued MSMs back to back -- more than MSM_BATCH = 3: the slot is taken again while its tail is still on the
    side stream -- then zkt_msm_g1_dev over other scalars, all behind one hold."""
    rig, R = world.keyed(cv), world.R
    ctx, srs = rig.ctx, world.srs(cv)
    rng = np.random.default_rng(41)
    lens = [N_KEY, 1000, N_KEY - 7, 1, N_KEY]
    real, decoy = [rand_fr(rng, k) for k in lens], [rand_fr(rng, k) for k in lens]
    bufs = [R.dev(x) for x in decoy]

    def body(m, data):
        m.begin(list(zip(bufs, data)))
        for j in range(4):
            m.enqueue("zkt_msm_enqueue_dev #%d" % j, ctx.msm_enqueue_dev, bufs[j].data_ptr(), lens[j])
        return m.blocking("zkt_msm_g1_dev", ctx.msm_dev, bufs[4].data_ptr(), lens[4])

    want, inf = K.msm_mont(cv, srs, real[4])
    assert not inf
    R.compare("zkt_msm_g1_dev after four zkt_msm_enqueue_dev", rig.three_ways(body, bufs, [R.dev(x) for x in decoy], [R.dev(x) for x in real]), want)


@pytest.mark.parametrize("cv", CURVES, ids=IDS)
def test_msm_bases_dev(world, cv):
    rig, R = world.rig(cv), world.R
    ctx, srs, n = rig.ctx, world.srs(cv), 1000
    rng = np.random.default_rng(51)
    real, decoy = [srs[100:100 + n], rand_fr(rng, n)], [srs[2000:2000 + n], rand_fr(rng, n)]
    bufs = [R.dev(x) for x in decoy]

    def body(m, data):
        m.begin(list(zip(bufs, data)))
        return m.blocking("zkt_msm_g1_bases_dev", ctx.msm_bases_dev, bufs[0].data_ptr(), bufs[1].data_ptr(), n)

    R.compare("zkt_msm_g1_bases_dev", rig.three_ways(body, bufs, [R.dev(x) for x in decoy], [R.dev(x) for x in real]),
              K.msm_mont(cv, real[0], real[1]))


# ---- the KZG seam and commitments of evaluations ---------------------------------------------------------------------------
KZG_LENS = [(1 << 10) + 3, 1 << 9, 1]


@pytest.mark.parametrize("cv", CURVES, ids=IDS)
def test_kzg_commit_batch_dev(world, cv):
    rig, R = world.keyed(cv), world.R
    ctx, srs = rig.ctx, world.srs(cv)
    rng = np.random.default_rng(61)
    real, decoy = [rand_fr(rng, k) for k in KZG_LENS], [rand_fr(rng, k) for k in KZG_LENS]
    bufs = [R.dev(x) for x in decoy]

    def body(m, data):
        m.begin(list(zip(bufs, data)))
        return m.blocking("zkt_kzg_commit_batch_dev", ctx.kzg_commit_batch_dev, [t.data_ptr() for t in bufs], KZG_LENS)

    R.compare("zkt_kzg_commit_batch_dev", rig.three_ways(body, bufs, [R.dev(x) for x in decoy], [R.dev(x) for x in real]),
              [K.msm_mont(cv, srs[:k], p) for p, k in zip(real, KZG_LENS)])


@pytest.mark.parametrize("cv", CURVES, ids=IDS)
def test_kzg_open_dev(world, cv):
    import test_gpu_kzg_seam as KS
    rig, R = world.keyed(cv), world.R
    ctx, srs = rig.ctx, world.srs(cv)
    rng = np.random.default_rng(71)
    real, decoy = [rand_fr(rng, k) for k in KZG_LENS], [rand_fr(rng, k) for k in KZG_LENS]
    ch, zm = rand_fr(rng, 3), rand_fr(rng, 1)[0]
    bufs = [R.dev(x) for x in decoy]

    def body(m, data):
        m.begin(list(zip(bufs, data)))
        return m.blocking("zkt_kzg_open_dev", ctx.kzg_open_dev, [t.data_ptr() for t in bufs], KZG_LENS, ch, zm)

    w, ev = KS._oracle_open(cv, srs, real, ch, zm)
    assert not w[1]
    R.compare("zkt_kzg_open_dev", rig.three_ways(body, bufs, [R.dev(x) for x in decoy], [R.dev(x) for x in real]), (w, ev))


@pytest.mark.parametrize("cv", CURVES, ids=IDS)
def test_commit_evals_dev(world, cv):
    import test_gpu_lagrange as LG
    R = world.R
    rig, case = world.circuit(cv)
    ctx, n, p = rig.ctx, case.n, cv.fr.p
    real, decoy, bl = field_elems(p, 81, n), field_elems(p, 82, n), field_elems(p, 83, 2)
    d_ev = R.dev(K.fr_to_mont(cv, decoy))

    def body(m, data):
        out = []
        for path in (0, 1):
            m.begin([(d_ev, data[0])])
            out.append(m.blocking("zkt_commit_evals_dev path %d" % path, ctx.commit_evals_dev, d_ev.data_ptr(), K.fr_to_mont(cv, bl), path))
            rig.fill([(d_ev, decoys[0])])
        return out

    decoys = [R.dev(K.fr_to_mont(cv, decoy))]
    want = (K.points_to_mont(cv, [LG._oracle_commit(cv, n.bit_length() - 1, case.srs, real, bl)])[0], False)
    R.compare("zkt_commit_evals_dev", rig.three_ways(body, [d_ev], decoys, [R.dev(K.fr_to_mont(cv, real))]), [want, want])


# ---- setup and witness checks ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cv", CURVES, ids=IDS)
def test_circuit_sigma_dev(world, cv):
    R = world.R
    rig, case = world.circuit(cv)
    ctx, n, cs = rig.ctx, case.n, case.css[0]
    idx = [np.ascontiguousarray(x, dtype=np.uint32) for x in WC.indices(cs)]
    real, decoy = idx, [idx[1], idx[2], idx[0]]                       # the columns rotated: another permutation
    bufs = [R.dev(x) for x in decoy]
    outs = [R.dev(np.zeros((n, 4), np.uint64)) for _ in range(3)]

    def body(m, data):
        m.begin(list(zip(bufs, data)))
        m.blocking("zkt_circuit_sigma_dev", ctx.circuit_sigma, n.bit_length() - 1, bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(),
                   len(idx[0]), len(cs.values), d_sigma=[t.data_ptr() for t in outs])
        return [m.consume(t) for t in outs]

    evals = P.setup_evals(case.be, cs)
    R.compare("zkt_circuit_sigma_dev", rig.three_ways(body, bufs, [R.dev(x) for x in decoy], [R.dev(x) for x in real], outs),
              [K.fr_to_mont(cv, evals[k]) for k in ("sigma1", "sigma2", "sigma3")])


def _report(cv, r):
    return (r.satisfied, r.checked, r.n_arithmetic, r.first_arithmetic, r.residual, r.n_lookup, r.first_lookup, r.n_wiring, r.first_wiring)


def _want_report(cv, d):
    return (d["satisfied"], d["checked"], d["n_arithmetic"], d["first_arithmetic"], K.fr_to_mont(cv, [d["residual"]])[0], d["n_lookup"],
            d["first_lookup"], d["n_wiring"], d["first_wiring"])


@pytest.mark.parametrize("broken", [False, True], ids=["satisfied", "broken"])
@pytest.mark.parametrize("cv", CURVES, ids=IDS)
def test_check_witness_on_device_inputs(world, cv, broken):
    """Device wires, and device variables plus wiring with ZKT_CHECK_WIRING: the witness under test is written behind the
    hold over the other one (a satisfied witness over a broken one and the reverse)."""
    R = world.R
    rig, case = world.circuit(cv)
    ctx, cs = rig.ctx, case.css[0]
    var = max(range(len(cs.values)), key=lambda v: sum(col.count(v) for col in (cs.w_l, cs.w_r, cs.w_o)))
    bad = WC.with_value(cs, var, cs.values[var] + 3)
    wit, other = (bad, cs) if broken else (cs, bad)
    mont = lambda x: K.fr_to_mont(cv, x)
    pos = sorted(cs.pi)
    tbl, pv = mont(cs.table), mont([cs.pi[k] for k in pos])
    idx = [np.ascontiguousarray(x, dtype=np.uint32) for x in WC.indices(cs)]
    side = lambda w: [mont(x) for x in w.wire_evals(w.n_gates)] + [mont(w.values)] + idx
    real, decoy = side(wit), side(other)
    bufs = [R.dev(x) for x in decoy]
    a, b, c, v, wl, wr, wo = [t.data_ptr() for t in bufs]
    p_wires = ctx.prepare_dev(a, b, c, cs.n_gates, tbl, pos, pv, None)
    p_vars = ctx.prepare_vars_dev(v, len(cs.values), wl, wr, wo, cs.n_gates, tbl, pos, pv, None)
    decoys = [R.dev(x) for x in decoy]

    def body(m, data):
        m.begin(list(zip(bufs, data)))
        r1 = m.blocking("zkt_circuit_check_witness, wires", ctx.check_witness, p_wires)
        rig.fill(list(zip(bufs, decoys)))
        m.begin(list(zip(bufs, data)))
        r2 = m.blocking("zkt_circuit_check_witness, variables", ctx.check_witness, p_vars, WC.CHECK_WIRING)
        return [_report(cv, r1), _report(cv, r2)]

    want = [_want_report(cv, WC.report_of_cs(wit, key=cs)), _want_report(cv, WC.report_of_cs(wit, key=cs, wiring=True))]
    assert want[0][0] == (not broken)
    R.compare("zkt_circuit_check_witness", rig.three_ways(body, bufs, decoys, [R.dev(x) for x in real]), want)


# ---- whole proofs ----------------------------------------------------------------------------------------------------------
def _proof_chain(world, cv, n, route, variables, role="circuit"):
    """Three proofs, every successor announced: the witness of proof i + 1 is written behind the hold of proof i, which reads
    it early (rounds 1 and 2), over a decoy witness (another witness of the circuit: refused, or other bytes)."""
    R, z = world.R, world.z
    rig, case = world.circuit(cv, n, role)
    ctx = rig.ctx
    mont = lambda x: K.fr_to_mont(cv, x)
    real, decoy, preps = [], [], []
    for k, seed in CHAIN:
        cs, other = case.css[k], case.css[2]
        ins = case.inputs(k, seed)
        if variables:
            idx = [np.ascontiguousarray(x, dtype=np.uint32) for x in WC.indices(cs)]
            real.append([mont(cs.values)] + idx)
            decoy.append([mont(other.values)] + [np.zeros_like(x) for x in idx])
        else:
            real.append(list(ins[:3]))
            decoy.append([mont(x) for x in other.wire_evals(other.n_gates)])
    bufs = [[R.dev(x) for x in d] for d in decoy]
    for (k, seed), b in zip(CHAIN, bufs):
        cs, ins = case.css[k], case.inputs(k, seed)
        ptr = [t.data_ptr() for t in b]
        preps.append(ctx.prepare_vars_dev(ptr[0], len(cs.values), ptr[1], ptr[2], ptr[3], cs.n_gates, *ins[3:]) if variables
                     else ctx.prepare_dev(ptr[0], ptr[1], ptr[2], cs.n_gates, *ins[3:]))

    def body(m, data):
        out = []
        for i in range(len(CHAIN)):
            m.begin([w for j in ([0, 1] if i == 0 else [i + 1]) if j < len(CHAIN) for w in zip(bufs[j], data[j])])
            try:
                out.append(m.blocking("zkt_prove #%d" % i, ctx.prove_prepared, preps[i], case.tr(z), preps[i + 1] if i + 1 < len(CHAIN) else None))
            except z.ZktError as e:
                out.append(("refused", e.code))
        return out

    flat = lambda xs: [t for x in xs for t in x]
    ctx.set_quotient_route(route)
    try:
        res = rig.three_ways(lambda m, data: body(m, [data[4 * j:4 * j + 4] if variables else data[3 * j:3 * j + 3] for j in range(len(CHAIN))]),
                             flat(bufs), [R.dev(x) for x in flat(decoy)], [R.dev(x) for x in flat(real)])
    finally:
        ctx.set_quotient_route(0)
    R.compare("zkt_prove chain, n = %d, route %d" % (n, route), res, [case.want(k, seed) for k, seed in CHAIN])


@pytest.mark.parametrize("route", [CLASSES, WHOLE], ids=["classes", "whole"])
@pytest.mark.parametrize("n", [128, 2048])
@pytest.mark.parametrize("cv", CURVES, ids=IDS)
def test_proof_chain_device_wires(world, cv, n, route):
    _proof_chain(world, cv, n, route, False)


@pytest.mark.parametrize("route", [CLASSES, WHOLE], ids=["classes", "whole"])
@pytest.mark.parametrize("n", [128, 2048])
@pytest.mark.parametrize("cv", CURVES, ids=IDS)
def test_proof_chain_device_variables(world, cv, n, route):
    _proof_chain(world, cv, n, route, True)


# ---- Poseidon ----------------------------------------------------------------------------------------------------------------
def _poseidon_load(ctx, cv, prm):
    return ctx.poseidon_load(prm.width, prm.half_full, prm.partial, K.fr_to_mont(cv, prm.rc),
                             K.fr_to_mont(cv, [x for row in prm.mds for x in row]), K.fr_to_mont(cv, [prm.domain_tag])[0])


def test_poseidon_hash_batch_dev(world):
    """Batch 300, arity 2, on the BN254 x3 tables of the withdraw circuit, hashes and round states."""
    cv, R = F.BN254, world.R
    rig = world.rig(cv)
    ctx, p, prm = rig.ctx, cv.fr.p, MC.shipped_params(3)
    batch, arity, rounds = 300, 2, 2 * prm.half_full + prm.partial
    ins = lambda seed: [field_elems(p, seed + b, arity) for b in range(batch)]
    real, decoy = ins(9000), ins(9500)
    mont = lambda rows: K.fr_to_mont(cv, [x for row in rows for x in row])
    h = _poseidon_load(ctx, cv, prm)
    d_in = R.dev(mont(decoy))
    d_out, d_st = R.dev(np.zeros((batch, 4), np.uint64)), R.dev(np.zeros((batch * (rounds + 1) * prm.width, 4), np.uint64))

    def body(m, data):
        m.begin([(d_in, data[0])])
        m.enqueue("zkt_poseidon_hash_batch_dev", ctx.poseidon_hash_batch_dev, h, d_in.data_ptr(), batch, arity, d_out.data_ptr(), d_st.data_ptr())
        return [m.consume(d_out), m.consume(d_st)]

    res = rig.three_ways(body, [d_in], [R.dev(mont(decoy))], [R.dev(mont(real))], [d_out, d_st])
    runs = [OP.permute(p, prm.width, prm.half_full, prm.partial, prm.rc, prm.mds, prm.domain_tag, x) for x in real]
    R.compare("zkt_poseidon_hash_batch_dev", res, [K.fr_to_mont(cv, [r[0] for r in runs]), mont([x for r in runs for x in r[1]])])
    ctx.poseidon_free(h)


@pytest.mark.parametrize("cv", CURVES, ids=IDS)
def test_poseidon_gadget_witness_dev(world, cv):
    """Inputs as values (dense traces behind a gap) and as variable indices (scattered traces), both behind the hold."""
    R = world.R
    rig = world.rig(cv)
    ctx, p = rig.ctx, cv.fr.p
    prm = MC.shipped_params(3) if cv.name == "bn254" else MC.synthetic_params(cv, 3)
    per, batch, arity = prm.gates_per_hash, 70, 2
    ins = lambda seed: [field_elems(p, seed + b, arity) for b in range(batch)]
    real, decoy = ins(9100), ins(9600)
    flat = lambda rows: [x for row in rows for x in row]
    h = _poseidon_load(ctx, cv, prm)
    assert ctx.poseidon_gadget_vars_per_hash(h) == per
    hash_at = per - 1 - (prm.width - 2) * prm.width
    traces = [OC.gadget_trace(prm, x) for x in real]
    # (a) values
    n_vars = 5 + batch * per
    d_in, d_vars, d_out = R.dev(K.fr_to_mont(cv, flat(decoy))), R.dev(np.zeros((n_vars, 4), np.uint64)), R.dev(np.zeros((batch, 4), np.uint64))

    def body_a(m, data):
        m.begin([(d_in, data[0])])
        m.enqueue("zkt_poseidon_gadget_witness_dev, values", ctx.poseidon_gadget_witness_dev, h, batch, arity, d_vars.data_ptr(), n_vars,
                  d_inputs=d_in.data_ptr(), trace_base0=5, d_out_hashes=d_out.data_ptr())
        return [m.consume(d_vars)[5:], m.consume(d_out)]

    res = rig.three_ways(body_a, [d_in], [R.dev(K.fr_to_mont(cv, flat(decoy)))], [R.dev(K.fr_to_mont(cv, flat(real)))], [d_vars, d_out])
    R.compare("zkt_poseidon_gadget_witness_dev, values", res, [K.fr_to_mont(cv, flat(traces)), K.fr_to_mont(cv, [t[hash_at] for t in traces])])
    # (b) variable indices, scattered bases: the map holds the inputs in front, every trace is followed by three untouched variables
    n_in = batch * arity
    n_vars = n_in + batch * (per + 3)
    bases = np.array([n_in + b * (per + 3) for b in reversed(range(batch))], dtype=np.uint32)
    idx = np.arange(n_in, dtype=np.uint32)
    whole = lambda rows: K.fr_to_mont(cv, flat(rows) + [7] * (n_vars - n_in))
    bufs = [R.dev(whole(decoy)), R.dev(np.zeros_like(idx)), R.dev(np.sort(bases))]
    decoys_b = [R.dev(whole(decoy)), R.dev(np.zeros_like(idx)), R.dev(np.sort(bases))]     # other inputs, every hash reads variable 0, other bases

    def body_b(m, data):
        m.begin(list(zip(bufs, data)))
        m.enqueue("zkt_poseidon_gadget_witness_dev, variables", ctx.poseidon_gadget_witness_dev, h, batch, arity, bufs[0].data_ptr(), n_vars,
                  d_input_vars=bufs[1].data_ptr(), d_trace_base=bufs[2].data_ptr(), d_out_hashes=d_out.data_ptr())
        got = [m.consume(bufs[0]), m.consume(d_out)]
        ctx.poseidon_gadget_check(h)
        return got

    want = flat(real) + [7] * (n_vars - n_in)
    for b, base in enumerate(bases):
        want[base:base + per] = traces[b]
    res = rig.three_ways(body_b, bufs, decoys_b, [R.dev(whole(real)), R.dev(idx), R.dev(bases)], [d_out])
    R.compare("zkt_poseidon_gadget_witness_dev, variables", res, [K.fr_to_mont(cv, want), K.fr_to_mont(cv, [t[hash_at] for t in traces])])
    ctx.poseidon_free(h)


@pytest.mark.parametrize("cv", CURVES, ids=IDS)
def test_poseidon_merkle_path_witness_dev(world, cv):
    """Height 8, PER_WAVE + 1 paths: the map (leaves, bits, siblings) and the index vectors are written behind the hold."""
    R = world.R
    rig = world.rig(cv)
    ctx, w, height = rig.ctx, 4, 8
    case, other = (MC.build(cv.name, w, False, height, MC.per_wave(w) + 1, "mixed", False, False, seed=s) for s in (1, 2))
    assert case.bases == other.bases and case.values != other.values
    h = _poseidon_load(ctx, cv, case.prm)

    def sides(c):
        vals = list(c.values)
        for b in c.bases:
            vals[b:b + c.span] = [0x0BAD0BAD0BAD0BAD0BAD0BAD0BAD0BAD] * c.span
        u32 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.uint32))
        return [K.fr_to_mont(cv, vals), u32(c.leaf), u32(c.bits), u32(c.sibs), u32(c.bases)]

    real, decoy = sides(case), sides(other)
    decoy[1:] = [np.zeros_like(x) for x in decoy[1:-1]] + [decoy[-1]]           # indices the caller has not written yet
    bufs = [R.dev(x) for x in decoy]
    d_roots = R.dev(np.zeros((case.batch, 4), np.uint64))

    def body(m, data):
        m.begin(list(zip(bufs, data)))
        m.enqueue("zkt_poseidon_merkle_path_witness_dev", ctx.poseidon_merkle_path_witness_dev, h, case.batch, height, bufs[0].data_ptr(),
                  case.n_vars, bufs[1].data_ptr(), bufs[2].data_ptr(), bufs[3].data_ptr(), d_path_base=bufs[4].data_ptr(),
                  d_out_roots=d_roots.data_ptr())
        return [m.consume(bufs[0]), m.consume(d_roots)]

    res = rig.three_ways(body, bufs, [R.dev(x) for x in decoy], [R.dev(x) for x in real], [d_roots])
    R.compare("zkt_poseidon_merkle_path_witness_dev", res, [K.fr_to_mont(cv, case.values), K.fr_to_mont(cv, case.roots)])
    ctx.poseidon_free(h)


# ---- the note tree -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cv", CURVES, ids=IDS)
def test_merkle_tree_append_and_paths(world, cv):
    """Height 8: 37 leaves, 64 more, then the paths of 5 and of 7 indices written into a variable map, all behind one hold.
    Both appends and the first paths call return while it lasts; the second paths call may wait for the first one's index
    table to have left the tree's pinned buffer (it goes up behind the hold), and for nothing else."""
    R = world.R
    rig = world.rig(cv)
    ctx, height = rig.ctx, 8
    prm = MC.synthetic_params(cv, 3)
    case, other = (TC._case(cv, prm, height, 101, (37, 101), seed) for seed in (11, 12))
    snap = case.snaps[101]
    h = _poseidon_load(ctx, cv, prm)
    d_leaves = R.dev(K.fr_to_mont(cv, other.leaves))
    idx = [[0, 36, 37, 100, 255], [1, 2, 63, 64, 99, 101, 200]]
    paths = idx[0] + idx[1]
    used, n_vars = 2 * height * len(paths), 512                 # the map goes on behind the paths: nothing may be written there
    bit0 = [np.array([2 * height * (len(idx[0]) * k + j) for j in range(len(ix))], dtype=np.uint32) for k, ix in enumerate(idx)]
    d_vars = R.dev(np.zeros((n_vars, 4), np.uint64))

    def body(m, data):
        t = ctx.merkle_tree_create(h, height, 1 << height)
        m.begin([(d_leaves, data[0])])
        assert m.enqueue("zkt_merkle_tree_append_dev 37", ctx.merkle_tree_append_dev, t, d_leaves.data_ptr(), 37) == 0
        assert m.enqueue("zkt_merkle_tree_append_dev 64", ctx.merkle_tree_append_dev, t, d_leaves.data_ptr() + 32 * 37, 64) == 37
        for k in (0, 1):
            m.enqueue("zkt_merkle_tree_paths_to_variables_dev #%d" % k, ctx.merkle_tree_paths_to_variables_dev, t, idx[k], d_vars.data_ptr(),
                      n_vars, bit0[k] + height, bit0[k], may_wait=k == 1)
        got = [m.consume(d_vars), ctx.merkle_tree_root(t)] + [ctx.merkle_tree_layer(t, L, 0, snap.stored(L)) for L in range(height)]
        ctx.merkle_tree_free(t)
        return got

    res = rig.three_ways(body, [d_leaves], [R.dev(K.fr_to_mont(cv, other.leaves))], [R.dev(K.fr_to_mont(cv, case.leaves))], [d_vars])
    one = [0, 1]
    want_vars = [x for i in paths for x in [one[(i >> L) & 1] for L in range(height)] + snap.merkle_path(i)]
    R.compare("zkt_merkle_tree_append_dev / _paths_to_variables_dev", res,
              [np.concatenate([K.fr_to_mont(cv, want_vars), np.full((n_vars - used, 4), R.POISON, np.uint64)]), K.fr_to_mont(cv, [snap.root])[0]] + [K.fr_to_mont(cv, snap.layer(L)) for L in range(height)])
    ctx.poseidon_free(h)


# ---- untrusted bytes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cv", CURVES, ids=IDS)
def test_g1_decompress_dev(world, cv):
    import test_gpu_g1_decompress as GD
    R = world.R
    rig = world.rig(cv)
    ctx, n = rig.ctx, 65
    data, status, want = GD._cases(cv, n)
    real = np.frombuffer(data, dtype=np.uint8).reshape(n, -1).copy()
    decoy = np.roll(real, 1, axis=0)
    d_in = R.dev(decoy)
    d_out, d_st = R.dev(np.zeros((n, 2 * cv.fq.limbs64), np.uint64)), R.dev(np.zeros(n, np.uint8))

    def body(m, data_):
        m.begin([(d_in, data_[0])])
        m.enqueue("zkt_g1_decompress_dev", ctx.g1_decompress_dev, d_in.data_ptr(), n, d_out.data_ptr(), d_st.data_ptr())
        return [m.consume(d_out), m.consume(d_st)]

    R.compare("zkt_g1_decompress_dev", rig.three_ways(body, [d_in], [R.dev(decoy)], [R.dev(real)], [d_out, d_st]), [want, status])


@pytest.mark.parametrize("cv", CURVES, ids=IDS)
def test_verify_batch_dev(world, cv):
    """The three oracle proofs of test_gpu_verify_batch with the stream held: accepted, rejected under the wrong beta_h, and
    the prepared pair (A, B) the same as on the idle stream.  The inputs are host memory: there is no decoy."""
    import test_gpu_verify_batch as VB
    from zkt_plonk_amd import _lib
    R = world.R
    rig = world.rig(cv)
    ctx = rig.ctx
    made, srs, h, beta_h, wrong = VB._made(cv)
    assert _lib.verify_batch(cv.name, VB._items(cv, made), h, beta_h)

    def body(m, data):
        out = []
        for bh in (beta_h, wrong):
            m.begin()
            out.append(m.blocking("zkt_verify_batch_dev", ctx.verify_batch_dev, VB._items(cv, made), h, bh))
        m.begin()
        out.append(m.blocking("zkt_verify_batch_prepare_dev", ctx.verify_batch_prepare_dev, VB._items(cv, made), h, beta_h))
        return out

    decoy, idle, held = rig.three_ways(body, [], [], [])
    assert idle[:2] == (True, False) and held[:2] == (True, False), (idle[:2], held[:2])
    assert held[2] == idle[2] == decoy[2]
    ab, inf, rho = (np.frombuffer(x, dtype=t) for x, t in zip(held[2], (np.uint64, np.bool_, np.uint64)))
    L = cv.fq.limbs64
    ab = ab.reshape(2, 2 * L).copy()
    assert not inf.any()
    neg_b = K.points_to_mont(cv, [(lambda pt: (pt[0], (-pt[1]) % cv.fq.p))(K.points_from_mont(cv, ab[1:2])[0])])[0]
    assert _lib.pairing_product_is_one(cv.name, np.stack([ab[0], neg_b]), np.stack([h, beta_h]))


# ---- stream switches and the default stream ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("cv", CURVES, ids=IDS)
def test_stream_switches(world, cv):
    """Key and circuit loaded on the context's own stream; set_stream to a torch stream and a proof at once; two enqueued
    MSMs on a held stream A, set_stream to B, the blocking MSM there; a proof announced on B and made on A; the context
    closed while both torch streams live on."""
    import test_gpu_quotient_classes as QC
    torch, z, R = world.torch, world.z, world.R
    case = QC._case(cv, 128)
    ctx = z.Context(cv.name, 0)
    try:
        case.load(z, ctx)                                           # on the stream zkt_ctx_create made
        A, B = torch.cuda.Stream(), torch.cuda.Stream()
        rig = R.Rig(ctx, A)
        rig.share_calibration(world.rig(cv))
        assert case.prove(z, ctx, 0, 900) == case.want(0, 900)
        k = case.n + 8
        rng = np.random.default_rng(91)
        real, decoy = [rand_fr(rng, k) for _ in range(3)], [rand_fr(rng, k) for _ in range(3)]
        bufs = [R.dev(x) for x in decoy]
        want, inf = K.msm_mont(cv, case.srs, real[2])
        assert not inf

        def body(m, data):
            ctx.set_stream(A.cuda_stream)
            m.begin(list(zip(bufs, data)))
            for j in range(2):
                m.enqueue("zkt_msm_enqueue_dev #%d" % j, ctx.msm_enqueue_dev, bufs[j].data_ptr(), k)
            ctx.set_stream(B.cuda_stream)                             # waits for A: the caller's writes are done
            return ctx.msm_dev(bufs[2].data_ptr(), k)

        R.compare("zkt_msm_g1_dev across a stream switch", rig.three_ways(body, bufs, [R.dev(x) for x in decoy], [R.dev(x) for x in real]), want)
        preps = [ctx.prepare_host(*case.inputs(w, seed)) for w, seed in CHAIN[:2]]
        assert ctx.prove_prepared(preps[0], case.tr(z), preps[1]) == case.want(*CHAIN[0])          # on B; announces the next
        ctx.set_stream(A.cuda_stream)
        assert ctx.prove_prepared(preps[1], case.tr(z)) == case.want(*CHAIN[1])                     # on A
    finally:
        ctx.close()
    for s in (A, B):
        with torch.cuda.stream(s):
            t = torch.arange(1000, device="cuda").sum()
        s.synchronize()
        assert t.item() == 499500


@pytest.mark.parametrize("cv", CURVES, ids=IDS)
def test_default_stream(world, cv):
    """The context on stream handle 0, torch's default stream: one MSM, one transform, one n = 128 chain of proofs."""
    R = world.R
    rig, case = world.circuit(cv, 128, "default")
    assert rig.stream.cuda_stream == 0
    ctx, k = rig.ctx, case.n + 8
    rng = np.random.default_rng(95)
    real, decoy = rand_fr(rng, 1 << 10), rand_fr(rng, 1 << 10)
    d_in, d_out = R.dev(decoy), R.dev(np.zeros((1 << 10, 4), np.uint64))

    def msm(m, data):
        m.begin([(d_in, data[0])])
        return m.blocking("zkt_msm_g1_dev", ctx.msm_dev, d_in.data_ptr(), k)

    R.compare("zkt_msm_g1_dev on stream 0", rig.three_ways(msm, [d_in], [R.dev(decoy)], [R.dev(real)]), K.msm_mont(cv, case.srs, real[:k])[0])

    def ntt(m, data):
        m.begin([(d_in, data[0])])
        m.enqueue("zkt_ntt_dev", ctx.ntt_dev, 10, d_in.data_ptr(), 1 << 10, d_out.data_ptr(), inverse=True, coset=True)
        return m.consume(d_out)

    R.compare("zkt_ntt_dev on stream 0", rig.three_ways(ntt, [d_in], [R.dev(decoy)], [R.dev(real)], [d_out]), K.ntt_mont(cv, 10, 1, 1, real))
    _proof_chain(world, cv, 128, 0, False, role="default")
