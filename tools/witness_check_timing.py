"""Times zkt_circuit_check_witness on the withdraw circuit, with and without ZKT_CHECK_WIRING, reads its "check_witness"
profiling scope (stream time of the selector transforms, the sigma launches and the check kernels), and times one
zkt_prove of the same inputs on the same build for scale.

    python tools/witness_check_timing.py [--logs 14,18,20] [--reps 5]

Rows (BN254, ms; wall times are the median of --reps and end in the call's stream synchronise; the witness -- variable map
and wiring -- is resident in HBM, as zkt_poseidon_gadget_witness_dev leaves it):
  check          zkt_circuit_check_witness, flags = 0, and its "check_witness" scope
  check+wiring   the same with ZKT_CHECK_WIRING
  bad            the check of a witness with one changed variable (the report is printed)
  prove          one zkt_prove of the same inputs (warm: the second of two)"""
import argparse
import os
import random
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import zkt_plonk_amd as z
import withdraw_workload as WW

P_BN254 = 21888242871839275222246405745257275088548364400416034343698204186575808495617
GEN = 5
R = 1 << 256


def _mont(ctx, vals):
    """canonical Python integers -> (n, 4) Montgomery limbs (the product by R^2 runs on the device, as in bench.py)"""
    arr = np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(-1, 4)
    r2 = np.frombuffer((R * R % P_BN254).to_bytes(32, "little"), dtype=np.uint64)
    return ctx.debug_fr_mul(arr, np.tile(r2, (len(vals), 1)))


def _wall(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def _median(fn, reps):
    fn()
    return float(np.median([_wall(fn)[0] for _ in range(reps)]))


def _scope(ctx, fn, reps):
    ctx.profile_enable(True)
    for _ in range(reps):
        fn()
    calls, ms = ctx.profile_get("check_witness")
    ctx.profile_enable(False)
    return ms / max(calls, 1)


def row(ctx, log_n, reps):
    width, inputs, height = WW.SHAPES[log_n]
    hs = WW.reference_hasher(P_BN254, width)
    inst = WW.make_instance(hs, inputs, height, seed=0x5EED)
    lay = WW.layout(hs, inst)
    n, n_vars, gates = 1 << log_n, len(lay.values), lay.n_gates
    sel = WW.setup_vectors(lay, log_n, GEN)
    evals = {k: _mont(ctx, sel[k]) for k in z.PK_ORDER}
    del sel
    ctx.srs_generate(0x5EED5EED, n + 8)
    z.GpuProver.setup(ctx, log_n, evals)
    del evals
    # the witness in HBM: host-made variables uploaded, the Poseidon gadget's variables made on the device
    gadget = z.PoseidonGadget(ctx, hs.width, hs.half_full, hs.partial, _mont(ctx, hs.rc), _mont(ctx, [x for r in hs.mds for x in r]),
                              _mont(ctx, [hs.tag])[0])
    for base, ins in lay.hash_calls:
        gadget.hash(base, ins)
    gadget.stage()
    idx = [np.asarray(w, dtype=np.uint32) for w in lay.w]
    held = [ctx.alloc(n_vars * 32)] + [ctx.alloc(x.nbytes) for x in idx] + [ctx.alloc(n_vars * 32)]
    try:
        d_vars, d_idx, d_bad = held[0], held[1:4], held[4]
        ctx.upload(d_vars, _mont(ctx, lay.values))
        for d, x in zip(d_idx, idx):
            ctx.upload(d, x)
        gadget.fill(d_vars, n_vars, check=True)
        vals = ctx.download(d_vars, (n_vars, 4))
        changed = int(next(v for v in idx[0][gates // 2:] if v != WW.ZERO))
        vals[changed, 0] ^= np.uint64(1)                                    # one variable's value, still canonical
        ctx.upload(d_bad, vals)
        table = _mont(ctx, inst["ident_set"])
        pi_pos = sorted(lay.pi)
        pi_vals = _mont(ctx, [lay.pi[k] for k in pi_pos])
        rnd = random.Random(99)
        blinders = _mont(ctx, [rnd.randrange(P_BN254) for _ in range(z.NUM_BLINDERS)])
        prep = ctx.prepare_vars_dev(d_vars, n_vars, d_idx[0], d_idx[1], d_idx[2], gates, table, pi_pos, pi_vals, blinders)
        bad = ctx.prepare_vars_dev(d_bad, n_vars, d_idx[0], d_idx[1], d_idx[2], gates, table, pi_pos, pi_vals, blinders)
        plain, wired = (lambda: ctx.check_witness(prep)), (lambda: ctx.check_witness(prep, z.CHECK_WIRING))
        rep = wired()
        assert rep.satisfied and rep.checked == 7, rep
        t_plain, t_wired = _median(plain, reps), _median(wired, reps)
        s_plain, s_wired = _scope(ctx, plain, reps), _scope(ctx, wired, reps)
        t_bad = _median(lambda: ctx.check_witness(bad), reps)
        bad_rep = ctx.check_witness(bad)
        assert not bad_rep.satisfied
        prove = lambda: ctx.prove_prepared(prep, z.Transcript("merlin", "ZKT Plonk"))
        prove()
        t_prove = _median(prove, reps)
    finally:
        gadget.close()
        for d in held:
            ctx.free(d)
    print("2^%d rows %d vars %d table %d | check %.3f (scope %.3f) | check+wiring %.3f (scope %.3f) | bad %.3f %r | prove %.2f | "
          "check / prove %.3f, with wiring %.3f" % (log_n, gates, n_vars, table.shape[0], t_plain, s_plain, t_wired, s_wired, t_bad,
                                                    bad_rep, t_prove, t_plain / t_prove, t_wired / t_prove), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", default="14,18,20")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    print("# zkt_circuit_check_witness against one zkt_prove; BN254 withdraw circuit, witness resident in HBM; ms", flush=True)
    ctx = z.Context("bn254", 0)
    for lg in (int(x) for x in a.logs.split(",")):
        row(ctx, lg, a.reps)
    ctx.close()


if __name__ == "__main__":
    main()
