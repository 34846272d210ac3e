"""Times setup from the wiring (zkt_circuit_setup_wiring) against setup fed by the host path (sigma_columns' argsort,
setup_vectors' 3 n Python integers, their conversion and upload inside zkt_circuit_setup) on the withdraw circuit, and
reads the "sigma" profiling scope (stream time of the key, sort, link and evaluation launches).

    python tools/sigma_timing.py [--logs 14,18,20] [--reps 3]

Rows (BN254, wall times in ms, median of --reps; every call ends in a stream synchronise):
  host sigma   sigma_columns + the sigma part of setup_vectors + conversion to Montgomery limbs (what a caller does today)
  setup        zkt_circuit_setup on ten host vectors (upload included)
  wiring       zkt_circuit_setup_wiring on seven host vectors and the host wiring (upload included)
  sigma_dev    zkt_circuit_sigma_dev alone on wiring resident in HBM, and its "sigma" scope
The ten commitments of both setups are compared on every row."""
import argparse
import os
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


def row(ctx, log_n, reps):
    width, inputs, height = WW.SHAPES[log_n]
    hs = WW.reference_hasher(P_BN254, width)
    lay = WW.layout(hs, WW.make_instance(hs, inputs, height, seed=0x5EED))
    n, n_vars = 1 << log_n, len(lay.values)
    idx = [np.asarray(w, dtype=np.uint32) for w in lay.w]
    t_vec, sel = _wall(lambda: WW.setup_vectors(lay, log_n, GEN))
    t_cols = _wall(lambda: WW.sigma_columns(lay, n))[0]
    t_conv, sig = _wall(lambda: {k: _mont(ctx, sel[k]) for k in ("sigma1", "sigma2", "sigma3")})
    evals = dict(sig)
    for k in z.PK_ORDER:
        if k not in evals:
            evals[k] = _mont(ctx, sel[k])
    del sel
    seven = {k: v for k, v in evals.items() if not k.startswith("sigma")}
    ctx.srs_generate(0x5EED5EED, n + 8)
    want = z.GpuProver.setup(ctx, log_n, evals)[1]
    got = z.GpuProver.setup_wiring(ctx, log_n, seven, idx[0], idx[1], idx[2], n_vars)[1]
    assert all(np.array_equal(got[k][0], want[k][0]) and got[k][1] == want[k][1] for k in z.PK_ORDER), log_n
    t_setup = _median(lambda: z.GpuProver.setup(ctx, log_n, evals), reps)
    t_wiring = _median(lambda: z.GpuProver.setup_wiring(ctx, log_n, seven, idx[0], idx[1], idx[2], n_vars), reps)
    d = []
    for x in idx:
        d.append(ctx.alloc(x.nbytes))
        ctx.upload(d[-1], x)
    out = [ctx.alloc(n * 32) for _ in range(3)]
    try:
        call = lambda: ctx.circuit_sigma(log_n, d[0], d[1], d[2], len(idx[0]), n_vars, out)
        t_dev = _median(call, reps)
        ctx.profile_enable(True)
        for _ in range(reps):
            call()
        calls, ms = ctx.profile_get("sigma")
        ctx.profile_enable(False)
        for j, name in enumerate(("sigma1", "sigma2", "sigma3")):
            assert np.array_equal(ctx.download(out[j], (n, 4)), evals[name]), (log_n, name)
    finally:
        for x in d + out:
            ctx.free(x)
    print("2^%d rows %d vars %d | host sigma: argsort %.1f + vectors (all ten) %.1f + to limbs %.1f | setup %.2f | wiring %.2f | "
          "sigma_dev call %.3f, \"sigma\" scope %.3f (stream, mean of %d)" %
          (log_n, lay.n_gates, n_vars, t_cols, t_vec, t_conv, t_setup, t_wiring, t_dev, ms / max(calls, 1), calls), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", default="14,18,20")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    print("# zkt_circuit_setup_wiring against zkt_circuit_setup fed by the host sigma path; BN254 withdraw wiring; ms", flush=True)
    ctx = z.Context("bn254", 0)
    for lg in (int(x) for x in a.logs.split(",")):
        row(ctx, lg, a.reps)
    ctx.close()


if __name__ == "__main__":
    main()
