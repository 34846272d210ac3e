"""Times the witness completion from the free variables (zkt_witness_plan_create, zkt_witness_complete_enqueue) on the withdraw
circuit of tools/withdraw_workload.py, beside the existing route in the same process: the two gadget kernels as bench.py's
device-witness leg drives them (PoseidonGadget.fill over a map in which the host made every other variable).

    python tools/witness_complete_bench.py [--logs 14,20] [--reps 21] [--sweep 64,256,1024,4096,2147483648] [--json OUT]

BN254; ms.  Device rows are HIP event times on the context's stream (torch events on a stream the context is bound to), warm,
the median of --reps (at least 20) runs; the plan's creation is a host wall time around the synchronising call.
  plan        zkt_witness_plan_create: five selector transforms, their download, the host planner, the upload
  complete    zkt_witness_complete_enqueue at batch 1, 8 and 64 under the default split, public inputs included
  sweep       the same at batch 1 and 8 under zkt_debug_witness_plan_split(wide_min_rows)
  gadgets     PoseidonGadget.fill (zkt_poseidon_gadget_witness_dev, one launch per dependency level)
Before anything is timed the completed map is compared with the map the gadget route makes: equal on every variable."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch
import zkt_plonk_amd as z
import withdraw_workload as WW

P_BN254 = 21888242871839275222246405745257275088548364400416034343698204186575808495617
R = 1 << 256
SELECTORS = ("q_m", "q_l", "q_r", "q_o", "q_c")


def _mont(ctx, vals):
    """canonical Python integers -> (n, 4) Montgomery limbs (the product by R^2 runs on the device, as in bench.py)"""
    arr = np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(-1, 4)
    r2 = np.frombuffer((R * R % P_BN254).to_bytes(32, "little"), dtype=np.uint64)
    return ctx.debug_fr_mul(arr, np.tile(r2, (len(vals), 1)))


def _event_median(stream, fn, reps):
    """median of `reps` event-timed runs of fn (which only enqueues on `stream`), after one warm run"""
    fn()
    stream.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return float(np.median(out)), float(min(out)), float(max(out))


def row(ctx, stream, log_n, reps, sweep):
    width, inputs, height = WW.SHAPES[log_n]
    hs = WW.reference_hasher(P_BN254, width)
    inst = WW.make_instance(hs, inputs, height, seed=0x5EED)
    lay = WW.layout(hs, inst)
    n, n_vars, gates = 1 << log_n, len(lay.values), lay.n_gates
    # the key: the five selectors' coefficients (inverse transforms on the device); the plan reads nothing else of it
    zeros = np.zeros((n, 4), dtype=np.uint64)
    polys = {k: zeros for k in z.PK_ORDER}
    for k in SELECTORS:
        polys[k] = ctx.ntt(log_n, _mont(ctx, lay.q[k] + [0] * (n - gates)), inverse=True)
    ctx.circuit_load(log_n, [polys[k] for k in z.PK_ORDER])
    idx = [np.asarray(w, dtype=np.uint32) for w in lay.w]
    pi_pos = sorted(lay.pi)

    t0 = time.perf_counter()
    plan = z.WitnessPlan(ctx, idx[0], idx[1], idx[2], n_vars, pi_pos)
    t_plan_first = (time.perf_counter() - t0) * 1e3
    plan.close()
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        plan = z.WitnessPlan(ctx, idx[0], idx[1], idx[2], n_vars, pi_pos)
        ts.append((time.perf_counter() - t0) * 1e3)
        if len(ts) < 3:
            plan.close()
    info = plan.info()
    kinds = plan.kinds()

    gadget = z.PoseidonGadget(ctx, hs.width, hs.half_full, hs.partial, _mont(ctx, hs.rc), _mont(ctx, [x for r in hs.mds for x in r]),
                              _mont(ctx, [hs.tag])[0])
    for base, ins in lay.hash_calls:
        gadget.hash(base, ins)
    gadget.stage()
    host_vals = _mont(ctx, lay.values)                              # zeros where the gadget kernels write
    d_ref = torch.from_numpy(host_vals.view(np.int64)).cuda()
    gadget.fill(d_ref.data_ptr(), n_vars, check=True)
    ctx.synchronize()
    ref = d_ref.cpu().numpy().view(np.uint64).reshape(n_vars, 4)

    # the completion starts from the free variables alone: every defined variable is overwritten first
    start = ref.copy()
    start[kinds >= 2] = np.uint64(0x0BAD0BAD)
    batch_max = 64
    d_maps = torch.from_numpy(np.tile(start, (batch_max, 1, 1)).view(np.int64)).cuda()
    d_pi = torch.zeros((batch_max, max(len(pi_pos), 1), 4), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    plan.complete_dev(d_maps.data_ptr(), n_vars, batch_max, d_pi.data_ptr())
    status = plan.status(batch_max)
    got = d_maps.cpu().numpy().view(np.uint64).reshape(batch_max, n_vars, 4)
    assert all(s == (0, None) for s in status), status
    for b in (0, batch_max - 1):
        assert np.array_equal(got[b], ref), "the completed map differs from the gadget route's"
    want_pi = _mont(ctx, [lay.pi[k] for k in pi_pos])
    assert np.array_equal(d_pi.cpu().numpy().view(np.uint64)[0], want_pi), "public inputs differ from the layout's"

    res = {"log_n": log_n, "shape": "x%d %dx%d" % (width, inputs, height), "gates": gates, "variables": n_vars, "info": info,
           "plan_ms_first": round(t_plan_first, 2), "plan_ms": round(float(np.median(ts)), 2), "reps": reps}
    complete = lambda batch: (lambda: plan.complete_dev(d_maps.data_ptr(), n_vars, batch, d_pi.data_ptr()))
    res["complete_ms"] = {str(b): [round(x, 3) for x in _event_median(stream, complete(b), reps)] for b in (1, 8, 64)}
    res["sweep_ms"] = {}
    for wide in sweep:
        plan.split(wide)
        res["sweep_ms"][str(wide)] = {"launches": plan.info()["launches"],
                                      "1": [round(x, 3) for x in _event_median(stream, complete(1), reps)],
                                      "8": [round(x, 3) for x in _event_median(stream, complete(8), reps)]}
    plan.split(0)
    res["gadgets_ms"] = [round(x, 3) for x in _event_median(stream, lambda: gadget.fill(d_ref.data_ptr(), n_vars, check=False), reps)]
    res["gadget_launches"] = len(gadget._staged)
    res["gadget_made_variables"] = len(lay.hash_calls) * hs.per_hash
    plan.complete_dev(d_maps.data_ptr(), n_vars, 1, d_pi.data_ptr())   # after the sweep the map is still the reference's
    ctx.synchronize()
    assert np.array_equal(d_maps[0].cpu().numpy().view(np.uint64).reshape(n_vars, 4), ref)
    plan.close()
    gadget.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", default="14,20")
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--sweep", default="64,256,1024,4096,2147483648")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    assert a.reps >= 20, "the median of at least 20 runs"
    stream = torch.cuda.Stream()
    ctx = z.Context("bn254", 0)
    ctx.set_stream(stream.cuda_stream)
    rows = []
    print("# witness completion from the free variables; BN254 withdraw shapes; ms; events: median [min max] of %d" % a.reps, flush=True)
    for lg in (int(x) for x in a.logs.split(",")):
        r = row(ctx, stream, lg, a.reps, [int(x) for x in a.sweep.split(",")])
        rows.append(r)
        i = r["info"]
        print("2^%d %s: %d gates, %d variables, %d free, %d rule R, depth %d, widest level %d, %d launches, %.1f MB on the device"
              % (r["log_n"], r["shape"], r["gates"], r["variables"], i["n_free"], i["n_right"], i["depth"], i["max_level_rows"], i["launches"],
                 i["device_bytes"] / 1e6), flush=True)
        print("  plan %.1f (first %.1f) | complete batch 1 / 8 / 64: %s | gadget route (%d launches, %d of the variables): %s"
              % (r["plan_ms"], r["plan_ms_first"], " / ".join("%.3f" % r["complete_ms"][b][0] for b in ("1", "8", "64")),
                 r["gadget_launches"], r["gadget_made_variables"], r["gadgets_ms"]), flush=True)
        for wide, s in r["sweep_ms"].items():
            print("  wide_min_rows %s: %d launches, batch 1 %s, batch 8 %s" % (wide, s["launches"], s["1"], s["8"]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
