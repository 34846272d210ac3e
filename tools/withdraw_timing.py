"""Times the withdraw circuit as a library component (zkt_withdraw_*) on the shapes of tools/withdraw_workload.py SHAPES,
beside the route it replaces on the same machine.

    python tools/withdraw_timing.py [--logs 14,18,20] [--batches 1,8,64] [--reps 5] [--step-timeout 900]

Every GPU step runs in a child process of its own under its own time limit; the steps are chained, so the first one that
fails or runs out of time ends the run.  BN254, the shipped tables; ms; the median of --reps after a warm-up.

  (a) per shape: zkt_withdraw_create (plan + the wiring stamped on the device) and zkt_withdraw_setup (selectors made on the
      device + zkt_circuit_setup_wiring) as wall time, with the "withdraw_layout" HIP-event scope (the row kernels alone);
      beside it the route without the component: `layout` + `setup_vectors` in Python, their conversion and upload, and
      zkt_circuit_setup_wiring.  At the largest shape also PoseidonGadget.fill over the same layout (every hash trace, the
      part of the witness that was made on the device before).
  (b) at the largest shape: zkt_withdraw_witness for batches of requests with siblings from a device tree, enqueue-only
      form, as wall time to the end of the stream and as the "withdraw_witness" HIP-event scope; every path must reach the
      root (bad_paths = 0)."""
import argparse
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

P_BN254 = 21888242871839275222246405745257275088548364400416034343698204186575808495617
R = 1 << 256
TABLE_SIZE = 1024
TAU = 0x5EED5


def _mont(ctx, vals):
    """canonical Python integers -> (n, 4) Montgomery limbs (the product by R^2 runs on the device, as in bench.py)"""
    import numpy as np
    arr = np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(-1, 4)
    r2 = np.frombuffer((R * R % P_BN254).to_bytes(32, "little"), dtype=np.uint64)
    return ctx.debug_fr_mul(arr, np.tile(r2, (len(vals), 1)))


def _params(ctx, hs):
    return (hs.width, hs.half_full, hs.partial, _mont(ctx, hs.rc[:(2 * hs.half_full + hs.partial) * hs.width]),
            _mont(ctx, [x for r in hs.mds for x in r]), _mont(ctx, [hs.tag])[0])


def step_setup(log_n, reps, with_fill):
    import numpy as np
    import zkt_plonk_amd as z
    import withdraw_workload as WW
    width, inputs, height = WW.SHAPES[log_n]
    hs = WW.reference_hasher(P_BN254, width)
    ctx = z.Context("bn254", 0)
    ctx.srs_generate(TAU, (1 << log_n) + 8)
    prm = _params(ctx, hs)
    ctx.profile_enable(True)

    def component():
        t0 = time.perf_counter()
        w = z.WithdrawCircuit(ctx, prm, inputs, height)
        t1 = time.perf_counter()
        commits = w.setup(log_n, TABLE_SIZE)
        t2 = time.perf_counter()
        info = w.info
        w.close()
        return (t1 - t0) * 1e3, (t2 - t1) * 1e3, commits, info

    component()                                                    # warm-up: transform plans, MSM state
    c0, ms0 = ctx.profile_get("withdraw_layout")
    runs = [component() for _ in range(reps)]
    c1, ms1 = ctx.profile_get("withdraw_layout")
    create, setup = float(np.median([r[0] for r in runs])), float(np.median([r[1] for r in runs]))
    info, commits = runs[0][3], runs[0][2]
    print("2^%d x%d %dx%d: %d gates, %d variables, handle %.1f MB | component: create %.2f + setup %.2f = %.2f ms "
          "(withdraw_layout scope: %.3f ms on average over the %d scopes of a create + setup, two row launches each)"
          % (log_n, width, inputs, height, info["n_gates"], info["n_vars"], info["device_bytes"] / 1e6, create, setup, create + setup,
             (ms1 - ms0) / max(c1 - c0, 1), (c1 - c0) // reps), flush=True)

    # the route without the component: the rows in Python, converted and uploaded, then the same setup call
    t0 = time.perf_counter()
    inst = WW.make_instance(hs, inputs, height, seed=0x5EED)
    lay = WW.layout(hs, inst)
    t1 = time.perf_counter()
    vec = WW.setup_vectors(lay, log_n, 5, TABLE_SIZE)
    t2 = time.perf_counter()
    evals = [None if k in ("sigma1", "sigma2", "sigma3") else _mont(ctx, vec[k]) for k in z.PK_ORDER]
    t3 = time.perf_counter()
    theirs = ctx.circuit_setup_wiring(log_n, evals, lay.w[0], lay.w[1], lay.w[2], len(lay.values))
    t4 = time.perf_counter()
    assert np.array_equal(theirs[0], commits[0]) and theirs[1].tolist() == commits[1].tolist(), "the two routes' commitments differ"
    print("2^%d   without it: layout %.0f + setup_vectors %.0f + conversion %.0f + upload and zkt_circuit_setup_wiring %.1f = %.0f ms "
          "(same ten commitments)" % (log_n, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t4 - t3) * 1e3, (t4 - t0) * 1e3), flush=True)
    if with_fill:
        gadget = z.PoseidonGadget(ctx, *prm)
        for base, ins in lay.hash_calls:
            gadget.hash(base, ins)
        n_vars = len(lay.values)
        d_vars = ctx.alloc(n_vars * 32)
        ctx.upload(d_vars, _mont(ctx, lay.values))

        def fill():
            gadget.fill(d_vars, n_vars, check=False)
            ctx.synchronize()
        fill()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fill()
            ts.append((time.perf_counter() - t0) * 1e3)
        print("2^%d   PoseidonGadget.fill of the %d hash calls over the Python-made map: %.2f ms" % (log_n, len(lay.hash_calls), float(np.median(ts))),
              flush=True)
        gadget.close()
        ctx.free(d_vars)
    ctx.close()


def step_witness(log_n, batches, reps):
    import random
    import numpy as np
    import zkt_plonk_amd as z
    import withdraw_workload as WW
    width, inputs, height = WW.SHAPES[log_n]
    hs = WW.reference_hasher(P_BN254, width)
    ctx = z.Context("bn254", 0)
    w = z.WithdrawCircuit(ctx, _params(ctx, hs), inputs, height)
    top = max(batches)
    m = top * inputs
    rnd = random.Random(0xD0E5)
    idents = [rnd.randrange(1, P_BN254) for _ in range(7)]
    secrets = _mont(ctx, [rnd.randrange(1, P_BN254) for _ in range(m)])
    ident = _mont(ctx, [rnd.choice(idents) for _ in range(m)])
    amounts = np.array([rnd.randrange(1, 1 << 40) for _ in range(m)], dtype=np.uint64)
    tree = z.MerkleTree(ctx, w.poseidon_handle, height, 1 << 12)
    d = [ctx.alloc(a.nbytes) for a in (secrets, ident, amounts)] + [ctx.alloc(m * 32)]
    for p, a in zip(d, (secrets, ident, amounts)):
        ctx.upload(p, a)
    ctx.note_leaves(w.poseidon_handle, d[0], d[1], d[2], m, d[3])     # Deposit: the leaves never visit the host
    tree.append(d_leaves=d[3], m=m)
    root = tree.root()
    fresh = _mont(ctx, [rnd.randrange(1, P_BN254) for _ in range(2 * top)])
    reqs = []
    for b in range(top):
        k = slice(b * inputs, (b + 1) * inputs)
        reqs.append(dict(secrets=secrets[k], identifiers=ident[k], amounts=amounts[k], leaf_indices=np.arange(k.start, k.stop, dtype=np.uint64),
                         siblings=None, root=root, new_secret=fresh[2 * b], new_identifier=ident[b], withdraw_amount=int(amounts[k].sum()) // 3))
    d_vars = ctx.alloc(top * w.n_vars * 32)
    ctx.profile_enable(True)
    for batch in batches:
        pi, status = w.witness(reqs[:batch], d_vars, tree=tree)       # warm-up, and the check: every path reaches the root
        assert status == [0] * batch, status
        assert np.array_equal(pi[:, 0], np.tile(root, (batch, 1)))
        c0, ms0 = ctx.profile_get("withdraw_witness")
        host, wall = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            w.witness(reqs[:batch], d_vars, tree=tree, want_pi=False, want_status=False)
            t1 = time.perf_counter()
            ctx.synchronize()
            host.append((t1 - t0) * 1e3)
            wall.append((time.perf_counter() - t0) * 1e3)
        c1, ms1 = ctx.profile_get("withdraw_witness")
        print("2^%d x%d %dx%d batch %d: %d variables each, siblings from a tree of %d leaves | enqueue %.2f ms of host time | to the end of "
              "the stream %.2f ms | withdraw_witness scope %.2f ms"
              % (log_n, width, inputs, height, batch, w.n_vars, m, float(np.median(host)), float(np.median(wall)), (ms1 - ms0) / max(c1 - c0, 1)),
              flush=True)
    for p in d + [d_vars]:
        ctx.free(p)
    tree.close()
    w.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", default="14,18,20")
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=900)
    ap.add_argument("--step", default=None, help="internal: setup:LOG:FILL or witness:LOG")
    a = ap.parse_args()
    if a.step:
        kind, log_n, *rest = a.step.split(":")
        if kind == "setup":
            step_setup(int(log_n), a.reps, rest[0] == "1")
        else:
            step_witness(int(log_n), [int(x) for x in a.batches.split(",")], a.reps)
        return 0
    logs = [int(x) for x in a.logs.split(",")]
    print("# the withdraw circuit as a component; BN254, shipped tables; ms, median of %d" % a.reps, flush=True)
    steps = ["setup:%d:%d" % (lg, lg == max(logs)) for lg in logs] + ["witness:%d" % max(logs)]
    for s in steps:
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", s, "--reps", str(a.reps), "--batches", a.batches],
                                timeout=a.step_timeout).returncode
        except subprocess.TimeoutExpired:
            print("step %s ran out of its %d s: stopping here" % (s, a.step_timeout), flush=True)
            return 124
        if rc:
            print("step %s ended with status %d: stopping here" % (s, rc), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
