"""Times zkt_circuit_check_witness_batch against a loop of zkt_circuit_check_witness over the same device maps, and the witness
completion with and without ZKT_WITNESS_RULE_IS_ZERO, on the withdraw circuit of tools/withdraw_workload.py (BN254).  Needs an
MI355X; run it under a time limit:

    timeout -k 10 600 python tools/witness_check_batch_timing.py [--legs check,complete] [--logs 14,20] [--batches 1,16,64] [--reps 21]

check     The maps are completed on the device from the free variables (batch copies of one withdrawal), so the batch call sees
          what a completion leaves.  Only the C calls are timed: the zkt_witness_batch and the zkt_prove_inputs of every witness
          are made before the clock starts.  Batch call and loop alternate within every repetition; the figures are the median,
          minimum and maximum wall time of whole calls (the loop: `batch` calls).  One more, profiled run of each gives the
          stream time of their scopes, "check_witness_batch" and "check_witness" (summed over the loop).  Before anything is
          timed every report of the batch is compared with the single call's, byte for byte.
complete  zkt_witness_complete_enqueue at batch 1, 8 and 64 as wall times from the enqueue to the end of zkt_ctx_synchronize (the
          call is tens of milliseconds long), warm, median [min max] of --reps runs, for a plan made with rules = 0 and one made
          with ZKT_WITNESS_RULE_IS_ZERO, alternating.  The circuit holds no is-zero pair, so the two plans are equal.  A library
          without zkt_witness_plan_create_ex (the parent's, loaded through ZKT_LIB_PATH) gets the rules = 0 column only, so that
          one job can hold both libraries against each other."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import zkt_plonk_amd as z
from zkt_plonk_amd import _lib

if os.environ.get("ZKT_LIB_PATH"):
    # an older library held against this one: the package refuses a library that lacks its newest entries, this tool takes it
    # for the legs that need none of them (the declarations of the older entries are made before the missing ones are met)
    _bind = _lib._bind_witness

    def _bind_what_there_is(L):
        try:
            _bind(L)
        except AttributeError as e:
            print("# %s: not exported by this library" % e, flush=True)
    _lib._bind_witness = _bind_what_there_is
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


class Setup:
    """the withdraw circuit of 2^log_n loaded into ctx (no SRS: the key's polynomials by inverse transforms on the device), its
    wiring in HBM, and `batch_max` maps completed from the free variables"""

    def __init__(self, ctx, log_n, batch_max, rules=0):
        width, inputs, height = WW.SHAPES[log_n]
        hs = WW.reference_hasher(P_BN254, width)
        inst = WW.make_instance(hs, inputs, height, seed=0x5EED)
        lay = WW.layout(hs, inst)
        self.ctx, self.log_n, self.n_vars, self.gates = ctx, log_n, len(lay.values), lay.n_gates
        sel = WW.setup_vectors(lay, log_n, GEN)
        ctx.circuit_load(log_n, [ctx.ntt(log_n, _mont(ctx, sel[k]), inverse=True) for k in z.PK_ORDER])
        del sel
        self.idx = [np.asarray(w, dtype=np.uint32) for w in lay.w]
        self.pi_pos = sorted(lay.pi)
        self.table = _mont(ctx, inst["ident_set"])
        self.plans = {0: z.WitnessPlan(ctx, self.idx[0], self.idx[1], self.idx[2], self.n_vars, self.pi_pos)}
        if rules and hasattr(z.lib(), "zkt_witness_plan_create_ex"):
            self.plans[rules] = z.WitnessPlan(ctx, self.idx[0], self.idx[1], self.idx[2], self.n_vars, self.pi_pos, rules=rules)
        start = _mont(ctx, lay.values)
        start[self.plans[0].kinds() >= 2] = np.uint64(0x0BAD0BAD)          # from the free variables alone
        n_pi = len(self.pi_pos)
        self.held = [ctx.alloc(batch_max * self.n_vars * 32), ctx.alloc(max(batch_max * n_pi * 32, 32))] + [ctx.alloc(x.nbytes) for x in self.idx]
        self.d_maps, self.d_pi, self.d_idx = self.held[0], self.held[1], self.held[2:]
        for k in range(batch_max):
            ctx.upload(self.d_maps + k * self.n_vars * 32, start)
        for d, x in zip(self.d_idx, self.idx):
            ctx.upload(d, x)
        self.batch_max = batch_max
        self.complete(self.plans[0], batch_max)
        assert all(s == (0, None) for s in self.plans[0].status(batch_max))
        self.pis = ctx.download(self.d_pi, (batch_max, n_pi, 4))
        assert np.array_equal(self.pis[0], _mont(ctx, [lay.pi[k] for k in self.pi_pos])), "public inputs differ from the layout's"

    def complete(self, plan, batch):
        plan.complete_dev(self.d_maps, self.n_vars, batch, self.d_pi)

    def close(self):
        for p in self.plans.values():
            p.close()
        for d in self.held:
            self.ctx.free(d)


def check_leg(ctx, log_n, batches, reps):
    s = Setup(ctx, log_n, max(batches))
    try:
        singles = [ctx.prepare_vars_dev(s.d_maps + k * s.n_vars * 32, s.n_vars, s.d_idx[0], s.d_idx[1], s.d_idx[2], s.gates, s.table, s.pi_pos,
                                        s.pis[k], None) for k in range(max(batches))]
        for batch in batches:
            wb = ctx.witness_batch(s.d_maps, s.n_vars, batch, s.n_vars, s.d_idx[0], s.d_idx[1], s.d_idx[2], s.pi_pos, s.d_pi, [s.table],
                                   n_rows=s.gates)
            as_batch = lambda: ctx.check_witness_batch(wb)
            as_loop = lambda: [ctx.check_witness(p) for p in singles[:batch]]
            got, want = as_batch(), as_loop()
            assert all(g.raw == w.raw for g, w in zip(got, want)) and all(g.satisfied for g in got), "the batch's reports differ from the loop's"
            tb, tl = [], []
            for _ in range(reps):
                tb.append(_wall(as_batch)[0])
                tl.append(_wall(as_loop)[0])
            ctx.profile_enable(True)
            as_batch()
            as_loop()
            sb, sl = ctx.profile_get("check_witness_batch")[1], ctx.profile_get("check_witness")[1]
            ctx.profile_enable(False)
            mb, ml = float(np.median(tb)), float(np.median(tl))
            print("2^%d rows %d vars %d | batch %3d | batch call %.3f [%.3f %.3f] scope %.3f | loop %.3f [%.3f %.3f] scopes %.3f | loop / batch %.2f"
                  % (log_n, s.gates, s.n_vars, batch, mb, min(tb), max(tb), sb, ml, min(tl), max(tl), sl, ml / mb), flush=True)
    finally:
        s.close()


def _sync_median(ctx, fn, reps):
    def run():
        fn()
        ctx.synchronize()
    run()
    out = [_wall(run)[0] for _ in range(reps)]
    return float(np.median(out)), float(min(out)), float(max(out))


def complete_leg(ctx, log_n, reps):
    s = Setup(ctx, log_n, 64, rules=1)
    try:
        infos = {r: p.info() for r, p in s.plans.items()}
        assert all(i == infos[0] for i in infos.values()), "the circuit holds no pair: the plans are equal"
        for batch in (1, 8, 64):
            cols = ["rules %d: %.3f [%.3f %.3f]" % ((r,) + _sync_median(ctx, lambda p=p: s.complete(p, batch), reps))
                    for _ in range(2) for r, p in sorted(s.plans.items())]
            print("2^%d complete batch %2d | %s" % (log_n, batch, " | ".join(cols)), flush=True)
    finally:
        s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="check,complete")
    ap.add_argument("--logs", default="14,20")
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--reps", type=int, default=21)
    a = ap.parse_args()
    legs, logs = a.legs.split(","), [int(x) for x in a.logs.split(",")]
    print("# library %s" % z.lib_path(), flush=True)
    if "check" in legs:
        print("# zkt_circuit_check_witness_batch against a loop of zkt_circuit_check_witness; BN254 withdraw circuit, completed maps in HBM; "
              "ms, median [min max] of %d whole calls" % a.reps, flush=True)
        ctx = z.Context("bn254", 0)
        for lg in logs:
            check_leg(ctx, lg, [int(x) for x in a.batches.split(",")], a.reps)
        ctx.close()
    if "complete" in legs:
        print("# zkt_witness_complete_enqueue under the rule bit; wall time to the end of the stream, ms, median [min max] of %d" % a.reps, flush=True)
        ctx = z.Context("bn254", 0)
        for lg in logs:
            complete_leg(ctx, lg, a.reps)
        ctx.close()


if __name__ == "__main__":
    main()
