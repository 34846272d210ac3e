"""Times batch verification on the host (zkt_verify_batch) against the device route (zkt_verify_batch_dev) in one run, on
batches of 1, 16, 256 and 4096 proofs made by repeating three oracle proofs (circuits of 150 / 90 / 150 gates, one SRS),
and then zkt_verify_batch_locate with 0, 1 and 8 bad proofs (a flipped evaluation byte) against a loop of zkt_verify
over the same batch.  Needs an MI355X; run it under a time limit:

    timeout -k 10 900 python tools/verify_batch_timing.py [--reps 3] [--counts 1,16,256,4096] [--curves bn254,bls12_381]

Only the C calls are timed (the argument arrays and the seeded transcripts are made before the clock starts); host and
device alternate within every repetition and the figure is the median wall time of whole calls.  Per-stage device times
come from the profile scopes "verify_decompress" and "verify_msm" ("verify_leaves" and "verify_tree" in the second table)
of one more, profiled call; "host part" is that call's wall time minus the scopes.  The zkt_verify loop runs once per
count, over the batch with one bad proof.  The last line per curve and table names the smallest measured count at which
the device route (the locate call) is faster.

A third table (--legs terms alone prints only this one) times zkt_verify_batch_dev with the per-proof term stage on the
host (zkt_ctx_set_verify_terms mode 0) and on the device (mode 1), the two modes alternating within every repetition:
median, minimum and maximum of whole C calls, then one profiled call per mode with its scopes ("verify_terms" is the new
stage) and the host time that is left per proof.  A library without the switch (the parent's, loaded through
ZKT_LIB_PATH) gets the mode-0 columns only, so that one job can hold both libraries against each other."""
import argparse
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import zkt_plonk_amd as z
from zkt_plonk_amd import _lib
from oracle import fields as F
from test_gpu_verify_batch import _made, _items, _cycle

CURVES = {"bn254": F.BN254, "bls12_381": F.BLS12_381}


def _call(fn, handle, cv, entries, h, beta_h):
    """one timed C call on fresh transcripts -> (ms, accepted)"""
    cid = _lib.curve_id(cv.name)
    ins, trs, k, hh, bh, keep = _lib._verify_batch_args(cid, _items(cv, entries), h, beta_h)
    ok = ctypes.c_int(0)
    u = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    t0 = time.perf_counter()
    rc = fn(handle if handle is not None else cid, ins, trs, k, u(hh), u(bh), ctypes.byref(ok))
    ms = (time.perf_counter() - t0) * 1e3
    assert rc == 0, rc
    return ms, bool(ok.value)


def _locate(L, ctx, cv, entries, h, beta_h):
    """one timed zkt_verify_batch_locate on fresh transcripts -> (ms, accepted, bad positions, n_checks)"""
    ins, trs, k, hh, bh, keep = _lib._verify_batch_args(ctx.curve, _items(cv, entries), h, beta_h)
    ok, n_bad, n_chk = ctypes.c_int(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    bad = np.zeros(k, dtype=np.uint8)
    u = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    t0 = time.perf_counter()
    rc = L.zkt_verify_batch_locate(ctx.handle, ins, trs, k, u(hh), u(bh), ctypes.byref(ok),
                                   bad.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), ctypes.byref(n_bad), ctypes.byref(n_chk))
    ms = (time.perf_counter() - t0) * 1e3
    assert rc == 0, rc
    return ms, bool(ok.value), np.flatnonzero(bad).tolist(), n_chk.value


def _verify_loop(L, cv, entries, h, beta_h):
    """zkt_verify proof by proof over the batch -> (ms, bad positions)"""
    cid = _lib.curve_id(cv.name)
    ins, trs, k, hh, bh, keep = _lib._verify_batch_args(cid, _items(cv, entries), h, beta_h)
    u = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    ph, pbh, ok, bad = u(hh), u(bh), ctypes.c_int(0), []
    t0 = time.perf_counter()
    for i in range(k):
        rc = L.zkt_verify(cid, ctypes.byref(ins[i]), trs[i], ph, pbh, ctypes.byref(ok))
        assert rc == 0, rc
        if not ok.value:
            bad.append(i)
    return (time.perf_counter() - t0) * 1e3, bad


def _flip(entries, positions):
    out = list(entries)
    for i in positions:
        vk, pis, proof, kind = out[i]
        raw = bytearray(proof)
        raw[-40] ^= 1
        out[i] = (vk, pis, bytes(raw), kind)
    return out


def locate_leg(L, ctx, cv, made, h, beta_h, counts, reps_arg):
    name = cv.name
    _lib.verify(cv.name, *_items(cv, made[:1])[0][:7], h, beta_h, _items(cv, made[:1])[0][7])   # binds zkt_verify's argument types
    _locate(L, ctx, cv, _flip(made, [1]), h, beta_h)                            # first use: allocations, code load
    print("%s: count | bad | locate ms | n_checks | stages: leaves ms, tree ms, rest ms | zkt_verify loop ms | loop/locate" % name)
    wins = None
    for count in counts:
        entries = _cycle(made, count)
        reps = reps_arg if count <= 256 else max(1, reps_arg // 3)
        one_bad = [count // 2]
        loop_ms, loop_bad = _verify_loop(L, cv, _flip(entries, one_bad), h, beta_h)
        assert loop_bad == one_bad
        for n_bad in (0, 1, 8):
            if n_bad > count:
                continue
            positions = one_bad if n_bad == 1 else [(2 * j + 1) * count // (2 * n_bad) for j in range(n_bad)]
            batch = _flip(entries, positions)
            t = []
            for _ in range(reps):
                ms, ok, bad, n_checks = _locate(L, ctx, cv, batch, h, beta_h)
                assert bad == sorted(positions) and ok == (not positions)
                t.append(ms)
            ctx.profile_enable(True)
            wall, ok, bad, n_checks = _locate(L, ctx, cv, batch, h, beta_h)
            leaves = ctx.profile_get("verify_leaves")[1] if n_bad else 0.0
            tree = ctx.profile_get("verify_tree")[1] if n_bad else 0.0
            ctx.profile_enable(False)
            loc = float(np.median(t))
            tail = "%9.2f | %6.2f" % (loop_ms, loop_ms / loc) if n_bad == 1 else "        - |      -"
            if n_bad == 1 and wins is None and loc < loop_ms:
                wins = count
            print("%s: %5d | %d | %9.2f | %3d | %8.2f %8.2f %8.2f | %s"
                  % (name, count, n_bad, loc, n_checks, leaves, tree, wall - leaves - tree, tail), flush=True)
    print("%s: locating one bad proof is faster than the zkt_verify loop from count = %s on (of the counts measured)" % (name, wins),
          flush=True)


def terms_leg(L, ctx, cv, made, h, beta_h, counts, reps_arg):
    name = cv.name
    modes = [0, 1] if hasattr(L, "zkt_ctx_set_verify_terms") else [0]
    for mode in modes:                                                          # first use of either route: allocations, code load
        if len(modes) > 1:
            ctx.set_verify_terms(mode)
        _call(L.zkt_verify_batch_dev, ctx.handle, cv, _cycle(made, max(counts)), h, beta_h)
    print("%s: library %s" % (name, os.path.basename(_lib.lib_path())))
    print("%s: count | mode | reps | median ms | min ms | max ms | scopes: decompress ms, terms ms, msm ms | host rest ms | host rest per proof ms"
          % name)
    wins = None
    for count in counts:
        entries = _cycle(made, count)
        reps = reps_arg if count <= 256 else max(3, reps_arg // 3)
        t = {m: [] for m in modes}
        for _ in range(reps):
            for mode in modes:
                if len(modes) > 1:
                    ctx.set_verify_terms(mode)
                ms, ok = _call(L.zkt_verify_batch_dev, ctx.handle, cv, entries, h, beta_h)
                assert ok
                t[mode].append(ms)
        for mode in modes:
            if len(modes) > 1:
                ctx.set_verify_terms(mode)
            ctx.profile_enable(True)
            before = {k: ctx.profile_get(k)[1] for k in ("verify_decompress", "verify_terms", "verify_msm")}
            wall, ok = _call(L.zkt_verify_batch_dev, ctx.handle, cv, entries, h, beta_h)
            dec, trm, msm = (ctx.profile_get(k)[1] - before[k] for k in ("verify_decompress", "verify_terms", "verify_msm"))
            ctx.profile_enable(False)
            rest = wall - dec - trm - msm
            print("%s: %5d | %d | %2d | %9.3f | %9.3f | %9.3f | %8.3f %8.3f %8.3f | %9.3f | %.4f"
                  % (name, count, mode, reps, float(np.median(t[mode])), min(t[mode]), max(t[mode]), dec, trm, msm, rest, rest / count),
                  flush=True)
        if len(modes) > 1 and wins is None and np.median(t[1]) < np.median(t[0]):
            wins = count
    if len(modes) > 1:
        ctx.set_verify_terms(0)
        print("%s: mode 1 is faster than mode 0 from count = %s on (of the counts measured)" % (name, wins), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="batch,locate,terms")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--counts", default="1,16,256,4096")
    ap.add_argument("--curves", default="bn254,bls12_381")
    args = ap.parse_args()
    counts = [int(x) for x in args.counts.split(",")]
    L = z.lib()
    for name in args.curves.split(","):
        cv = CURVES[name]
        made, srs, h, beta_h, wrong = _made(cv)
        ctx = z.Context(cv.name, 0)
        try:
            assert _lib.verify_batch(cv.name, _items(cv, made), h, beta_h)      # binds the host entry's argument types
            _call(L.zkt_verify_batch_dev, ctx.handle, cv, made, h, beta_h)      # first use: allocations, code load
            legs = args.legs.split(",")
            if "terms" in legs:
                terms_leg(L, ctx, cv, made, h, beta_h, counts, args.reps)
            if "batch" not in legs:
                if "locate" in legs:
                    locate_leg(L, ctx, cv, made, h, beta_h, counts, args.reps)
                continue
            print("%s: count | host ms | dev ms | host/dev | dev stages: decompress ms, msm ms, host part ms | per proof host, dev ms" % name)
            crossover = None
            for count in counts:
                entries = _cycle(made, count)
                reps = args.reps if count <= 256 else max(1, args.reps // 3)
                th, td = [], []
                for _ in range(reps):
                    ms, ok = _call(L.zkt_verify_batch, None, cv, entries, h, beta_h)
                    assert ok
                    th.append(ms)
                    ms, ok = _call(L.zkt_verify_batch_dev, ctx.handle, cv, entries, h, beta_h)
                    assert ok
                    td.append(ms)
                ctx.profile_enable(True)
                wall, ok = _call(L.zkt_verify_batch_dev, ctx.handle, cv, entries, h, beta_h)
                dec, msm = ctx.profile_get("verify_decompress")[1], ctx.profile_get("verify_msm")[1]
                ctx.profile_enable(False)
                host, dev = float(np.median(th)), float(np.median(td))
                if crossover is None and dev < host:
                    crossover = count
                print("%s: %5d | %9.2f | %9.2f | %5.2f | %8.2f %8.2f %8.2f | %.3f %.3f"
                      % (name, count, host, dev, host / dev, dec, msm, wall - dec - msm, host / count, dev / count), flush=True)
            print("%s: the device route is faster from count = %s on (of the counts measured)" % (name, crossover), flush=True)
            if "locate" in legs:
                locate_leg(L, ctx, cv, made, h, beta_h, counts, args.reps)
        finally:
            ctx.close()


if __name__ == "__main__":
    main()
