"""Times the KZG commitment seam (zkt_kzg_commit_batch / zkt_kzg_open) against what a KZG10 wrapper did before it: one
blocking zkt_msm_g1 per polynomial.  Everything runs in one process; old and new alternate within every repetition, and
every figure is the median wall time of whole calls (each call ends in a host finish and a stream synchronise).

    python tools/kzg_seam_timing.py [--reps 5] [--quick]

Rows:
  commit  <curve> 2^<log> k=<k>  dev batch vs zkt_msm_g1_dev loop, host batch vs zkt_msm_g1 loop  (ms per commitment)
  open    <curve> 2^<log> k=10   zkt_kzg_open host / _dev (ms per call) and the profiling scopes of one profiled call
The results of the batch and of the loop are compared on every row."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import zkt_plonk_amd as z

SCOPES = ["kzg_open_upload", "kzg_open_combine", "kzg_open_divide", "kzg_open_msm", "kzg_commit_batch"]


def _fr(n, rng):
    """n random values below 2^254 (valid Montgomery limbs on both curves)"""
    s = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) * np.uint64(2)
    s[:, 3] &= np.uint64((1 << 61) - 1)
    return s


def _wall(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def _alternate(fns, reps):
    """median ms of each fn, the fns called in turn within every repetition (after one warm-up round)"""
    for f in fns:
        f()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, f in enumerate(fns):
            ts[i].append(_wall(f)[0])
    return [float(np.median(t)) for t in ts]


def commit_rows(ctx, curve, lg, ks, reps, rng):
    n = 1 << lg
    kmax = max(ks)
    polys = [_fr(n, rng) for _ in range(kmax)]
    d = []
    for p in polys:
        d.append(ctx.alloc(p.nbytes))
        ctx.upload(d[-1], p)
    try:
        for k in ks:
            ps, ds, lens = polys[:k], d[:k], [n] * k
            got = ctx.kzg_commit_batch_dev(ds, lens)
            want = [ctx.msm_dev(ds[j], n) for j in range(k)]
            assert all(np.array_equal(g[0], w) for g, w in zip(got, want)), (curve, lg, k)
            got_h = ctx.kzg_commit_batch(ps)
            assert all(np.array_equal(g[0], w) for g, w in zip(got_h, want)), (curve, lg, k, "host")
            t = _alternate([lambda: ctx.kzg_commit_batch_dev(ds, lens),
                            lambda: [ctx.msm_dev(ds[j], n) for j in range(k)],
                            lambda: ctx.kzg_commit_batch(ps),
                            lambda: [ctx.msm(ps[j]) for j in range(k)]], reps)
            print("commit %-9s 2^%d k=%d  dev batch %.3f  dev loop %.3f  (%.2fx)   host batch %.3f  host loop %.3f  (%.2fx)"
                  "  ms/commitment" % (curve, lg, k, t[0] / k, t[1] / k, t[1] / t[0], t[2] / k, t[3] / k, t[3] / t[2]),
                  flush=True)
    finally:
        for x in d:
            ctx.free(x)


def open_rows(ctx, curve, lg, k, reps, rng):
    n = 1 << lg
    polys = [_fr(n - j, rng) for j in range(k)]
    ch = _fr(k, rng)
    zz = _fr(1, rng)[0]
    d = []
    for p in polys:
        d.append(ctx.alloc(p.nbytes))
        ctx.upload(d[-1], p)
    lens = [p.shape[0] for p in polys]
    try:
        a = ctx.kzg_open(polys, ch, zz)
        b = ctx.kzg_open_dev(d, lens, ch, zz)
        assert np.array_equal(a[0][0], b[0][0]) and np.array_equal(a[1], b[1]), (curve, lg, "open host / dev")
        t = _alternate([lambda: ctx.kzg_open(polys, ch, zz), lambda: ctx.kzg_open_dev(d, lens, ch, zz)], reps)
        print("open   %-9s 2^%d k=%d  host %.3f  dev %.3f  ms/call" % (curve, lg, k, t[0], t[1]), flush=True)
        for form, fn in (("host", lambda: ctx.kzg_open(polys, ch, zz)), ("dev", lambda: ctx.kzg_open_dev(d, lens, ch, zz))):
            ctx.profile_enable(True)
            fn()
            ctx.synchronize()
            parts = []
            for s in SCOPES[:4]:
                c, ms = ctx.profile_get(s)
                if c:
                    parts.append("%s %.3f" % (s[9:], ms))
            ctx.profile_enable(False)
            print("open   %-9s 2^%d k=%d  %s scopes (ms, stream time): %s" % (curve, lg, k, form, "  ".join(parts)), flush=True)
    finally:
        for x in d:
            ctx.free(x)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="BN254 only, smaller sizes (a check that the tool runs)")
    a = ap.parse_args()
    rng = np.random.default_rng(20)
    print("# zkt_kzg_commit_batch / zkt_kzg_open against per-polynomial zkt_msm_g1 calls; median of %d, ms" % a.reps, flush=True)
    for curve in (["bn254"] if a.quick else ["bn254", "bls12_381"]):
        ctx = z.Context(curve, 0)
        lg = 14 if a.quick else 20
        ctx.srs_generate(0x5EED, 1 << lg)
        commit_rows(ctx, curve, lg, [1, 3, 6], a.reps, rng)
        open_rows(ctx, curve, lg, 10, a.reps, rng)
        if curve == "bn254" and not a.quick:
            ctx.srs_generate(0x5EED, 1 << 18)      # the size where grouped launches are on
            commit_rows(ctx, curve, 18, [3], a.reps, rng)
        ctx.close()


if __name__ == "__main__":
    main()
