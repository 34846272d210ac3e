"""Times zkt_srs_check on keys of service size, resident in HBM (the points_on_device = 1 form): the two profiling scopes
"srs_check_points" (status kernel and its reduction) and "srs_check_msm" (the powers of rho and the MSM, host finish of
each chunk's sum included: the scope closes behind the chunk's synchronise), read with zkt_profile_get, and the wall time
of the call.  One untimed warm-up call, then one timed call.

    python tools/srs_check_timing.py [--cases bn254:20,bls12_381:22] [--decompress-log 22]

The key is count = 2^log + 8 powers of a test trapdoor (zkt_srs_generate, read back and uploaded again as a caller's buffer).
Beside them: zkt_g1_decompress_dev, the existing per-point check, on 2^22 compressed points in HBM (4096 distinct points of
the same key, repeated: the kernel's time does not depend on the points being distinct), wall time of enqueue + synchronise."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import zkt_plonk_amd as z
from zkt_plonk_amd import _lib
from oracle import fields as F, coracle as K, curve as C

TAU = 0x5EED5EED
SEED = bytes(range(1, 33))


def _wall(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def _key(cv, count):
    gen = z.Context(cv.name, 0)
    try:
        gen.srs_generate(TAU, count)
        return gen.srs_download(0, count)
    finally:
        gen.close()


def check_row(cv, log):
    count = (1 << log) + 8
    key = _key(cv, count)
    h, bh = _lib.srs_generate_g2(cv.name, TAU)
    ctx = z.Context(cv.name, 0)
    d = ctx.alloc(key.nbytes)
    try:
        ctx.upload(d, key)
        rep = ctx.srs_check(d, h, bh, SEED, n=count)                    # warm-up: allocations, code objects
        assert rep.ok, rep
        ctx.profile_enable(True)
        wall, rep = _wall(lambda: ctx.srs_check(d, h, bh, SEED, n=count))
        assert rep.ok, rep
        (pc, pms), (mc, mms) = ctx.profile_get("srs_check_points"), ctx.profile_get("srs_check_msm")
        ctx.profile_enable(False)
        print("%s count 2^%d + 8 = %d (%d MiB): call %.1f ms | srs_check_points %.2f ms in %d scopes | srs_check_msm %.1f ms in %d scopes"
              % (cv.name, log, count, key.nbytes >> 20, wall, pms, pc, mms, mc), flush=True)
        swapped = key[:4096].copy()
        swapped[[1000, 1001]] = swapped[[1001, 1000]]
        assert not ctx.srs_check(swapped, h, bh, SEED).structure_ok      # the verdict is a verdict
    finally:
        ctx.free(d)
        ctx.close()
    return key


def decompress_row(cv, key, log):
    n, distinct = 1 << log, 4096
    enc = b"".join(C.point_serialize_compressed(cv, p) for p in K.points_from_mont(cv, key[:distinct]))
    nb = len(enc) // distinct
    data = np.tile(np.frombuffer(enc, dtype=np.uint8), n // distinct)
    ctx = z.Context(cv.name, 0)
    d_in, d_out, d_st = ctx.alloc(n * nb), ctx.alloc(n * 2 * nb), ctx.alloc(n)
    try:
        ctx.upload(d_in, data)

        def run():
            ctx.g1_decompress_dev(d_in, n, d_out, d_st)
            ctx.synchronize()

        run()
        wall, _ = _wall(run)
        st = ctx.download(d_st, (n,), dtype=np.uint8)
        assert not st.any()
        print("%s zkt_g1_decompress_dev 2^%d points: %.2f ms (enqueue + synchronise)" % (cv.name, log, wall), flush=True)
    finally:
        for p in (d_in, d_out, d_st):
            ctx.free(p)
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="bn254:20,bls12_381:22")
    ap.add_argument("--decompress-log", type=int, default=22)
    a = ap.parse_args()
    print("# zkt_srs_check on a key in HBM: one untimed warm-up, one timed call; ms", flush=True)
    for case in a.cases.split(","):
        name, log = case.split(":")
        cv = F.CURVES[name]
        key = check_row(cv, int(log))
        decompress_row(cv, key, a.decompress_log)


if __name__ == "__main__":
    main()
