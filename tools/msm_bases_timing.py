"""Times zkt_msm_g1_bases_dev (variable bases) against zkt_msm_g1_dev (the loaded key's window table) on the same
scalars, with the bases equal to the loaded SRS, using HIP events on the context's stream.  Both calls end in a host
finish and a stream synchronise, so each figure is a whole call.  Every size checks that the two results agree.

    python tools/msm_bases_timing.py [--curves bn254,bls12_381] [--logs 10-22] [--reps 5] [--host-log 14]
    ZKT_LIB_PATH=$PWD/_ab/libzkt_exp.so python tools/msm_bases_timing.py --cbits 12,13,14   # digit-width A/B

--cbits sets ZKT_MSMB_CBITS between calls (honoured by the experiments build only: zkt-plonk_amd/build.py --exp) and
times the variable-base call once per width, after the rule's own choice.  --host-log times
zkt_g1_msm_host (one CPU core) once at that size for the ratio."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch
import zkt_plonk_amd as z


def _range(spec):
    if "-" in spec:
        a, b = spec.split("-")
        return list(range(int(a), int(b) + 1))
    return [int(x) for x in spec.split(",")]


def _time(fn, reps, stream):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()                                           # warm-up (scratch allocation, code objects)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0.record(stream)
        fn()
        e1.record(stream)
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), float(min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--curves", default="bn254,bls12_381")
    ap.add_argument("--logs", default="10-22")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cbits", default="")
    ap.add_argument("--host-log", type=int, default=0)
    a = ap.parse_args()
    widths = [int(x) for x in a.cbits.split(",") if x]
    stream = torch.cuda.current_stream()
    print("# %s  lib %s" % (torch.cuda.get_device_name(0), os.path.basename(z.lib_path())), flush=True)
    print("# curve log_n c W  bases_ms(median,min)  srs_ms(median,min)  ratio", flush=True)
    for curve in a.curves.split(","):
        ctx = z.Context(curve, 0)
        ctx.set_stream(stream.cuda_stream)
        for lg in _range(a.logs):
            n = 1 << lg
            ctx.srs_generate(0x1234567 + lg, n)
            bases = torch.from_numpy(ctx.srs_download(0, n).view(np.int64)).cuda()
            g = torch.Generator(device="cuda").manual_seed(lg)
            sc = torch.randint(0, 1 << 62, (n, 4), dtype=torch.int64, device="cuda", generator=g)   # < r: either form
            torch.cuda.synchronize()
            got, _ = ctx.msm_bases_dev(bases.data_ptr(), sc.data_ptr(), n)
            want = ctx.msm_dev(sc.data_ptr(), n)
            assert np.array_equal(got, want), (curve, lg)
            fixed = _time(lambda: ctx.msm_dev(sc.data_ptr(), n), a.reps, stream)
            info = ctx.msm_bases_info(n)
            runs = [(None, info["window_bits"], info["windows"])]
            for c in widths:
                os.environ["ZKT_MSMB_CBITS"] = str(c)
                i2 = ctx.msm_bases_info(n)
                del os.environ["ZKT_MSMB_CBITS"]
                runs.append((c, i2["window_bits"], i2["windows"]))
            for env, c, W in runs:
                if env is not None:
                    os.environ["ZKT_MSMB_CBITS"] = str(env)
                try:
                    if env is not None:
                        got, _ = ctx.msm_bases_dev(bases.data_ptr(), sc.data_ptr(), n)
                        assert np.array_equal(got, want), (curve, lg, env)
                    var = _time(lambda: ctx.msm_bases_dev(bases.data_ptr(), sc.data_ptr(), n), a.reps, stream)
                finally:
                    os.environ.pop("ZKT_MSMB_CBITS", None)
                tag = "rule" if env is None else "cbits=%d" % env
                if env is None:
                    rule = var
                print("%s 2^%d c=%d W=%d  bases %.3f %.3f  srs %.3f %.3f  ratio %.2f  %s" % (
                    curve, lg, c, W, var[0], var[1], fixed[0], fixed[1], var[0] / fixed[0], tag), flush=True)
            if lg == a.host_log:
                pts = ctx.srs_download(0, n)
                sch = sc.cpu().numpy().view(np.uint64)
                t0 = time.perf_counter()
                hres, _ = z._lib.g1_msm_host(curve, pts, sch, True)
                th = (time.perf_counter() - t0) * 1e3
                assert np.array_equal(hres, want), (curve, lg, "host")
                print("%s 2^%d host zkt_g1_msm_host %.1f ms  ->  host / bases %.0fx" % (curve, lg, th, th / rule[0]), flush=True)
            del bases, sc
        ctx.close()


if __name__ == "__main__":
    main()
