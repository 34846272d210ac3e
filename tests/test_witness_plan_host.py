"""CPU: the host planner of the witness completion (csrc/witness_plan.hpp) against the Python restatement of the rule
(tests/witness_plan_cases.py): through zkt_debug_witness_plan_host (no device), and once more as a stand-alone program
(tests/witness_plan_host_main.cpp) built with AddressSanitizer + UndefinedBehaviorSanitizer and run as a child process."""
import importlib.util
import os
import subprocess

import pytest

from oracle import fields as F
import witness_plan_cases as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = {"bn254": F.BN254, "bls12_381": F.BLS12_381}


def _same(c):
    pl = W.plan(c)
    kind, def_row, level = W.host_plan(c)
    assert kind == pl.kind, c.name
    assert def_row == pl.def_row, c.name
    assert level == pl.level, c.name
    return pl


@pytest.mark.parametrize("log_n", [3, 4])
@pytest.mark.parametrize("cvname", sorted(CURVES))
def test_handmade_circuits(cvname, log_n):
    for c, free, kinds, bad in W.handmade_cases(CURVES[cvname], log_n):
        pl = _same(c)
        for v, k in kinds.items():
            assert pl.kind[v] == k, (c.name, v)
        assert W.complete(c, pl, W.prefill(c, pl, W.handmade_values(c, free)))[2] == bad, c.name


@pytest.mark.parametrize("cvname,params", [("bn254", "synthetic"), ("bls12_381", "synthetic"), ("bn254", "shipped")])
def test_withdraw_circuits(cvname, params):
    c = W.withdraw(cvname, params, 1)[0]
    pl = _same(c)
    assert pl.n_free == W.withdraw_free_count(2, 3)


def test_an_index_outside_the_map_reads_as_zero_and_bad_arguments_are_refused():
    import zkt_plonk_amd._lib as L
    cv = F.BN254
    c = W.handmade_cases(cv, 3)[0][0]
    sel = [W.mont(cv, q) for q in c.sel]
    kind, def_row, level = L.debug_witness_plan_host(cv.name, sel, c.idx(0), c.idx(1), c.idx(2), 3, c.pi_pos)   # the map cut short
    assert kind.tolist() == [W.FREE, W.FREE, W.OUT]
    with pytest.raises(L.ZktError):
        L.debug_witness_plan_host(cv.name, sel, c.idx(0), c.idx(1), c.idx(2), c.n_vars, [2, 1])
    with pytest.raises(L.ZktError):
        L.debug_witness_plan_host(cv.name, sel, c.idx(0), c.idx(1), c.idx(2), c.n_vars, [1, 1])


# ---- the stand-alone sanitizer run ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    spec = importlib.util.spec_from_file_location("zkt_build", os.path.join(ROOT, "zkt-plonk_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    tmp = tmp_path_factory.mktemp("witness_plan")
    exe = str(tmp / "witness_plan_host_main")
    r = subprocess.run([b.CLANG, "-x", "hip", "--cuda-host-only", "-I/opt/rocm/include", "-O1", "-g", "-std=c++17", "-Wno-psabi",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                        os.path.join(ROOT, "tests", "witness_plan_host_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]

    def run(c, wide_min_rows):
        words = lambda arr: " ".join(str(int(x)) for x in arr.view("<u4").reshape(-1))
        sel = [W.mont(c.cv, q).reshape(-1, 4) for q in c.sel]
        idx = [c.idx(k) for k in range(3)]
        path = str(tmp / "case.txt")
        with open(path, "w") as f:
            f.write("%d %d %d %d %d\n" % (0 if c.cv.name == "bn254" else 1, c.n_rows, c.n_vars, len(c.pi_pos), wide_min_rows))
            f.write(" ".join(str(p) for p in c.pi_pos) + "\n")
            for i in range(c.n_rows):
                f.write(" ".join(words(q[i]) for q in sel) + " %d %d %d\n" % (idx[0][i], idx[1][i], idx[2][i]))
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (c.name, r.returncode, r.stderr[-3000:])
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
        lines = r.stdout.splitlines()
        head = [int(x) for x in lines[0].split()[1:]]
        per_var = [[int(x) for x in l.split()] for l in lines[1:1 + c.n_vars]]
        sched = [[int(x) for x in l.split()] for l in lines[1 + c.n_vars:]]
        return head, per_var, sched
    return run


def _check_driver(run, c, wide_min_rows):
    pl = W.plan(c)
    head, per_var, sched = run(c, wide_min_rows)
    depth, widest, n_free, n_out, n_right, n_unused, scheduled, tuples, launches = head
    assert (depth, widest, n_free, n_out, n_right, n_unused) == (pl.depth, pl.max_level_rows, pl.n_free, pl.n_out, pl.n_right, pl.n_unused)
    assert scheduled == len(pl.rows) == len(sched) and launches == W.launches(pl, wide_min_rows)
    assert 0 <= tuples <= max(scheduled, 0) and (tuples > 0) == (scheduled > 0)
    assert [v[0] for v in per_var] == pl.kind and [v[1] for v in per_var] == pl.def_row and [v[2] for v in per_var] == pl.level
    assert [s[0] for s in sched] == pl.rows                      # by level, stable in the row
    return tuples


@pytest.mark.parametrize("cvname", sorted(CURVES))
def test_sanitized_planner_on_the_handmade_circuits(cvname, driver):
    for log_n in (3, 4):
        for c, _, _, _ in W.handmade_cases(CURVES[cvname], log_n):
            _check_driver(driver, c, 2)


@pytest.mark.parametrize("cvname,wide", [("bn254", 87), ("bls12_381", 40)])
def test_sanitized_planner_on_the_withdraw_circuit(cvname, wide, driver):
    c = W.withdraw(cvname, "synthetic", 1)[0]
    tuples = _check_driver(driver, c, wide)
    assert tuples < c.n_rows // 4, "equal coefficient tuples are kept once"
