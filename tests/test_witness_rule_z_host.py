"""CPU: the host planner under ZKT_WITNESS_RULE_IS_ZERO (csrc/witness_plan.hpp) against the Python restatement of rule Z
(tests/is_zero_cases.py): through zkt_debug_witness_plan_host_ex (no device), with the bit set and cleared, and once more as a
stand-alone program (tests/witness_rule_z_host_main.cpp) that also evaluates the schedule on the host, built with
AddressSanitizer + UndefinedBehaviorSanitizer and run as a child process."""
import importlib.util
import os
import subprocess

import numpy as np
import pytest

from oracle import fields as F
import is_zero_cases as Z
import witness_plan_cases as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = {"bn254": F.BN254, "bls12_381": F.BLS12_381}


def _same(c, rules):
    pl = Z.plan(c, rules)
    kind, def_row, level = Z.host_plan(c, rules)
    assert kind == pl.kind, (c.name, rules)
    assert def_row == pl.def_row, (c.name, rules)
    assert level == pl.level, (c.name, rules)
    return pl


@pytest.mark.parametrize("log_n", [3, 4])
@pytest.mark.parametrize("cvname", sorted(CURVES))
def test_cases_with_the_bit_set_and_cleared(cvname, log_n):
    for case in Z.cases(CURVES[cvname], log_n):
        pl = _same(case.c, Z.RULE_IS_ZERO)
        for v, k in case.kinds.items():
            assert pl.kind[v] == k, (case.c.name, v)
        _same(case.c, 0)
    for c, _, _, _ in W.handmade_cases(CURVES[cvname], log_n):
        _same(c, Z.RULE_IS_ZERO)
        _same(c, 0)


@pytest.mark.parametrize("cvname", sorted(CURVES))
def test_wide_case(cvname):
    c = Z.wide_case(CURVES[cvname]).c
    assert _same(c, Z.RULE_IS_ZERO).n_pairs == Z.WIDE_PAIRS
    assert _same(c, 0).n_pairs == 0


@pytest.mark.parametrize("cvname,params", [("bn254", "synthetic"), ("bls12_381", "synthetic"), ("bn254", "shipped")])
def test_no_false_positive_in_the_withdraw_circuit(cvname, params):
    c = W.withdraw(cvname, params, 1)[0]
    assert Z.host_plan(c, Z.RULE_IS_ZERO) == Z.host_plan(c, 0) == W.host_plan(c)


def test_unknown_rule_bits_are_refused():
    import zkt_plonk_amd._lib as L
    c = Z.cases(F.BN254, 3)[0].c
    sel = [W.mont(c.cv, q) for q in c.sel]
    for rules in (2, 3, 1 << 31):
        with pytest.raises(L.ZktError):
            L.debug_witness_plan_host(c.cv.name, sel, c.idx(0), c.idx(1), c.idx(2), c.n_vars, c.pi_pos, rules=rules)


# ---- the stand-alone sanitizer run ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    spec = importlib.util.spec_from_file_location("zkt_build", os.path.join(ROOT, "zkt-plonk_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    tmp = tmp_path_factory.mktemp("witness_rule_z")
    exe = str(tmp / "witness_rule_z_host_main")
    r = subprocess.run([b.CLANG, "-x", "hip", "--cuda-host-only", "-I/opt/rocm/include", "-O1", "-g", "-std=c++17", "-Wno-psabi",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                        os.path.join(ROOT, "tests", "witness_rule_z_host_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]

    def run(c, rules, maps):
        words = lambda arr: " ".join(str(int(x)) for x in np.ascontiguousarray(arr).view("<u4").reshape(-1))
        sel = [W.mont(c.cv, q).reshape(-1, 4) for q in c.sel]
        idx = [c.idx(k) for k in range(3)]
        path = str(tmp / "case.txt")
        with open(path, "w") as f:
            f.write("%d %d %d %d %d %d\n" % (0 if c.cv.name == "bn254" else 1, c.n_rows, c.n_vars, len(c.pi_pos), rules, len(maps)))
            f.write(" ".join(str(p) for p in c.pi_pos) + "\n")
            for i in range(c.n_rows):
                f.write(" ".join(words(q[i]) for q in sel) + " %d %d %d\n" % (idx[0][i], idx[1][i], idx[2][i]))
            for m in maps:
                f.write(words(W.mont(c.cv, m)) + "\n")
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (c.name, r.returncode, r.stderr[-3000:])
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
        lines = r.stdout.splitlines()
        head = [int(x) for x in lines[0].split()[1:]]
        ints = lambda ls: [[int(x) for x in l.split()] for l in ls]
        per_var = ints(lines[1:1 + c.n_vars])
        at = 1 + c.n_vars + head[7]
        sched = ints(lines[1 + c.n_vars:at])
        done = [np.array(ints(lines[at + k * c.n_vars:at + (k + 1) * c.n_vars]), dtype="<u4").view("<u8") for k in range(len(maps))]
        return head, per_var, sched, done
    return run


def _check_driver(run, c, rules, witnesses):
    pl = Z.plan(c, rules)
    starts = [Z.prefill(c, pl, v, salt=k + 1) for k, v in enumerate(witnesses)]
    head, per_var, sched, done = run(c, rules, starts)
    assert head[:7] == [pl.depth, pl.max_level_rows, pl.n_free, pl.n_out, pl.n_right, pl.n_unused, pl.n_pairs], c.name
    assert head[7] == len(pl.rows) == len(sched) and 0 <= head[8] <= head[7]
    assert [v[0] for v in per_var] == pl.kind and [v[1] for v in per_var] == pl.def_row and [v[2] for v in per_var] == pl.level
    assert [s[0] for s in sched] == pl.rows, c.name                 # by level, stable in the row
    for s in sched:                                                 # a pair's record names y and z of its first row
        row, out, out2, level = s
        if pl.kind[out] == Z.ZINV:
            assert (out, out2) == (c.w[1][row], c.w[2][row]) and pl.kind[out2] == Z.ZFLAG
        else:
            assert out2 == W.ZERO
    for start, got in zip(starts, done):
        want = Z.complete(c, pl, start)[0]
        assert np.array_equal(got.reshape(-1, 4), W.mont(c.cv, want).reshape(-1, 4)), c.name
    return head


@pytest.mark.parametrize("cvname", sorted(CURVES))
def test_sanitized_planner_and_host_evaluation_on_the_cases(cvname, driver):
    for log_n in (3, 4):
        for case in Z.cases(CURVES[cvname], log_n):
            _check_driver(driver, case.c, Z.RULE_IS_ZERO, case.witnesses)
            if not case.near_miss and log_n == 3:                   # without the bit y is the caller's, and stays
                _check_driver(driver, case.c, 0, case.witnesses[:1])


def test_sanitized_planner_on_the_wide_case_keeps_equal_tuples_once(driver):
    case = Z.wide_case(F.BN254)
    head = _check_driver(driver, case.c, Z.RULE_IS_ZERO, case.witnesses[:2])
    assert head[8] == 1, "300 pairs of the reference's selectors share one coefficient tuple"
