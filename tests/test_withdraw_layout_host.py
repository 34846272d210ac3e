"""CPU: the host planner of the withdraw circuit (csrc/withdraw_layout.hpp) against the oracle's restatement of the
reference composer (oracle/composer.py withdraw_synthesize, through tests/withdraw_cases.py): through
zkt_debug_withdraw_layout_host (no device), and once more as a stand-alone program (tests/withdraw_layout_host_main.cpp)
built with AddressSanitizer + UndefinedBehaviorSanitizer and run as a child process."""
import importlib.util
import os
import subprocess

import numpy as np
import pytest

from oracle import composer as OC, coracle as K

import withdraw_cases as WC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = [(s, False) for s in WC.SHAPES] + [(WC.SHIPPED, True)]
IDS = ["%s-x%d-%dx%d%s" % (s + ("-shipped" if sh else "",)) for s, sh in ALL]


def _check_rows(c, sel, wires, pi_pos, calls):
    """row for row: six selectors, three wires, the public-input positions, the hash-call list"""
    for name, got, want in zip(("q_m", "q_l", "q_r", "q_o", "q_c", "q_lookup"), sel, c.selectors()):
        assert len(got) == c.n_gates and got == want, name
    for name, got, want in zip(("w_l", "w_r", "w_o"), wires, c.wires()):
        assert got == want, name
    assert pi_pos == c.pi_pos
    assert calls == c.hash_calls()


@pytest.mark.parametrize("shape,shipped", ALL, ids=IDS)
def test_host_rows_equal_the_composer(shape, shipped):
    import zkt_plonk_amd._lib as L
    cvname, w, inputs, height = shape
    c = WC.case(cvname, w, inputs, height, shipped)
    out = L.debug_withdraw_layout_host(cvname, c.words, inputs, height)
    assert out["n_gates"] == c.n_gates == OC.withdraw_gate_count(c.prm, inputs, height)
    assert out["n_vars"] == c.n_vars and out["n_pi"] == inputs + 4 and out["n_hashes"] == inputs * (3 + height) + 2
    assert out["vars_per_hash"] == c.prm.gates_per_hash and (out["inputs"], out["height"], out["width"]) == (inputs, height, w)
    assert (1 << out["log_n_min"]) >= c.n_gates > (1 << (out["log_n_min"] - 1)) and out["device_bytes"] == 0
    _check_rows(c, [K.fr_from_mont(c.cv, a) for a in out["selectors"]], [a.tolist() for a in out["wires"]], out["pi_pos"],
                out["hash_calls"].tolist())


def test_the_rows_do_not_depend_on_the_request():
    """Another wallet, another withdrawal, amount_out = 0: the same circuit."""
    a, b = WC.case("bn254", 4, 3, 2), WC.case("bn254", 4, 3, 2, seed=7, mode="all")
    assert a.req["secrets"] != b.req["secrets"]
    assert a.selectors() == b.selectors() and a.wires() == b.wires() and a.pi_pos == b.pi_pos


def test_shapes_the_circuit_does_not_have_are_refused():
    import zkt_plonk_amd._lib as L
    cv = WC.case("bn254", 4, 1, 1).cv
    good = WC.params_words(cv, WC.params("bn254", 4))
    assert L.debug_withdraw_layout_host("bn254", good, 32, 1, rows=False)["n_pi"] == 36
    assert L.debug_withdraw_layout_host("bn254", good, 1, 64, rows=False)["n_hashes"] == 69
    for words, inputs, height in [(WC.params_words(cv, WC.params("bn254", 3)), 1, 1), (good, 0, 1), (good, 33, 1), (good, 1, 0), (good, 1, 65)]:
        with pytest.raises(L.ZktError) as e:
            L.debug_withdraw_layout_host("bn254", words, inputs, height, rows=False)
        assert e.value.code == 1, (words[0], inputs, height)


# ---- the stand-alone sanitizer run ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    spec = importlib.util.spec_from_file_location("zkt_build", os.path.join(ROOT, "zkt-plonk_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    tmp = tmp_path_factory.mktemp("withdraw_layout")
    exe = str(tmp / "withdraw_layout_host_main")
    r = subprocess.run([b.CLANG, "-x", "hip", "--cuda-host-only", "-I/opt/rocm/include", "-O1", "-g", "-std=c++17", "-Wno-psabi",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                        os.path.join(ROOT, "tests", "withdraw_layout_host_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]

    def run(cvname, prm_words, inputs, height):
        width, half_full, partial, rc, mds, tag = prm_words
        words = lambda arr: " ".join(str(int(x)) for x in np.ascontiguousarray(arr).view("<u4").reshape(-1))
        path = str(tmp / "case.txt")
        with open(path, "w") as f:
            f.write("%d %d %d %d %d %d\n" % (0 if cvname == "bn254" else 1, width, half_full, partial, inputs, height))
            f.write(words(rc) + "\n" + words(mds) + "\n" + words(tag) + "\n")
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
        return r.returncode, r.stdout
    return run


@pytest.mark.parametrize("shape,shipped", [ALL[1], ALL[3], ALL[4], ALL[5]], ids=[IDS[1], IDS[3], IDS[4], IDS[5]])
def test_sanitized_planner_equals_the_composer(shape, shipped, driver):
    cvname, w, inputs, height = shape
    c = WC.case(cvname, w, inputs, height, shipped)
    code, out = driver(cvname, c.words, inputs, height)
    assert code == 0, code
    lines = out.splitlines()
    assert [int(x) for x in lines[0].split()[1:]] == [c.n_gates, c.n_vars, inputs * (3 + height) + 2, c.prm.gates_per_hash, inputs + 4]
    pi_pos = [int(x) for x in lines[1].split()]
    n_h = inputs * (3 + height) + 2
    calls = [[int(x) for x in l.split()] for l in lines[2:2 + n_h]]
    rows = np.array([[int(x) for x in l.split()] for l in lines[2 + n_h:]], dtype=np.uint64)
    assert rows.shape == (c.n_gates, 51)
    sel = [K.fr_from_mont(c.cv, np.ascontiguousarray(rows[:, 8 * q:8 * q + 8].astype(np.uint32)).view(np.uint64).reshape(-1, 4)) for q in range(6)]
    _check_rows(c, sel, [rows[:, 48 + x].tolist() for x in range(3)], pi_pos, calls)


def test_sanitized_planner_refuses_width_3(driver):
    c = WC.case("bn254", 4, 1, 1)
    assert driver("bn254", WC.params_words(c.cv, WC.params("bn254", 3)), 1, 1)[0] == 9
