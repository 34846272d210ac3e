"""CPU pins of zkt_circuit_check_witness: the plain-Python restatement of its rules (tests/witness_cases.py) against the
oracle's ConstraintSystem.check_satisfied and a hand-computed case, and the declaration in the public header against its
ctypes and Rust mirrors."""
import ctypes
import os
import re
import subprocess

import pytest

from oracle import fields as F

import witness_cases as WC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zkt_plonk.h")
FIELDS = ["satisfied", "checked", "n_arithmetic", "first_arithmetic", "residual", "n_lookup", "first_lookup", "n_wiring",
          "first_wiring_row", "first_wiring_column"]


@pytest.fixture(scope="module")
def cases():
    return WC.cs_cases(F.BN254)


def test_restatement_agrees_with_check_satisfied(cases):
    """satisfied (arithmetic and lookup rules) == cs.check_satisfied() for every case that is a ConstraintSystem; both
    outcomes occur."""
    seen = set()
    for name, (wit, key) in cases.items():
        rep = WC.report_of_cs(wit, key)
        assert rep["checked"] == 3 and rep["n_wiring"] == 0
        assert rep["satisfied"] == WC.combined(wit, key).check_satisfied(), name
        assert rep["satisfied"] == (rep["n_arithmetic"] == 0 and rep["n_lookup"] == 0)
        seen.add(rep["satisfied"])
    assert seen == {True, False}


def test_what_the_cases_are_meant_to_break(cases):
    p = F.BN254.fr.p
    for base in ("test_circuit", "synthetic_700", "synthetic_1024"):
        cs = cases[base][0]
        assert WC.report_of_cs(cs, wiring=True) == dict(satisfied=True, checked=7, n_arithmetic=0, first_arithmetic=None,
                                                        residual=0, n_lookup=0, first_lookup=None, n_wiring=0,
                                                        first_wiring=None)
        several = WC.report_of_cs(*cases[base + "/one_value_changed"])
        assert several["n_arithmetic"] >= 1 and several["residual"] != 0
        rnd = WC.report_of_cs(*cases[base + "/random_witness"])
        assert rnd["first_arithmetic"] == 0 and rnd["n_arithmetic"] >= cs.n_gates * 9 // 10
        for label, row in (("row0", 0), ("last_gate", cs.n_gates - 1)):
            for sign, want in (("plus", 1), ("minus", p - 1)):
                rep = WC.report_of_cs(*cases["%s/qc_%s_1_%s" % (base, sign, label)])
                assert (rep["n_arithmetic"], rep["first_arithmetic"], rep["residual"], rep["n_lookup"]) == (1, row, want, 0)
        pi_row = sorted(cs.pi)[0]
        rep = WC.report_of_cs(*cases[base + "/wrong_public_input"])
        assert (rep["n_arithmetic"], rep["first_arithmetic"], rep["residual"]) == (1, pi_row, 5)
        rep = WC.report_of_cs(*cases[base + "/moved_public_input"])
        assert rep["n_arithmetic"] == 2 and rep["first_arithmetic"] == 0
        rep = WC.report_of_cs(*cases[base + "/table_value_removed"])
        assert rep["n_arithmetic"] == 0 and rep["n_lookup"] >= 1
        assert WC.report_of_cs(*cases[base + "/table_reversed"])["satisfied"]
        assert WC.report_of_cs(*cases[base + "/table_empty"])["n_lookup"] == len(WC.lookup_rows(cs))
        swap = WC.report_of_cs(*cases[base + "/equal_value_swap"], wiring=True)
        assert swap["n_arithmetic"] == 0 and swap["n_lookup"] == 0 and swap["n_wiring"] > 1 and not swap["satisfied"]
    assert cases["synthetic_1024"][0].n_gates == cases["synthetic_1024"][0].circuit_bound() == 1024
    assert WC.third_kind_rows(cases["synthetic_700"][0])


def test_hand_computed_two_row_case():
    """n = 4, two gate rows, p = the BN254 scalar field.  Row 0: 3 * 5 - 15 = 0 (a mul gate).  Row 1: a + b - c + pi with
    (a, b, c) = (5, 15, 21) and pi = 2 gives 1; c = 21 is looked up in {7, 20}: not there.  Rows 2 and 3 are padding:
    all-zero wires; row 3 carries q_c = 9 in the key, so it fails as well with 9."""
    p = F.BN254.fr.p
    sel = dict(q_m=[1, 0], q_l=[0, 1], q_r=[0, 1], q_o=[p - 1, p - 1], q_c=[0, 0, 0, 9], q_lookup=[0, 1])
    rep = WC.expected_report(p, 4, sel, [3, 5], [5, 15], [15, 21], [7, 20], {1: 2})
    assert rep == dict(satisfied=False, checked=3, n_arithmetic=2, first_arithmetic=1, residual=1, n_lookup=1, first_lookup=1,
                       n_wiring=0, first_wiring=None)
    ok = WC.expected_report(p, 4, dict(sel, q_c=[0, 0]), [3, 5], [5, 15], [15, 22], [7, 22], {1: 2})
    assert ok["satisfied"] and ok["first_arithmetic"] is None and ok["residual"] == 0
    # a looked-up zero passes whatever the table holds; the wiring rule counts wires in the order 3 row + column
    zero = WC.expected_report(p, 4, dict(sel, q_c=[0, 0]), [3, 5], [5, p - 7], [15, 0], [], {1: 2})
    assert zero["n_lookup"] == 0 and zero["n_arithmetic"] == 0
    Z = 0xFFFFFFFF
    key_w = ([0, 1], [1, 2], [2, Z])
    got_w = ([0, 1], [1, 2], [2, 0])           # the last output wire now joins variable 0's cycle
    rep = WC.expected_report(p, 4, dict(sel, q_c=[0, 0]), [3, 5], [5, 15], [15, 22], [7, 22], {1: 2}, key_w, got_w)
    assert rep["checked"] == 7 and rep["n_wiring"] == 2 and rep["first_wiring"] == (0, 0) and not rep["satisfied"]


def _header_code():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_the_call_and_the_report():
    code = _header_code()
    m = re.search(r"int\s+zkt_circuit_check_witness\s*\(([^)]*)\)\s*;", code)
    assert m, "zkt_circuit_check_witness is not declared"
    params = [x.strip() for x in m.group(1).split(",")]
    assert len(params) == 4
    assert params[0].startswith("zkt_ctx*") and "zkt_prove_inputs*" in params[1] and params[2].startswith("int ")
    assert "zkt_witness_report*" in params[3]
    assert code.index("zkt_prove_with") < code.index("zkt_circuit_check_witness")
    body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*zkt_witness_report\s*;", code).group(1)
    names = [re.match(r".*?(\w+)\s*(\[\d+\])?$", d.strip()).group(1) for d in body.split(";") if d.strip()]
    assert names == FIELDS
    assert re.search(r"ZKT_CHECK_WIRING\s*=\s*1\b", code) and re.search(r"#define\s+ZKT_CHECK_NONE\s+\(\(uint64_t\)-1\)", code)


def test_ctypes_mirror_has_the_c_layout(tmp_path):
    from zkt_plonk_amd import _lib
    assert [f[0] for f in _lib.WitnessReport._fields_] == FIELDS
    offsets = ", ".join("(unsigned long)offsetof(zkt_witness_report, %s)" % f for f in FIELDS)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "zkt_plonk.h"\n'
                   'int main(void) { unsigned long v[] = {(unsigned long)sizeof(zkt_witness_report), %s}; '
                   'for (unsigned i = 0; i < sizeof v / sizeof v[0]; ++i) printf("%%lu\\n", v[i]); return 0; }\n' % offsets)
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert ctypes.sizeof(_lib.WitnessReport) == got[0]
    assert [getattr(_lib.WitnessReport, f).offset for f in FIELDS] == got[1:]
    assert [getattr(_lib.WitnessReport, f).size for f in FIELDS] == [4, 4, 8, 8, 32, 8, 8, 8, 8, 4]
    assert _lib.CHECK_WIRING == WC.CHECK_WIRING == 1 and _lib.CHECK_NONE == (1 << 64) - 1


def test_library_and_mirrors_name_the_call():
    import zkt_plonk_amd as z
    from zkt_plonk_amd import _lib
    assert "zkt_circuit_check_witness" in z.declared_symbols()
    assert hasattr(z.lib(), "zkt_circuit_check_witness")
    assert len(z.lib().zkt_circuit_check_witness.argtypes) == 4
    assert callable(_lib.Context.check_witness) and callable(z.GpuProver.check_witness)
    ffi = open(os.path.join(ROOT, "shim", "src", "ffi.rs")).read()
    assert re.search(r"pub fn zkt_circuit_check_witness\(", ffi) and "pub struct ZktWitnessReport" in ffi
    rust = re.search(r"pub struct ZktWitnessReport \{(.*?)\}", ffi, flags=re.S).group(1)
    assert re.findall(r"pub (\w+):", rust) == FIELDS
