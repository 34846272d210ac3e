"""CPU: the C-ABI of zkt_circuit_check_witness_batch, zkt_witness_plan_create_ex and zkt_debug_witness_plan_host_ex as the
header declares them, as _lib.py and witness.py mirror them and as the built library exports them; zkt_witness_batch's size and
field offsets against the header, compiled; zkt_witness_plan_report keeps its size."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zkt_plonk.h")
FUNCS = {"zkt_circuit_check_witness_batch": 4, "zkt_witness_plan_create_ex": 11, "zkt_debug_witness_plan_host_ex": 11}
BATCH_FIELDS = ["d_variables", "stride", "batch", "n_vars", "w_l", "w_r", "w_o", "n_rows", "wiring_on_device", "pi_pos", "n_pi",
                "d_pi_vals", "tables", "table_lens", "n_tables"]
REPORT_FIELDS = ["n_free", "n_out", "n_right", "n_unused", "depth", "max_level_rows", "launches", "reserved", "device_bytes"]


def _code():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


@pytest.mark.parametrize("name", sorted(FUNCS))
def test_header_declares_the_entry_points(name):
    m = re.search(r"\b%s\s*\((.*?)\)\s*;" % re.escape(name), _code(), flags=re.S)
    assert m, "%s is not declared" % name
    params = [x.strip() for x in m.group(1).split(",")]
    assert len(params) == FUNCS[name]
    if name == "zkt_witness_plan_create_ex":
        assert params[-2].startswith("uint32_t rules") and params[-1].startswith("zkt_witness_plan**")
    if name == "zkt_circuit_check_witness_batch":
        assert params[1].startswith("const zkt_witness_batch*") and params[3].startswith("zkt_witness_report*")


def test_header_states_rule_z_and_the_batch_contract():
    text = open(HEADER).read()
    assert re.search(r"enum\s*\{\s*ZKT_WITNESS_RULE_IS_ZERO\s*=\s*1\s*\}", _code())
    doc = text[text.index("Witness completion from the circuit's free variables"):text.index("int zkt_witness_plan_create")]
    for said in ("Rule Z", "Rule O", "Rule R", "ZKT_WITNESS_RULE_IS_ZERO", "mod.rs:243-289", "q_l = q_r = 0", "-q_c / q_o", "-q_c / (q_m x)",
                 "never unsolvable", "mul_gate on a first-seen right operand", "opt-in"):
        assert said in doc, said
    assert "exactly its\n * direct assign_variable calls" not in doc
    doc = text[text.index("int zkt_circuit_check_witness("):text.index("int zkt_circuit_check_witness_batch")]
    for said in ("field for field", "synchronises once", "copied into every report", "no _dev suffix", "n_tables not 0, 1 or batch",
                 "On an error no report is written"):
        assert said in doc, said
    assert "32 B a scheduled row" in text
    kinds = text[text.index("int zkt_witness_plan_info"):text.index("int zkt_witness_plan_kinds")]
    assert "4 rule Z" in kinds and "5 rule Z" in kinds


def test_struct_layouts_against_the_compiled_header(tmp_path):
    from zkt_plonk_amd import _lib
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "zkt_plonk.h"', "int main(void) {",
             '    printf("%zu %zu %zu\\n", sizeof(zkt_witness_batch), sizeof(zkt_witness_plan_report), sizeof(zkt_witness_report));']
    lines += ['    printf("%%zu\\n", offsetof(zkt_witness_batch, %s));' % f for f in BATCH_FIELDS]
    lines += ['    printf("%%zu\\n", offsetof(zkt_witness_plan_report, %s));' % f for f in REPORT_FIELDS]
    lines += ["    return 0;", "}"]
    src.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "layout")
    r = subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.split()
    sizes, offs = [int(x) for x in out[:3]], [int(x) for x in out[3:]]
    assert sizes == [ctypes.sizeof(_lib.WitnessBatch), ctypes.sizeof(_lib.WitnessPlanReport), ctypes.sizeof(_lib.WitnessReport)]
    assert sizes[0] == 120 and sizes[1] == 56
    assert offs[:len(BATCH_FIELDS)] == [getattr(_lib.WitnessBatch, f).offset for f in BATCH_FIELDS]
    assert offs[len(BATCH_FIELDS):] == [getattr(_lib.WitnessPlanReport, f).offset for f in REPORT_FIELDS]
    assert [f for f, _ in _lib.WitnessBatch._fields_] == BATCH_FIELDS


def test_library_and_mirrors_name_the_calls():
    import inspect
    import zkt_plonk_amd as z
    from zkt_plonk_amd import _lib, witness
    syms = z.declared_symbols()
    L = z.lib()
    for f, n in FUNCS.items():
        assert f in syms
        assert hasattr(L, f), "%s is not exported" % f
        assert len(getattr(L, f).argtypes) == n, f
    assert not any(s.startswith("zkt_circuit_check_witness_batch_") for s in syms)      # no _dev twin: the stream table stays
    for m in ("check_witness_batch", "witness_batch", "witness_plan_create"):
        assert callable(getattr(_lib.Context, m))
    assert inspect.signature(_lib.Context.witness_plan_create).parameters["rules"].default == 0
    assert inspect.signature(_lib.debug_witness_plan_host).parameters["rules"].default == 0
    assert inspect.signature(z.WitnessPlan.__init__).parameters["rules"].default == 0
    assert (_lib.WITNESS_RULE_IS_ZERO, witness.RULE_IS_ZERO, witness.ZINV, witness.ZFLAG) == (1, 1, 4, 5)


def test_null_arguments_are_refused_without_a_device():
    import zkt_plonk_amd as z
    from zkt_plonk_amd import _lib
    L = z.lib()
    assert L.zkt_circuit_check_witness_batch(None, ctypes.byref(_lib.WitnessBatch()), 0, ctypes.byref(_lib.WitnessReport())) != 0
    assert L.zkt_witness_plan_create_ex(None, None, None, None, 0, 0, 0, None, 0, 1, ctypes.byref(ctypes.c_void_p())) != 0
    assert L.zkt_debug_witness_plan_host_ex(0, None, None, 0, 0, None, 0, 0, None, None, None) != 0
