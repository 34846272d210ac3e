"""CPU: the C-ABI of the witness completion (zkt_witness_plan_*, zkt_witness_complete*, the two debug hooks) as the header
declares it, as _lib.py and witness.py mirror it and as the built library exports it."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zkt_plonk.h")
FUNCS = {"zkt_witness_plan_create": 10, "zkt_witness_plan_free": 2, "zkt_witness_plan_info": 2, "zkt_witness_plan_kinds": 2,
         "zkt_witness_complete_enqueue": 6, "zkt_witness_complete_status": 4, "zkt_witness_complete": 7,
         "zkt_debug_witness_plan_host": 10, "zkt_debug_witness_plan_split": 2}


def _code():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


@pytest.mark.parametrize("name", sorted(FUNCS))
def test_header_declares_the_entry_points(name):
    m = re.search(r"\b%s\s*\((.*?)\)\s*;" % re.escape(name), _code(), flags=re.S)
    assert m, "%s is not declared" % name
    params = [x.strip() for x in m.group(1).split(",")]
    assert len(params) == FUNCS[name]
    if name.startswith("zkt_witness_complete") or name in ("zkt_witness_plan_create", "zkt_witness_plan_free"):
        assert params[0].startswith("zkt_ctx*")
    if name == "zkt_witness_plan_create":
        assert params[-1].startswith("zkt_witness_plan**")
    elif name != "zkt_debug_witness_plan_host":
        assert any("zkt_witness_plan*" in p for p in params[:2])


def test_header_states_the_rule_and_the_limits():
    code = _code()
    assert code.index("zkt_circuit_check_witness") < code.index("zkt_witness_plan_create") < code.index("zkt_poseidon_hash_batch")
    assert code.index("zkt_debug_wire_elimination") < code.index("zkt_debug_witness_plan_host")
    assert re.search(r"#define\s+ZKT_WITNESS_BATCH_MAX\s+256\b", code)
    text = open(HEADER).read()
    doc = text[text.index("Witness completion from the circuit's free variables"):text.index("int zkt_witness_plan_create")]
    for said in ("Rule O", "Rule R", "public-input row", "no left-wire rule", "arithmetic.rs:104-130", "unseen", "(q_m a + q_r)",
                 "read only by the workgroup that wrote it", "docs/EXPERIMENTS.md"):
        assert said in doc, said
    m = re.search(r"typedef struct \{(.*?)\} zkt_witness_plan_report;", code, flags=re.S)
    for field in ("n_free", "n_out", "n_right", "n_unused", "depth", "max_level_rows", "launches", "device_bytes"):
        assert re.search(r"\b%s;" % field, m.group(1)), field


def test_library_and_mirrors_name_the_calls():
    import zkt_plonk_amd as z
    from zkt_plonk_amd import _lib
    syms = z.declared_symbols()
    L = z.lib()
    for f, n in FUNCS.items():
        assert f in syms
        assert hasattr(L, f), "%s is not exported" % f
        assert len(getattr(L, f).argtypes) == n, f
    for m in ("witness_plan_create", "witness_plan_free", "witness_plan_info", "witness_plan_kinds", "witness_complete_enqueue",
              "witness_complete_status", "witness_complete", "debug_witness_plan_split"):
        assert callable(getattr(_lib.Context, m))
    assert callable(_lib.debug_witness_plan_host)
    for m in ("complete_dev", "complete", "status", "info", "kinds", "split", "close"):
        assert callable(getattr(z.WitnessPlan, m))
    assert "WitnessPlan" in z.__all__
    assert _lib.WITNESS_BATCH_MAX == 256
    assert ctypes.sizeof(_lib.WitnessPlanReport) == 56 and ctypes.sizeof(_lib.WitnessStatus) == 16


def test_null_handles_are_refused_without_a_device():
    import zkt_plonk_amd as z
    from zkt_plonk_amd import _lib
    L = z.lib()
    assert L.zkt_witness_plan_info(None, ctypes.byref(_lib.WitnessPlanReport())) != 0
    assert L.zkt_witness_plan_kinds(None, None) != 0
    assert L.zkt_debug_witness_plan_split(None, 4) != 0
    assert L.zkt_witness_plan_free(None, None) is None
