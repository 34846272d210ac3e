"""CPU: the C-ABI of the withdraw circuit as a component (zkt_withdraw_*, zkt_debug_withdraw_layout_host, zkt_note_leaves) as
the header declares it, as _lib.py, withdraw.py and the Rust shim mirror it and as the built library exports it."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zkt_plonk.h")
FUNCS = {"zkt_withdraw_create": 5, "zkt_withdraw_free": 2, "zkt_withdraw_poseidon": 1, "zkt_withdraw_get_info": 2, "zkt_withdraw_pi_pos": 2,
         "zkt_withdraw_rows": 4, "zkt_debug_withdraw_layout_host": 9, "zkt_withdraw_setup": 6, "zkt_withdraw_witness": 9,
         "zkt_withdraw_prove_inputs": 7, "zkt_note_leaves": 7}
WRAPPERS = {"zkt_withdraw_create": "withdraw_create", "zkt_withdraw_free": "withdraw_free", "zkt_withdraw_poseidon": "withdraw_poseidon",
            "zkt_withdraw_get_info": "withdraw_get_info", "zkt_withdraw_pi_pos": "withdraw_pi_pos", "zkt_withdraw_rows": "withdraw_rows",
            "zkt_withdraw_setup": "withdraw_setup", "zkt_withdraw_witness": "withdraw_witness", "zkt_withdraw_prove_inputs": "withdraw_prepare",
            "zkt_note_leaves": "note_leaves"}


def _code():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


@pytest.mark.parametrize("name", sorted(FUNCS))
def test_header_declares_the_entry_points(name):
    m = re.search(r"\b%s\s*\((.*?)\)\s*;" % re.escape(name), _code(), flags=re.S)
    assert m, "%s is not declared" % name
    params = [x.strip() for x in m.group(1).split(",")]
    assert len(params) == FUNCS[name]
    if name in ("zkt_withdraw_create", "zkt_withdraw_free", "zkt_withdraw_rows", "zkt_withdraw_setup", "zkt_withdraw_witness", "zkt_note_leaves"):
        assert params[0].startswith("zkt_ctx*")
    if name == "zkt_withdraw_create":
        assert "const zkt_poseidon_params*" in params[1] and params[4].startswith("zkt_withdraw**")
    if name == "zkt_withdraw_witness":
        assert "const zkt_withdraw_request*" in params[2] and "zkt_merkle_tree*" in params[4] and "zkt_withdraw_status*" in params[8]


def test_header_places_and_documents_the_circuit():
    code = _code()
    assert code.index("zkt_merkle_tree_paths_to_variables_dev") < code.index("zkt_withdraw_create") < code.index("zkt_verify_prepare")
    text = open(HEADER).read()
    doc = text[text.index("(5) The withdraw circuit"):text.index("zkt_verify_prepare")]
    for cited in ("withdraw.rs:57-150", "main.rs:90-112", "main.rs:190-300", "main.rs:266-271", "withdraw.rs:59", "main.rs:257", "main.rs:160-163"):
        assert cited in doc, cited
    for said in ("ZKT_ERR_ZERO_DENOMINATOR", "ZKT_WITNESS_BATCH_MAX", "a second call waits", "no synchronisation", "Synchronises the stream"):
        assert said in doc, said
    prof = text[text.index("Timing with HIP events"):text.index("int zkt_profile_enable")]
    assert '"withdraw_layout"' in prof and '"withdraw_witness"' in prof


def test_structs_have_the_headers_layout():
    from zkt_plonk_amd import _lib
    code = _code()
    for cname, mirror in (("zkt_withdraw_info", _lib.WithdrawInfo), ("zkt_withdraw_request", _lib.WithdrawRequest)):
        m = re.search(r"typedef struct \{([^{}]*)\}\s*%s\s*;" % cname, code)
        assert m, cname
        fields = []
        for decl in m.group(1).split(";"):
            decl = decl.strip()
            if decl:
                fields += [f.strip().lstrip("*").strip() for f in re.sub(r"^(const\s+)?\w+\s*\*?", "", decl, count=1).split(",")]
        assert fields == [k for k, _ in mirror._fields_], cname
    assert ctypes.sizeof(_lib.WithdrawInfo) == 4 * 4 + 6 * ctypes.sizeof(ctypes.c_size_t)
    assert ctypes.sizeof(_lib.WithdrawRequest) == 9 * 8


def test_library_and_mirrors_name_the_calls():
    import zkt_plonk_amd as z
    from zkt_plonk_amd import _lib
    syms = z.declared_symbols()
    L = z.lib()
    for f in FUNCS:
        assert f in syms
        assert hasattr(L, f), "%s is not exported" % f
    for f, wname in WRAPPERS.items():
        assert callable(getattr(_lib.Context, wname)), wname
    assert callable(_lib.debug_withdraw_layout_host)
    for m in ("rows", "setup", "witness", "prepare", "close"):
        assert callable(getattr(z.WithdrawCircuit, m))
    assert "WithdrawCircuit" in z.__all__
    ffi = open(os.path.join(ROOT, "shim", "src", "ffi.rs")).read()
    for f, n in FUNCS.items():
        m = re.search(r"pub fn %s\((.*?)\)" % f, ffi, flags=re.S)
        assert m, f
        assert m.group(1).count(":") == n, f
