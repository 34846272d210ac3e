"""CPU: zkt_ctx_set_fused_passes as the header declares it, as _lib.py and the Rust shim mirror it and as the built library
exports it."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zkt_plonk.h")
NAME = "zkt_ctx_set_fused_passes"


def _code():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_and_documents_the_switch():
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % NAME, _code(), flags=re.S)
    assert m, "%s is not declared" % NAME
    params = [x.strip() for x in m.group(1).split(",")]
    assert len(params) == 2 and params[0].startswith("zkt_ctx*") and params[1].startswith("int")
    code = _code()
    assert code.index("zkt_ctx_set_quotient_route") < code.index(NAME) < code.index("zkt_lagrange_info")
    text = open(HEADER).read()
    doc = text[text.index("Fused streaming passes"):text.index("int %s" % NAME)]
    for said in ("0 = automatic", "1 = fused", "2 = one launch per step", "Forks inherit the mode", "zkt_debug_grand_products",
                 "Sharded contexts"):
        assert said in doc, said


def test_library_and_mirrors_name_the_call():
    import zkt_plonk_amd as z
    from zkt_plonk_amd import _lib
    assert NAME in z.declared_symbols()
    assert hasattr(z.lib(), NAME), "%s is not exported" % NAME
    assert callable(getattr(_lib.Context, NAME[len("zkt_ctx_"):]))
    ffi = open(os.path.join(ROOT, "shim", "src", "ffi.rs")).read()
    m = re.search(r"pub fn %s\((.*?)\)\s*->\s*c_int;" % NAME, ffi, flags=re.S)
    assert m and m.group(1).count(":") == 2
    assert re.search(r"\bint fused_passes\b", open(os.path.join(ROOT, "zkt-plonk_amd", "csrc", "ctx.hpp")).read())
