"""CPU: the C-ABI of the batch verifier's term stage on the device -- the switch zkt_ctx_set_verify_terms and the test
hooks -- as the header declares it, as the built library exports it, as the Python binding and the Rust shim offer it."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zkt_plonk.h")
FUNCS = {"zkt_ctx_set_verify_terms": 2, "zkt_debug_verify_terms": 11, "zkt_debug_verify_terms_host": 11,
         "zkt_debug_verify_terms_transcript": 6}


def _code():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


@pytest.mark.parametrize("name", sorted(FUNCS))
def test_header_declares_the_entry_points(name):
    m = re.search(r"\b%s\s*\((.*?)\)\s*;" % re.escape(name), _code(), flags=re.S)
    assert m, "%s is not declared" % name
    assert m.group(1).count(",") + 1 == FUNCS[name]


def test_library_exports_the_entry_points():
    import zkt_plonk_amd as z
    syms = z.declared_symbols()
    L = z.lib()
    for f in FUNCS:
        assert f in syms
        assert hasattr(L, f), "%s is not exported" % f
        assert not f.endswith("_dev")            # host arguments: no row in the stream contract table is owed


def test_python_binding_and_shim_have_them():
    import zkt_plonk_amd as z
    from zkt_plonk_amd import _lib
    for m in ("set_verify_terms", "debug_verify_terms"):
        assert callable(getattr(z.Context, m))
    assert callable(_lib.debug_verify_terms_host) and callable(_lib.debug_verify_terms_transcript)
    ffi = open(os.path.join(ROOT, "shim", "src", "ffi.rs")).read()
    assert re.search(r"pub\s+fn\s+zkt_ctx_set_verify_terms\s*\(\s*ctx:\s*\*mut\s+ZktCtx,\s*mode:\s*c_int\s*\)\s*->\s*c_int", ffi)


def test_the_switch_refuses_every_mode_but_0_and_1():
    """a null context is refused whatever the mode; with a device, a context takes 0 and 1 and refuses the rest (the GPU
    suite repeats that in tests/test_gpu_verify_terms.py)"""
    import ctypes
    import zkt_plonk_amd as z
    L = z.lib()
    L.zkt_ctx_set_verify_terms.argtypes = [ctypes.c_void_p, ctypes.c_int]
    for mode in (0, 1, 2):
        assert L.zkt_ctx_set_verify_terms(None, mode) == 1                      # ZKT_ERR_INVALID_ARGUMENT
    import torch
    if torch.cuda.is_available():
        c = z.Context("bn254", 0)
        c.set_verify_terms(1)
        c.set_verify_terms(0)
        with pytest.raises(z.ZktError) as e:
            c.set_verify_terms(2)
        assert e.value.code == 1
        with pytest.raises(z.ZktError):
            c.set_verify_terms(-1)
        c.close()


def test_header_keeps_what_other_tests_quote():
    text = open(HEADER).read()
    assert "UNMEASURED" not in text
    assert len(re.findall(r"does\s+not\s+say\s+which\s+proof\s+failed", text)) == 2
    assert "On an error NO state is written back" in text
