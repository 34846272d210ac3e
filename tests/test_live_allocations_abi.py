"""CPU: zkt_debug_live_allocations as the header declares it, as _lib.py and the Rust shim mirror it and as the built library
exports it.  It needs no context and no device."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zkt_plonk.h")
NAME = "zkt_debug_live_allocations"
INVALID_ARGUMENT = 1                  # ZKT_ERR_INVALID_ARGUMENT (include/zkt_plonk.h)


def test_header_and_shim_declare_the_call():
    code = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % NAME, code, flags=re.S)
    assert m, "%s is not declared" % NAME
    assert [x.strip() for x in m.group(1).split(",")] == ["uint64_t* count", "uint64_t* bytes"]
    assert re.search(r"ZKT_ERR_INVALID_ARGUMENT\s*=\s*%d\b" % INVALID_ARGUMENT, code)
    ffi = open(os.path.join(ROOT, "shim", "src", "ffi.rs")).read()
    m = re.search(r"pub fn %s\((.*?)\)\s*->\s*c_int;" % NAME, ffi, flags=re.S)
    assert m and m.group(1).count("*mut u64") == 2


def test_library_answers_without_a_context():
    import zkt_plonk_amd as z
    from zkt_plonk_amd import _lib
    assert NAME in z.declared_symbols()
    count, nbytes = _lib.debug_live_allocations()
    assert (count == 0) == (nbytes == 0) and nbytes >= 16 * count      # no allocation is shorter than 16 bytes
    assert _lib.debug_live_allocations() == (count, nbytes)            # reading it allocates nothing
    n = ctypes.c_uint64(7)
    assert z.lib().zkt_debug_live_allocations(None, ctypes.byref(n)) == INVALID_ARGUMENT
    assert z.lib().zkt_debug_live_allocations(ctypes.byref(n), None) == INVALID_ARGUMENT and n.value == 7
