"""CPU: the C-ABI of zkt_verify_batch_locate and its two test hooks as the header declares it, as the built library
exports it and as the Python binding offers it."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zkt_plonk.h")
FUNCS = {"zkt_verify_batch_locate": 10, "zkt_debug_verify_batch_tree": 9, "zkt_debug_verify_locate_host": 13}


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


def test_python_binding_has_the_methods():
    import zkt_plonk_amd as z
    from zkt_plonk_amd import _lib
    for m in ("verify_batch_locate", "debug_verify_batch_tree"):
        assert callable(getattr(z.Context, m))
    assert callable(_lib.debug_verify_locate_host)
    assert _lib.verify_tree_levels(1) == [1] and _lib.verify_tree_levels(5) == [5, 3, 2, 1]
    assert _lib.verify_tree_levels(67) == [67, 34, 17, 9, 5, 3, 2, 1]


def test_header_points_to_the_call_where_a_rejected_batch_is_mentioned():
    text = open(HEADER).read()
    assert "UNMEASURED" not in text
    said = [m.end() for m in re.finditer(r"does\s+not\s+say\s+which\s+proof\s+failed", text)]
    assert len(said) == 2                                        # zkt_verify_batch and zkt_verify_batch_dev
    for at in said:
        assert "zkt_verify_batch_locate" in text[at:at + 80]
