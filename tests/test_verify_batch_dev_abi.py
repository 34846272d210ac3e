"""CPU: the C-ABI of batch verification on the device (zkt_g1_decompress / _dev, zkt_verify_batch_prepare_dev,
zkt_verify_batch_dev) as the header declares it and as the built library exports it."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zkt_plonk.h")
FUNCS = {"zkt_g1_decompress": 5, "zkt_g1_decompress_dev": 5, "zkt_verify_batch_prepare_dev": 9, "zkt_verify_batch_dev": 7}


def _code():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _params(text, name):
    m = re.search(r"\b%s\s*\((.*?)\)\s*;" % re.escape(name), text, flags=re.S)
    assert m, "%s is not declared" % name
    return m.group(1).count(",") + 1


@pytest.mark.parametrize("name", sorted(FUNCS))
def test_header_declares_the_entry_points(name):
    assert _params(_code(), name) == FUNCS[name]


def test_header_defines_the_limits_and_the_status_codes():
    text = _code()
    assert re.search(r"#define\s+ZKT_G1_DECOMPRESS_MAX\s+\(\(size_t\)1\s*<<\s*22\)", text)
    assert re.search(r"#define\s+ZKT_VERIFY_BATCH_DEV_MAX\s+\(ZKT_MSM_BASES_MAX\s*/\s*24\)", text)
    for k, name in enumerate(["VALID", "IDENTITY", "NOT_CANONICAL", "BOTH_FLAGS", "NOT_ON_CURVE", "NOT_IN_SUBGROUP"]):
        assert re.search(r"\bZKT_G1_%s\s*=\s*%d\b" % (name, k), text), name
    from zkt_plonk_amd import _lib
    assert _lib.G1_DECOMPRESS_MAX == 1 << 22
    assert _lib.VERIFY_BATCH_DEV_MAX == _lib.MSM_BASES_MAX // 24 and 24 * _lib.VERIFY_BATCH_DEV_MAX <= _lib.MSM_BASES_MAX
    assert 13 * _lib.VERIFY_BATCH_DEV_MAX <= _lib.G1_DECOMPRESS_MAX     # one decompression launch takes a whole batch


def test_library_exports_the_entry_points():
    import zkt_plonk_amd as z
    syms = z.declared_symbols()
    L = z.lib()
    for f in FUNCS:
        assert f in syms
        assert hasattr(L, f), "%s is not exported" % f


def test_python_binding_has_the_three_methods():
    import zkt_plonk_amd as z
    for m in ("g1_decompress", "g1_decompress_dev", "verify_batch_prepare_dev", "verify_batch_dev"):
        assert callable(getattr(z.Context, m))
