"""CPU: the C-ABI of the store files and of zkt_withdraw_prove as the header declares it, as _lib.py and the Rust shim mirror it
and as the built library exports it; the layout of the new structs as a C compiler sees the header against the ctypes mirrors."""
import ctypes
import importlib.util
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zkt_plonk.h")
FUNCS = {"zkt_withdraw_prove": 10, "zkt_merkle_tree_save_file": 3, "zkt_merkle_tree_load_file": 7, "zkt_notes_read_file": 8,
         "zkt_notes_write_file": 7, "zkt_debug_store_chunk": 2}
STRUCTS = {"zkt_withdraw_prove_args": ("WithdrawProveArgs", "ZktWithdrawProveArgs"), "zkt_withdraw_result": ("WithdrawResult", "ZktWithdrawResult"),
           "zkt_tree_file_report": ("TreeFileReport", "ZktTreeFileReport")}


def _code():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _header_fields(name):
    """The field names of `typedef struct { ... } name;` in declaration order."""
    m = re.search(r"typedef struct \{([^}]*)\}\s*%s;" % name, _code())
    assert m, name
    out = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if decl:
            head, *more = decl.split(",")
            out += [re.search(r"(\w+)\s*$", head).group(1)] + [re.search(r"(\w+)\s*$", x).group(1) for x in more]
    return out


@pytest.mark.parametrize("name", sorted(FUNCS))
def test_header_library_and_mirrors_name_the_calls(name):
    import zkt_plonk_amd as z
    m = re.search(r"\b%s\s*\((.*?)\)\s*;" % re.escape(name), _code(), flags=re.S)
    assert m, "%s is not declared" % name
    assert len(m.group(1).split(",")) == FUNCS[name]
    assert name in z.declared_symbols() and hasattr(z.lib(), name), "%s is not exported" % name
    ffi = open(os.path.join(ROOT, "shim", "src", "ffi.rs")).read()
    f = re.search(r"pub fn %s\((.*?)\)" % name, ffi, flags=re.S)
    assert f and f.group(1).count(":") == FUNCS[name], name
    src = open(os.path.join(ROOT, "zkt-plonk_amd", "_lib.py")).read()
    assert "L.%s(" % name in src, "_lib.py does not call %s" % name


def test_python_wrappers_exist():
    import zkt_plonk_amd as z
    from zkt_plonk_amd import _lib
    for m in ("withdraw_prove", "merkle_tree_save_file", "merkle_tree_load_file", "debug_store_chunk"):
        assert callable(getattr(_lib.Context, m))
    assert callable(_lib.notes_read_file) and callable(_lib.notes_write_file)
    assert callable(z.WithdrawCircuit.prove) and callable(z.MerkleTree.save_file) and callable(z.MerkleTree.load_file)


@pytest.mark.parametrize("name", sorted(STRUCTS))
def test_field_order_in_header_ctypes_and_shim(name):
    from zkt_plonk_amd import _lib
    fields = _header_fields(name)
    assert [f[0] for f in getattr(_lib, STRUCTS[name][0])._fields_] == fields
    ffi = open(os.path.join(ROOT, "shim", "src", "ffi.rs")).read()
    m = re.search(r"#\[repr\(C\)\]\s*pub struct %s \{(.*?)\}" % STRUCTS[name][1], ffi, flags=re.S)
    assert m and re.findall(r"pub (\w+):", m.group(1)) == fields


def test_struct_layout_as_a_c_compiler_sees_the_header(tmp_path):
    from zkt_plonk_amd import _lib
    spec = importlib.util.spec_from_file_location("zkt_build", os.path.join(ROOT, "zkt-plonk_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "%s"' % HEADER, "int main(void) {"]
    for name in sorted(STRUCTS):
        lines.append('printf("%s %%zu", sizeof(%s));' % (name, name))
        lines += ['printf(" %%zu", offsetof(%s, %s));' % (name, f) for f in _header_fields(name)]
        lines.append('printf("\\n");')
    lines += ["return 0; }"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    r = subprocess.run([b.CLANG.replace("clang++", "clang"), "-x", "c", "-std=c11", "-Wall", str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60).stdout.splitlines()
    for line, name in zip(out, sorted(STRUCTS)):
        mirror = getattr(_lib, STRUCTS[name][0])
        want = [name, str(ctypes.sizeof(mirror))] + [str(getattr(mirror, f[0]).offset) for f in mirror._fields_]
        assert line.split() == want, name
    assert (ctypes.sizeof(_lib.WithdrawResult), ctypes.sizeof(_lib.TreeFileReport)) == (24, 40)
