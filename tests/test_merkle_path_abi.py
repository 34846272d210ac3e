"""CPU: the C-ABI of the Merkle-path witness (zkt_merkle_path_vars_per_level, zkt_poseidon_merkle_path_witness_dev,
zkt_poseidon_merkle_path_validate, zkt_merkle_path_args) as the header declares it, as _lib.py and the Rust shim mirror it
and as the built library exports it."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zkt_plonk.h")
FUNCS = {"zkt_merkle_path_vars_per_level": 1, "zkt_poseidon_merkle_path_witness_dev": 3, "zkt_poseidon_merkle_path_validate": 3}
FIELDS = ["batch", "height", "d_variables", "n_vars", "d_leaf_var", "d_bit_vars", "d_sibling_vars", "d_path_base", "path_base0",
          "d_out_roots"]


def _code():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


@pytest.mark.parametrize("name", sorted(FUNCS))
def test_header_declares_the_entry_points(name):
    m = re.search(r"\b%s\s*\((.*?)\)\s*;" % re.escape(name), _code(), flags=re.S)
    assert m, "%s is not declared" % name
    assert m.group(1).count(",") + 1 == FUNCS[name]
    if FUNCS[name] == 3:
        params = [x.strip() for x in m.group(1).split(",")]
        assert params[0].startswith("zkt_ctx*") and "const zkt_poseidon*" in params[1] and "const zkt_merkle_path_args*" in params[2]


def test_header_declares_the_struct_next_to_the_gadget_entries():
    code = _code()
    body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*zkt_merkle_path_args\s*;", code).group(1)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    assert [re.match(r".*?(\w+)$", d).group(1) for d in decls] == FIELDS
    types = dict(zip(FIELDS, [re.match(r"(.*?)\s*\w+$", d).group(1).replace(" ", "") for d in decls]))
    assert types["batch"] == types["n_vars"] == types["path_base0"] == "size_t" and types["height"] == "int"
    assert types["d_variables"] == types["d_out_roots"] == "void*"
    assert all(types[f] == "constuint32_t*" for f in ("d_leaf_var", "d_bit_vars", "d_sibling_vars", "d_path_base"))
    assert code.index("zkt_poseidon_gadget_validate") < code.index("zkt_merkle_path_args") < code.index("zkt_verify_prepare")
    text = open(HEADER).read()
    doc = text[text.index("merkle_proof"):text.index("} zkt_merkle_path_args;")]
    assert "coeff 1, offset 0" in doc and "may not be a variable the same launch writes" in doc


def test_ctypes_mirror_has_the_c_layout(tmp_path):
    from zkt_plonk_amd import _lib
    assert [f[0] for f in _lib.MerklePathArgs._fields_] == FIELDS
    offsets = ", ".join("(unsigned long)offsetof(zkt_merkle_path_args, %s)" % f for f in FIELDS)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "zkt_plonk.h"\n'
                   'int main(void) { unsigned long v[] = {(unsigned long)sizeof(zkt_merkle_path_args), %s}; '
                   'for (unsigned i = 0; i < sizeof v / sizeof v[0]; ++i) printf("%%lu\\n", v[i]); return 0; }\n' % offsets)
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert ctypes.sizeof(_lib.MerklePathArgs) == got[0]
    assert [getattr(_lib.MerklePathArgs, f).offset for f in FIELDS] == got[1:]
    assert [getattr(_lib.MerklePathArgs, f).size for f in FIELDS] == [8, 4, 8, 8, 8, 8, 8, 8, 8, 8]


def test_library_and_mirrors_name_the_calls():
    import zkt_plonk_amd as z
    from zkt_plonk_amd import _lib
    syms = z.declared_symbols()
    L = z.lib()
    for f in FUNCS:
        assert f in syms
        assert hasattr(L, f), "%s is not exported" % f
    for m in ("merkle_path_vars_per_level", "poseidon_merkle_path_witness_dev"):
        assert callable(getattr(_lib.Context, m))
    assert callable(z.PoseidonGadget.merkle_path)
    ffi = open(os.path.join(ROOT, "shim", "src", "ffi.rs")).read()
    for f in FUNCS:
        assert re.search(r"pub fn %s\(" % f, ffi), f
    rust = re.search(r"pub struct ZktMerklePathArgs \{(.*?)\}", ffi, flags=re.S).group(1)
    assert re.findall(r"pub (\w+):", rust) == FIELDS
