"""CPU: the C-ABI of the note tree (zkt_merkle_tree_*, zkt_debug_merkle_tree_split) as the header declares it, as _lib.py,
merkle.py and the Rust shim mirror it and as the built library exports it."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zkt_plonk.h")
FUNCS = {"zkt_merkle_tree_create": 5, "zkt_merkle_tree_free": 2, "zkt_merkle_tree_append_dev": 5, "zkt_merkle_tree_append": 5,
         "zkt_merkle_tree_root": 3, "zkt_merkle_tree_info": 4, "zkt_merkle_tree_layer": 6, "zkt_merkle_tree_paths": 5,
         "zkt_merkle_tree_paths_to_variables_dev": 8, "zkt_debug_merkle_tree_split": 2}


def _code():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


@pytest.mark.parametrize("name", sorted(FUNCS))
def test_header_declares_the_entry_points(name):
    m = re.search(r"\b%s\s*\((.*?)\)\s*;" % re.escape(name), _code(), flags=re.S)
    assert m, "%s is not declared" % name
    params = [x.strip() for x in m.group(1).split(",")]
    assert len(params) == FUNCS[name]
    if name not in ("zkt_merkle_tree_info", "zkt_debug_merkle_tree_split"):
        assert params[0].startswith("zkt_ctx*")
    if name == "zkt_merkle_tree_create":
        assert "const zkt_poseidon*" in params[1] and params[4].startswith("zkt_merkle_tree**")
    else:
        assert "zkt_merkle_tree*" in params[0 if name in ("zkt_merkle_tree_info", "zkt_debug_merkle_tree_split") else 1]


def test_header_places_and_documents_the_tree():
    code = _code()
    assert code.index("zkt_poseidon_merkle_path_validate") < code.index("zkt_merkle_tree_create") < code.index("zkt_verify_prepare")
    assert code.index("zkt_debug_ntt_split") < code.index("zkt_debug_merkle_tree_split")
    assert re.search(r"#define\s+ZKT_MERKLE_TREE_MAX\s+\(\(size_t\)1 << 24\)", code)
    assert re.search(r"#define\s+ZKT_MERKLE_TREE_PATHS_MAX\s+4096\b", code)
    text = open(HEADER).read()
    doc = text[text.index("(4) The note tree"):text.index("zkt_verify_prepare")]
    for cited in ("merkle_tree.rs:57-75", "merkle_tree.rs:89-106", "merkle_tree.rs:77-87", "merkle_tree.rs:108-110", "binary.rs:42-78"):
        assert cited in doc, cited
    for scope in ("MerkleTreeStore file", "deleting or updating leaves", "sharded over ranks"):
        assert scope in doc, scope
    prof = text[text.index("Timing with HIP events"):text.index("int zkt_profile_enable")]
    assert '"merkle_append"' in prof and '"merkle_paths"' in prof


def test_library_and_mirrors_name_the_calls():
    import zkt_plonk_amd as z
    from zkt_plonk_amd import _lib
    syms = z.declared_symbols()
    L = z.lib()
    for f in FUNCS:
        assert f in syms
        assert hasattr(L, f), "%s is not exported" % f
        assert callable(getattr(_lib.Context, f[len("zkt_"):]))
    for m in ("append", "root", "paths", "paths_to_variables", "layer", "close"):
        assert callable(getattr(z.MerkleTree, m))
    assert "MerkleTree" in z.__all__
    ffi = open(os.path.join(ROOT, "shim", "src", "ffi.rs")).read()
    for f, n in FUNCS.items():
        m = re.search(r"pub fn %s\((.*?)\)" % f, ffi, flags=re.S)
        assert m, f
        assert m.group(1).count(":") == n, f
