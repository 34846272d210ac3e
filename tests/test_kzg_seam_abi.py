"""CPU: the KZG commitment seam's C-ABI (zkt_kzg_commit_batch / zkt_kzg_open and their _dev forms) as the header declares
it, as the Rust FFI mirrors it, and as shim/src/kzg.rs calls it from PC::commit / PC::open."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zkt_plonk.h")
FFI = os.path.join(ROOT, "shim", "src", "ffi.rs")
KZG_RS = os.path.join(ROOT, "shim", "src", "kzg.rs")
FUNCS = ["zkt_kzg_commit_batch", "zkt_kzg_commit_batch_dev", "zkt_kzg_open", "zkt_kzg_open_dev"]


def _strip_c_comments(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _params(text, name):
    """parameter count of `name(...)` in a declaration (C or Rust)"""
    m = re.search(r"\b%s\s*\((.*?)\)\s*(?:;|->)" % re.escape(name), text, flags=re.S)
    assert m, "%s is not declared" % name
    body = m.group(1).strip()
    return 0 if body in ("", "void") else body.count(",") + 1


def _rust_fn_body(text, name):
    """the body of `fn name` (brace matched)"""
    m = re.search(r"\bfn\s+%s\b" % re.escape(name), text)
    assert m, "fn %s not found" % name
    i = text.index("{", m.end())
    depth = 0
    for j in range(i, len(text)):
        if text[j] == "{":
            depth += 1
        elif text[j] == "}":
            depth -= 1
            if depth == 0:
                return text[i:j + 1]
    raise AssertionError("unbalanced braces in fn %s" % name)


def test_header_declares_the_seam():
    text = _strip_c_comments(open(HEADER).read())
    m = re.search(r"#define\s+ZKT_KZG_BATCH_MAX\s+(\d+)", text)
    assert m and int(m.group(1)) == 32
    assert _params(text, "zkt_kzg_commit_batch") == 7
    assert _params(text, "zkt_kzg_commit_batch_dev") == 7
    assert _params(text, "zkt_kzg_open") == 9
    assert _params(text, "zkt_kzg_open_dev") == 9


def test_header_still_compiles_as_c99():
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", HEADER],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_python_binding_lists_the_seam():
    import zkt_plonk_amd as z
    syms = z.declared_symbols()
    for f in FUNCS:
        assert f in syms


@pytest.mark.parametrize("name", FUNCS)
def test_rust_ffi_matches_the_header(name):
    header = _strip_c_comments(open(HEADER).read())
    ffi = open(FFI).read()
    assert re.search(r"pub\s+fn\s+%s\s*\(" % name, ffi), "%s missing from shim/src/ffi.rs" % name
    assert _params(ffi, name) == _params(header, name)
    m = re.search(r"pub\s+const\s+ZKT_KZG_BATCH_MAX\s*:\s*usize\s*=\s*(\d+)", ffi)
    assert m and int(m.group(1)) == 32


def test_shim_commit_and_open_use_the_seam():
    text = open(KZG_RS).read()
    commit = _rust_fn_body(text, "commit")
    opening = _rust_fn_body(text, "open_individual_opening_challenges")
    helper = _rust_fn_body(text, "commit_batch")
    # commit goes through the batch helper, which makes the one zkt_kzg_commit_batch call
    assert "commit_batch(" in commit and "zkt_kzg_commit_batch(" in helper
    assert "zkt_msm_g1" not in commit and "zkt_msm_g1" not in helper
    assert "degree_bound().is_none()" in commit and "hiding_bound().is_none()" in commit
    assert "zkt_kzg_open(" in opening and "zkt_msm_g1" not in opening
    assert "commit_one" not in text
