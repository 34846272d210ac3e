"""CPU: zkt_g1_check's per-point rules run on the host (zkt_debug_g1_check_host, the text the kernel compiles) against
oracle.curve, the host's end of zkt_srs_check's structure test (zkt_debug_srs_check_finish_host) on keys of
oracle.curve.srs_powers, and the C-ABI of both calls as the header declares it, the library exports it and the Python
binding mirrors it."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import coracle as K, curve as C

import srs_check_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zkt_plonk.h")
FUNCS = {"zkt_g1_check": 5, "zkt_debug_g1_check_host": 4, "zkt_srs_check": 9, "zkt_debug_srs_check_chunk": 2,
         "zkt_debug_srs_check_finish_host": 10}
FIELDS = ["count", "n_bad", "first_bad", "by_status", "first_bad_status", "points_ok", "structure_checked", "structure_ok", "ok",
          "sum_xy_mont", "sum_is_infinity"]
IDS = lambda v: getattr(v, "name", str(v))


# ---- symbols and layout -------------------------------------------------------------------------------------------------
def _code():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


@pytest.mark.parametrize("name", sorted(FUNCS))
def test_header_declares_the_entry_points(name):
    m = re.search(r"\b%s\s*\((.*?)\)\s*;" % re.escape(name), _code(), flags=re.S)
    assert m, "%s is not declared" % name
    assert m.group(1).count(",") + 1 == FUNCS[name]
    assert not name.endswith("_dev")


def test_library_exports_the_entry_points_and_the_binding_has_them():
    import zkt_plonk_amd as z
    from zkt_plonk_amd import _lib
    syms, L = z.declared_symbols(), z.lib()
    for f in FUNCS:
        assert f in syms
        assert hasattr(L, f), "%s is not exported" % f
        assert len(getattr(L, f).argtypes) == FUNCS[f]
    for m in ("g1_check", "srs_check", "debug_srs_check_chunk"):
        assert callable(getattr(z.Context, m))
    assert callable(_lib.debug_g1_check_host) and callable(_lib.debug_srs_check_finish_host)
    assert re.search(r"#define\s+ZKT_SRS_CHECK_MAX\s+\(\(\(size_t\)1\s*<<\s*24\)\s*\+\s*1\)", open(HEADER).read())
    assert _lib.SRS_CHECK_MAX == (1 << 24) + 1


def test_ctypes_mirror_has_the_c_layout(tmp_path):
    from zkt_plonk_amd import _lib
    assert [f[0] for f in _lib.SrsReport._fields_] == FIELDS
    offsets = ", ".join("(unsigned long)offsetof(zkt_srs_report, %s)" % f for f in FIELDS)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "zkt_plonk.h"\n'
                   'int main(void) { unsigned long v[] = {(unsigned long)sizeof(zkt_srs_report), %s}; '
                   'for (unsigned i = 0; i < sizeof v / sizeof v[0]; ++i) printf("%%lu\\n", v[i]); return 0; }\n' % offsets)
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert ctypes.sizeof(_lib.SrsReport) == got[0]
    assert [getattr(_lib.SrsReport, f).offset for f in FIELDS] == got[1:]


def _governing(symbol):
    """The words of the block comment that begins a line in front of the declaration of `symbol`."""
    text = open(HEADER).read()
    comments = [(m.start(), m.end(), m.group(0)) for m in re.finditer(r"^/\*.*?\*/", text, flags=re.S | re.M)]
    stripped = re.sub(r"/\*.*?\*/", lambda m: " " * len(m.group(0)), text, flags=re.S)
    at = re.search(r"\b%s\s*\(" % re.escape(symbol), stripped).start()
    body = [c for c in comments if c[1] <= at][-1][2][2:-2]
    return " ".join(re.sub(r"^\s*\*\s?", "", line).strip() for line in body.splitlines())


@pytest.mark.parametrize("name", ["zkt_g1_check", "zkt_srs_check"])
def test_the_governing_comment_says_that_the_call_synchronises(name):
    own = _governing(name)
    assert "Synchronises the stream" in own
    assert name in own
    if name == "zkt_srs_check":
        assert "count / r" in own                      # the soundness bound


# ---- the per-point rules ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cv", SC.CURVES, ids=IDS)
def test_g1_check_host_gives_every_point_the_oracles_status(cv):
    """260 points (i + 1) G and their negations, every bad point in turn at index 0, 63, 64, 65, ... and the last one."""
    from zkt_plonk_amd import _lib
    g, b = SC.good(cv), SC.bad(cv)
    n = len(g)
    assert n == 260 and {0, 63, 64, 65, n - 1} <= set(SC.spots(n))
    got = _lib.debug_g1_check_host(cv.name, SC.rows(cv, g))
    assert got.tolist() == [SC.VALID] * n                                   # every multiple of G passes
    assert all(SC.oracle_status(cv, *xy) == SC.VALID for xy in g)
    for name, xy, st in b:                                                  # each on its own
        assert _lib.debug_g1_check_host(cv.name, SC.rows(cv, [xy])).tolist() == [st], name
    assert sorted({st for _, _, st in b}) == ([1, 2, 4, 5] if cv.name == "bls12_381" else [1, 2, 4])
    for rot in range(len(b)):                                               # every bad point at every spot
        pts, want = SC.scattered(cv, n, rot)
        got = _lib.debug_g1_check_host(cv.name, pts)
        assert np.array_equal(got, want), (rot, np.nonzero(got != want)[0][:8])
    assert _lib.debug_g1_check_host(cv.name, SC.rows(cv, [])).shape == (0,)
    assert _lib.lib().zkt_debug_g1_check_host(7, None, 0, None) == 1         # no such curve


# ---- the host's end of the structure test -------------------------------------------------------------------------------
def _finish(cv, pts_mont, rho, h, bh, S=None):
    from zkt_plonk_amd import _lib
    if S is None:
        pts = K.points_from_mont(cv, pts_mont)
        S = C.msm_naive(cv, pts, [pow(rho, i, cv.fr.p) for i in range(len(pts))])
    Sm = K.points_to_mont(cv, [S])[0]
    return _lib.debug_srs_check_finish_host(cv.name, Sm, S is None, pts_mont[0], pts_mont[-1], pts_mont.shape[0], rho, h, bh)


@pytest.mark.parametrize("count", [1, 2, 3, 40])
@pytest.mark.parametrize("cv", SC.CURVES, ids=IDS)
def test_finish_host_accepts_the_true_key_and_nothing_else(cv, count):
    from zkt_plonk_amd import _lib
    key = SC.key(cv, SC.TAU, 40)[:count]
    assert np.array_equal(key, K.points_to_mont(cv, C.srs_powers(cv, SC.TAU, count)))
    h, bh = _lib.srs_generate_g2(cv.name, SC.TAU)
    _, bh1 = _lib.srs_generate_g2(cv.name, SC.TAU + 1)
    rho = SC.rho_of(cv, SC.SEED_A)
    assert _finish(cv, key, rho, h, bh)
    assert _finish(cv, key, 1, h, bh)                                       # rho = 1: the plain sums
    assert _finish(cv, key, SC.rho_of(cv, SC.SEED_B), h, bh)
    if count == 1:                                                          # one power relates to nothing
        assert _finish(cv, key, rho, h, bh1)
        return
    assert not _finish(cv, key, rho, h, bh1)                                # beta_h of tau + 1
    for k in sorted({0, 1, count // 2, count - 1}):
        assert not _finish(cv, SC.double_point(cv, key, k), rho, h, bh), k   # 2 P_k, S recomputed
    swapped = key.copy()
    swapped[[0, count - 1]] = key[[count - 1, 0]]
    assert not _finish(cv, swapped, rho, h, bh)
    if count > 3:
        swapped = key.copy()
        swapped[[17, 18]] = key[[18, 17]]
        assert not _finish(cv, swapped, rho, h, bh)
    pts = K.points_from_mont(cv, key)
    S = C.msm_naive(cv, pts, [pow(rho, i, cv.fr.p) for i in range(count)])
    assert not _finish(cv, key, rho, h, bh, S=C.add(cv, S, C.generator(cv)))   # S off by G


def test_finish_host_refuses_what_it_cannot_use():
    from zkt_plonk_amd import _lib
    cv = SC.CURVES[0]
    key = SC.key(cv, SC.TAU, 40)[:3]
    h, bh = _lib.srs_generate_g2(cv.name, SC.TAU)
    with pytest.raises(_lib.ZktError):
        _finish(cv, key, 0, h, bh, S=C.generator(cv))                       # rho = 0
    ok, r4 = ctypes.c_int(0), np.array([5, 0, 0, 0], dtype=np.uint64)
    p = _lib.u64p
    args = (p(key[0].copy()), 0, p(key[0].copy()), p(key[2].copy()), 3, p(r4), p(h), p(bh), ctypes.byref(ok))
    assert _lib.lib().zkt_debug_srs_check_finish_host(7, *args) == 1        # no such curve
    assert _lib.lib().zkt_debug_srs_check_finish_host(0, *args[:4], 0, *args[5:]) == 1   # count = 0
