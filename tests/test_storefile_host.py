"""CPU: the host side of the store files (csrc/storefile.hpp).  The notes file through zkt_notes_write_file / _read_file against
the Python restatement (tests/store_cases.py), and the same header once more as a stand-alone program
(tests/storefile_host_main.cpp) built with AddressSanitizer + UndefinedBehaviorSanitizer and run as a child process: it writes
and reads notes files, writes a tree file, and runs the chunked reader of the tree file over every malformed case of the table.
"Parity unpinned": the reference holds no such file."""
import importlib.util
import os
import subprocess

import numpy as np
import pytest

from oracle import fields as F, coracle as K
from zkt_plonk_amd import _lib

import merkle_tree_cases as MTC
import store_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = {"bn254": F.BN254, "bls12_381": F.BLS12_381}
U64 = (1 << 64) - 1


def _notes(cv):
    p = cv.fr.p
    return [(0, 5, 100, 7), (3, p - 1, U64, 1), (U64, 0, 0, p - 2), (9, 0x1234567890ABCDEF << 100, 1 << 63, (p >> 1) + 3)]


def _mont(cv, vals):
    return K.fr_to_mont(cv, list(vals)) if len(vals) else np.zeros((0, 4), dtype=np.uint64)


@pytest.mark.parametrize("cvname", sorted(CURVES))
def test_notes_file_bytes_and_round_trip(cvname, tmp_path):
    cv = CURVES[cvname]
    path = str(tmp_path / "notes.bin")
    for notes in (_notes(cv), []):
        _lib.notes_write_file(path, cvname, [n[0] for n in notes], _mont(cv, [n[1] for n in notes]), [n[2] for n in notes],
                              _mont(cv, [n[3] for n in notes]))
        assert open(path, "rb").read() == SC.notes_bytes(notes)
        li, idn, am, sec = _lib.notes_read_file(path, cvname)
        assert [int(x) for x in li] == [n[0] for n in notes] and [int(x) for x in am] == [n[2] for n in notes]
        assert (K.fr_from_mont(cv, idn) if notes else []) == [n[1] for n in notes]
        assert (K.fr_from_mont(cv, sec) if notes else []) == [n[3] for n in notes]
        assert np.array_equal(idn, _mont(cv, [n[1] for n in notes]))
        assert _lib.keyfile_last_error() == ""
    assert os.listdir(tmp_path) == ["notes.bin"], "a temporary file stayed"


@pytest.mark.parametrize("cvname", sorted(CURVES))
def test_notes_file_refusals_name_the_path_and_the_offset(cvname, tmp_path):
    cv = CURVES[cvname]
    p = cv.fr.p
    good = SC.notes_bytes(_notes(cv))
    path = str(tmp_path / "n.bin")
    for data in (good[:-1], good[:3], good + b"\0", SC.notes_bytes([(1, p, 2, 3)]), SC.notes_bytes([(1, 2, 3, 4), (1, 2, 2, p + 1)])):
        kind, off, _ = SC.parse_notes(data, p)
        assert kind != SC.ACCEPTED
        open(path, "wb").write(data)
        with pytest.raises(_lib.ZktError) as e:
            _lib.notes_read_file(path, cvname)
        assert e.value.code == 1 and path in str(e.value) and "(offset %d)" % off in str(e.value), str(e.value)
    with pytest.raises(_lib.ZktError) as e:
        _lib.notes_read_file(str(tmp_path / "missing.bin"), cvname)
    assert "missing.bin" in str(e.value)
    # a secret whose limbs equal the modulus is not written, and nothing is left behind
    out = tmp_path / "out"
    out.mkdir()
    limbs = np.array([[(p >> (64 * i)) & U64 for i in range(4)]], dtype=np.uint64)
    with pytest.raises(_lib.ZktError) as e:
        _lib.notes_write_file(str(out / "w.bin"), cvname, [1], _mont(cv, [2]), [3], limbs)
    assert "w.bin" in str(e.value) and os.listdir(out) == []


# ---- the stand-alone sanitizer run ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    spec = importlib.util.spec_from_file_location("zkt_build", os.path.join(ROOT, "zkt-plonk_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    exe = str(tmp_path_factory.mktemp("storefile") / "storefile_host_main")
    # plain C++: the layouts' header includes nothing of HIP
    r = subprocess.run([b.CLANG, "-x", "c++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                        os.path.join(ROOT, "tests", "storefile_host_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def _words(a):
    return " ".join(str(int(x)) for x in np.ascontiguousarray(a, dtype=np.uint64).reshape(-1))


@pytest.mark.parametrize("cvname,height,count", [("bn254", 3, 5), ("bn254", 64, 5), ("bls12_381", 3, 8)])
def test_sanitized_stand_alone_readers_and_writers(cvname, height, count, driver, tmp_path):
    cv = CURVES[cvname]
    p = cv.fr.p
    snap = MTC.build(cvname, 4, height).snaps[count]
    entries = sorted(snap.tree.items())
    table = SC.malformed_tree_files(entries, snap.root, count, p, height, 8)
    notes = _notes(cv)
    bad_notes = [SC.notes_bytes(notes)[:-1], SC.notes_bytes(notes) + b"\0", SC.notes_bytes([(1, 2, 3, p)]), b""]
    out = tmp_path / "out"
    out.mkdir()
    lines = ["curve %d" % (0 if cvname == "bn254" else 1), "notes %d" % len(notes)]
    idm, sem = _mont(cv, [n[1] for n in notes]), _mont(cv, [n[3] for n in notes])
    lines += ["%d %d %s %s" % (n[0], n[2], _words(idm[i]), _words(sem[i])) for i, n in enumerate(notes)]
    for i, data in enumerate(bad_notes):
        (tmp_path / ("badnotes%d.bin" % i)).write_bytes(data)
        lines.append("badnotes %s" % (tmp_path / ("badnotes%d.bin" % i)))
    vm = _mont(cv, [v for _, v in entries])
    lines.append("treeout %d %d" % (len(entries), count))
    lines += ["%d %d %s" % (k[0], k[1], _words(vm[i])) for i, (k, _) in enumerate(entries)]
    lines.append(_words(_mont(cv, [snap.root])[0]))
    lines.append("badwrite")
    chunks = (1, 4, 1000)
    for name, data, h, cap, _, _ in table:
        (tmp_path / (name + ".bin")).write_bytes(data)
        lines += ["tree %s %d %d %d" % (tmp_path / (name + ".bin"), h, cap, chunk) for chunk in chunks]
    lines.append("tree %s %d %d 2" % (out / "tree.bin", height, 8))
    (tmp_path / "manifest.txt").write_text("\n".join(lines) + "\n")
    r = subprocess.run([driver, str(tmp_path / "manifest.txt"), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    assert sorted(os.listdir(out)) == ["notes.bin", "tree.bin"], "bad.bin or a temporary file stayed"
    assert (out / "notes.bin").read_bytes() == SC.notes_bytes(notes)
    assert (out / "tree.bin").read_bytes() == SC.store_bytes(snap.tree, snap.root, count)
    got = r.stdout.splitlines()
    assert got[0] == "notes_roundtrip ok %d %d" % (len(notes), SC.TOO_MANY_NOTES)
    for i, data in enumerate(bad_notes):
        kind, off, _ = SC.parse_notes(data, p)
        assert kind != SC.ACCEPTED and got[1 + i] == "notes %d %d" % (kind, off)
    at = 1 + len(bad_notes)
    assert got[at] == "tree_written %d" % len(entries)
    last = got[at + 1].split(" ", 2)
    assert last[:2] == ["refused", "1"] and "bad.bin" in last[2]
    at += 2
    for name, data, h, cap, kind, off in table:
        for chunk in chunks:
            f = got[at].split()
            at += 1
            assert f[:3] == ["tree", str(kind), str(off)], (name, chunk, got[at - 1])
            if kind == SC.ACCEPTED:
                assert f[3:] == [str(len(entries)), str(count), str(len(entries))], name
    assert got[at] == "tree 0 0 %d %d %d" % (len(entries), count, len(entries)) and len(got) == at + 1
