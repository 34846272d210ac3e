"""CPU: the writers of the reference CLI's --ck / --pk / --vk files (csrc/keyfile_write.hpp through zkt_keyfile_write_*): their
bytes against the oracle's writers (oracle/keyfile.py), the round trip through the library's own readers, the refusals (which
leave no file behind), and the same layout once more as a stand-alone program (tests/keyfile_write_host_main.cpp) built with
AddressSanitizer + UndefinedBehaviorSanitizer and run as a child process.  "Parity unpinned": the reference holds no key file."""
import importlib.util
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import fields as F, plonk as P, coracle as K, keyfile as KF
from zkt_plonk_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = {"bn254": F.BN254, "bls12_381": F.BLS12_381}
N_POWERS = 40
_CASES = {}


def _case(cv):
    """One circuit's keys per curve, with the edge each writer has to carry: an identity at index 3 of the powers, one
    polynomial of length 0, an identity among the commitments."""
    if cv.name not in _CASES:
        cs = P.test_circuit(cv)
        n = cs.circuit_bound()
        srs = K.srs_mont(cv, 0xF11E, n + 8)
        pk, epk, vk = P.setup(K.CBackend(cv, srs), [None] * (n + 8), cs, False)
        powers = srs[:N_POWERS].copy()
        powers[3] = 0
        pts = K.points_from_mont(cv, powers)
        assert pts[3] is None and pts.count(None) == 1
        pk0 = SimpleNamespace(polys=dict(pk.polys, q_c=[]))
        vk0 = SimpleNamespace(n=vk.n, pi_roots=list(vk.pi_roots), commits=dict(vk.commits, q_lookup=None))
        assert len(vk0.pi_roots) > 0 and all(len(pk0.polys[k]) > 0 for k in P.PK_POLYS if k != "q_c")
        polys = [K.fr_to_mont(cv, pk0.polys[k]) if pk0.polys[k] else np.zeros((0, 4), dtype=np.uint64) for k in P.PK_POLYS]
        commits = K.points_to_mont(cv, [vk0.commits[k] for k in P.PK_POLYS])
        inf = [vk0.commits[k] is None for k in P.PK_POLYS]
        _CASES[cv.name] = SimpleNamespace(cv=cv, powers=powers, pts=pts, pk=pk0, vk=vk0, polys=polys, roots=K.fr_to_mont(cv, vk0.pi_roots),
                                          commits=commits, inf=inf, want_ck=KF.committer_key_bytes(cv, pts),
                                          want_pk=KF.prover_key_bytes(cv, pk0), want_vk=KF.verifier_key_bytes(cv, vk0))
    return _CASES[cv.name]


@pytest.mark.parametrize("cvname", sorted(CURVES))
def test_the_three_writers_give_the_oracle_writers_bytes(cvname, tmp_path):
    c = _case(CURVES[cvname])
    ck, pk, vk = (str(tmp_path / x) for x in ("ck.bin", "pk.bin", "vk.bin"))
    _lib.keyfile_write_committer_key(ck, cvname, c.powers)
    assert open(ck, "rb").read() == c.want_ck
    _lib.keyfile_write_prover_key(pk, cvname, c.polys)
    assert open(pk, "rb").read() == c.want_pk
    _lib.keyfile_write_verifier_key(vk, cvname, c.vk.n, c.roots, c.commits, c.inf)
    assert open(vk, "rb").read() == c.want_vk
    _lib.keyfile_write_verifier_key(vk, cvname, c.vk.n, c.roots, c.commits, None)     # (0, 0) alone marks the identity
    assert open(vk, "rb").read() == c.want_vk
    assert sorted(os.listdir(tmp_path)) == ["ck.bin", "pk.bin", "vk.bin"], "a temporary file stayed"
    assert _lib.keyfile_last_error() == ""


@pytest.mark.parametrize("cvname", sorted(CURVES))
def test_written_files_read_back_value_for_value(cvname, tmp_path):
    c = _case(CURVES[cvname])
    cv = c.cv
    ck, pk, vk = (str(tmp_path / x) for x in ("ck.bin", "pk.bin", "vk.bin"))
    _lib.keyfile_write_committer_key(ck, cvname, c.powers)
    assert np.array_equal(_lib.keyfile_committer_key(ck, cvname), c.powers)
    assert np.array_equal(_lib.keyfile_committer_key(ck, cvname, max_powers=7), c.powers[:7])
    _lib.keyfile_write_prover_key(pk, cvname, c.polys)
    got = _lib.keyfile_prover_key(pk, cvname)
    for k, name in enumerate(P.PK_POLYS):
        assert got[k].shape == c.polys[k].shape and np.array_equal(got[k], c.polys[k]), name
        assert K.fr_from_mont(cv, got[k]) == list(c.pk.polys[name]), name
    _lib.keyfile_write_verifier_key(vk, cvname, c.vk.n, c.roots, c.commits, c.inf)
    n, roots, commits, inf = _lib.keyfile_verifier_key(vk, cvname)
    assert n == c.vk.n and np.array_equal(roots, c.roots) and np.array_equal(commits, c.commits)
    assert [bool(x) for x in inf] == c.inf and c.inf[P.PK_POLYS.index("q_lookup")]


def _limbs(v, words):
    return np.array([(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(words)], dtype=np.uint64)


@pytest.mark.parametrize("cvname", sorted(CURVES))
def test_refused_writes_leave_no_file_behind(cvname, tmp_path):
    c = _case(CURVES[cvname])
    cv = c.cv
    fql = cv.fq.limbs64
    out = tmp_path / "out"
    out.mkdir()
    path = str(out / "key.bin")

    def refused(call, *args, **kw):
        with pytest.raises(_lib.ZktError) as e:
            call(*args, **kw)
        assert e.value.code == 1, "ZKT_ERR_INVALID_ARGUMENT"
        assert os.listdir(out) == [], "a refused write left %s" % os.listdir(out)
        return str(e.value)

    # a limb vector equal to the modulus: a coefficient, a root, either coordinate of a point (the readers refuse these)
    polys = [a.copy() for a in c.polys]
    polys[4] = np.zeros((2, 4), dtype=np.uint64)
    polys[4][1] = _limbs(cv.fr.p, 4)
    assert path in refused(_lib.keyfile_write_prover_key, path, cvname, polys)
    roots = c.roots.copy()
    roots[-1] = _limbs(cv.fr.p, 4)
    assert path in refused(_lib.keyfile_write_verifier_key, path, cvname, c.vk.n, roots, c.commits, c.inf)
    for half in (0, 1):
        commits = c.commits.copy()
        commits[9, half * fql:(half + 1) * fql] = _limbs(cv.fq.p, fql)
        assert path in refused(_lib.keyfile_write_verifier_key, path, cvname, c.vk.n, c.roots, commits, c.inf)
        powers = c.powers.copy()
        powers[5, half * fql:(half + 1) * fql] = _limbs(cv.fq.p, fql)
        assert path in refused(_lib.keyfile_write_committer_key, path, cvname, powers)
    # n_pi > 0 with NULL roots; no power at all
    refused(_lib.keyfile_write_verifier_key, path, cvname, c.vk.n, None, c.commits, c.inf, n_pi=2)
    refused(_lib.keyfile_write_committer_key, path, cvname, np.zeros((0, 2 * fql), dtype=np.uint64))
    # a directory that cannot be written to: one that is not there, one that is a file and (for an ordinary user) a read-only one
    (tmp_path / "plain").write_bytes(b"x")
    targets = [str(out / "missing" / "key.bin"), str(tmp_path / "plain" / "key.bin")]
    locked = tmp_path / "locked"
    locked.mkdir()
    if os.geteuid() != 0:
        os.chmod(locked, 0o555)
        targets.append(str(locked / "key.bin"))
    try:
        for t in targets:
            for call, args in ((_lib.keyfile_write_committer_key, (c.powers,)), (_lib.keyfile_write_prover_key, (c.polys,)),
                               (_lib.keyfile_write_verifier_key, (c.vk.n, c.roots, c.commits, c.inf))):
                assert t in refused(call, t, cvname, *args)
                assert not os.path.exists(t)
        assert os.listdir(locked) == []
    finally:
        os.chmod(locked, 0o755)
    # a failing write over a good file leaves the good file as it was
    _lib.keyfile_write_prover_key(path, cvname, c.polys)
    with pytest.raises(_lib.ZktError):
        _lib.keyfile_write_prover_key(path, cvname, polys)
    assert open(path, "rb").read() == c.want_pk and os.listdir(out) == ["key.bin"]


# ---- the stand-alone sanitizer run ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    spec = importlib.util.spec_from_file_location("zkt_build", os.path.join(ROOT, "zkt-plonk_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    exe = str(tmp_path_factory.mktemp("keyfile_write") / "keyfile_write_host_main")
    # plain C++: the writers' header includes nothing of HIP
    r = subprocess.run([b.CLANG, "-x", "c++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                        os.path.join(ROOT, "tests", "keyfile_write_host_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


@pytest.mark.parametrize("cvname", sorted(CURVES))
def test_sanitized_stand_alone_writers(cvname, driver, tmp_path):
    c = _case(CURVES[cvname])
    cv = c.cv
    words = lambda a: " ".join(str(int(x)) for x in np.ascontiguousarray(a, dtype=np.uint64).reshape(-1))
    case = tmp_path / "case.txt"
    with open(case, "w") as f:
        f.write("%d %d %d %d\n" % (0 if cvname == "bn254" else 1, len(c.powers), c.vk.n, len(c.roots)))
        for p in c.powers:
            f.write(words(p) + "\n")
        for a in c.polys:
            f.write("%d %s\n" % (a.shape[0], words(a)))
        for r_ in c.roots:
            f.write(words(r_) + "\n")
        for k in range(10):
            f.write("%s %d\n" % (words(c.commits[k]), int(c.inf[k])))
    out = tmp_path / "out"
    out.mkdir()
    r = subprocess.run([driver, str(case), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    assert sorted(os.listdir(out)) == ["ck.bin", "pk.bin", "vk.bin"], "bad.bin or a temporary file stayed"
    assert (out / "ck.bin").read_bytes() == c.want_ck
    assert (out / "pk.bin").read_bytes() == c.want_pk
    assert (out / "vk.bin").read_bytes() == c.want_vk
    # what the program's own parser found in the files
    lines = r.stdout.splitlines()
    point = lambda l: None if l.split()[2] == "1" else (int(l.split()[0], 16), int(l.split()[1], 16))
    assert lines[0].split() == ["ck", str(N_POWERS), "0", str(N_POWERS - 1)]
    assert [point(l) for l in lines[1:1 + N_POWERS]] == c.pts
    assert lines[1 + 3].split()[:2] == ["0" * (16 * cv.fq.limbs64), "0" * (16 * cv.fq.limbs64 - 1) + "1"], "GroupAffine::zero() is (0, 1)"
    at = 1 + N_POWERS
    assert lines[at] == "pk"
    at += 1
    for name in P.PK_POLYS:
        want = list(c.pk.polys[name])
        assert lines[at].split() == [name, str(len(want))]
        assert [int(x, 16) for x in lines[at + 1:at + 1 + len(want)]] == want, name
        at += 1 + len(want)
    assert lines[at].split() == ["vk", str(c.vk.n), str(len(c.vk.pi_roots))]
    at += 1
    assert [int(x, 16) for x in lines[at:at + len(c.vk.pi_roots)]] == c.vk.pi_roots
    at += len(c.vk.pi_roots)
    assert [point(l) for l in lines[at:at + 10]] == [c.vk.commits[k] for k in P.PK_POLYS]
    last = lines[at + 10].split(" ", 2)
    assert last[:2] == ["refused", "1"] and "bad.bin" in last[2] and len(lines) == at + 11
