"""CPU: the code the host verifier and the batch verifier's kernel share (csrc/transcript_core.hpp, csrc/transcript.hip,
compute_r0 of csrc/linearisation.hpp) as a stand-alone program (tests/verify_core_host_main.cpp) built with
AddressSanitizer + UndefinedBehaviorSanitizer and run as a child process: the known answers at a stride of 1 and of 64, a
Merlin message across two STROBE block edges, compute_r0 with no public input, with one, and with a root on xi."""
import importlib.util
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sanitized_transcript_core_and_r0(tmp_path):
    spec = importlib.util.spec_from_file_location("zkt_build", os.path.join(ROOT, "zkt-plonk_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    exe = str(tmp_path / "verify_core_host_main")
    r = subprocess.run([b.CLANG, "-x", "hip", "--cuda-host-only", "-I/opt/rocm/include", "-O1", "-g", "-std=c++17", "-Wno-psabi",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                        os.path.join(ROOT, "tests", "verify_core_host_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.stdout.strip() == "ok"
