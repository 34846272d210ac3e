#!/usr/bin/env python3
"""tests/golden/verify_terms_pinned.json: per curve and per batch of tests/verify_terms_cases.py pinned_batches, for every
proof the SHA-256 of what the batch verifier's term stage returns for it (status, seven challenges, r0, the 24 sums) and of
where its transcript handle is left, taken from the host route (zkt_debug_verify_terms_host route 0) of the library as
built.  DATA only: it freezes the term stage against itself, so that routes which share their code are still held to
something (tests/test_verify_terms_pinned.py, tests/test_gpu_verify_terms_pinned.py).  Regenerate only from a commit whose
routes 0 and 1 are known to agree with the oracle.

Run from the repo root:  python tests/golden/make_golden_verify_terms.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import fields as F  # noqa: E402
import verify_terms_cases as TC  # noqa: E402


def main():
    from zkt_plonk_amd import _lib
    out = {}
    for cv in (F.BN254, F.BLS12_381):
        out[cv.name] = {}
        for name, rows, rho in TC.pinned_batches(cv):
            its = TC.items(cv, rows)
            res = _lib.debug_verify_terms_host(cv.name, its, rho, TC.forced_array(cv, rows), 0)
            out[cv.name][name] = dict(zip((r.name for r in rows), TC.digests(res, TC.probes(its))))
            assert len(out[cv.name][name]) == len(rows)
    with open(TC.PINNED, "w") as f:
        json.dump(out, f, indent=0, separators=(",", ":"))
    print("wrote", TC.PINNED, os.path.getsize(TC.PINNED), "bytes,", sum(len(b) for c in out.values() for b in c.values()), "digests")


if __name__ == "__main__":
    main()
