"""CPU: routes 0 and 1 of zkt_debug_verify_terms_host reproduce tests/golden/verify_terms_pinned.json -- per proof of the
table of tests/verify_terms_cases.py the status, the seven challenges, r0, the 24 sums and where the handle is left, as
the host route computed them before the routes came to share one replay and one transcript core."""
import pytest

from oracle import fields as F

import verify_terms_cases as TC

CURVES = [F.BN254, F.BLS12_381]
IDS = lambda c: c.name  # noqa: E731


@pytest.mark.parametrize("route", [0, 1])
@pytest.mark.parametrize("cv", CURVES, ids=IDS)
def test_both_host_routes_reproduce_every_pinned_digest(cv, route):
    from zkt_plonk_amd import _lib
    seen = 0
    for name, rows, rho in TC.pinned_batches(cv):
        its = TC.items(cv, rows)
        res = _lib.debug_verify_terms_host(cv.name, its, rho, TC.forced_array(cv, rows), route)
        got = dict(zip((r.name for r in rows), TC.digests(res, TC.probes(its))))
        assert got == TC.pinned()[cv.name][name], name
        seen += len(got)
    assert seen == sum(len(b) for b in TC.pinned()[cv.name].values()) >= 50
