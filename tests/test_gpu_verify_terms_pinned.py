"""GPU: the kernel (zkt_debug_verify_terms route 2) reproduces tests/golden/verify_terms_pinned.json at the batch sizes of
tests/test_gpu_verify_terms.py -- one workgroup, its edge, a second one -- and on the forced and refused batches."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import fields as F

import verify_terms_cases as TC

CURVES = [F.BN254, F.BLS12_381]
IDS = lambda c: c.name  # noqa: E731


@pytest.fixture(scope="module")
def ctxs():
    import zkt_plonk_amd as z
    made = {cv.name: z.Context(cv.name, 0) for cv in CURVES}
    yield made
    for c in made.values():
        c.close()


def _kernel_digests(ctx, cv, rows, rho):
    its = TC.items(cv, rows)
    res = ctx.debug_verify_terms(its, rho, TC.forced_array(cv, rows), 2)
    return TC.digests(res, TC.probes(its))


@pytest.mark.parametrize("count", [1, 3, 64, 65, 67])
@pytest.mark.parametrize("cv", CURVES, ids=IDS)
def test_the_kernel_reproduces_the_pinned_table(ctxs, cv, count):
    """row i of the batch is row i mod 20 of the table, with that row's pinned coefficients"""
    name, table, rho = TC.pinned_batches(cv)[0]
    at = [i % len(table) for i in range(count)]
    got = _kernel_digests(ctxs[cv.name], cv, [table[i] for i in at], rho.reshape(len(table), 2, 4)[at].reshape(2 * count, 4))
    assert got == [TC.pinned()[cv.name][name][table[i].name] for i in at]


@pytest.mark.parametrize("cv", CURVES, ids=IDS)
def test_the_kernel_reproduces_the_pinned_forced_and_refused_batches(ctxs, cv):
    for name, rows, rho in TC.pinned_batches(cv)[1:]:
        assert _kernel_digests(ctxs[cv.name], cv, rows, rho) == [TC.pinned()[cv.name][name][r.name] for r in rows], name
