"""GPU: every routine of fx.hpp / ecx.hpp at its stated bounds (tests/fx_contracts.py) through the device's own code,
the ordered multiply-add chains of the products (zkt_debug_fx_op / zkt_debug_xyzz_op, one record per thread, one launch
per field and row).  Each result must meet the contract and equal the host build's result bit for bit: both run the same
algorithm (the Montgomery digits are unique, the Shoup quotient's truncated columns fixed)."""
import random

import numpy as np
import pytest

import zkt_plonk_amd as z
from zkt_plonk_amd import _lib
import fx_contracts as K

N_DEV = 1500          # tuples per row and field (plus every edge value of every operand)
N_CURVE = 1024


def fd_of(curve, which, f):
    L, B, SH = _lib.fx_layout(curve, which)
    return K.Fd(f, which, L, B, SH)


@pytest.fixture(scope="module")
def ctxs():
    cs = {c: z.Context(c, 0) for c in (0, 1)}
    yield cs
    for c in cs.values():
        c.close()


def _diff(host, dev):
    bad = np.nonzero((host != dev).any(axis=1))[0]
    return "%d records differ, first %d: host %s device %s" % (
        len(bad), bad[0], [hex(int(x)) for x in host[bad[0]]], [hex(int(x)) for x in dev[bad[0]]]) if len(bad) else ""


@pytest.mark.gpu
@pytest.mark.parametrize("curve,which,f", K.FIELDS, ids=lambda x: getattr(x, "name", str(x)))
def test_device_fx_ops_meet_their_contracts_and_match_the_host(ctxs, curve, which, f):
    fd = fd_of(curve, which, f)
    ops = _lib.fx_ops()
    failures = []
    for row in K.ROWS:
        if not row.only(fd):
            continue
        tuples, recs = K.build(fd, row, random.Random("dev/%s/%s" % (f.name, row.name)), N_DEV)
        recs = np.asarray(recs, dtype=np.uint32)
        dev = ctxs[curve].debug_fx_op(which, ops[row.op], recs)
        host = _lib.host_fx_op(curve, which, ops[row.op], recs)
        d = _diff(host, dev)
        if d:
            failures.append("%s (%s): device != host: %s" % (row.name, row.src, d))
        try:
            K.check(fd, row, tuples, dev)
        except AssertionError as e:
            failures.append("device: %s" % str(e).splitlines()[0])
    assert not failures, "\n".join(failures)


@pytest.mark.gpu
def test_device_refuses_ops_a_field_does_not_support(ctxs):
    ops = _lib.fx_ops()
    fd = fd_of(1, 1, K.F.BLS12_381_FQ)
    for name in ("REDUCE_LAZY", "MUL_SHOUP"):
        with pytest.raises(z.ZktError) as e:
            ctxs[1].debug_fx_op(1, ops[name], np.zeros((4, fd.W), dtype=np.uint32))
        assert e.value.code == 1


@pytest.mark.gpu
@pytest.mark.parametrize("curve,cv", K.CURVES, ids=["bn254", "bls12_381"])
def test_device_xyzz_ops_meet_their_contracts_and_match_the_host(ctxs, curve, cv):
    fd = fd_of(curve, 1, cv.fq)
    failures = []
    for op in K.CURVE_OPS:
        want, recs = K.curve_records(cv, fd, op, random.Random("dev/%s/%s" % (cv.name, op)), N_CURVE)
        recs = np.asarray(recs, dtype=np.uint32)
        dev = ctxs[curve].debug_xyzz_op(_lib.xyzz_ops()[op], recs)
        host = _lib.host_xyzz_op(curve, _lib.xyzz_ops()[op], recs)
        d = _diff(host, dev)
        if d:
            failures.append("%s: device != host: %s" % (op, d))
        try:
            K.check_curve(cv, fd, op, want, dev)
        except AssertionError as e:
            failures.append("device: %s" % str(e).splitlines()[0])
    assert not failures, "\n".join(failures)
