"""CPU: every routine of fx.hpp / ecx.hpp on operands at its stated bounds (tests/fx_contracts.py), run on the host
through zkt_host_fx_op / zkt_host_xyzz_op (the C++ loops of the products), against Python big integers."""
import random

import pytest

import zkt_plonk_amd as z
from zkt_plonk_amd import _lib
import fx_contracts as K

N_HOST = 160          # tuples per row and field, on top of every edge value of every operand


def fd_of(curve, which, f):
    L, B, SH = _lib.fx_layout(curve, which)
    return K.Fd(f, which, L, B, SH)


CASES = [(c, w, f, row) for c, w, f in K.FIELDS for row in K.ROWS if row.only(fd_of(c, w, f))]


def test_layout_matches_the_limb_form():
    for c, w, f in K.FIELDS:
        fd = fd_of(c, w, f)
        assert fd.B == 29 and fd.B * fd.L == 32 * fd.N + fd.SH and fd.B * fd.L >= f.bits + 6, (f.name, fd)


def test_every_op_has_a_row_and_every_row_an_op():
    ops = _lib.fx_ops()
    assert {r.op for r in K.ROWS} == set(ops), set(ops) ^ {r.op for r in K.ROWS}
    assert set(_lib.xyzz_ops()) == set(K.CURVE_OPS)


@pytest.mark.parametrize("curve,which,f,row", CASES, ids=lambda x: getattr(x, "name", str(x)))
def test_fx_op_meets_its_contract(curve, which, f, row):
    fd = fd_of(curve, which, f)
    op = _lib.fx_ops()[row.op]
    tuples, recs = K.build(fd, row, random.Random("%s/%s" % (f.name, row.name)), N_HOST)
    out = _lib.host_fx_op(curve, which, op, recs)
    K.check(fd, row, tuples, out)


def test_ops_a_field_does_not_support_are_refused():
    ops = _lib.fx_ops()
    fd = fd_of(1, 1, K.F.BLS12_381_FQ)
    for name in ("REDUCE_LAZY", "MUL_SHOUP"):     # the 381-bit field's narrow top limb; fourteen-limb Shoup columns
        with pytest.raises(z.ZktError) as e:
            _lib.host_fx_op(1, 1, ops[name], [[0] * fd.W])
        assert e.value.code == 1
    with pytest.raises(z.ZktError):
        _lib.host_fx_op(0, 0, len(ops), [[0] * 36])
    with pytest.raises(z.ZktError):
        _lib.host_xyzz_op(0, len(K.CURVE_OPS), [[0] * 74])


@pytest.mark.parametrize("curve,cv", K.CURVES, ids=["bn254", "bls12_381"])
@pytest.mark.parametrize("op", K.CURVE_OPS)
def test_xyzz_op_meets_its_contract(curve, cv, op):
    fd = fd_of(curve, 1, cv.fq)
    want, recs = K.curve_records(cv, fd, op, random.Random("%s/%s" % (cv.name, op)), 96)
    out = _lib.host_xyzz_op(curve, _lib.xyzz_ops()[op], recs)
    K.check_curve(cv, fd, op, want, out)
