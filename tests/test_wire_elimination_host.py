"""The host pass behind the wire tables over free variables (csrc/wire_elim.hpp through zkt_debug_wire_elimination; no
device): which rows define their output, and the affine forms x_v = kappa_v + sum_f M[v][f] x_f they leave, checked with
Python integers against satisfying witnesses."""
import numpy as np
import pytest

from oracle import fields as F, plonk as P
import wire_elim_cases as W

CV = F.BN254
Z = P.ZERO_VAR


def _withdraw(height):
    from oracle import composer as OC
    import test_gpu_poseidon as TP
    return OC.withdraw_instance(CV, TP._gadget_params(CV, 4), inputs=1, height=height, seed=11)[0]


_CIRCUITS = {}


def _circuit(name):
    if name not in _CIRCUITS:
        if name.startswith("synthetic"):
            _CIRCUITS[name] = P.synthetic_circuit(CV, int(name[9:]) - 3, 4, seed=3, n_public=2)
        else:
            _CIRCUITS[name] = _withdraw(int(name[8:]))
        assert _CIRCUITS[name].check_satisfied()
    return _CIRCUITS[name]


@pytest.mark.parametrize("K", [1, 2, 16])
@pytest.mark.parametrize("name", ["synthetic64", "synthetic512", "withdraw2", "withdraw7"])
def test_forms_hold_on_the_satisfying_witness(name, K):
    cs = _circuit(name)
    p = cs.p
    kind, free, forms = W.eliminate(CV, cs, K)
    on_wire = {v for ws in (cs.w_l, cs.w_r, cs.w_o) for v in ws if v != Z}
    assert set(free) | set(forms) == on_wire and not set(free) & set(forms)
    assert len(set(free)) == len(free)
    assert forms, "nothing was eliminated"
    for v, (terms, kappa) in forms.items():
        assert kind[v] == W.DEFINED and len(terms) <= K
        assert all(kind[f] == W.FREE and c % p != 0 for f, c in terms.items())
        assert cs.values[v] == (kappa + sum(c * cs.values[f] for f, c in terms.items())) % p, v
    for f in free:
        assert kind[f] == W.FREE
    again = W.raw(CV, cs, K)
    for x, y in zip(W.raw(CV, cs, K), again):
        assert np.array_equal(x, y)


def test_the_withdraw_circuit_is_mostly_defined():
    cs = _circuit("withdraw7")
    kind, free, forms = W.eliminate(CV, cs, 16)
    assert len(free) < 0.3 * cs.n_gates < len(forms)
    assert W.predicted_routes(cs, kind, free, forms) == [2, 2, 2]


def _cs():
    return P.ConstraintSystem(CV, [1, 2, 5], 8)


def test_a_chain_longer_than_the_cap_still_closes():
    cs = _cs()
    p = cs.p
    x, y = cs.assign_variable(11), cs.assign_variable(13)
    chain = [x]
    for i in range(10):                                    # one free variable all along: support 1
        v = cs.assign_variable(3 * cs.value_of(chain[-1]) + 5)
        cs.arith_constrain(chain[-1], Z, v, q_l=3, q_o=-1, q_c=5)
        chain.append(v)
    s = cs.add_gate(chain[-1], y)                          # support 2: free under K = 1
    t = cs.assign_variable(2 * cs.value_of(s) + 1)
    cs.arith_constrain(s, Z, t, q_l=2, q_o=-1, q_c=1)      # and the chain goes on from it
    assert cs.check_satisfied()
    kind, free, forms = W.eliminate(CV, cs, 1)
    assert free == [x, y, s]
    assert forms[chain[10]] == ({x: pow(3, 10, p)}, 5 * (pow(3, 10, p) - 1) * pow(2, -1, p) % p)
    assert forms[t] == ({s: 2}, 1)
    kind, free, forms = W.eliminate(CV, cs, 2)
    assert free == [x, y] and forms[s][0] == {x: pow(3, 10, p), y: 1}
    assert forms[t][0] == {x: 2 * pow(3, 10, p) % p, y: 2}


def test_public_input_rows_never_define():
    cs = _cs()
    x, y = cs.assign_variable(4), cs.assign_variable(9)
    z = cs.add_gate(x, y)                                  # row 0
    w = cs.assign_variable(cs.value_of(z))
    cs.arith_constrain(z, Z, w, q_l=1, q_o=-1, pi=0)       # row 1: linear, but a public-input position
    cs.set_variable_public(z)                              # row 2
    u = cs.add_gate(w, x)                                  # row 3
    assert cs.check_satisfied() and sorted(cs.pi) == [1, 2]
    kind, free, forms = W.eliminate(CV, cs)
    assert free == [x, y, w] and set(forms) == {z, u}
    assert forms[u] == ({w: 1, x: 1}, 0)
    # the positions are the proof's: without row 1 among them w is defined, with row 0 among them z is free
    kind, free, forms = W.eliminate(CV, cs, pi_pos=[2])
    assert free == [x, y] and forms[w] == ({x: 1, y: 1}, 0)
    kind, free, forms = W.eliminate(CV, cs, pi_pos=[0, 1, 2])
    assert free == [x, y, z, w] and set(forms) == {u}


def test_rows_that_do_not_define():
    cs = _cs()
    p = cs.p
    x, y = cs.assign_variable(6), cs.assign_variable(10)
    half = cs.assign_variable((6 + 10) * pow(2, -1, p))
    cs.arith_constrain(x, y, half, q_l=1, q_r=1, q_o=-2)               # q_o is neither 1 nor -1
    prod = cs.mul_gate(x, y)                                           # q_m != 0
    both = cs.assign_variable(7)
    cs.arith_constrain(x, y, both, q_m=1, q_l=1, q_o=-1, q_c=7 - 60 - 6)   # q_m != 0 with linear terms
    cs.arith_constrain(x, y, Z, q_l=5, q_r=-3)                         # Variable::Zero on the output wire
    same = cs.assign_variable(0)
    cs.arith_constrain(same, x, same, q_l=1, q_o=-1, q_r=0)            # the output is one of the inputs
    cs.arith_constrain(x, y, prod, q_l=10, q_o=-1)                     # the output was seen on an earlier row
    plus = cs.assign_variable(-(6 + 2 * 10 + 3))
    cs.arith_constrain(x, y, plus, q_l=1, q_r=2, q_o=1, q_c=3)         # q_o = +1 defines
    assert cs.check_satisfied()
    kind, free, forms = W.eliminate(CV, cs)
    assert free == [x, y, half, prod, both, same]
    assert forms == {plus: ({x: p - 1, y: p - 2}, p - 3)}


def test_zero_inputs_and_zero_selectors_contribute_nothing():
    cs = _cs()
    x, y = cs.assign_variable(21), cs.assign_variable(22)
    a = cs.assign_variable(3 * 22 + 7)
    cs.arith_constrain(Z, y, a, q_l=5, q_r=3, q_o=-1, q_c=7)           # Zero on the left wire under a selector
    b = cs.assign_variable(4 * 21)
    cs.arith_constrain(x, y, b, q_l=4, q_r=0, q_o=-1)                  # y under a zero selector
    c = cs.assign_variable(9)
    cs.arith_constrain(Z, Z, c, q_o=-1, q_c=9)                         # a constant
    d = cs.assign_variable(0)
    cs.arith_constrain(a, a, d, q_l=2, q_r=-2, q_o=-1)                 # the terms cancel: an empty form
    assert cs.check_satisfied()
    kind, free, forms = W.eliminate(CV, cs)
    assert free == [y, x]
    assert forms == {a: ({y: 3}, 7), b: ({x: 4}, 0), c: ({}, 9), d: ({}, 0)}
