"""Shapes and requests for the withdraw circuit as a library component (zkt_withdraw_*), with the oracle twin of each: the
reference composer's restatement (oracle/composer.py withdraw_synthesize) run on the same request.  Shared by the CPU pin of
the host planner (test_withdraw_layout_host.py) and the device tests (test_gpu_withdraw.py); a case is computed once and
never changed.

A request is a dictionary of Python integers in the manner of tools/withdraw_workload.py make_instance: `inputs` notes spent
out of a tree that also holds decoys."""
import functools
import random

import numpy as np

from oracle import composer as OC, fields as F, coracle as K, plonk as P

import merkle_path_cases as MC

ZERO = 0xFFFFFFFF            # ZKT_VARIABLE_ZERO
TABLE_SIZE = 16

# (curve, width, inputs, height): no addition rows and one level; three levels; two notes; three notes (two running sums);
# the other curve; the width bound
SHAPES = [("bn254", 4, 1, 1), ("bn254", 4, 1, 3), ("bn254", 5, 2, 2), ("bn254", 4, 3, 2), ("bls12_381", 5, 2, 1), ("bn254", 8, 2, 2)]
SHIPPED = ("bn254", 5, 1, 1)     # the BN254 x5 tables: rows only


@functools.lru_cache(maxsize=None)
def params(cvname, w, shipped=False):
    return MC.shipped_params(w) if shipped else MC.synthetic_params(F.CURVES[cvname], w)


def params_words(cv, prm):
    """The library's (width, half_full, partial, round_constants, mds, domain_tag), constants in Montgomery words."""
    return (prm.width, prm.half_full, prm.partial, K.fr_to_mont(cv, prm.rc[:(2 * prm.half_full + prm.partial) * prm.width]),
            K.fr_to_mont(cv, [x for row in prm.mds for x in row]), K.fr_to_mont(cv, [prm.domain_tag])[0])


def make_request(prm, inputs, height, seed, mode="random"):
    """mode: "random"; "all" withdraws everything (amount_out = 0); "top" has amounts summing to 2^64 - 1 and withdraws so
    little that amount_out keeps bit 63; "bits" places the notes so that every level sees both bit values (height >= 1,
    inputs >= 2 or a tree with more than one leaf)."""
    rnd = random.Random(0xD0E5 + 1000 * seed + 31 * inputs + height)
    p = prm.p
    ident_set = [random.Random(0x1D5E7 + k).randrange(1, p) for k in range(7)]
    total = min(2 * inputs + 3, 1 << height)
    tree = OC.NativeMerkleTree(prm, height)
    notes = []
    for k in range(total):
        secret, ident, amount = rnd.randrange(1, p), rnd.choice(ident_set), rnd.randrange(1, 1 << 40)
        notes.append([secret, ident, amount, k])
    if mode == "bits":                       # the last leaf and leaf 0: bits all set (as far as the tree goes) and all clear
        spent = ([notes[-1], notes[0]] + notes[1:-1])[:inputs]
    else:
        spent = rnd.sample(notes, inputs)
    if mode == "top":                        # the spent amounts sum to 2^64 - 1
        left = (1 << 64) - 1
        for i, nt in enumerate(spent):
            nt[2] = left if i == inputs - 1 else rnd.randrange(1, 1 << 60)
            left -= nt[2]
    leaves = []
    for secret, ident, amount, _ in notes:
        leaves.append(prm.native([ident, amount, prm.native([secret])]))
        tree.add_leaf(leaves[-1])
    amount_in = sum(nt[2] for nt in spent)
    if mode == "all":
        withdraw = amount_in
    elif mode == "top":
        withdraw = 5
        assert (amount_in - withdraw) >> 63 == 1
    else:
        withdraw = rnd.randrange(1, amount_in) if amount_in > 1 else 0
    return dict(secrets=[nt[0] for nt in spent], identifiers=[nt[1] for nt in spent], amounts=[nt[2] for nt in spent],
                poes=[(nt[3], tree.merkle_path(nt[3])) for nt in spent], root=tree.root, new_secret=rnd.randrange(1, p),
                new_identifier=rnd.choice(ident_set), withdraw_amount=withdraw, ident_set=ident_set, leaves=leaves,
                notes=[tuple(nt) for nt in notes])


def synthesize(cv, prm, req, table_size=TABLE_SIZE):
    cs = OC.Composer(cv, req["ident_set"], table_size)
    OC.withdraw_synthesize(cs, prm, req["secrets"], req["identifiers"], req["amounts"], req["poes"], req["root"], req["new_secret"],
                           req["new_identifier"], req["withdraw_amount"])
    return cs


class Case:
    """One shape with one request and its oracle twin."""

    def __init__(self, cvname, w, inputs, height, shipped, seed, mode):
        self.cv, self.w, self.inputs, self.height = F.CURVES[cvname], w, inputs, height
        self.prm = params(cvname, w, shipped)
        self.req = make_request(self.prm, inputs, height, seed, mode)
        self.cs = synthesize(self.cv, self.prm, self.req)
        self.n_gates, self.n_vars = self.cs.n_gates, len(self.cs.values)
        self.pi_pos = sorted(self.cs.pi)
        p = self.prm.p
        amount_out = sum(self.req["amounts"]) - self.req["withdraw_amount"]
        nullifiers = [self.prm.native([pow(s, -1, p)]) for s in self.req["secrets"]]
        new_leaf = self.prm.native([self.req["new_identifier"], amount_out, self.prm.native([self.req["new_secret"]])])
        # bin/src/main.rs:266-271
        self.cli_pi = [self.req["root"]] + nullifiers + [self.req["withdraw_amount"] % p, self.req["new_identifier"], new_leaf]

    @property
    def words(self):
        return params_words(self.cv, self.prm)

    def selectors(self):
        return [getattr(self.cs, k) for k in ("q_m", "q_l", "q_r", "q_o", "q_c", "q_lookup")]

    def wires(self):
        conv = lambda ws: [ZERO if v == P.ZERO_VAR else v for v in ws]
        return [conv(self.cs.w_l), conv(self.cs.w_r), conv(self.cs.w_o)]

    def hash_calls(self):
        """(first variable, arity, three input variables padded with ZERO) per call, in call order"""
        out = []
        for base, ins in self.cs.hash_calls:
            assert all(c == 1 and o == 0 for (_, c, o) in ins)
            vs = [v for (v, _, _) in ins]
            out.append([base, len(vs)] + vs + [ZERO] * (3 - len(vs)))
        return out


@functools.lru_cache(maxsize=None)
def case(cvname, w, inputs, height, shipped=False, seed=1, mode="random"):
    c = Case(cvname, w, inputs, height, shipped, seed, mode)
    assert c.cs.check_satisfied()
    assert c.n_gates == OC.withdraw_gate_count(c.prm, inputs, height)
    assert [c.cs.pi[i] for i in c.pi_pos] == c.cli_pi
    return c


def request_words(cv, req, siblings=True, root=True):
    """The request as Context.withdraw_witness takes it."""
    m = lambda xs: K.fr_to_mont(cv, list(xs))
    return dict(secrets=m(req["secrets"]), identifiers=m(req["identifiers"]), amounts=np.array(req["amounts"], dtype=np.uint64),
                leaf_indices=np.array([i for i, _ in req["poes"]], dtype=np.uint64),
                siblings=m([x for _, path in req["poes"] for x in path]) if siblings else None,
                root=m([req["root"]])[0] if root else None, new_secret=m([req["new_secret"]])[0],
                new_identifier=m([req["new_identifier"]])[0], withdraw_amount=req["withdraw_amount"])
