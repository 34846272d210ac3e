"""Cases for zkt_poseidon_merkle_path_witness_dev, built from the oracle's restatement of the reference's Merkle-path gadget
(oracle/composer.py poe_synthesize = PoECircuit::synthesize + merkle_proof, plonk-hashing/src/merkle/binary.rs:8-78) run on
a composer seeded with a leaf variable.  Shared by the CPU pin of the layout (test_merkle_path_cases_oracle.py) and the
device test (test_gpu_merkle_path.py); a case is computed once and never changed (callers copy what they alter).

A case holds the FULL variable map (the composer's `values`), the indices of every path's leaf, bits and siblings, the
first variable of every path and the expected roots.  Per level the composer allocates the six variables of the two
conditional_selects and then the hash's: S = 6 + vars_per_hash consecutive variables, level k of a path at base + k S."""
import functools
import json
import os

import numpy as np

from oracle import composer as OC, fields as F

from helpers import field_elems, splitmix64

ZERO = 0xFFFFFFFF            # ZKT_VARIABLE_ZERO
HERE = os.path.dirname(os.path.abspath(__file__))


def lanes_per_hash(w):
    """PoseidonLanes<W>::LPH of csrc/poseidon.hip: 16 lanes up to width 4, 32 for width 5, 64 beyond."""
    return 4 if w * w <= 4 else 16 if w * w <= 16 else 32 if w * w <= 32 else 64


def per_wave(w):
    return 64 // lanes_per_hash(w)


def synthetic_params(cv, w, half_full=2, partial=3):
    """Splitmix constants with a short schedule: every kind of round (full, partial, full) at a few hundred variables."""
    p = cv.fr.p
    rc = field_elems(p, 90 + w, (2 * half_full + partial) * w)
    mds = [field_elems(p, 900 + 7 * w + i, w) for i in range(w)]
    return OC.PoseidonParams(p, w, half_full, partial, rc, mds)


def shipped_params(w):
    """The BN254 x3 / x4 / x5 tables the withdraw circuit hashes with (tests/golden/poseidon_bn254.*)."""
    arr = np.load(os.path.join(HERE, "golden", "poseidon_bn254.npz"))
    with open(os.path.join(HERE, "golden", "poseidon_bn254.json")) as f:
        meta = json.load(f)["x%d" % w]
    to_int = lambda a: [sum(int(v) << (64 * i) for i, v in enumerate(row)) for row in a]
    rc, mds = to_int(arr["rc_x%d" % w]), to_int(arr["mds_x%d" % w])
    return OC.PoseidonParams(F.BN254.fr.p, w, meta["full_rounds"] // 2, meta["partial_rounds"], rc,
                             [mds[i * w:(i + 1) * w] for i in range(w)], meta["domain_tag"])


class Case:
    """values: the whole map; leaf[p], bits[p][k], sibs[p][k]: variable indices (ZERO allowed); bases[p]: first variable of
    path p; roots[p]: expected root value; root_vars[p]: the variable holding it; dense: the bases are base0 + p * height * S."""

    def __init__(self, cv, prm, height, values, leaf, bits, sibs, bases, roots, dense):
        self.cv, self.prm, self.height, self.values = cv, prm, height, values
        self.leaf, self.bits, self.sibs, self.bases, self.roots, self.dense = leaf, bits, sibs, bases, roots, dense
        self.per_hash = prm.gates_per_hash
        self.per_level = 6 + self.per_hash
        self.span = height * self.per_level
        self.hash_var_offset = self.per_hash - 1 - (prm.width - 2) * prm.width
        self.root_vars = [b + (height - 1) * self.per_level + 6 + self.hash_var_offset for b in bases]
        self.batch, self.n_vars = len(bases), len(values)

    def value(self, idx):
        return 0 if idx == ZERO else self.values[idx]

    def written(self):
        """Every variable index the launch writes."""
        return [v for b in self.bases for v in range(b, b + self.span)]


def _one_path(cs, prm, height, leaf_value, leaf_index, siblings):
    """poe_synthesize on `cs`, seeded with a fresh leaf variable.  Returns (leaf, bits, sibs, base, root value, root
    variable): the bits and the siblings are the 2 height variables PoECircuit::synthesize assigns first (binary.rs:49-66),
    the levels follow."""
    leaf = cs.assign_variable(leaf_value)
    first = len(cs.values)
    root = OC.poe_synthesize(cs, prm, leaf_index, siblings, cs.lt(leaf))
    bits = list(range(first, first + height))
    sibs = list(range(first + height, first + 2 * height))
    return leaf, bits, sibs, first + 2 * height, cs.value_of_lt(root), root.var


@functools.lru_cache(maxsize=None)
def build(cvname, w, shipped, height, batch, bits_mode, dense, zeros, seed=1):
    """One case.  bits_mode: "zeros", "ones" or "mixed" path bits.  dense: the paths' ranges follow each other without a
    gap (the path_base0 form: every path is synthesised on a composer of its own and the maps are laid out inputs first);
    otherwise ONE composer synthesises all the paths and the case is its map as it stands.  zeros: path 0's leaf and one
    sibling of the last path hold 0 and are given as ZKT_VARIABLE_ZERO."""
    cv = F.CURVES[cvname]
    p = cv.fr.p
    prm = shipped_params(w) if shipped else synthetic_params(cv, w)
    rnd = splitmix64(1000 * seed + 97 * w + 13 * height + batch)
    inputs = []
    for pth in range(batch):
        leaf_value, siblings = field_elems(p, next(rnd), 1)[0], field_elems(p, next(rnd), height)
        index = {"zeros": 0, "ones": (1 << height) - 1, "mixed": next(rnd) & ((1 << height) - 1)}[bits_mode]
        if bits_mode == "mixed" and height > 1 and index in (0, (1 << height) - 1):
            index = 1 if height == 2 else 0b101 & ((1 << height) - 1)
        if zeros and pth == 0:
            leaf_value = 0
        if zeros and pth == batch - 1:
            siblings[height // 2] = 0
        inputs.append((leaf_value, index, siblings))
    leaf, bits, sibs, bases, roots = [], [], [], [], []
    if not dense:
        cs = OC.Composer(cv, [1], 8)
        cs.assign_variable(field_elems(p, 5, 1)[0])          # something in front of the first leaf
        for leaf_value, index, siblings in inputs:
            lf, bt, sb, base, root, root_var = _one_path(cs, prm, height, leaf_value, index, siblings)
            leaf.append(lf)
            bits.append(bt)
            sibs.append(sb)
            bases.append(base)
            roots.append(root)
            assert root_var == base + (height - 1) * (6 + prm.gates_per_hash) + 6 + prm.gates_per_hash - 1 - (w - 2) * w
        assert cs.check_satisfied()
        values = list(cs.values)
    else:
        span = height * (6 + prm.gates_per_hash)
        n_in = 1 + 2 * height
        base0 = batch * n_in + 3
        values = [0] * (base0 + batch * span)
        values[batch * n_in:base0] = field_elems(p, 6, 3)     # a gap the launch must leave alone
        for k, (leaf_value, index, siblings) in enumerate(inputs):
            cs = OC.Composer(cv, [1], 8)
            lf, bt, sb, base, root, _ = _one_path(cs, prm, height, leaf_value, index, siblings)
            assert cs.check_satisfied() and (lf, base) == (0, n_in) and len(cs.values) == n_in + span
            values[k * n_in:(k + 1) * n_in] = cs.values[:n_in]
            values[base0 + k * span:base0 + (k + 1) * span] = cs.values[n_in:]
            leaf.append(k * n_in)
            bits.append([k * n_in + 1 + i for i in range(height)])
            sibs.append([k * n_in + 1 + height + i for i in range(height)])
            bases.append(base0 + k * span)
            roots.append(root)
    if zeros:
        assert values[leaf[0]] == 0 and values[sibs[-1][height // 2]] == 0
        leaf[0] = ZERO
        sibs[-1][height // 2] = ZERO
    return Case(cv, prm, height, values, leaf, bits, sibs, bases, roots, dense)


def derive_path(case, pth):
    """The height * S values of path `pth`, WITHOUT the composer: the select formulas (constraint_system/mod.rs:339-354,
    x = bit * a, y = (1 - bit) * b, z = x + y; merkle_proof selects (node, cur) on the left and (cur, node) on the right,
    binary.rs:23-24) and gadget_trace for hash_two(z_l, z_r).  Returns (values, root)."""
    p, prm = case.prm.p, case.prm
    cur = case.value(case.leaf[pth])
    out = []
    for k in range(case.height):
        b, s = case.value(case.bits[pth][k]), case.value(case.sibs[pth][k])
        assert b in (0, 1)
        x_l, y_l = b * s % p, (1 - b) * cur % p
        x_r, y_r = b * cur % p, (1 - b) * s % p
        z_l, z_r = (x_l + y_l) % p, (x_r + y_r) % p
        trace = OC.gadget_trace(prm, [z_l, z_r])
        out += [x_l, y_l, z_l, x_r, y_r, z_r] + trace
        cur = trace[case.hash_var_offset]
        assert cur == prm.native([z_l, z_r])
    return out, cur


# ---- the shapes of the device test ------------------------------------------------------------------------------------
def shapes(w):
    """(height, batch, bits_mode, dense, zeros) for one width: heights 1, 2, 3 and 7; batches 1, PER_WAVE + 1 (the last
    partial segment of a wavefront) and 4 PER_WAVE + 1 (of a block); both base forms; bits all 0, all 1 and mixed; a leaf
    and a sibling given as ZKT_VARIABLE_ZERO."""
    pw = per_wave(w)
    return [(3, 4 * pw + 1, "mixed", False, True), (2, pw + 1, "ones", True, False), (1, 1, "zeros", True, False),
            (7, pw + 1, "mixed", False, False), (2, 4 * pw + 1, "zeros", True, True)]
