"""Host-side mirror of the reference's Poseidon hasher for the prover's witness.

``PoseidonGadget`` ~ ``PoseidonRef<ConstraintSystem, PlonkSpecRef, G, WIDTH>`` (plonk-hashing/src/hasher/poseidon/spec.rs:
223-375) seen from the PROVING composer: ``hash(cs, inputs)`` assigns ``vars_per_hash`` fresh variables per call
(constraint_system/arithmetic.rs:19,79 via spec.rs:174-219).  The caller keeps the bookkeeping the composer does -- where a
call's variables start in ``VariableMap::values`` and which variables it was fed -- and ``fill`` has the device compute all
of them at once (zkt_poseidon_gadget_witness_dev), straight into the variable map ``zkt_prove`` gathers its wires from.
``merkle_path`` records a whole ``merkle_proof`` (plonk-hashing/src/merkle/binary.rs:8-30): a chain of hashes fed by
conditional_selects on the level below, which the device walks in one launch (zkt_poseidon_merkle_path_witness_dev).
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

from ._lib import Context

VARIABLE_ZERO = 0xFFFFFFFF   # ZKT_VARIABLE_ZERO = Variable::Zero (constraint_system/variable.rs:10-15)


class PoseidonGadget:
    """PoseidonConstants resident in HBM (zkt_poseidon_load) + the record of hash calls whose variables are to be made.
    All arrays are (count, 4) uint64 Montgomery limbs."""

    def __init__(self, ctx: Context, width: int, half_full_rounds: int, partial_rounds: int, round_constants, mds, domain_tag):
        self.ctx, self.width = ctx, width
        self._h = ctx.poseidon_load(width, half_full_rounds, partial_rounds, round_constants, mds, domain_tag)
        self.vars_per_hash = ctx.poseidon_gadget_vars_per_hash(self._h)
        # elements[1] after the last product_mds (spec.rs:315): the running sum j = 1, i = W - 1
        self.hash_var_offset = self.vars_per_hash - 1 - (width - 2) * width
        self.vars_per_level = ctx.merkle_path_vars_per_level(self._h)      # 6 select variables + the hash
        self.calls: List[Tuple[int, Sequence[int]]] = []
        self.paths: List[Tuple[int, int, Tuple[int, ...], Tuple[int, ...]]] = []
        self._staged = []
        self._staged_paths = []

    def close(self):
        if self._h:
            self.unstage()
            self.ctx.poseidon_free(self._h)
            self._h = None

    def hash(self, first_variable: int, input_variables: Sequence[int]) -> int:
        """Records one FieldHasher::hash call whose variables occupy [first_variable, first_variable + vars_per_hash) and
        whose inputs are the plain variables `input_variables` (VARIABLE_ZERO allowed).  Returns the variable holding the
        hash."""
        if len(input_variables) > self.width - 1:
            raise ValueError("Poseidon Error: FullBuffer")      # spec.rs:253-255
        self.calls.append((first_variable, tuple(input_variables)))
        return first_variable + self.hash_var_offset

    def merkle_path(self, first_variable: int, leaf_var: int, bit_vars: Sequence[int], sibling_vars: Sequence[int]) -> int:
        """Records one merkle_proof call (binary.rs:8-30) of height len(bit_vars) whose variables -- per level the six of
        the two conditional_selects, then the hash's -- occupy [first_variable, first_variable + height * vars_per_level),
        fed by the plain variables `leaf_var`, `bit_vars` and `sibling_vars` (level 0 first; VARIABLE_ZERO allowed).  Returns
        the variable holding the root."""
        if self.width < 3:
            raise ValueError("Poseidon Error: FullBuffer")      # hash_two on width 2, spec.rs:253-255
        if len(bit_vars) != len(sibling_vars) or not len(bit_vars):
            raise ValueError("a Merkle path has one bit and one sibling per level, and at least one level")
        self.paths.append((first_variable, leaf_var, tuple(bit_vars), tuple(sibling_vars)))
        return first_variable + (len(bit_vars) - 1) * self.vars_per_level + 6 + self.hash_var_offset

    def _check_paths(self):
        """The paths run in ONE launch after every hash call: nothing a path makes may feed a hash call, and no leaf, bit or
        sibling may be a variable a path makes.  A C caller who needs either orders the launches itself."""
        import bisect
        spans = sorted((base, base + len(bits) * self.vars_per_level) for base, _, bits, _ in self.paths)
        starts = [lo for lo, _ in spans]

        def made_by_a_path(v):
            at = bisect.bisect_right(starts, v) - 1
            return v != VARIABLE_ZERO and at >= 0 and v < spans[at][1]

        for _, ins in self.calls:
            if any(made_by_a_path(v) for v in ins):
                raise ValueError("a hash call is fed by a variable a Merkle path makes: the paths run after every hash call")
        for _, leaf, bits, sibs in self.paths:
            if any(made_by_a_path(v) for v in (leaf,) + bits + sibs):
                raise ValueError("a Merkle path's leaf, bit or sibling is a variable a Merkle path makes: all paths run in one launch")

    def levels(self) -> List[List[int]]:
        """Calls grouped by dependency depth: a call whose input is a variable another call makes (the leaf hash of
        circuits/src/withdraw.rs:91-94 takes the commitment hash) must run in a later launch than that call."""
        import bisect
        order = sorted(range(len(self.calls)), key=lambda k: self.calls[k][0])
        bases = [self.calls[k][0] for k in order]
        depth = [-1] * len(self.calls)

        def maker(v):
            at = bisect.bisect_right(bases, v) - 1
            return order[at] if at >= 0 and v < bases[at] + self.vars_per_hash else None

        def depth_of(k, seen=()):
            if depth[k] < 0:
                if k in seen:
                    raise ValueError("Poseidon calls feed each other in a cycle")
                deps = [maker(v) for v in self.calls[k][1] if v != VARIABLE_ZERO]
                depth[k] = 1 + max([depth_of(d, seen + (k,)) for d in deps if d is not None], default=-1)
            return depth[k]

        out: List[List[int]] = []
        for k in range(len(self.calls)):
            d = depth_of(k)
            while len(out) <= d:
                out.append([])
            out[d].append(k)
        return out

    def stage(self):
        """Uploads the recorded calls' trace bases and input indices (structure of the circuit: the same for every witness).
        An absent input and an input that is Variable::Zero are the same LTVariable (Zero, 1, 0) (spec.rs:239-245 reset /
        variable.rs:62-64), so calls of every arity go out together, as launches of arity width - 1 padded with
        VARIABLE_ZERO: ONE launch per dependency level (`levels`), in order on the context's stream.  The recorded Merkle
        paths follow as one launch per height (`_check_paths` refuses what that order cannot serve)."""
        self.unstage()
        arity = self.width - 1
        for lvl in self.levels():
            bases = np.array([self.calls[k][0] for k in lvl], dtype=np.uint32)
            idx = np.full((len(lvl), max(arity, 1)), VARIABLE_ZERO, dtype=np.uint32)
            for row, k in enumerate(lvl):
                ins = self.calls[k][1]
                idx[row, :len(ins)] = ins
            d_base, d_idx = self.ctx.alloc(bases.nbytes), self.ctx.alloc(idx.nbytes)
            self.ctx.upload(d_base, bases)
            self.ctx.upload(d_idx, idx)
            self._staged.append((arity, len(lvl), d_base, d_idx))
        # the recorded paths: one launch per height
        self._check_paths()
        for height in sorted({len(bits) for _, _, bits, _ in self.paths}):
            group = [pth for pth in self.paths if len(pth[2]) == height]
            arrays = [np.array([pth[0] for pth in group], dtype=np.uint32), np.array([pth[1] for pth in group], dtype=np.uint32),
                      np.array([pth[2] for pth in group], dtype=np.uint32), np.array([pth[3] for pth in group], dtype=np.uint32)]
            d_arrays = []
            for arr in arrays:
                d = self.ctx.alloc(arr.nbytes)
                self.ctx.upload(d, arr)
                d_arrays.append(d)
            self._staged_paths.append((height, len(group), d_arrays))

    def unstage(self):
        for _, _, d_base, d_idx in getattr(self, "_staged", []):
            self.ctx.free(d_base)
            if d_idx:
                self.ctx.free(d_idx)
        for _, _, d_arrays in getattr(self, "_staged_paths", []):
            for d in d_arrays:
                self.ctx.free(d)
        self._staged = []
        self._staged_paths = []

    def fill(self, d_variables: int, n_vars: int, check: bool = True) -> int:
        """Enqueues the gadget kernel for every recorded call on the context's stream: ONE launch per dependency level
        (`levels`: a call fed by another call's output runs in a later launch), then the recorded Merkle paths, ONE launch
        per height.  Inputs that no call and no path makes must already be in the map at d_variables.  Returns the number
        of launches.  With check=True synchronises and raises when an index lay outside the map or a path's bit was not 0
        or 1."""
        if not getattr(self, "_staged", None) and not getattr(self, "_staged_paths", None):
            self.stage()
        for arity, count, d_base, d_idx in self._staged:
            self.ctx.poseidon_gadget_witness_dev(self._h, count, arity, d_variables, n_vars, d_input_vars=d_idx if arity else 0,
                                                 d_trace_base=d_base)
        for height, count, (d_base, d_leaf, d_bits, d_sibs) in self._staged_paths:
            self.ctx.poseidon_merkle_path_witness_dev(self._h, count, height, d_variables, n_vars, d_leaf, d_bits, d_sibs,
                                                      d_path_base=d_base)
        if check:
            self.ctx.poseidon_gadget_check(self._h)
        return len(self._staged) + len(self._staged_paths)
