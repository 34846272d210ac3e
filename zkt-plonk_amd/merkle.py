"""Host-side mirror of the reference's note tree (gadgets/src/merkle_tree.rs:39-111) kept on the device.

``MerkleTree`` ~ ``MerkleTree<F, G, H, HEIGHT>``: ``append`` is ``add_leaf`` for a batch of leaves (hashed level by level on
the device), ``root`` is ``root``, ``paths`` is ``merkle_path``; ``paths_to_variables`` writes the same siblings (and the
position bits) into the variable map ``zkt_poseidon_merkle_path_witness_dev`` reads them from.  All arrays are (count, 4)
uint64 Montgomery limbs.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

from ._lib import Context


class MerkleTree:
    """zkt_merkle_tree over a loaded Poseidon handle (``Context.poseidon_load`` / ``PoseidonGadget._h``), which is borrowed:
    free it after the tree."""

    def __init__(self, ctx: Context, poseidon_handle: int, height: int, capacity: int):
        self.ctx, self.height, self.capacity = ctx, height, capacity
        self._t = ctx.merkle_tree_create(poseidon_handle, height, capacity)

    @classmethod
    def load_file(cls, ctx: Context, poseidon_handle: int, height: int, capacity: int, path: str):
        """zkt_merkle_tree_load_file: a reference --merkle-tree file -> (the tree rebuilt from its leaves, the report on how
        the file's other nodes and root compare with it: entries, mismatches, first_layer, first_idx, root_matches)."""
        t = cls.__new__(cls)
        t.ctx, t.height, t.capacity = ctx, height, capacity
        t._t, report = ctx.merkle_tree_load_file(poseidon_handle, height, capacity, path)
        return t, report

    def save_file(self, path: str):
        """zkt_merkle_tree_save_file: the tree as the reference CLI's --merkle-tree file (MerkleTreeStore)."""
        self.ctx.merkle_tree_save_file(self._t, path)

    def close(self):
        if self._t:
            self.ctx.merkle_tree_free(self._t)
            self._t = None

    @property
    def handle(self) -> int:
        return self._t

    @property
    def count(self) -> int:
        return self.ctx.merkle_tree_info(self._t)[1]

    def append(self, leaves=None, d_leaves: int = 0, m: Optional[int] = None) -> int:
        """add_leaf for every leaf, in order -> index of the first.  Host leaves (synchronises), or a device pointer and a
        count (enqueue only)."""
        if d_leaves:
            return self.ctx.merkle_tree_append_dev(self._t, d_leaves, m)
        return self.ctx.merkle_tree_append(self._t, leaves)

    def root(self) -> np.ndarray:
        return self.ctx.merkle_tree_root(self._t)

    def layer(self, layer: int, first: int = 0, n: Optional[int] = None) -> np.ndarray:
        """The stored nodes (layer, first .. first + n); n defaults to all that follow `first`."""
        if n is None:
            count = self.count
            n = ((count - 1 >> layer) + 1 if count else 0) - first
        return self.ctx.merkle_tree_layer(self._t, layer, first, n)

    def paths(self, indices: Sequence[int]) -> np.ndarray:
        """merkle_path of every index: (k, height, 4), level 0 first."""
        return self.ctx.merkle_tree_paths(self._t, indices)

    def paths_to_variables(self, indices: Sequence[int], d_variables: int, n_vars: int, sibling_var0: Sequence[int],
                           bit_var0: Optional[Sequence[int]] = None):
        """Path p's siblings to d_variables[sibling_var0[p] + layer], its bits to d_variables[bit_var0[p] + layer]; enqueue only."""
        self.ctx.merkle_tree_paths_to_variables_dev(self._t, indices, d_variables, n_vars, sibling_var0, bit_var0)

    def split(self, wide_min_parents: int):
        """zkt_debug_merkle_tree_split (tests): 1 = every level wide, 2^31 - 1 = every level in the tail, 0 = the policy."""
        self.ctx.debug_merkle_tree_split(self._t, wide_min_parents)
