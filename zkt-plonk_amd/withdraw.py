"""Host-side mirror of the withdraw circuit as a library component (include/zkt_plonk.h, "(5) The withdraw circuit").

``WithdrawCircuit`` ~ ``WithdrawCircuit<F, u64, G, H, INPUTS, HEIGHT>`` (circuits/src/withdraw.rs:57-150): ``setup`` is the
CLI's ``Compile`` (bin/src/main.rs:90-112), ``witness`` + ``prepare`` + ``Context.prove_prepared`` its ``ProveWithdraw``
(bin/src/main.rs:190-300).  The rows, the setup vectors and the variable maps are made on the device; requests are
dictionaries of (count, 4) uint64 Montgomery limbs and plain integers (``Context.withdraw_witness``).
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

from ._lib import Context


class WithdrawCircuit:
    """zkt_withdraw.  params: (width, half_full, partial, round_constants, mds, domain_tag), constants in Montgomery words."""

    def __init__(self, ctx: Context, params, inputs: int, height: int):
        self.ctx = ctx
        self._w = ctx.withdraw_create(params, inputs, height)
        self.info = ctx.withdraw_get_info(self._w)
        self.pi_pos = ctx.withdraw_pi_pos(self._w)
        self.n_vars, self.n_gates, self.n_pi = self.info["n_vars"], self.info["n_gates"], self.info["n_pi"]

    def close(self):
        if self._w:
            self.ctx.withdraw_free(self._w)
            self._w = None

    @property
    def handle(self) -> int:
        return self._w

    @property
    def poseidon_handle(self) -> int:
        """The circuit's own Poseidon tables, borrowed: what a MerkleTree feeding ``witness`` must be bound to."""
        return self.ctx.withdraw_poseidon(self._w)

    def rows(self, selectors: bool = True, wires: bool = True):
        """(q_m, q_l, q_r, q_o, q_c, q_lookup), (w_l, w_r, w_o): regenerated on the device, downloaded."""
        return self.ctx.withdraw_rows(self._w, selectors, wires)

    def setup(self, log_n: int, table_size: int):
        """proof_system::setup of the circuit -> (the ten commitments, is_infinity); the circuit stays loaded."""
        return self.ctx.withdraw_setup(self._w, log_n, table_size)

    def witness(self, requests: Sequence[dict], d_variables: int, stride: Optional[int] = None, tree=None, want_pi: bool = True,
                want_status: bool = True):
        """The variable maps of the requests at d_variables (device), `stride` scalars apart -> (public inputs
        (batch, n_pi, 4), [bad_paths]); with neither wanted the call only enqueues.  tree: a MerkleTree for requests whose
        siblings or root are None."""
        return self.ctx.withdraw_witness(self._w, requests, d_variables, self.n_vars if stride is None else stride,
                                         tree.handle if tree is not None else 0, want_pi, want_status)

    def prove(self, requests: Sequence[dict], d_variables: int, slots: int, identifiers_set, blinders, stride: Optional[int] = None, tree=None,
              transcript_kind: str = "merlin", label: str = "ZKT Plonk", verify_key=None, append: bool = False):
        """zkt_withdraw_prove, the CLI's ProveWithdraw for every request in one call: witness, proof, the CLI's own check of
        the proof (verify_key = (g, h, beta_h)) and the new leaves appended to `tree` -> ([proof bytes], public inputs
        (batch, n_pi, 4), [{code, bad_paths, verified, new_leaf_index}]).  d_variables: `slots` maps, `stride` scalars apart."""
        return self.ctx.withdraw_prove(self._w, requests, d_variables, self.n_vars if stride is None else stride, slots, identifiers_set,
                                       blinders, tree.handle if tree is not None else 0, transcript_kind, label, verify_key, append)

    def prepare(self, d_variables: int, stride: int, b: int, table, pi_vals, blinders):
        """zkt_prove_inputs of request b over the device wiring, for Context.prove_prepared / check_witness."""
        return self.ctx.withdraw_prepare(self._w, d_variables, stride, b, table, np.asarray(pi_vals, dtype=np.uint64), blinders)
