"""Host-side mirror of the witness completion (include/zkt_plonk.h, zkt_witness_plan_* / zkt_witness_complete*).

``WitnessPlan`` plans the circuit loaded in a context under a wiring and its public-input positions: which variables the
caller supplies (``kinds() == FREE``: for a circuit written against the reference's composer, its direct ``assign_variable``
calls -- less the two that ``should_be_zero_with_output`` makes when the plan is made with ``rules=RULE_IS_ZERO``) and the
schedule by which the device fills in every variable that a gate defines.  ``complete_dev`` completes maps that
are resident in HBM, enqueue only, so a ``prove`` with ``wires_on_device`` follows without a wait; ``complete`` is the
host-pointer form.  All values are (count, 4) uint64 Montgomery limbs.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

from ._lib import Context

UNUSED, FREE, OUT, RIGHT, ZINV, ZFLAG = 0, 1, 2, 3, 4, 5      # zkt_witness_plan_kinds (4, 5: rule Z's inverse y and flag z)
RULE_IS_ZERO = 1                                             # ZKT_WITNESS_RULE_IS_ZERO


class WitnessPlan:
    """zkt_witness_plan over the circuit loaded in ``ctx``.  The plan owns its device memory and outlives a circuit reload;
    any context of the same curve and device (a fork, say) may be passed to the completion calls.  ``rules=RULE_IS_ZERO``
    adds rule Z (zkt_witness_plan_create_ex): a row (x, y, z) with q_m, q_o != 0 and q_l = q_r = 0 on unseen y and z, followed
    by a row asserting x z = 0, defines y = -q_c / (q_m x) (0 at x = 0) and z = -q_c / q_o at x = 0 (0 otherwise) -- the
    composer's ``should_be_zero_with_output`` / ``should_eq_with_output``; ``info()["n_pairs"]`` counts such pairs."""

    def __init__(self, ctx: Context, w_l, w_r, w_o, n_vars: int, pi_pos: Sequence[int] = (), n_rows: Optional[int] = None,
                 rules: int = 0):
        self.ctx, self.n_vars, self.n_pi = ctx, n_vars, len(pi_pos)
        self._p = ctx.witness_plan_create(w_l, w_r, w_o, n_vars, pi_pos, n_rows, rules)

    def close(self):
        if self._p:
            self.ctx.witness_plan_free(self._p)
            self._p = None

    @property
    def handle(self) -> int:
        return self._p

    def info(self) -> dict:
        return self.ctx.witness_plan_info(self._p)

    def kinds(self) -> np.ndarray:
        """Per variable: UNUSED (on no wire), FREE, OUT (rule O), RIGHT (rule R), ZINV / ZFLAG (rule Z's y / z)."""
        return self.ctx.witness_plan_kinds(self._p, self.n_vars)

    def complete_dev(self, d_variables: int, stride: Optional[int] = None, batch: int = 1, d_out_pi: int = 0, ctx: Optional[Context] = None):
        (ctx or self.ctx).witness_complete_enqueue(self._p, d_variables, self.n_vars if stride is None else stride, batch, d_out_pi)

    def status(self, batch: int = 1, ctx: Optional[Context] = None):
        """[(unsolvable rows, the smallest such row or None)] per witness; synchronises and clears."""
        return (ctx or self.ctx).witness_complete_status(self._p, batch)

    def complete(self, variables, ctx: Optional[Context] = None):
        """Host maps (batch, stride, 4) or (stride, 4) -> (completed maps, public inputs (batch, n_pi, 4), status)."""
        return (ctx or self.ctx).witness_complete(self._p, variables, self.n_pi)

    def split(self, wide_min_rows: int):
        """zkt_debug_witness_plan_split (tests, sweeps): 0 = the policy."""
        self.ctx.debug_witness_plan_split(self._p, wide_min_rows)
