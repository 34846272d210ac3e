"""The sigma permutation of a wiring (permutation/mod.rs:76-177), restated in numpy, and the raw index vectors the GPU
tests feed to zkt_circuit_sigma_dev.  tests/test_sigma_rule_host.py pins the restatement against the oracle's
ConstraintSystem.sigma_mappings; tests/test_gpu_sigma.py takes its expected values from here."""
import numpy as np

ZERO = 0xFFFFFFFF          # ZKT_VARIABLE_ZERO
KS = (1, 7, 13)            # permutation/constants.rs: the coset representatives of the three wire columns


def sigma_targets(w_l, w_r, w_o, n):
    """(n, 3) int64: entry [g, col] = the wire 3 g' + col' that wire (col, g) maps to.  A stable argsort of the
    gate-major keys puts every variable's wires side by side in insertion order; each maps to its neighbour, the last
    of a run to the first; rows >= len(w_l) map to themselves."""
    w = np.stack([np.asarray(c, dtype=np.int64) for c in (w_l, w_r, w_o)], axis=1).reshape(-1)
    sig = np.arange(3 * n, dtype=np.int64)
    if w.size:
        order = np.argsort(w, kind="stable")
        ws = w[order]
        first = np.r_[True, ws[1:] != ws[:-1]]
        last = np.r_[first[1:], True]
        nxt = np.roll(order, -1)
        nxt[last] = order[first][np.cumsum(first)[last] - 1]
        sig[order] = nxt
    return sig.reshape(n, 3)


def sigma_values(p, log_n, targets, root):
    """Three lists of n Python integers k_col' * root^g' mod p for the targets of sigma_targets (root: the domain's generator)."""
    n = 1 << log_n
    roots = [1] * n
    for i in range(1, n):
        roots[i] = roots[i - 1] * root % p
    kroots = [[k * x % p for x in roots] for k in KS]
    row, col = np.divmod(targets, 3)
    return [[kroots[c][r] for r, c in zip(row[:, j].tolist(), col[:, j].tolist())] for j in range(3)]


def to_index(ws, zero_var):
    """A ConstraintSystem wire list (zero_var = its Variable::Zero) as the uint32 vector of the C ABI."""
    return np.array([ZERO if v == zero_var else v for v in ws], dtype=np.uint32)


def _case_b(rng):
    rows = 8191
    w = np.empty((rows, 3), dtype=np.uint32)
    pool = np.repeat(np.arange(1, 6000, dtype=np.uint32), rng.integers(1, 5, size=5999))   # one to four occurrences each
    w[:] = rng.choice(pool, size=(rows, 3))
    heavy = rng.random((rows, 3))
    w[heavy < 0.2] = 0              # variable 0: about 5 000 positions over all three columns, several workgroups apart
    w[heavy > 0.85] = ZERO          # and a heavy Variable::Zero run
    return dict(log_n=13, n_vars=6000, w=w)


def _case_e(rng):
    rows = 3000
    w = rng.integers(0, 70000, size=(rows, 3)).astype(np.uint32)    # both sides of 65 536, most variables unwired
    w[::7, 0] = 65535
    w[::11, 1] = 65536
    w[::13, 2] = 69999
    return dict(log_n=12, n_vars=70000, w=w)


def _case_f(rng):
    rows = 1000
    n_vars = (1 << 24) + 3
    special = np.array([0, 255, 256, 65535, 65536, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, (1 << 24) + 2, ZERO], dtype=np.uint32)
    w = rng.integers(0, n_vars, size=(rows, 3)).astype(np.uint32)
    pick = rng.random((rows, 3)) < 0.5
    w[pick] = rng.choice(special, size=int(pick.sum()))
    return dict(log_n=10, n_vars=n_vars, w=w)


def raw_cases():
    """name -> dict(log_n, n_vars, w (n_rows, 3) uint32): index vectors that need satisfy no circuit, shaped where a
    sort can go wrong.  Deterministic."""
    rng = np.random.default_rng(0x51C3A)
    cases = {}
    cases["a_below_one_wave"] = dict(log_n=3, n_vars=4, w=rng.integers(0, 4, size=(5, 3)).astype(np.uint32))
    cases["b_long_runs_odd_rows"] = _case_b(rng)
    cases["c_all_distinct_no_padding"] = dict(log_n=12, n_vars=3 << 12, w=rng.permutation(3 << 12).astype(np.uint32).reshape(-1, 3))
    cases["d_one_variable"] = dict(log_n=12, n_vars=9, w=np.full((3001, 3), 5, dtype=np.uint32))
    cases["e_third_digit"] = _case_e(rng)
    cases["f_fourth_digit"] = _case_f(rng)
    cases["g_no_rows"] = dict(log_n=4, n_vars=7, w=np.zeros((0, 3), dtype=np.uint32))
    return cases
