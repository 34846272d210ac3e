"""Inputs of Plookup's combine_split (lookup/multiset.rs:103-146) at the shapes where the device split can go wrong:
key counts around its 1024-key scan chunks and its 8192-key LDS histogram, the zero key that the padding of t to n
adds (absent from the table, or already in it at a chosen place) and f vectors whose counts place odd keys on those
boundaries.  Shared by the CPU check of the oracle (test_coracle.py) and the device test (test_gpu_lookup.py).

Values are Montgomery words of random field elements below 2^252 (< r on both curves); the split only compares them."""
import numpy as np

# keys of the padded table t, the zero key included (plus n itself at each n)
KEY_COUNTS = (1, 2, 1023, 1024, 1025, 2047, 2048, 2049, 8191, 8192, 8193)
ZERO_AT = ("absent", "first", "middle", "last")
F_KINDS = ("zeros", "one_key", "each_once", "odd_straddle", "uniform")
CHUNK_EDGES = (1024, 2048, 8192)   # k_lookup_starts' chunks of 1024 keys; the LDS histogram holds 8192


def key_counts(n: int):
    return [k for k in KEY_COUNTS if k <= n] + ([n] if n not in KEY_COUNTS else [])


def random_values(rng, count: int, avoid=None) -> np.ndarray:
    """count distinct nonzero values, none of them a row of `avoid`."""
    v = np.frombuffer(rng.bytes(32 * count), dtype=np.uint64).reshape(count, 4).copy()
    v[:, 3] &= np.uint64((1 << 60) - 1)
    rows = {r.tobytes() for r in v}
    assert len(rows) == count and not (v == 0).all(axis=1).any()
    if avoid is not None:
        assert not rows & {r.tobytes() for r in np.asarray(avoid, dtype=np.uint64).reshape(-1, 4)}
    return v


def make_table(rng, nkeys: int, zero_at: str) -> np.ndarray:
    """The table (insertion order) whose padding to n gives `nkeys` keys: nkeys - 1 values when 0 is absent (the padding
    appends the zero key), nkeys values with 0 at the first / middle / last place otherwise."""
    if zero_at == "absent":
        return random_values(rng, nkeys - 1)
    vals = random_values(rng, nkeys - 1)
    pos = {"first": 0, "middle": nkeys // 2, "last": nkeys - 1}[zero_at]
    return np.insert(vals, pos, 0, axis=0)


def padded_keys(table: np.ndarray) -> np.ndarray:
    """Keys in the order combine_split walks them: the table's, then the zero key if the padding added it."""
    if table.shape[0] and (table == 0).all(axis=1).any():
        return table
    return np.vstack([table, np.zeros((1, 4), dtype=np.uint64)])


def pad(table: np.ndarray, n: int) -> np.ndarray:
    """t padded with zeros to n (lookup/table.rs:52-61): what the oracle is handed."""
    t = np.zeros((n, 4), dtype=np.uint64)
    t[:table.shape[0]] = table
    return t


def make_f(rng, n: int, keys: np.ndarray, kind: str) -> np.ndarray:
    """n looked-up values, all among `keys`.
    zeros: every table key keeps count 1 (odd): the parity alternates on every key.
    one_key: one nonzero key (the middle one) hit n times.
    each_once: every key hit exactly once, the rest of f zeros.
    odd_straddle: table keys hit once (even counts) except runs around the chunk edges (and the LDS limit) hit 0 or 2
      times (odd counts): three odd keys end a chunk, so the next chunk starts on the other half.
    uniform: n draws among the keys."""
    nk = keys.shape[0]
    if kind == "zeros":
        return np.zeros((n, 4), dtype=np.uint64)
    if kind == "one_key":
        nz = np.flatnonzero(~(keys == 0).all(axis=1))
        k = nz[np.searchsorted(nz, nk // 2) % nz.shape[0]] if nz.shape[0] else 0
        return np.repeat(keys[k:k + 1], n, axis=0)
    if kind == "uniform":
        return keys[rng.integers(0, nk, size=n)].copy()
    hits = np.ones(nk, dtype=np.int64)
    if kind == "odd_straddle":
        for e in CHUNK_EDGES:
            for j, h in zip(range(e - 3, e + 3), (0, 2, 0, 2, 0, 2)):
                if 0 <= j < nk:
                    hits[j] = h
    elif kind != "each_once":
        raise ValueError(kind)
    assert hits.sum() <= n
    f = np.zeros((n, 4), dtype=np.uint64)
    f[:hits.sum()] = np.repeat(keys, hits, axis=0)
    return f[rng.permutation(n)]


def cases(rng, n: int, counts=None, zero_at=ZERO_AT, kinds=F_KINDS):
    """(label, table, [f per kind]) for every key count and zero placement that a table of < n values allows."""
    for nk in (key_counts(n) if counts is None else counts):
        for z in zero_at:
            if z != "absent" and nk >= n:     # table_len = nk would reach n
                continue
            if z != "absent" and nk < 1:
                continue
            table = make_table(rng, nk, z)
            keys = padded_keys(table)
            assert keys.shape[0] == nk
            yield "keys=%d zero=%s" % (nk, z), table, [(k, make_f(rng, n, keys, k)) for k in kinds]
