"""Times the note tree on the device (zkt_merkle_tree_append_dev, zkt_merkle_tree_paths_to_variables_dev) against what a
caller could do with this library before it had a tree: one zkt_poseidon_hash_batch_dev launch per level over layer arrays
of its own.

    python tools/merkle_tree_timing.py [--ms 1,8,1024,65536,1048576] [--reps 7] [--sweep-m 1024]

BN254 x5 (the withdraw circuit's tables), height 64.  Every figure is a host clock around calls that end in a stream
synchronise, the median of --reps after one warm-up of the same shape, the two sides of a shape one after the other in one run.
  tree       zkt_merkle_tree_append_dev of m leaves that are already in HBM, on a fresh tree or on one that holds 2^20 + 1
             leaves; "scope" is the same call by the library's own "merkle_append" HIP-event scope
  baseline   the same append as 64 dependent zkt_poseidon_hash_batch_dev launches (children of consecutive parents are a
             contiguous batch x 2 input).  The leaves are already in layer 0 and the empty fillers already in place: neither
             their copy nor the patches are charged to it.  What IS in its figure besides the kernels: the host's 64 calls
             through ctypes (a C caller pays 64 launches too, only cheaper ones); the tool prints what one such call costs
             the host, so that 64 of them can be set against the figure
  sweep      the append of --sweep-m leaves under zkt_debug_merkle_tree_split(T): levels with >= T parents wide, the rest tail
  paths      zkt_merkle_tree_paths_to_variables_dev for 8 paths, bits included
The roots of the two sides are compared after every shape."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import zkt_plonk_amd as z
import withdraw_workload as WW

P_BN254 = 21888242871839275222246405745257275088548364400416034343698204186575808495617
R = 1 << 256
HEIGHT = 64
PREFILL = (1 << 20) + 1
INT_MAX = 2 ** 31 - 1


def _mont(ctx, vals):
    arr = np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(-1, 4)
    r2 = np.frombuffer((R * R % P_BN254).to_bytes(32, "little"), dtype=np.uint64)
    return ctx.debug_fr_mul(arr, np.tile(r2, (len(vals), 1)))


def _leaves(n, seed):
    """n canonical scalars as Montgomery words (any value below 2^253 is one)"""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
    x[:, 3] >>= np.uint64(3)
    return x


def _wall(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


class Baseline:
    """Layer arrays of the caller's own and one hash launch per level."""

    def __init__(self, ctx, h, capacity):
        self.ctx, self.h = ctx, h
        self.len = [max(1, ((capacity - 1) >> L) + 1) + 2 for L in range(HEIGHT + 1)]     # room for the filler
        self.off = np.concatenate([[0], np.cumsum(self.len)]).tolist()
        self.d = ctx.alloc(32 * self.off[-1])
        # the empty-subtree values, by the same launches (set-up, not timed)
        d_e = ctx.alloc(32 * (HEIGHT + 2))
        ctx.upload(d_e, np.zeros((2, 4), np.uint64))
        self.empties = [np.zeros((1, 4), np.uint64)]
        for L in range(HEIGHT - 1):
            ctx.poseidon_hash_batch_dev(h, d_e, 1, 2, d_e + 64)
            e = ctx.download(d_e + 64, (1, 4))
            self.empties.append(e)
            ctx.upload(d_e, np.concatenate([e, e]))
        ctx.free(d_e)

    def ptr(self, L, idx):
        return self.d + 32 * (self.off[L] + idx)

    def put_leaves(self, s, leaves):
        self.ctx.upload(self.ptr(0, s), leaves)

    def patch(self, s, m):
        """The empty fillers of the append of m leaves at s, put in place AHEAD of the timed window (the slot right of the
        last child of a level is not written by the launches, so the patch survives every repetition): the baseline is
        charged nothing for them."""
        last = s + m - 1
        for L in range(HEIGHT):
            if not (last >> L) & 1:
                self.ctx.upload(self.ptr(L, (last >> L) + 1), self.empties[L])

    def append(self, s, m):
        """The timed part: 64 dependent launches and one synchronise."""
        last = s + m - 1
        for L in range(HEIGHT):
            p_lo, p_hi = s >> (L + 1), last >> (L + 1)
            self.ctx.poseidon_hash_batch_dev(self.h, self.ptr(L, 2 * p_lo), p_hi - p_lo + 1, 2, self.ptr(L + 1, p_lo))
        self.ctx.synchronize()

    def root(self):
        return self.ctx.download(self.ptr(HEIGHT, 0), (1, 4))[0]

    def close(self):
        self.ctx.free(self.d)


def _fresh_tree(ctx, h, d_prefill, prefill, room, split=0):
    t = ctx.merkle_tree_create(h, HEIGHT, max(1, prefill + room))
    if prefill:
        ctx.merkle_tree_append_dev(t, d_prefill, prefill)
    ctx.debug_merkle_tree_split(t, split)
    ctx.synchronize()
    return t


def _time_tree(ctx, h, d_prefill, prefill, d_leaves, m, reps, split=0):
    """-> (median wall ms, median scope ms, root) of one append of m leaves; a fresh tree per repetition"""
    wall, scope, root = [], [], None
    for r in range(reps + 1):
        t = _fresh_tree(ctx, h, d_prefill, prefill, m, split)
        c0, ms0 = ctx.profile_get("merkle_append")

        def run():
            ctx.merkle_tree_append_dev(t, d_leaves, m)
            ctx.synchronize()

        w = _wall(run)
        c1, ms1 = ctx.profile_get("merkle_append")
        assert c1 == c0 + 1
        if r:
            wall.append(w)
            scope.append(ms1 - ms0)
        root = ctx.merkle_tree_root(t)
        ctx.merkle_tree_free(t)
    return float(np.median(wall)), float(np.median(scope)), root


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ms", default="1,8,1024,65536,1048576")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sweep-m", default="1024,65536")
    ap.add_argument("--sweep", default="2,4,8,16,32,64,128,256,512")
    a = ap.parse_args()
    ms = [int(x) for x in a.ms.split(",")]
    ctx = z.Context("bn254", 0)
    ctx.profile_enable(True)
    hs = WW.reference_hasher(P_BN254, 5)
    h = ctx.poseidon_load(hs.width, hs.half_full, hs.partial, _mont(ctx, hs.rc), _mont(ctx, [x for r in hs.mds for x in r]),
                          _mont(ctx, [hs.tag])[0])
    prefill, leaves = _leaves(PREFILL, 1), _leaves(max(ms), 2)
    d_prefill, d_leaves = ctx.alloc(prefill.nbytes), ctx.alloc(leaves.nbytes)
    ctx.upload(d_prefill, prefill)
    ctx.upload(d_leaves, leaves)
    print("# note tree on the device; BN254 x5, height %d; ms, median of %d after one warm-up" % (HEIGHT, a.reps), flush=True)
    print("# %-10s %9s | %10s %10s | %10s | %8s" % ("tree holds", "m", "tree wall", "tree scope", "baseline", "factor"), flush=True)
    for held in (0, PREFILL):
        base = Baseline(ctx, h, held + max(ms))
        if held:
            base.put_leaves(0, prefill)
            base.patch(0, held)
            base.append(0, held)
        for m in ms:
            base.put_leaves(held, leaves[:m])
            base.patch(held, m)
            t_tree, t_scope, root = _time_tree(ctx, h, d_prefill, held, d_leaves, m, a.reps)
            t_base = []
            for r in range(a.reps + 1):
                w = _wall(lambda: base.append(held, m))
                if r:
                    t_base.append(w)
            t_base = float(np.median(t_base))
            assert np.array_equal(root, base.root()), "the tree's root differs from the baseline's"
            print("  %-10d %9d | %10.3f %10.3f | %10.3f | %7.2fx" % (held, m, t_tree, t_scope, t_base, t_base / t_tree), flush=True)
            if m == 1:
                print("    the tail: %.4f ms per level (scope / %d)" % (t_scope / HEIGHT, HEIGHT), flush=True)
        base.close()
    # what one baseline call costs the host: 640 enqueues of a one-hash launch without a synchronise in between
    d_tmp = ctx.alloc(32 * 3)
    ctx.upload(d_tmp, np.zeros((3, 4), np.uint64))
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(640):
        ctx.poseidon_hash_batch_dev(h, d_tmp, 1, 2, d_tmp + 64)
    t_enq = (time.perf_counter() - t0) * 1e3 / 640
    ctx.synchronize()
    ctx.free(d_tmp)
    print("# host cost of one zkt_poseidon_hash_batch_dev call through ctypes (enqueue only): %.4f ms" % t_enq, flush=True)
    for m in (int(x) for x in a.sweep_m.split(",")):
        print("# threshold sweep, m = %d on a fresh tree (scope ms): T = levels with >= T parents are wide" % m, flush=True)
        for T in [int(x) for x in a.sweep.split(",")] + [INT_MAX]:
            _, t_scope, _ = _time_tree(ctx, h, d_prefill, 0, d_leaves, m, a.reps, split=T)
            print("  T = %-10d %10.3f" % (T, t_scope), flush=True)
    # paths into a variable map
    t = _fresh_tree(ctx, h, d_prefill, PREFILL, 0)
    k, n_vars = 8, 8 * 2 * HEIGHT
    d_vars = ctx.alloc(32 * n_vars)
    idx = [0, 1, 12345, PREFILL - 1, PREFILL // 2, 777777, 4242, PREFILL - 2]
    bit0 = [p * 2 * HEIGHT for p in range(k)]
    sib0 = [b + HEIGHT for b in bit0]

    def paths():
        ctx.merkle_tree_paths_to_variables_dev(t, idx, d_vars, n_vars, sib0, bit0)
        ctx.synchronize()

    paths()
    c0, ms0 = ctx.profile_get("merkle_paths")
    wall = [_wall(paths) for _ in range(a.reps)]
    c1, ms1 = ctx.profile_get("merkle_paths")
    print("# paths_to_variables_dev, 8 paths x %d levels with bits, tree of %d leaves: wall %.4f ms, scope %.4f ms"
          % (HEIGHT, PREFILL, float(np.median(wall)), (ms1 - ms0) / (c1 - c0)), flush=True)
    ctx.merkle_tree_free(t)
    for d in (d_vars, d_prefill, d_leaves):
        ctx.free(d)
    ctx.poseidon_free(h)
    ctx.close()


if __name__ == "__main__":
    main()
