"""Times the Merkle-path launch (zkt_poseidon_merkle_path_witness_dev) on the withdraw circuit's shapes against what it
replaces: one launch of the same INPUTS x HEIGHT hashes with their inputs already in the map, and the host's walk of the
paths that produces those inputs.

    python tools/merkle_path_timing.py [--logs 14,18,20] [--reps 5]

Rows (BN254; ms; the median of --reps on a warm context; device rows are wall times from the enqueue to the end of the
stream synchronise, the whole map resident in HBM):
  (a) path     zkt_poseidon_merkle_path_witness_dev: INPUTS paths of HEIGHT levels, the levels serial inside the kernel
  (b) hashes   zkt_poseidon_gadget_witness_dev, kernel = 2 (lanes), the same INPUTS x HEIGHT hashes as independent calls
               fed by select variables the HOST computed
  (c) native   what the host pays for (b)'s inputs: HEIGHT sequential Hasher.native calls per note
               (tools/withdraw_workload.py: plain Python integers, NOT an optimised native hasher)
After (a) the roots it returns are compared with the instance's root and the map with the one the hash launches made."""
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


def _mont(ctx, vals):
    """canonical Python integers -> (n, 4) Montgomery limbs (the product by R^2 runs on the device, as in bench.py)"""
    arr = np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(-1, 4)
    r2 = np.frombuffer((R * R % P_BN254).to_bytes(32, "little"), dtype=np.uint64)
    return ctx.debug_fr_mul(arr, np.tile(r2, (len(vals), 1)))


def _median(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def row(ctx, log_n, reps):
    width, inputs, height = WW.SHAPES[log_n]
    hs = WW.reference_hasher(P_BN254, width)
    inst = WW.make_instance(hs, inputs, height, seed=0x5EED)
    lay = WW.layout(hs, inst)
    n_vars = len(lay.values)
    gadget = z.PoseidonGadget(ctx, hs.width, hs.half_full, hs.partial, _mont(ctx, hs.rc), _mont(ctx, [x for r in hs.mds for x in r]),
                              _mont(ctx, [hs.tag])[0])
    S = gadget.vars_per_level
    for base, ins in lay.hash_calls:
        gadget.hash(base, ins)
    # the levels of the paths: the hash calls fed by the two selects in front of their trace; their bit, sibling and leaf
    # from the rows that make x_l = bit * sibling and y_l = (1 - bit) * cur
    levels = [(base, ins) for base, ins in lay.hash_calls if tuple(ins) == (base - 4, base - 1)]
    assert len(levels) == inputs * height
    row_of = {o: k for k, o in enumerate(lay.w[2])}
    leaf, bits, sibs, bases = [], [], [], []
    for k in range(inputs):
        mine = levels[k * height:(k + 1) * height]
        assert [b for b, _ in mine] == [mine[0][0] + lvl * S for lvl in range(height)]
        bases.append(mine[0][0] - 6)
        leaf.append(lay.w[1][row_of[mine[0][0] - 5]])
        bits.append([lay.w[0][row_of[b - 6]] for b, _ in mine])
        sibs.append([lay.w[1][row_of[b - 6]] for b, _ in mine])
    u32 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.uint32))
    arrays = [u32(bases), u32(leaf), u32(bits), u32(sibs), u32([b for b, _ in levels]), u32([ins for _, ins in levels])]
    held = [ctx.alloc(n_vars * 32), ctx.alloc(inputs * 32)] + [ctx.alloc(a.nbytes) for a in arrays]
    try:
        d_vars, d_roots, d_base, d_leaf, d_bits, d_sibs, d_hbase, d_hins = held
        for d, a in zip(held[2:], arrays):
            ctx.upload(d, a)
        ctx.upload(d_vars, _mont(ctx, lay.values))
        gadget.fill(d_vars, n_vars, check=True)                     # every hash, as today: the leaves are in the map now
        before = ctx.download(d_vars, (n_vars, 4))

        def path():
            ctx.poseidon_merkle_path_witness_dev(gadget._h, inputs, height, d_vars, n_vars, d_leaf, d_bits, d_sibs, d_path_base=d_base,
                                                 d_out_roots=d_roots)
            ctx.synchronize()

        def hashes():
            ctx.poseidon_gadget_witness_dev(gadget._h, len(levels), 2, d_vars, n_vars, d_input_vars=d_hins, d_trace_base=d_hbase,
                                            kernel=2)
            ctx.synchronize()

        leaves = [hs.native([i, a, hs.native([s])]) for i, a, s in zip(inst["identifiers"], inst["amounts"], inst["secrets"])]

        def native():
            for cur, (leaf_index, path_nodes) in zip(leaves, inst["poes"]):
                for layer, node in enumerate(path_nodes):
                    cur = hs.native([node, cur]) if (leaf_index >> layer) & 1 else hs.native([cur, node])

        ctx.poseidon_merkle_path_witness_dev(gadget._h, inputs, height, d_vars, n_vars, d_leaf, d_bits, d_sibs, d_path_base=d_base,
                                             d_out_roots=d_roots, validate_only=True)
        t_path = _median(path, reps)
        ctx.poseidon_gadget_check(gadget._h)
        assert np.array_equal(ctx.download(d_vars, (n_vars, 4)), before), "the path launch changed the map"
        roots = ctx.download(d_roots, (inputs, 4))
        assert np.array_equal(roots, np.tile(_mont(ctx, [inst["root"]]), (inputs, 1))), "a root differs from the tree's"
        t_hashes = _median(hashes, reps)
        t_native = _median(native, reps)
    finally:
        gadget.close()
        for d in held:
            ctx.free(d)
    print("2^%d x%d %dx%d: %d hashes | (a) path launch %.3f (%.4f per level) | (b) one lanes launch of the same hashes %.3f | "
          "(c) Hasher.native chain in Python %.1f" % (log_n, width, inputs, height, len(levels), t_path, t_path / height, t_hashes,
                                                       t_native), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", default="14,18,20")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    print("# Merkle path on the device; BN254 withdraw shapes; ms, median of %d" % a.reps, flush=True)
    ctx = z.Context("bn254", 0)
    for lg in (int(x) for x in a.logs.split(",")):
        row(ctx, lg, a.reps)
    ctx.close()


if __name__ == "__main__":
    main()
