"""Times ProveWithdraw for a batch of requests through zkt_withdraw_prove (verify = 1, append = 1) beside the sequence of calls
it replaces (zkt_withdraw_witness, zkt_prove chained with zkt_prove_set_next, zkt_verify, zkt_merkle_tree_append), and the
MerkleTreeStore file calls on a large tree.

    python tools/withdraw_prove_timing.py prove [--log 20] [--batch 8] [--reps 5] [--assembled-only]
    python tools/withdraw_prove_timing.py tree  [--leaves 1048576] [--reps 3] [--dir /tmp]

BN254, the shipped tables, the shape of tools/withdraw_workload.py SHAPES; wall time, the two routes alternating, the median
of --reps after a warm-up of each.  --assembled-only leaves the one call out, so that the script also runs against a library
that does not have it yet (ZKT_LIB_PATH).  Both routes prove against the tree as it is and append to it, so every repetition
meets a tree eight leaves larger; the paths and the root come from the tree (siblings = root = None)."""
import argparse
import os
import random
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

P_BN254 = 21888242871839275222246405745257275088548364400416034343698204186575808495617
Q_BN254 = 21888242871839275222246405745257275088696311157297823662689037894645226208583
R = 1 << 256
TABLE_SIZE = 1024
TAU = 0x5EED5


def _mont(ctx, vals):
    arr = np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(-1, 4)
    r2 = np.frombuffer((R * R % P_BN254).to_bytes(32, "little"), dtype=np.uint64)
    return ctx.debug_fr_mul(arr, np.tile(r2, (len(vals), 1)))


def _params(ctx, hs):
    return (hs.width, hs.half_full, hs.partial, _mont(ctx, hs.rc[:(2 * hs.half_full + hs.partial) * hs.width]),
            _mont(ctx, [x for r in hs.mds for x in r]), _mont(ctx, [hs.tag])[0])


def _affine(commits, inf):
    rinv = pow(R, -1, Q_BN254)
    val = lambda limbs: sum(int(v) << (64 * i) for i, v in enumerate(limbs)) * rinv % Q_BN254
    return [None if inf[k] else (val(commits[k][:4]), val(commits[k][4:])) for k in range(10)]


def prove(log_n, batch, reps, assembled_only):
    import zkt_plonk_amd as z
    from zkt_plonk_amd import _lib
    import withdraw_workload as WW
    width, inputs, height = WW.SHAPES[log_n]
    hs = WW.reference_hasher(P_BN254, width)
    ctx = z.Context("bn254", 0)
    ctx.srs_generate(TAU, (1 << log_n) + 8)
    w = z.WithdrawCircuit(ctx, _params(ctx, hs), inputs, height)
    commits, inf = w.setup(log_n, TABLE_SIZE)
    pts = dict(zip(z.PK_ORDER, _affine(commits, inf)))
    n = 1 << log_n
    g = ctx.srs_download(0, 1)[0]
    h, beta_h = _lib.srs_generate_g2("bn254", TAU)
    m = batch * inputs
    rnd = random.Random(0xD0E5)
    idents = [rnd.randrange(1, P_BN254) for _ in range(7)]
    set_mont = _mont(ctx, idents)
    secrets = _mont(ctx, [rnd.randrange(1, P_BN254) for _ in range(m)])
    ident = _mont(ctx, [rnd.choice(idents) for _ in range(m)])
    amounts = np.array([rnd.randrange(1, 1 << 40) for _ in range(m)], dtype=np.uint64)
    tree = z.MerkleTree(ctx, w.poseidon_handle, height, min(1 << 12, 1 << height))
    d = [ctx.alloc(a.nbytes) for a in (secrets, ident, amounts)] + [ctx.alloc(m * 32)]
    for p, a in zip(d, (secrets, ident, amounts)):
        ctx.upload(p, a)
    ctx.note_leaves(w.poseidon_handle, d[0], d[1], d[2], m, d[3])
    tree.append(d_leaves=d[3], m=m)
    fresh = _mont(ctx, [rnd.randrange(1, P_BN254) for _ in range(batch)])
    blinders = _mont(ctx, [rnd.randrange(1, P_BN254) for _ in range(batch * 19)]).reshape(batch, 19, 4)
    reqs = []
    for b in range(batch):
        k = slice(b * inputs, (b + 1) * inputs)
        reqs.append(dict(secrets=secrets[k], identifiers=ident[k], amounts=amounts[k], leaf_indices=np.arange(k.start, k.stop, dtype=np.uint64),
                         siblings=None, root=None, new_secret=fresh[b], new_identifier=ident[b], withdraw_amount=int(amounts[k].sum()) // 3))
    d_vars = ctx.alloc(batch * w.n_vars * 32)
    pi_roots = None
    tr = lambda: z.seed_transcript(z.Transcript("merlin", "ZKT Plonk"), n, pts)

    def assembled():
        nonlocal pi_roots
        pi, status = w.witness(reqs, d_vars, tree=tree)
        assert status == [0] * batch
        if pi_roots is None:
            omega = pow(5, (P_BN254 - 1) >> log_n, P_BN254)
            pi_roots = _mont(ctx, [pow(omega, int(pos), P_BN254) for pos in w.pi_pos])
        preps = [w.prepare(d_vars, w.n_vars, b, set_mont, pi[b], blinders[b]) for b in range(batch)]
        proofs = []
        for b in range(batch):
            proofs.append(ctx.prove_prepared(preps[b], tr(), preps[b + 1] if b + 1 < batch else None))
            assert _lib.verify("bn254", n, commits, list(inf), pi_roots, pi[b], proofs[b], g, h, beta_h, tr())
        tree.append(np.ascontiguousarray(pi[:, -1]))
        return proofs

    def one_call():
        proofs, _, res = w.prove(reqs, d_vars, batch, set_mont, blinders, tree=tree, verify_key=(g, h, beta_h), append=True)
        assert all(r["code"] == 0 and r["verified"] and r["new_leaf_index"] != (1 << 64) - 1 for r in res), res
        return proofs

    routes = [("assembled", assembled)] + ([] if assembled_only else [("one call", one_call)])
    for _, f in routes:
        f()                                                        # warm-up: plans, the Lagrange table, the commitments
    times = {name: [] for name, _ in routes}
    for _ in range(reps):
        for name, f in routes:
            t0 = time.perf_counter()
            f()
            times[name].append((time.perf_counter() - t0) * 1e3 / batch)
    print("2^%d x%d %dx%d, %d requests, verify and append; ms per proof, %d runs each, alternating" % (log_n, width, inputs, height, batch, reps))
    for name, ts in times.items():
        print("  %-10s median %.2f  min %.2f  max %.2f  (%s)" % (name, float(np.median(ts)), min(ts), max(ts), " ".join("%.2f" % t for t in ts)),
              flush=True)
    for p in d + [d_vars]:
        ctx.free(p)
    tree.close()
    w.close()
    ctx.close()


def tree_file(leaves, reps, where):
    import zkt_plonk_amd as z
    import withdraw_workload as WW
    hs = WW.reference_hasher(P_BN254, 5)
    ctx = z.Context("bn254", 0)
    pos = ctx.poseidon_load(*_params(ctx, hs))
    rng = np.random.default_rng(7)
    vals = rng.integers(0, 1 << 62, size=(leaves, 4), dtype=np.uint64)     # below 2^254: valid Montgomery words
    vals[:, 3] >>= np.uint64(2)
    tree = z.MerkleTree(ctx, pos, 64, leaves)
    tree.append(vals)
    path = os.path.join(where, "zkt_tree_timing_%d.bin" % os.getpid())
    ctx.profile_enable(True)
    try:
        save, load = [], []
        for _ in range(reps + 1):
            t0 = time.perf_counter()
            tree.save_file(path)
            save.append((time.perf_counter() - t0) * 1e3)
            before = {k: ctx.profile_get(k) for k in ("store_upload", "merkle_append", "store_leaves", "store_compare")}
            t0 = time.perf_counter()
            t2, rep = z.MerkleTree.load_file(ctx, pos, 64, leaves, path)
            load.append((time.perf_counter() - t0) * 1e3)
            after = {k: ctx.profile_get(k) for k in before}
            assert rep["mismatches"] == 0 and rep["root_matches"] and np.array_equal(t2.root(), tree.root())
            t2.close()
        scopes = {k: after[k][1] - before[k][1] for k in before}
        print("MerkleTreeStore file of %d leaves, height 64, BN254 x5: %.1f MB, %d entries" % (leaves, os.path.getsize(path) / 1e6, rep["entries"]))
        print("  save %.0f ms | load %.0f ms: parse and upload (store_upload scope) %.0f, rebuild (store_leaves + merkle_append) %.1f, "
              "compare (store_compare) %.2f   [medians of %d after a warm-up; scopes of the last run]"
              % (float(np.median(save[1:])), float(np.median(load[1:])), scopes["store_upload"], scopes["store_leaves"] + scopes["merkle_append"],
                 scopes["store_compare"], reps), flush=True)
    finally:
        if os.path.exists(path):
            os.remove(path)
    tree.close()
    ctx.poseidon_free(pos)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["prove", "tree"])
    ap.add_argument("--log", type=int, default=20)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--assembled-only", action="store_true")
    ap.add_argument("--leaves", type=int, default=1 << 20)
    ap.add_argument("--dir", default="/tmp")
    a = ap.parse_args()
    if a.mode == "prove":
        prove(a.log, a.batch, a.reps, a.assembled_only)
    else:
        tree_file(a.leaves, a.reps, a.dir)
    return 0


if __name__ == "__main__":
    sys.exit(main())
