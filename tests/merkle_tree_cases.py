"""Cases for zkt_merkle_tree (the note tree kept on the device), built from the oracle's restatement of the reference's tree
(oracle/composer.py NativeMerkleTree = gadgets/src/merkle_tree.rs:57-111) with the leaves added ONE BY ONE.  Shared by the
CPU pin of the equality the device append relies on (test_merkle_tree_cases_oracle.py) and the device test
(test_gpu_merkle_tree.py); a case is computed once and never changed.

A case holds the leaves and, for every leaf count asked for, a snapshot of the oracle tree after that many add_leaf calls:
its stored nodes layer by layer, its root, its merkle_path.  `dense_rebuild` is the other side of the equality: a plain
level-by-level rebuild in which every stored node (layer, idx) is hash_two of its two children, nodes[layer] standing in
for a right child that does not exist yet."""
import functools

from oracle import composer as OC, fields as F

from helpers import field_elems

import merkle_path_cases as MC

HEIGHTS = [1, 2, 3, 7, 64]
WIDTHS = [3, 4, 5, 8]
CURVES = ["bn254", "bls12_381"]


def leaf_counts(height):
    """1, 2, 3, 5, 8 and min(2^height, 37), as far as the tree has room."""
    top = min(1 << height, 37)
    return sorted({n for n in (1, 2, 3, 5, 8, top) if n <= top})


class Snapshot:
    """The oracle tree after `count` add_leaf calls."""

    def __init__(self, tree, count):
        self.count, self.height, self.root, self.nodes = count, tree.height, tree.root, list(tree.nodes)
        self.tree = dict(tree.tree)

    def stored(self, layer):
        """How many nodes the layer holds: ceil(count / 2^layer)."""
        return ((self.count - 1) >> layer) + 1 if self.count else 0

    def layer(self, layer):
        """The stored nodes of a layer by index; a hole (a KeyError) would contradict the dense layout."""
        return [self.tree[(layer, idx)] for idx in range(self.stored(layer))]

    def merkle_path(self, index):
        return [self.tree.get((layer, (index >> layer) ^ 1), self.nodes[layer]) for layer in range(self.height)]

    def path_indices(self):
        """Every index below the count, the count itself (when the tree has room for it) and 2^height - 1."""
        return sorted(set(range(min(self.count + 1, 1 << self.height))) | {(1 << self.height) - 1})


class Case:
    def __init__(self, cv, prm, height, leaves, snaps):
        self.cv, self.prm, self.height, self.leaves, self.snaps = cv, prm, height, leaves, snaps


def _case(cv, prm, height, n_leaves, counts, seed):
    leaves = field_elems(cv.fr.p, 7000 + 31 * prm.width + height + seed, n_leaves)
    tree = OC.NativeMerkleTree(prm, height)
    snaps = {0: Snapshot(tree, 0)}
    for k, leaf in enumerate(leaves):
        assert tree.add_leaf(leaf) == k
        if k + 1 in counts:
            snaps[k + 1] = Snapshot(tree, k + 1)
    assert sorted(snaps) == sorted(set(counts) | {0})
    return Case(cv, prm, height, leaves, snaps)


@functools.lru_cache(maxsize=None)
def build(cvname, w, height, seed=1):
    """The synthetic short schedule: min(2^height, 37) leaves, snapshots at every count of leaf_counts(height) -- the leaves
    of a smaller count are a prefix of the larger one's."""
    cv = F.CURVES[cvname]
    counts = leaf_counts(height)
    return _case(cv, MC.synthetic_params(cv, w), height, counts[-1], tuple(counts), seed)


@functools.lru_cache(maxsize=None)
def build_shipped():
    """Height 64 on the shipped BN254 x5 tables: 13 leaves, snapshots after 5 and after 13 (the shape of withdraw_instance)."""
    return _case(F.BN254, MC.shipped_params(5), 64, 13, (5, 13), 2)


LARGE = (11, 1100)     # height, leaves


@functools.lru_cache(maxsize=None)
def build_large():
    """BN254, width 3, height 11, 1100 leaves: level 0 has 550 parents -- more than one 128-thread block of the wide kernel and
    more than the 512 parents a level of the tail may hold, so that level is a wide launch whatever split is asked for and the
    tail starts at level 1 on 275 parents, both of its LDS buffers in use.  Snapshots after 1001 leaves and after all."""
    cv = F.CURVES["bn254"]
    return _case(cv, MC.synthetic_params(cv, 3), LARGE[0], LARGE[1], (1001, LARGE[1]), 3)


def dense_rebuild(prm, height, leaves):
    """-> (layers, root, empties): layers[L] = the ceil(n / 2^L) stored nodes of layer L, 0 <= L < height."""
    empties, h = [], 0
    for _ in range(height):
        empties.append(h)
        h = prm.native([h, h])
    layers, cur = [], list(leaves)
    for L in range(height):
        layers.append(cur)
        cur = [prm.native([cur[2 * p], cur[2 * p + 1] if 2 * p + 1 < len(cur) else empties[L]]) for p in range((len(cur) + 1) // 2)]
    root = cur[0] if leaves else 0          # MerkleTreeStore::default().root
    return layers, root, empties


def dense_path(layers, empties, index):
    return [layers[L][(index >> L) ^ 1] if (index >> L) ^ 1 < len(layers[L]) else empties[L] for L in range(len(layers))]


# ---- how the device test splits an append ------------------------------------------------------------------------------
def tail_groups(w):
    """Parents the tail workgroup hashes at once: 256 threads = 4 wavefronts of PER_WAVE lane groups."""
    return 4 * MC.per_wave(w)


def uneven_batches(n, w):
    """One leaf, then batches that START AT AN ODD INDEX (their first parent has a stored left neighbour) and END ON A LEFT
    CHILD (their last parent takes the empty filler) wherever the count allows; the second batch spans 4 PER_WAVE + 2
    parents: one round of the tail's lane groups, then a round in which all but two groups have no hash."""
    out, s = [1], 1
    big = 2 * (tail_groups(w) + 1)
    while s < n:
        m = min(n - s, big)
        if m > 1 and (s + m - 1) & 1:
            m -= 1
        out.append(m)
        s += m
    assert sum(out) == n
    return out


def splits(n, w):
    return {"one": [n], "single": [1] * n, "uneven": uneven_batches(n, w)}


def level_parents(s, m, level):
    """Parents of layer level + 1 that appending m leaves at s recomputes."""
    return ((s + m - 1) >> (level + 1)) - (s >> (level + 1)) + 1
