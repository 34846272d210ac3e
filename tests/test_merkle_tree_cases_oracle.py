"""CPU: the equality zkt_merkle_tree_append relies on.  The reference's tree after add_leaf leaf by leaf
(oracle/composer.py NativeMerkleTree = gadgets/src/merkle_tree.rs:89-106) equals a dense level-by-level rebuild in which every
stored node (layer, idx) is hash_two of its two children, nodes[layer] standing in for a right child that does not exist
yet: the stored nodes, the root and merkle_path -- on every case the device test (test_gpu_merkle_tree.py) uses."""
import pytest

import merkle_tree_cases as TC


def _check(case):
    for count, snap in sorted(case.snaps.items()):
        layers, root, empties = TC.dense_rebuild(case.prm, case.height, case.leaves[:count])
        assert empties == snap.nodes
        assert root == snap.root
        # the oracle's map holds exactly the dense layers: nothing more, no hole
        assert len(snap.tree) == sum(snap.stored(L) for L in range(case.height))
        for L in range(case.height):
            assert snap.layer(L) == layers[L], (count, L)
        for index in snap.path_indices():
            assert snap.merkle_path(index) == TC.dense_path(layers, empties, index), (count, index)


@pytest.mark.parametrize("height", TC.HEIGHTS)
@pytest.mark.parametrize("w", TC.WIDTHS)
@pytest.mark.parametrize("cvname", TC.CURVES)
def test_sequential_add_leaf_equals_the_dense_rebuild(cvname, w, height):
    case = TC.build(cvname, w, height)
    assert sorted(case.snaps) == [0] + TC.leaf_counts(height)
    _check(case)


def test_the_shipped_height_64_case():
    case = TC.build_shipped()
    assert (case.height, len(case.leaves), sorted(case.snaps)) == (64, 13, [0, 5, 13])
    _check(case)


def test_the_large_case():
    case = TC.build_large()
    assert (case.height, len(case.leaves), sorted(case.snaps)) == (11, 1100, [0, 1001, 1100])
    assert TC.level_parents(0, 1100, 0) == 550 and TC.level_parents(0, 1100, 1) == 275
    assert TC.level_parents(1001, 99, 0) == 50
    for count, snap in sorted(case.snaps.items()):
        layers, root, empties = TC.dense_rebuild(case.prm, case.height, case.leaves[:count])
        assert (root, empties) == (snap.root, snap.nodes)
        assert [snap.layer(L) for L in range(case.height)] == layers
        for index in (0, max(count - 1, 0), count, 2047):
            assert snap.merkle_path(index) == TC.dense_path(layers, empties, index)


def test_a_fresh_tree_has_the_root_zero_not_the_empty_hash():
    snap = TC.build("bn254", 3, 3).snaps[0]
    assert snap.root == 0 and snap.tree == {} and snap.nodes[0] == 0 and snap.nodes[1] != 0
    assert snap.merkle_path(0) == snap.nodes == snap.merkle_path(7)


@pytest.mark.parametrize("w", TC.WIDTHS)
def test_the_uneven_split_starts_odd_ends_even_and_overfills_the_tail(w):
    groups = TC.tail_groups(w)
    assert groups == {3: 16, 4: 16, 5: 8, 8: 4}[w]
    for n in (1, 2, 3, 5, 8, 37):
        batches = TC.uneven_batches(n, w)
        assert sum(batches) == n and batches[0] == 1
        s = 1
        for k, m in enumerate(batches[1:]):
            assert s & 1                                              # a stored left neighbour
            if s + m < n or k == 0 and n >= 1 + 2 * (groups + 1):
                assert not (s + m - 1) & 1                            # ends on a left child: an empty right filler
            s += m
    assert TC.level_parents(1, TC.uneven_batches(37, w)[1], 0) == groups + 2
