"""CPU: the plain-Python restatement of the store files (tests/store_cases.py) pinned against the oracle's tree model as
tests/merkle_tree_cases.py builds it (oracle/composer.py NativeMerkleTree, leaves added one by one): the BTreeMap the
reference would serialise is the dense set, the file of its items is the file of the layers zkt_merkle_tree_layer returns, and
the restated reader accepts it and refuses each malformed variant where the table says."""
import pytest

import merkle_tree_cases as MTC
import store_cases as SC

COUNTS = [0, 1, 2, 3, 5, 8]
HEIGHTS = [3, 64]                      # 64: every layer above the third holds a single node


def _snap(height, count):
    return MTC.build("bn254", 4, height).snaps[count]


@pytest.mark.parametrize("height", HEIGHTS)
@pytest.mark.parametrize("count", COUNTS)
def test_the_oracle_trees_map_is_the_dense_set_and_its_file_parses(height, count):
    case = MTC.build("bn254", 4, height)
    snap = case.snaps[count]
    p = case.cv.fr.p
    assert sorted(snap.tree) == SC.dense_keys(count, height)
    assert [len(snap.layer(L)) for L in range(height)] == [SC.dense_layer_len(count, L) for L in range(height)]
    data = SC.store_bytes(snap.tree, snap.root, count)
    assert len(data) == SC.FIXED + SC.ENTRY * len(snap.tree)
    assert data == SC.store_of_layers([snap.layer(L) for L in range(height)], snap.root, count)
    kind, off, entries, root, next_index = SC.parse_tree(data, p, height, 1 << 3)
    assert (kind, off) == (SC.ACCEPTED, 0)
    assert dict(entries) == snap.tree and [k for k, _ in entries] == sorted(snap.tree) and root == snap.root and next_index == count
    if count:
        # HEIGHT is max layer + 1, and the fields lie where the layout says
        assert max(L for L, _ in snap.tree) + 1 == height
        assert data[:8] == SC.u64(len(snap.tree)) and data[8:24] == SC.u64(0) + SC.u64(0)
        assert int.from_bytes(data[24:56], "little") == case.leaves[0]
        assert data[-40:-8] == SC.scalar(snap.root) and data[-8:] == SC.u64(count)


def test_the_default_store_is_48_zero_bytes():
    assert SC.DEFAULT_STORE == bytes(48)
    snap = _snap(3, 0)
    assert SC.store_bytes(snap.tree, snap.root, snap.count) == SC.DEFAULT_STORE
    assert SC.parse_tree(SC.DEFAULT_STORE, MTC.build("bn254", 4, 3).cv.fr.p, 64, 1) == (SC.ACCEPTED, 0, [], 0, 0)


@pytest.mark.parametrize("height,count", [(3, 5), (3, 8), (64, 5)])
def test_the_restated_reader_refuses_each_malformed_file_where_the_table_says(height, count):
    case = MTC.build("bn254", 4, height)
    snap = case.snaps[count]
    p = case.cv.fr.p
    table = SC.malformed_tree_files(sorted(snap.tree.items()), snap.root, count, p, height, 8)
    names = [t[0] for t in table]
    assert len(set(names)) == len(names) and len(names) >= 22
    for name, data, h, cap, kind, off in table:
        assert SC.parse_tree(data, p, h, cap)[:2] == (kind, off), name
    assert {t[4] for t in table} == {SC.ACCEPTED, SC.TRUNCATED, SC.TRAILING, SC.NOT_BELOW_MODULUS, SC.NOT_ASCENDING, SC.NOT_DENSE, SC.TOO_FEW,
                                     SC.OVER_CAPACITY}


def test_notes_layout_round_trip_and_refusals():
    p = MTC.build("bn254", 4, 3).cv.fr.p
    notes = [(0, 5, 100, 7), (3, p - 1, (1 << 64) - 1, 1), ((1 << 64) - 1, 0, 0, p - 2)]
    data = SC.notes_bytes(notes)
    assert len(data) == 8 + SC.NOTE * 3 and data[:8] == SC.u64(3)
    assert data[8:16] == SC.u64(0) and data[16:48] == SC.scalar(5) and data[48:56] == SC.u64(100) and data[56:88] == SC.scalar(7)
    assert SC.parse_notes(data, p) == (SC.ACCEPTED, 0, notes)
    assert SC.parse_notes(SC.notes_bytes([]), p) == (SC.ACCEPTED, 0, []) and SC.notes_bytes([]) == bytes(8)
    assert SC.parse_notes(data[:-1], p)[:2] == (SC.TRUNCATED, len(data) - 1)
    assert SC.parse_notes(data[:5], p)[:2] == (SC.TRUNCATED, 5)
    assert SC.parse_notes(data + b"\1", p)[:2] == (SC.TRAILING, len(data))
    assert SC.parse_notes(SC.notes_bytes([notes[0], (1, p, 2, 3)]), p)[:2] == (SC.NOT_BELOW_MODULUS, 8 + SC.NOTE + 8)
    assert SC.parse_notes(SC.notes_bytes([notes[0], (1, 2, 2, p)]), p)[:2] == (SC.NOT_BELOW_MODULUS, 8 + SC.NOTE + 48)
