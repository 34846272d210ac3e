"""zkt_merkle_tree_save_file / _load_file: the note tree as the reference CLI's --merkle-tree file (MerkleTreeStore).  The bytes
against the plain-Python restatement of the layout (tests/store_cases.py, pinned to the oracle's tree on the CPU by
test_store_cases_oracle.py), the round trip, and the device comparison of every node the file claims with the tree rebuilt from
its leaves.  The reference tree is the dense rebuild of tests/merkle_tree_cases.py, computed once per shape."""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import fields as F, coracle as K

from helpers import field_elems
import merkle_path_cases as MC
import merkle_tree_cases as TC
import store_cases as SC

CV = F.BN254
WIDTH = 4
# counts 64 and 65 sit on both sides of the append's narrow / wide level threshold (64 parents need 127 or 128 leaves at level
# 0: 200 crosses it); height 3 where the count fits, else 8; height 64: single-node upper layers
SHAPES = [(3, 0), (3, 1), (3, 2), (3, 5), (8, 64), (8, 65), (8, 200), (64, 5)]
SMALL_CHUNK = 7                     # nodes per staging chunk: every shape with more than 7 nodes in a layer crosses chunks


@functools.lru_cache(maxsize=None)
def _prm():
    return MC.synthetic_params(CV, WIDTH)


@functools.lru_cache(maxsize=None)
def _ref(height, count, flip=None):
    """-> (leaves, layers, root, empties) of the dense tree; flip = (index, delta) alters one leaf."""
    leaves = field_elems(CV.fr.p, 0x57E0 + height, count)
    if flip:
        leaves[flip[0]] = (leaves[flip[0]] + flip[1]) % CV.fr.p
    layers, root, empties = TC.dense_rebuild(_prm(), height, leaves)
    return leaves, layers, root, empties


@pytest.fixture(scope="module")
def world():
    import zkt_plonk_amd as z
    prm = _prm()
    ctx = z.Context("bn254", 0)
    h = ctx.poseidon_load(prm.width, prm.half_full, prm.partial, K.fr_to_mont(CV, prm.rc), K.fr_to_mont(CV, [x for row in prm.mds for x in row]),
                          K.fr_to_mont(CV, [prm.domain_tag])[0])
    yield z, ctx, h
    ctx.poseidon_free(h)
    ctx.close()


def _capacity(height, count):
    return min(1 << height, max(count + 3, 8))


def _device_tree(z, ctx, h, height, count):
    t = z.MerkleTree(ctx, h, height, _capacity(height, count))
    leaves = _ref(height, count)[0]
    if leaves:
        assert t.append(K.fr_to_mont(CV, leaves)) == 0
    return t


def _check_tree(t, height, count, layers, root, empties):
    assert t.ctx.merkle_tree_info(t.handle)[:2] == (height, count)
    assert K.fr_from_mont(CV, t.root().reshape(1, 4))[0] == root
    for L in range(height):
        got = t.layer(L)
        assert (K.fr_from_mont(CV, got) if len(got) else []) == (layers[L] if count else []), L
    idx = sorted({0, count // 2, max(count - 1, 0), min(count, (1 << height) - 1)})
    assert [K.fr_from_mont(CV, g) for g in t.paths(idx)] == [TC.dense_path(layers, empties, i) if count else list(empties) for i in idx]


@pytest.mark.parametrize("height,count", SHAPES)
def test_save_and_load_round_trip(world, height, count, tmp_path):
    """The file's bytes are the restatement's, under the default staging chunk and under one of 7 nodes (several chunks a
    layer, in the writer and in the reader); the loaded tree has the original's layers, root and paths; the report is clean."""
    z, ctx, h = world
    leaves, layers, root, empties = _ref(height, count)
    want = SC.store_of_layers(layers if count else [], root, count)
    assert len(want) == 48 + 48 * sum(SC.dense_layer_len(count, L) for L in range(height))
    before = z._lib.debug_live_allocations()
    t = _device_tree(z, ctx, h, height, count)
    path = str(tmp_path / "tree.bin")
    try:
        for chunk in (0, SMALL_CHUNK):
            ctx.debug_store_chunk(chunk)
            t.save_file(path)
            assert open(path, "rb").read() == want, chunk
            assert os.listdir(tmp_path) == ["tree.bin"], "a temporary file stayed"
            t2, rep = z.MerkleTree.load_file(ctx, h, height, _capacity(height, count), path)
            try:
                assert rep == {"entries": (len(want) - 48) // 48, "mismatches": 0, "first_layer": -1, "first_idx": 0, "root_matches": True}
                _check_tree(t2, height, count, layers, root, empties)
                # the loaded tree goes on as the original would: one more leaf, the same root
                if count < _capacity(height, count):
                    t2.append(K.fr_to_mont(CV, [12345]))
                    assert K.fr_from_mont(CV, t2.root().reshape(1, 4))[0] == TC.dense_rebuild(_prm(), height, leaves + [12345])[1]
            finally:
                t2.close()
    finally:
        ctx.debug_store_chunk(0)
        t.close()
    assert z._lib.debug_live_allocations() == before


FLIP_SHAPE = (8, 65)
FLIPS = {"layer0": [(0, 3)], "middle": [(4, 2)], "top": [(7, 0)], "root": ["root"], "two_reports_the_smaller_key": [(5, 1), (2, 9)],
         "layer0_last_leaf_and_root": [(0, 64), "root"]}


@pytest.mark.parametrize("name", sorted(FLIPS))
@pytest.mark.parametrize("chunk", [0, SMALL_CHUNK])
def test_flipped_scalars_are_found_on_the_device(world, name, chunk, tmp_path):
    """One scalar of the file altered at layer 0, a middle layer, the top layer and the root, and two at once: the report
    names exactly the (layer, idx), the count and the root flag the restatement predicts.  A layer-0 flip changes the rebuilt
    path, so every ancestor the file holds mismatches (and its root); a flip higher up mismatches that node only.  The tree
    returned is the one rebuilt from the file's leaves."""
    z, ctx, h = world
    height, count = FLIP_SHAPE
    leaves, layers, root, empties = _ref(height, count)
    entries = {(L, i): v for L, lay in enumerate(layers) for i, v in enumerate(lay)}
    file_root, flip = root, None
    for f in FLIPS[name]:
        if f == "root":
            file_root = (root + 1) % CV.fr.p
        else:
            entries[f] = (entries[f] + 1) % CV.fr.p
            if f[0] == 0:
                flip = (f[1], 1)
    path = str(tmp_path / "tree.bin")
    open(path, "wb").write(SC.store_bytes(entries, file_root, count))
    _, r_layers, r_root, r_empties = _ref(height, count, flip)
    want = SC.expected_report(sorted(entries.items()), file_root, r_layers, r_root)
    if name == "layer0":
        assert (want["mismatches"], want["first_layer"], want["first_idx"], want["root_matches"]) == (height - 1, 1, 1, False)
    elif name == "middle":
        assert (want["mismatches"], want["first_layer"], want["first_idx"], want["root_matches"]) == (1, 4, 2, True)
    elif name == "two_reports_the_smaller_key":
        assert (want["mismatches"], want["first_layer"], want["first_idx"]) == (2, 2, 9)
    ctx.debug_store_chunk(chunk)
    try:
        t, rep = z.MerkleTree.load_file(ctx, h, height, _capacity(height, count), path)
    finally:
        ctx.debug_store_chunk(0)
    try:
        assert rep == want
        _check_tree(t, height, count, r_layers, r_root, r_empties)
    finally:
        t.close()


def test_malformed_files_are_refused_with_path_and_offset(world, tmp_path):
    """Every malformed case of the table (tests/store_cases.py), through the chunked reader with several chunks a file: the
    refusal the restatement predicts, by text and offset, ZKT_ERR_INVALID_ARGUMENT, and nothing created."""
    z, ctx, h = world
    height, count = 3, 5
    leaves, layers, root, _ = _ref(height, count)
    entries = sorted({(L, i): v for L, lay in enumerate(layers) for i, v in enumerate(lay)}.items())
    table = SC.malformed_tree_files(entries, root, count, CV.fr.p, height, 8)
    texts = {SC.TRUNCATED: "truncated", SC.TRAILING: "trailing bytes", SC.NOT_BELOW_MODULUS: "not below the modulus", SC.NOT_ASCENDING: "not ascending",
             SC.NOT_DENSE: "outside the dense set", SC.TOO_FEW: "fewer entries than the dense set", SC.OVER_CAPACITY: "above the capacity"}
    before = z._lib.debug_live_allocations()
    ctx.debug_store_chunk(2)
    try:
        for name, data, hgt, cap, _, _ in table:
            cap = min(cap, 1 << hgt)
            kind, off = SC.parse_tree(data, CV.fr.p, hgt, cap)[:2]
            path = str(tmp_path / (name + ".bin"))
            open(path, "wb").write(data)
            if kind == SC.ACCEPTED:
                t, rep = z.MerkleTree.load_file(ctx, h, hgt, cap, path)
                t.close()
                assert rep["mismatches"] == 0 and rep["root_matches"]
                continue
            with pytest.raises(z.ZktError) as e:
                z.MerkleTree.load_file(ctx, h, hgt, cap, path)
            msg = str(e.value)
            assert e.value.code == 1 and path in msg and texts[kind] in msg and "(offset %d)" % off in msg, (name, msg)
        with pytest.raises(z.ZktError) as e:
            z.MerkleTree.load_file(ctx, h, 3, 8, str(tmp_path / "missing.bin"))
        assert "missing.bin" in str(e.value)
    finally:
        ctx.debug_store_chunk(0)
    assert z._lib.debug_live_allocations() == before
