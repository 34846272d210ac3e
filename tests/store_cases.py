"""The two store files of the reference CLI, restated in plain Python (csrc/storefile.hpp holds the C++ side):

  --merkle-tree  MerkleTreeStore { tree: BTreeMap<(usize, usize), F>, root: F, next_index: usize }  (gadgets/src/merkle_tree.rs:8-13)
      u64 E | E x (u64 layer, u64 idx, scalar) ascending (layer, idx) | scalar root | u64 next_index
  --notes        Vec<Note { leaf_index: usize, identifier: F, amount: u64, secret: F }>               (gadgets/src/note.rs)
      u64 count | count x (u64 leaf_index, scalar identifier, u64 amount, scalar secret)

under ark-serialize 0.3's rules for serialize_unchecked: usize and u64 are 8 bytes little endian, a scalar is 32 canonical
little-endian bytes, a Vec or BTreeMap is a u64 length and then its items.  The layouts are derived from those rules; the
reference holds no such file to compare with.

Also here: the dense-set rule, the reader's refusals in the order it makes them, and the table of malformed files every reader
of the tree file is run over.  Values are plain integers (canonical, not Montgomery)."""
import struct

ENTRY, FIXED, NOTE = 48, 48, 80

# what a reader refuses, as csrc/storefile.hpp numbers it
ACCEPTED, UNREADABLE, TRUNCATED, TRAILING, NOT_BELOW_MODULUS, NOT_ASCENDING, NOT_DENSE, TOO_FEW, OVER_CAPACITY, TOO_MANY_NOTES = range(10)


def u64(v):
    return struct.pack("<Q", v)


def scalar(v):
    return int(v).to_bytes(32, "little")


def dense_layer_len(count, layer):
    """Nodes of a layer after add_leaf of `count` leaves: ceil(count / 2^layer) (merkle_tree.rs:92-95)."""
    return ((count - 1) >> layer) + 1 if count else 0


def dense_keys(count, height):
    return [(L, i) for L in range(height) for i in range(dense_layer_len(count, L))]


def tree_bytes(entries, root, next_index):
    """entries: [((layer, idx), value)] in the order they are to lie in the file."""
    out = [u64(len(entries))]
    for (layer, idx), v in entries:
        out += [u64(layer), u64(idx), scalar(v)]
    return b"".join(out + [scalar(root), u64(next_index)])


def store_bytes(tree, root, next_index):
    """A MerkleTreeStore: `tree` is the BTreeMap as a dict {(layer, idx): value}."""
    return tree_bytes(sorted(tree.items()), root, next_index)


def store_of_layers(layers, root, count):
    """The file of a tree given as its stored layers (layers[L][idx]), as zkt_merkle_tree_layer returns them."""
    return tree_bytes([((L, i), v) for L, lay in enumerate(layers) for i, v in enumerate(lay)], root, count)


DEFAULT_STORE = tree_bytes([], 0, 0)


def parse_tree(data, p, height, capacity):
    """The reader of csrc/storefile.hpp, refusal for refusal -> (kind, offset, entries, root, next_index); entries and the
    rest are None after a refusal.  Order: the file's size; then entry by entry the scalar, the key against the one before
    it, the key against the dense set; then the entry count, the root, next_index against the capacity."""
    bad = lambda kind, off: (kind, off, None, None, None)
    size = len(data)
    if size < 8:
        return bad(TRUNCATED, size)
    E = struct.unpack_from("<Q", data)[0]
    if size < FIXED or E > (size - FIXED) // ENTRY:
        return bad(TRUNCATED, size)
    want = FIXED + E * ENTRY
    if size > want:
        return bad(TRAILING, want)
    root = int.from_bytes(data[want - 40:want - 8], "little")
    next_index = struct.unpack_from("<Q", data, want - 8)[0]
    entries, prev = [], None
    for k in range(E):
        at = 8 + k * ENTRY
        layer, idx = struct.unpack_from("<QQ", data, at)
        v = int.from_bytes(data[at + 16:at + 48], "little")
        if v >= p:
            return bad(NOT_BELOW_MODULUS, at + 16)
        if prev is not None and (layer, idx) <= prev:
            return bad(NOT_ASCENDING, at)
        if layer >= height or idx >= dense_layer_len(next_index, layer):
            return bad(NOT_DENSE, at)
        prev = (layer, idx)
        entries.append(((layer, idx), v))
    if E != sum(dense_layer_len(next_index, L) for L in range(height)):
        return bad(TOO_FEW, 0)
    if root >= p:
        return bad(NOT_BELOW_MODULUS, want - 40)
    if next_index > capacity:
        return bad(OVER_CAPACITY, want - 8)
    return ACCEPTED, 0, entries, root, next_index


def malformed_tree_files(entries, root, count, p, height, capacity):
    """The malformed variants of one good file -> [(name, bytes, height, capacity, kind, offset)], the refusal each must
    get.  entries: the good file's sorted [((layer, idx), value)]; it needs count >= 3 and height >= 2."""
    assert count >= 3 and height >= 2 and [k for k, _ in entries] == dense_keys(count, height)
    good = tree_bytes(entries, root, count)
    E = len(entries)
    root_at, next_at = 8 + E * ENTRY, 8 + E * ENTRY + 32
    out = [("good", good, height, capacity, ACCEPTED, 0)]
    add = lambda name, data, kind, off, h=height, cap=capacity: out.append((name, data, h, cap, kind, off))
    # truncated at each field boundary: inside and after the count, after a key's halves, after an entry, after the root
    for name, cut in (("empty", 0), ("in_count", 5), ("after_count", 8), ("after_layer", 16), ("after_idx", 24), ("after_entry", 8 + ENTRY),
                      ("before_root", root_at), ("after_root", next_at), ("in_next_index", next_at + 7)):
        add("truncated_" + name, good[:cut], TRUNCATED, cut)
    add("trailing_byte", good + b"\0", TRAILING, len(good))
    k = E // 2
    swap = list(entries)
    swap[k], swap[k + 1] = swap[k + 1], swap[k]
    add("scalar_is_modulus", tree_bytes(entries[:k] + [(entries[k][0], p)] + entries[k + 1:], root, count), NOT_BELOW_MODULUS, 8 + k * ENTRY + 16)
    add("root_is_modulus", tree_bytes(entries, p, count), NOT_BELOW_MODULUS, root_at)
    # the first of the two lies above its predecessor and inside the dense set: the second is the one that descends
    add("keys_swapped", tree_bytes(swap, root, count), NOT_ASCENDING, 8 + (k + 1) * ENTRY)
    add("key_repeated", tree_bytes(entries[:k + 1] + [entries[k]] + entries[k + 2:], root, count), NOT_ASCENDING, 8 + (k + 1) * ENTRY)
    # layer 0's last entry missing: every key that is left belongs to the set, one too few
    last0 = dense_layer_len(count, 0) - 1
    add("missing_at_layer_end", tree_bytes(entries[:last0] + entries[last0 + 1:], root, count), TOO_FEW, 0)
    add("extra_at_layer_end", tree_bytes(entries[:last0 + 1] + [((0, last0 + 1), 7)] + entries[last0 + 1:], root, count), NOT_DENSE,
        8 + (last0 + 1) * ENTRY)
    add("extra_layer", tree_bytes(entries + [((height, 0), 7)], root, count), NOT_DENSE, root_at)
    # next_index one too small: leaf count - 1 is outside its set; one too large: all inside, too few of them
    add("next_index_too_small", tree_bytes(entries, root, count - 1), NOT_DENSE, 8 + (count - 1) * ENTRY)
    add("next_index_too_large", tree_bytes(entries, root, count + 1), TOO_FEW, 0)
    first_top = next(i for i, (key, _) in enumerate(entries) if key[0] == height - 1)
    add("height_one_more", good, TOO_FEW, 0, h=height + 1)
    add("height_one_less", good, NOT_DENSE, 8 + first_top * ENTRY, h=height - 1)
    add("over_capacity", good, OVER_CAPACITY, next_at, cap=count - 1)
    return out


def notes_bytes(notes):
    """notes: [(leaf_index, identifier, amount, secret)]."""
    out = [u64(len(notes))]
    for leaf_index, identifier, amount, secret in notes:
        out += [u64(leaf_index), scalar(identifier), u64(amount), scalar(secret)]
    return b"".join(out)


def parse_notes(data, p):
    """-> (kind, offset, notes)"""
    size = len(data)
    if size < 8:
        return TRUNCATED, size, None
    n = struct.unpack_from("<Q", data)[0]
    if n > (size - 8) // NOTE:
        return TRUNCATED, size, None
    if size > 8 + n * NOTE:
        return TRAILING, 8 + n * NOTE, None
    notes = []
    for i in range(n):
        at = 8 + i * NOTE
        leaf_index, = struct.unpack_from("<Q", data, at)
        amount, = struct.unpack_from("<Q", data, at + 40)
        ident, secret = int.from_bytes(data[at + 8:at + 40], "little"), int.from_bytes(data[at + 48:at + 80], "little")
        for v, off in ((ident, at + 8), (secret, at + 48)):
            if v >= p:
                return NOT_BELOW_MODULUS, off, None
        notes.append((leaf_index, ident, amount, secret))
    return ACCEPTED, 0, notes


def expected_report(file_entries, file_root, layers, root):
    """What zkt_merkle_tree_load_file reports for a file against the tree rebuilt from its layer 0 (layers, root)."""
    bad = sorted(key for key, v in file_entries if layers[key[0]][key[1]] != v)
    return {"entries": len(file_entries), "mismatches": len(bad), "first_layer": bad[0][0] if bad else -1, "first_idx": bad[0][1] if bad else 0,
            "root_matches": file_root == root}
