"""zkt_merkle_tree: the reference's note tree (gadgets/src/merkle_tree.rs:57-111) kept and appended on the device, bit for bit
against the oracle's tree after add_leaf leaf by leaf (tests/merkle_tree_cases.py; the equality with the dense rebuild the
append relies on is pinned on the CPU by test_merkle_tree_cases_oracle.py)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import fields as F, coracle as K, plonk as P

import merkle_path_cases as MC
import merkle_tree_cases as TC

POISON = 0x0BAD0BAD0BAD0BAD0BAD0BAD0BAD0BAD
INT_MAX = 2 ** 31 - 1
POLICIES = {"policy": 0, "wide": 1, "tail": INT_MAX}


def _load(ctx, cv, prm):
    return ctx.poseidon_load(prm.width, prm.half_full, prm.partial, K.fr_to_mont(cv, prm.rc),
                             K.fr_to_mont(cv, [x for row in prm.mds for x in row]), K.fr_to_mont(cv, [prm.domain_tag])[0])


def _root(ctx, cv, t):
    return K.fr_from_mont(cv, ctx.merkle_tree_root(t).reshape(1, 4))[0]


def _check_tree(ctx, cv, t, snap):
    """Count, root and every stored node of every layer equal the oracle's."""
    height, count, _ = ctx.merkle_tree_info(t)
    assert (height, count) == (snap.height, snap.count)
    assert _root(ctx, cv, t) == snap.root
    for L in range(height):
        assert K.fr_from_mont(cv, ctx.merkle_tree_layer(t, L, 0, snap.stored(L))) == snap.layer(L), L


def _append(ctx, t, d_leaves, batches, host_leaves=None):
    """The batches in order from the device buffer (or, with host_leaves, through the host entry)."""
    s = 0
    for m in batches:
        if host_leaves is not None:
            assert ctx.merkle_tree_append(t, host_leaves[s:s + m]) == s
        else:
            assert ctx.merkle_tree_append_dev(t, d_leaves + 32 * s, m) == s
        s += m


@pytest.mark.parametrize("w", TC.WIDTHS)
@pytest.mark.parametrize("cvname", TC.CURVES)
def test_append_equals_the_reference(cvname, w):
    """Widths 3, 4, 5 and 8 (16, 16, 32, 64 lanes per hash) with the short synthetic schedule on both curves; heights 1, 2, 3,
    7 and 64; 1, 2, 3, 5, 8 and min(2^height, 37) leaves; appended as one batch, leaf by leaf (through the host entry) and in
    uneven batches that start at an odd index and end on a left child, the second of them 4 PER_WAVE + 2 parents wide; each
    under the policy, with every level in the wide kernel and with every level in the tail."""
    import zkt_plonk_amd as z
    ctx = z.Context(cvname, 0)
    over = 0
    for height in TC.HEIGHTS:
        case = TC.build(cvname, w, height)
        cv = case.cv
        h = _load(ctx, cv, case.prm)
        mont = K.fr_to_mont(cv, case.leaves)
        d_leaves = ctx.alloc(mont.nbytes)
        ctx.upload(d_leaves, mont)
        for n in TC.leaf_counts(height):
            for name, batches in TC.splits(n, w).items():
                over += any(TC.level_parents(sum(batches[:k]), m, 0) > TC.tail_groups(w) for k, m in enumerate(batches))
                for split in POLICIES.values():
                    t = ctx.merkle_tree_create(h, height, min(1 << height, 64))
                    ctx.debug_merkle_tree_split(t, split)
                    _append(ctx, t, d_leaves, batches, mont if name == "single" else None)
                    _check_tree(ctx, cv, t, case.snaps[n])
                    ctx.merkle_tree_free(t)
        ctx.free(d_leaves)
        ctx.poseidon_free(h)
    assert over >= 4            # heights 7 and 64, 37 leaves, as one batch and uneven: more parents than the tail's lane groups
    ctx.close()


@pytest.mark.parametrize("policy", sorted(POLICIES))
def test_a_level_wider_than_a_block_and_than_the_tail(policy):
    """1100 leaves at height 11 as one batch: 550 parents at level 0 are five blocks of the wide kernel and more than a level
    of the tail may hold, so even with every level sent to the tail that one is a wide launch and the tail starts at level 1
    on 275 parents.  Then 99 more from a second tree state (1001 + 99): an odd start with a stored left neighbour."""
    import zkt_plonk_amd as z
    case = TC.build_large()
    cv = case.cv
    ctx = z.Context("bn254", 0)
    h = _load(ctx, cv, case.prm)
    mont = K.fr_to_mont(cv, case.leaves)
    d_leaves = ctx.alloc(mont.nbytes)
    ctx.upload(d_leaves, mont)
    t = ctx.merkle_tree_create(h, case.height, 2048)
    ctx.debug_merkle_tree_split(t, POLICIES[policy])
    assert ctx.merkle_tree_append_dev(t, d_leaves, 1100) == 0
    _check_tree(ctx, cv, t, case.snaps[1100])
    ctx.merkle_tree_free(t)
    t = ctx.merkle_tree_create(h, case.height, 1100)
    ctx.debug_merkle_tree_split(t, POLICIES[policy])
    assert ctx.merkle_tree_append_dev(t, d_leaves, 1001) == 0
    _check_tree(ctx, cv, t, case.snaps[1001])
    assert ctx.merkle_tree_append_dev(t, d_leaves + 32 * 1001, 99) == 1001
    _check_tree(ctx, cv, t, case.snaps[1100])
    ctx.merkle_tree_free(t)
    ctx.free(d_leaves)
    ctx.poseidon_free(h)
    ctx.close()


def test_height_64_on_the_shipped_tables():
    """BN254 x5 as the withdraw circuit hashes, height 64, 13 leaves appended as 5 + 8 (the shape of withdraw_instance): root
    and all 64 layers after each append; merkle_path of every index up to the count and of 2^64 - 1."""
    import zkt_plonk_amd as z
    case = TC.build_shipped()
    cv = case.cv
    ctx = z.Context("bn254", 0)
    h = _load(ctx, cv, case.prm)
    mont = K.fr_to_mont(cv, case.leaves)
    d_leaves = ctx.alloc(mont.nbytes)
    ctx.upload(d_leaves, mont)
    t = ctx.merkle_tree_create(h, 64, 13)
    assert ctx.merkle_tree_append_dev(t, d_leaves, 5) == 0
    _check_tree(ctx, cv, t, case.snaps[5])
    assert ctx.merkle_tree_append_dev(t, d_leaves + 32 * 5, 8) == 5
    snap = case.snaps[13]
    _check_tree(ctx, cv, t, snap)
    idx = snap.path_indices()
    assert idx[-1] == 2 ** 64 - 1 and 13 in idx
    got = ctx.merkle_tree_paths(t, idx)
    assert [K.fr_from_mont(cv, g) for g in got] == [snap.merkle_path(i) for i in idx]
    ctx.merkle_tree_free(t)
    ctx.free(d_leaves)
    ctx.poseidon_free(h)
    ctx.close()


def test_capacity_and_argument_errors():
    """A tree filled exactly to 2^height (heights 1, 2, 3) and to a capacity below it: one leaf more is refused with
    ZKT_ERR_INVALID_ARGUMENT and count, layers and root are what they were; m = 0 changes nothing; a fresh tree has the root
    0; create refuses a height outside 1 .. 64, a capacity outside 1 .. min(2^height, ZKT_MERKLE_TREE_MAX) and width 2;
    zkt_merkle_tree_layer refuses layer = height and a range past the stored nodes."""
    import zkt_plonk_amd as z
    import zkt_plonk_amd._lib as L
    cvname, w = "bn254", 4
    ctx = z.Context(cvname, 0)
    cv = F.CURVES[cvname]
    for height, capacity, n in ((1, 2, 2), (2, 4, 3), (3, 8, 8), (3, 5, 5), (7, 3, 3)):
        case = TC.build(cvname, w, height)
        h = _load(ctx, cv, case.prm)
        mont = K.fr_to_mont(cv, case.leaves)
        t = ctx.merkle_tree_create(h, height, capacity)
        assert ctx.merkle_tree_info(t) == (height, 0, capacity)
        assert _root(ctx, cv, t) == 0                                  # MerkleTreeStore::default().root, not the empty hash
        assert ctx.merkle_tree_append(t, mont[:0]) == 0                # m = 0
        assert ctx.merkle_tree_append_dev(t, 0, 0) == 0
        _check_tree(ctx, cv, t, case.snaps[0])
        assert ctx.merkle_tree_append(t, mont[:n]) == 0
        _check_tree(ctx, cv, t, case.snaps[n])
        if n < capacity:                                               # (2, 4, 3): two more do not fit, one does
            with pytest.raises(L.ZktError) as e:
                ctx.merkle_tree_append(t, mont[:2])
            assert e.value.code == 1
            _check_tree(ctx, cv, t, case.snaps[n])
            assert ctx.merkle_tree_append(t, mont[n:n + 1]) == n
            n += 1
        assert ctx.merkle_tree_info(t)[1] == n == capacity
        before = [ctx.merkle_tree_layer(t, k, 0, ((n - 1) >> k) + 1) for k in range(height)], ctx.merkle_tree_root(t)
        for extra in (mont[:1], mont[:2]):
            with pytest.raises(L.ZktError) as e:
                ctx.merkle_tree_append(t, extra)
            assert e.value.code == 1 and "capacity" in str(e.value)
        assert ctx.merkle_tree_append(t, mont[:0]) == n
        assert ctx.merkle_tree_info(t) == (height, n, capacity)
        after = [ctx.merkle_tree_layer(t, k, 0, ((n - 1) >> k) + 1) for k in range(height)], ctx.merkle_tree_root(t)
        assert all(np.array_equal(x, y) for x, y in zip(before[0], after[0])) and np.array_equal(before[1], after[1])
        for layer, first, cnt in ((height, 0, 1), (-1, 0, 1), (0, 0, n + 1), (0, n, 1), (height - 1, ((n - 1) >> (height - 1)) + 1, 1)):
            with pytest.raises(L.ZktError) as e:
                ctx.merkle_tree_layer(t, layer, first, cnt)
            assert e.value.code == 1
        assert ctx.merkle_tree_layer(t, 0, n, 0).shape == (0, 4)       # an empty range at the end is a range
        ctx.merkle_tree_free(t)
        ctx.poseidon_free(h)
    h = _load(ctx, cv, MC.synthetic_params(cv, 4))
    for height, capacity in ((0, 1), (65, 1), (-1, 1), (3, 0), (3, 9), (1, 3), (64, (1 << 24) + 1), (30, (1 << 24) + 1)):
        with pytest.raises(L.ZktError) as e:
            ctx.merkle_tree_create(h, height, capacity)
        assert e.value.code == 1, (height, capacity)
    ctx.poseidon_free(h)
    h2 = _load(ctx, cv, MC.synthetic_params(cv, 2))
    with pytest.raises(L.ZktError) as e:
        ctx.merkle_tree_create(h2, 3, 8)
    assert e.value.code == 1 and "width" in str(e.value)
    ctx.poseidon_free(h2)
    ctx.close()


def _var_layout(height, k, n_extra=3):
    """k paths in a map: per path a gap element, `height` bits, `height` siblings (PoECircuit::synthesize's order)."""
    bit0 = [n_extra + p * (2 * height + 1) + 1 for p in range(k)]
    sib0 = [b + height for b in bit0]
    return bit0, sib0, sib0[-1] + height + n_extra


@pytest.mark.parametrize("height,w", [(3, 3), (7, 5), (2, 8), (64, 4)])
def test_paths_and_paths_to_variables(height, w):
    """After each of several appends: merkle_path of every index below the count, of the count itself and of 2^height - 1;
    the same paths written into a poisoned variable map sit where they are asked for, with their bits, and nothing else
    changes; bit_var0 = NULL leaves the bit ranges poisoned.  Overlapping or out-of-range ranges, an index >= 2^height and k
    above the cap are refused with nothing written."""
    import zkt_plonk_amd as z
    import zkt_plonk_amd._lib as L
    cvname = "bls12_381" if w == 5 else "bn254"
    case = TC.build(cvname, w, height)
    cv = case.cv
    ctx = z.Context(cvname, 0)
    h = _load(ctx, cv, case.prm)
    tree = z.MerkleTree(ctx, h, height, min(1 << height, 64))
    mont = K.fr_to_mont(cv, case.leaves)
    have = 0
    for n in [0] + TC.leaf_counts(height):
        assert tree.append(mont[have:n]) == have
        have = n
        snap = case.snaps[n]
        idx = snap.path_indices()
        want = [snap.merkle_path(i) for i in idx]
        assert [K.fr_from_mont(cv, g) for g in tree.paths(idx)] == want
        bit0, sib0, n_vars = _var_layout(height, len(idx))
        d_vars = ctx.alloc(32 * n_vars)
        poisoned = K.fr_to_mont(cv, [POISON] * n_vars)
        for with_bits in (True, False):
            ctx.upload(d_vars, poisoned)
            tree.paths_to_variables(idx, d_vars, n_vars, sib0, bit0 if with_bits else None)
            expect = [POISON] * n_vars
            for p, i in enumerate(idx):
                expect[sib0[p]:sib0[p] + height] = want[p]
                if with_bits:
                    expect[bit0[p]:bit0[p] + height] = [(i >> k) & 1 for k in range(height)]
            assert K.fr_from_mont(cv, ctx.download(d_vars, (n_vars, 4))) == expect
        ctx.free(d_vars)
    assert tree.count == have and np.array_equal(tree.layer(0), mont[:have])
    # refusals: everything is checked on the host, nothing is written
    idx = [0, 1]
    bit0, sib0, n_vars = _var_layout(height, 2)
    d_vars = ctx.alloc(32 * n_vars)
    poisoned = K.fr_to_mont(cv, [POISON] * n_vars)
    ctx.upload(d_vars, poisoned)
    bad = [dict(sibling_var0=[sib0[0], sib0[0] + height - 1], bit_var0=None),          # two sibling ranges overlap
           dict(sibling_var0=sib0, bit_var0=[bit0[0], sib0[1] - height + 1]),         # a bit range runs into a sibling range
           dict(sibling_var0=sib0, bit_var0=[bit0[0], bit0[0]]),                      # the same range twice
           dict(sibling_var0=[sib0[0], n_vars - height + 1], bit_var0=None),           # one element past the map
           dict(sibling_var0=[sib0[0], n_vars], bit_var0=None),
           dict(sibling_var0=sib0, bit_var0=[0xFFFFFFFF, bit0[1]])]
    for kw in bad:
        with pytest.raises(L.ZktError) as e:
            tree.paths_to_variables(idx, d_vars, n_vars, **kw)
        assert e.value.code == 1, kw
    tree.paths_to_variables(idx, d_vars, n_vars, [sib0[0], n_vars - height], None)     # the last range the map has room for
    ctx.upload(d_vars, poisoned)
    if height < 64:
        for call in (lambda: tree.paths([0, 1 << height]), lambda: tree.paths_to_variables([1 << height, 0], d_vars, n_vars, sib0, bit0)):
            with pytest.raises(L.ZktError) as e:
                call()
            assert e.value.code == 1 and "2^height" in str(e.value)
    many = [0] * 4097                                                                    # ZKT_MERKLE_TREE_PATHS_MAX + 1
    for call in (lambda: tree.paths(many), lambda: tree.paths_to_variables(many, d_vars, 1 << 30, list(range(0, 4097 * height, height)))):
        with pytest.raises(L.ZktError) as e:
            call()
        assert e.value.code == 1 and "ZKT_MERKLE_TREE_PATHS_MAX" in str(e.value)
    assert tree.paths([]).shape == (0, height, 4)
    tree.paths_to_variables([], d_vars, n_vars, [], [])
    assert np.array_equal(ctx.download(d_vars, (n_vars, 4)), poisoned)
    ctx.free(d_vars)
    tree.close()
    ctx.poseidon_free(h)
    ctx.close()


@pytest.mark.parametrize("height,w", [(3, 3), (3, 5), (7, 3), (7, 5)])
def test_the_tree_feeds_the_merkle_path_witness(height, w):
    """The seam the tree exists for: append leaves, write the paths of some indices into a variable map with
    paths_to_variables_dev, put the leaf values in as variables, run zkt_poseidon_merkle_path_witness_dev on that map: every
    root it computes is zkt_merkle_tree_root."""
    import zkt_plonk_amd as z
    case = TC.build("bn254", w, height)
    cv = case.cv
    ctx = z.Context("bn254", 0)
    h = _load(ctx, cv, case.prm)
    n = len(case.leaves)
    tree = z.MerkleTree(ctx, h, height, n)
    mont = K.fr_to_mont(cv, case.leaves)
    assert tree.append(mont[:n // 2]) == 0 and tree.append(mont[n // 2:]) == n // 2
    idx = sorted({0, 1, n // 2 - 1, n // 2, n - 2, n - 1})
    k, span = len(idx), height * ctx.merkle_path_vars_per_level(h)
    n_in = 1 + 2 * height                                  # the leaf, `height` bits, `height` siblings
    base0 = k * n_in
    n_vars = base0 + k * span
    host = [POISON] * n_vars
    leaf_var = [p * n_in for p in range(k)]
    bit0 = [v + 1 for v in leaf_var]
    sib0 = [v + 1 + height for v in leaf_var]
    for p, i in enumerate(idx):
        host[leaf_var[p]] = case.leaves[i]
    u32 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.uint32))
    arrays = [K.fr_to_mont(cv, host), u32(leaf_var), u32([[b + j for j in range(height)] for b in bit0]),
              u32([[s + j for j in range(height)] for s in sib0]), np.zeros((k, 4), np.uint64)]
    d = []
    for a in arrays:
        d.append(ctx.alloc(a.nbytes))
        ctx.upload(d[-1], a)
    d_vars, d_leaf, d_bits, d_sibs, d_roots = d
    tree.paths_to_variables(idx, d_vars, n_vars, sib0, bit0)
    ctx.poseidon_merkle_path_witness_dev(h, k, height, d_vars, n_vars, d_leaf, d_bits, d_sibs, validate_only=True, path_base0=base0)
    ctx.poseidon_merkle_path_witness_dev(h, k, height, d_vars, n_vars, d_leaf, d_bits, d_sibs, path_base0=base0, d_out_roots=d_roots)
    ctx.poseidon_gadget_check(h)
    root = K.fr_from_mont(cv, tree.root().reshape(1, 4))[0]
    assert root == case.snaps[n].root
    assert K.fr_from_mont(cv, ctx.download(d_roots, (k, 4))) == [root] * k
    assert POISON not in K.fr_from_mont(cv, ctx.download(d_vars, (n_vars, 4)))
    for x in d:
        ctx.free(x)
    tree.close()
    ctx.poseidon_free(h)
    ctx.close()


def _tree_round_trip(ctx, cv, case):
    """Create, append in two batches, read paths and the root, free: everything the tree enqueues, on `ctx`."""
    h = _load(ctx, cv, case.prm)
    tree = ctx.merkle_tree_create(h, case.height, len(case.leaves))
    mont = K.fr_to_mont(cv, case.leaves)
    ctx.merkle_tree_append(tree, mont[:5])
    d_leaves = ctx.alloc(mont.nbytes)
    ctx.upload(d_leaves, mont)
    ctx.merkle_tree_append_dev(tree, d_leaves + 32 * 5, len(case.leaves) - 5)
    paths = ctx.merkle_tree_paths(tree, [0, 5, len(case.leaves)])
    root = _root(ctx, cv, tree)
    ctx.merkle_tree_free(tree)
    ctx.free(d_leaves)
    ctx.poseidon_free(h)
    return root, paths


def test_the_tree_leaves_the_prover_alone_and_works_on_a_fork():
    """On a context with a loaded SRS and circuit a proof announced with zkt_prove_set_next has the same bytes whether or not
    a tree is created, appended to and read on that context before it runs; a tree on a forked context gives the root of one
    on its parent."""
    import zkt_plonk_amd as z
    cv = F.BN254
    case = TC.build("bn254", 5, 7)
    cs = P.test_circuit(cv)
    n = cs.circuit_bound()
    srs = K.srs_mont(cv, 0x5EED, n + 8)
    be = K.CBackend(cv, srs)
    pk, _, vk = P.setup(be, [None] * (n + 8), cs, True)
    blinders = [[(i + 1 + 100 * k) * 0x9E3779B97F4A7C15 % cv.fr.p for i in range(P.NUM_BLINDERS)] for k in range(2)]
    ctx = z.Context(cv.name, 0)
    try:
        ctx.srs_load(srs)
        z.GpuProver(ctx, n.bit_length() - 1, {k: K.fr_to_mont(cv, pk.polys[k]) for k in z.PK_ORDER})
        wires = [K.fr_to_mont(cv, x) for x in cs.wire_evals(cs.n_gates)]
        table = K.fr_to_mont(cv, cs.table)
        pi_pos = sorted(cs.pi)
        pi_vals = K.fr_to_mont(cv, [cs.pi[k] for k in pi_pos])
        d = []
        for x in wires:
            d.append(ctx.alloc(x.nbytes))
            ctx.upload(d[-1], x)

        def tr():
            return z.seed_transcript(z.Transcript("merlin", "ZKT Plonk"), vk.n, vk.commits)

        def two_proofs(between):
            preps = [ctx.prepare_dev(d[0], d[1], d[2], cs.n_gates, table, pi_pos, pi_vals, K.fr_to_mont(cv, x)) for x in blinders]
            first = ctx.prove_prepared(preps[0], tr(), preps[1])            # proof 1 is announced
            got = between()
            return first, ctx.prove_prepared(preps[1], tr()), got

        plain = two_proofs(lambda: None)
        with_tree = two_proofs(lambda: _tree_round_trip(ctx, cv, case))
        assert with_tree[:2] == plain[:2] and len(plain[0]) > 0 and plain[0] != plain[1]
        root, paths = with_tree[2]
        snap = case.snaps[len(case.leaves)]
        assert root == snap.root
        assert [K.fr_from_mont(cv, g) for g in paths] == [snap.merkle_path(i) for i in (0, 5, len(case.leaves))]
        fork = ctx.fork()
        try:
            f_root, f_paths = _tree_round_trip(fork, cv, case)
        finally:
            fork.close()
        assert f_root == root and np.array_equal(f_paths, paths)
        assert two_proofs(lambda: None)[:2] == plain[:2]                    # and the parent is none the worse
        for x in d:
            ctx.free(x)
    finally:
        ctx.close()
