"""zkt_poseidon_merkle_path_witness_dev: the witness of the reference's Merkle-path gadget (merkle_proof,
plonk-hashing/src/merkle/binary.rs:8-30) made on the device in ONE launch, bit for bit against the oracle composer's map
(tests/merkle_path_cases.py; the layout is pinned on the CPU by test_merkle_path_cases_oracle.py)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import fields as F, coracle as K, plonk as P
from helpers import field_elems

import merkle_path_cases as MC

POISON = 0x0BAD0BAD0BAD0BAD0BAD0BAD0BAD0BAD      # what every device-written range holds before the launch


def _load(ctx, cv, prm):
    return ctx.poseidon_load(prm.width, prm.half_full, prm.partial, K.fr_to_mont(cv, prm.rc),
                             K.fr_to_mont(cv, [x for row in prm.mds for x in row]), K.fr_to_mont(cv, [prm.domain_tag])[0])


def _poisoned(case):
    host = list(case.values)
    for b in case.bases:
        host[b:b + case.span] = [POISON] * case.span
    return host


class _Launch:
    """One case on the device: the map (poisoned where the launch writes) and the index vectors, freed on exit."""

    def __init__(self, ctx, case, host=None, leaf=None, bits=None, sibs=None, bases=None, n_vars=None):
        self.ctx, self.case, self.cv = ctx, case, case.cv
        self.n_vars = case.n_vars if n_vars is None else n_vars
        u32 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.uint32))
        arrays = [K.fr_to_mont(case.cv, _poisoned(case) if host is None else host), u32(case.leaf if leaf is None else leaf),
                  u32(case.bits if bits is None else bits), u32(case.sibs if sibs is None else sibs),
                  u32(case.bases if bases is None else bases), np.zeros((case.batch, 4), np.uint64)]
        self.d = []
        for a in arrays:
            d = ctx.alloc(a.nbytes)
            ctx.upload(d, a)
            self.d.append(d)
        self.d_vars, self.d_leaf, self.d_bits, self.d_sibs, self.d_base, self.d_roots = self.d

    def run(self, h, dense=False, validate_only=False):
        c = self.case
        kw = dict(path_base0=c.bases[0]) if dense else dict(d_path_base=self.d_base)
        self.ctx.poseidon_merkle_path_witness_dev(h, c.batch, c.height, self.d_vars, self.n_vars, self.d_leaf, self.d_bits, self.d_sibs,
                                                  d_out_roots=self.d_roots, validate_only=validate_only, **kw)

    def map(self):
        return K.fr_from_mont(self.cv, self.ctx.download(self.d_vars, (self.case.n_vars, 4)))

    def roots(self):
        return K.fr_from_mont(self.cv, self.ctx.download(self.d_roots, (self.case.batch, 4)))

    def free(self):
        for d in self.d:
            self.ctx.free(d)


def _check_whole_map(case, launch):
    """The whole map equals the oracle's: the paths are right and nothing outside them changed (the host map differs from
    the oracle's only inside the path ranges, where it holds the poison)."""
    got = launch.map()
    assert got == case.values
    assert launch.roots() == case.roots == [got[v] for v in case.root_vars]


@pytest.mark.parametrize("shape", range(5), ids=lambda k: "shape%d" % k)
@pytest.mark.parametrize("w", [3, 4, 5, 8])
@pytest.mark.parametrize("cvname", ["bn254", "bls12_381"])
def test_paths_equal_the_composers_map(cvname, w, shape):
    """Widths 3, 4, 5 and 8 (16, 16, 32 and 64 lanes per path) with a short synthetic schedule on both curves; heights 1, 2,
    3, 7; 1, PER_WAVE + 1 and 4 PER_WAVE + 1 paths; scattered (d_path_base) and dense (path_base0) ranges; bits all 0, all 1
    and mixed; a leaf and a sibling given as ZKT_VARIABLE_ZERO."""
    import zkt_plonk_amd as z
    height, batch, bits_mode, dense, zeros = MC.shapes(w)[shape]
    case = MC.build(cvname, w, False, height, batch, bits_mode, dense, zeros)
    ctx = z.Context(cvname, 0)
    h = _load(ctx, case.cv, case.prm)
    assert ctx.merkle_path_vars_per_level(h) == case.per_level == 6 + ctx.poseidon_gadget_vars_per_hash(h)
    launch = _Launch(ctx, case)
    launch.run(h, validate_only=True)
    launch.run(h, dense=dense)
    ctx.poseidon_gadget_check(h)
    _check_whole_map(case, launch)
    if dense:                          # the same ranges named one by one
        ctx.upload(launch.d_vars, K.fr_to_mont(case.cv, _poisoned(case)))
        launch.run(h, dense=False)
        ctx.poseidon_gadget_check(h)
        _check_whole_map(case, launch)
    launch.free()
    ctx.poseidon_free(h)
    ctx.close()


@pytest.mark.parametrize("w", [4, 5])
def test_paths_on_the_shipped_parameter_sets(w):
    """The BN254 x4 / x5 tables of the withdraw circuit (1288 / 1888 variables per hash) at height 2, PER_WAVE + 1 paths."""
    import zkt_plonk_amd as z
    case = MC.build("bn254", w, True, 2, MC.per_wave(w) + 1, "mixed", False, False)
    assert case.per_hash == {4: 1288, 5: 1888}[w]
    ctx = z.Context("bn254", 0)
    h = _load(ctx, case.cv, case.prm)
    launch = _Launch(ctx, case)
    launch.run(h)
    ctx.poseidon_gadget_check(h)
    _check_whole_map(case, launch)
    launch.free()
    ctx.poseidon_free(h)
    ctx.close()


@pytest.mark.parametrize("w", [4, 5, 8])
def test_a_bad_path_is_skipped_as_a_whole(w):
    """A bit of value 2, an index >= n_vars, a range running past the map: zkt_poseidon_gadget_check reports
    ZKT_ERR_INVALID_ARGUMENT, that path's range still holds the poison, the other paths of the launch are correct."""
    import zkt_plonk_amd as z
    import zkt_plonk_amd._lib as L
    case = MC.build("bn254", w, False, *MC.shapes(w)[0])
    assert case.batch == 4 * MC.per_wave(w) + 1 and case.height == 3
    ctx = z.Context("bn254", 0)
    h = _load(ctx, case.cv, case.prm)
    last = case.batch - 1
    faults = []
    host = _poisoned(case)                                   # the bit of level 1 of path 1 holds 2
    host[case.bits[1][1]] = 2
    faults.append((1, dict(host=host), {case.bits[1][1]: 2}))
    sibs = [list(s) for s in case.sibs]                      # a sibling index of the last path = n_vars
    sibs[last][2] = case.n_vars
    faults.append((last, dict(sibs=sibs), {}))
    leaf = list(case.leaf)                                   # a leaf index beyond the map
    leaf[2] = case.n_vars + 7
    faults.append((2, dict(leaf=leaf), {}))
    bits = [list(s) for s in case.bits]
    bits[0][0] = case.n_vars
    faults.append((0, dict(bits=bits), {}))
    # a range running past the map: the map handed over ends one variable before the end of the last path's range (the
    # allocation keeps its full size, so even a kernel that did not check would stay inside it)
    short = case.bases[last] + case.span - 1
    assert short == case.n_vars - 1 and max(v for v in [case.leaf[last]] + case.bits[last] + case.sibs[last] if v != MC.ZERO) < short
    faults.append((last, dict(n_vars=short), {}))
    for bad, kwargs, changed in faults:
        launch = _Launch(ctx, case, **kwargs)
        launch.run(h)
        with pytest.raises(L.ZktError) as e:
            ctx.poseidon_gadget_check(h)
        assert e.value.code == 1                             # ZKT_ERR_INVALID_ARGUMENT
        ctx.poseidon_gadget_check(h)                         # raised once, then cleared
        want = list(case.values)
        want[case.bases[bad]:case.bases[bad] + case.span] = [POISON] * case.span
        for k, v in changed.items():
            want[k] = v
        assert launch.map() == want, kwargs.keys()
        roots = launch.roots()
        assert [r for k, r in enumerate(roots) if k != bad] == [r for k, r in enumerate(case.roots) if k != bad] and roots[bad] == 0
        launch.free()
    ctx.poseidon_free(h)
    ctx.close()


def test_argument_errors_and_validate():
    """width = 2 is refused at the call (hash_two would hit FullBuffer), a negative height and a NULL required pointer too;
    height = 0 and batch = 0 enqueue nothing.  zkt_poseidon_merkle_path_validate accepts the good layout and names
    overlapping ranges and an input inside a written range."""
    import zkt_plonk_amd as z
    import zkt_plonk_amd._lib as L
    cv = F.BN254
    case = MC.build("bn254", 4, False, *MC.shapes(4)[1])       # dense, PER_WAVE + 1 paths of height 2
    ctx = z.Context("bn254", 0)
    h = _load(ctx, cv, case.prm)
    launch = _Launch(ctx, case)
    args = (case.batch, case.height, launch.d_vars, case.n_vars, launch.d_leaf, launch.d_bits, launch.d_sibs)
    prm2 = MC.synthetic_params(cv, 2)
    h2 = _load(ctx, cv, prm2)
    with pytest.raises(L.ZktError) as e:
        ctx.poseidon_merkle_path_witness_dev(h2, *args, d_path_base=launch.d_base)
    assert e.value.code == 1 and "width" in str(e.value)
    ctx.poseidon_free(h2)
    with pytest.raises(L.ZktError):
        ctx.poseidon_merkle_path_witness_dev(h, case.batch, -1, *args[2:], d_path_base=launch.d_base)
    for missing in (2, 4, 5, 6):                             # the map, the leaves, the bits, the siblings
        broken = list(args)
        broken[missing] = 0
        with pytest.raises(L.ZktError):
            ctx.poseidon_merkle_path_witness_dev(h, *broken, d_path_base=launch.d_base)
    with pytest.raises(L.ZktError):                          # dense ranges that do not fit the map are refused on the host
        ctx.poseidon_merkle_path_witness_dev(h, case.batch, case.height, launch.d_vars, case.n_vars - 1, *args[4:],
                                             path_base0=case.bases[0])
    before = launch.map()
    ctx.poseidon_merkle_path_witness_dev(h, case.batch, 0, *args[2:], d_path_base=launch.d_base)     # height 0: a no-op
    ctx.poseidon_merkle_path_witness_dev(h, 0, case.height, *args[2:], d_path_base=launch.d_base)    # no path: a no-op
    ctx.poseidon_merkle_path_witness_dev(h, case.batch, 0, 0, 0, 0, 0, 0)                             # ... whatever the pointers
    ctx.poseidon_gadget_check(h)
    assert launch.map() == before == _poisoned(case)
    # validate
    launch.run(h, validate_only=True)
    launch.run(h, dense=True, validate_only=True)
    bases = list(case.bases)
    bases[1] = bases[0] + case.span - 1
    overlap = _Launch(ctx, case, bases=bases)
    with pytest.raises(L.ZktError) as e:
        overlap.run(h, validate_only=True)
    assert e.value.code == 1 and "overlap" in str(e.value)
    overlap.free()
    bases[1] = case.n_vars - case.span + 1
    outside = _Launch(ctx, case, bases=bases)
    with pytest.raises(L.ZktError) as e:
        outside.run(h, validate_only=True)
    assert "outside the variable map" in str(e.value)
    outside.free()
    for kwargs in (dict(leaf=[case.leaf[0], case.bases[0] + 3] + list(case.leaf[2:])),
                   dict(sibs=[list(case.sibs[0][:-1]) + [case.bases[-1] + case.span - 1]] + [list(s) for s in case.sibs[1:]]),
                   dict(bits=[[case.bases[1]] + list(case.bits[0][1:])] + [list(s) for s in case.bits[1:]])):
        inside = _Launch(ctx, case, **kwargs)
        with pytest.raises(L.ZktError) as e:
            inside.run(h, validate_only=True)
        assert e.value.code == 1 and "the same launch writes" in str(e.value), kwargs.keys()
        inside.free()
    assert launch.map() == before                             # validation launches nothing
    launch.free()
    ctx.poseidon_free(h)
    ctx.close()


def _prove_from_device_witness(ctx, cv, cs, d_vars, blinders, vk_n, vk_commits):
    import zkt_plonk_amd as z
    to_idx = lambda ws: np.array([0xFFFFFFFF if v == P.ZERO_VAR else v for v in ws], dtype=np.uint32)
    d_idx = []
    for ws in (cs.w_l, cs.w_r, cs.w_o):
        d = ctx.alloc(4 * len(ws))
        ctx.upload(d, to_idx(ws))
        d_idx.append(d)
    pi_pos = sorted(cs.pi)
    prep = ctx.prepare_vars_dev(d_vars, len(cs.values), d_idx[0], d_idx[1], d_idx[2], cs.n_gates, K.fr_to_mont(cv, cs.table),
                                pi_pos, K.fr_to_mont(cv, [cs.pi[k] for k in pi_pos]), K.fr_to_mont(cv, blinders))
    tr = z.seed_transcript(z.Transcript("merlin", "ZKT Plonk", fr_bits=cv.fr.bits, fq_bytes=8 * cv.fq.limbs64), vk_n, vk_commits)
    try:
        return ctx.prove_prepared(prep, tr)
    finally:
        for d in d_idx:
            ctx.free(d)


def test_the_withdraw_circuit_with_its_merkle_path_made_on_the_device():
    """WithdrawCircuit on BN254 x4, one note, HEIGHT 7 (15 640 gates, n = 2^14), synthesised by the oracle composer.  The
    host map holds poison in every hash trace AND in every select variable of the path: the host walks no path.
    PoseidonGadget records three hash calls of depth 0, two of depth 1 and ONE path, fill is three launches, the map equals
    the composer's, the nullifier and the new leaf read back from it are the public inputs, the proof bytes equal the CPU
    oracle's and its verifier accepts."""
    import zkt_plonk_amd as z
    from oracle import composer as OC, fastplonk as FP
    cv = F.BN254
    p = cv.fr.p
    prm = MC.shipped_params(4)
    cs, public_inputs = OC.withdraw_instance(cv, prm, inputs=1, height=7, seed=11)
    assert cs.n_gates == 15640 and cs.check_satisfied() and len(cs.hash_calls) == 3 + 7 + 2
    n = cs.circuit_bound()
    assert n == 1 << 14
    tau = 0x5EED5EED1234567890ABCDEF % p
    srs = K.srs_mont(cv, tau, n + 8)
    be = K.CBackend(cv, srs)
    evals = {k: K.fr_to_mont(cv, v) for k, v in P.setup_evals(be, cs).items()}
    keys = FP.setup(cv, srs, 14, evals)
    vk = keys.verifier_key(cv, cs.pi.keys())
    a, b, c = cs.wire_evals(cs.n_gates)
    blinders = field_elems(p, 1414, P.NUM_BLINDERS)
    want = FP.prove(cv, srs, keys, K.fr_to_mont(cv, a), K.fr_to_mont(cv, b), K.fr_to_mont(cv, c), K.fr_to_mont(cv, cs.table),
                    dict(cs.pi), P.new_seeded_transcript(cv, vk), blinders)
    ctx = z.Context(cv.name, 0)
    ctx.srs_load(srs)
    z.GpuProver.setup(ctx, 14, evals)
    g = z.PoseidonGadget(ctx, prm.width, prm.half_full, prm.partial, K.fr_to_mont(cv, prm.rc),
                         K.fr_to_mont(cv, [x for row in prm.mds for x in row]), K.fr_to_mont(cv, [prm.domain_tag])[0])
    per, S = g.vars_per_hash, g.vars_per_level
    assert (per, S) == (1288, 1294)
    host = list(cs.values)
    plain = lambda ins: [0xFFFFFFFF if v == P.ZERO_VAR else v for (v, co, off) in ins if (co, off) == (1, 0)]
    levels = []
    for base, ins in cs.hash_calls:
        host[base:base + per] = [POISON] * per
        if plain(ins) == [base - 4, base - 1]:           # a level of the path: hash_two of the two selects in front of it
            host[base - 6:base] = [POISON] * 6
            levels.append(base)
        else:
            assert len(plain(ins)) == len(ins)
            g.hash(base, plain(ins))
    assert levels == [levels[0] + k * S for k in range(7)]
    # the path's inputs from the wiring: the gate making x_l has wires (bit, sibling, x_l), the one making y_l (bit, cur, y_l)
    bit_vars, sibling_vars = [], []
    for base in levels:
        row = cs.w_o.index(base - 6)
        bit_vars.append(cs.w_l[row])
        sibling_vars.append(cs.w_r[row])
    leaf_var = cs.w_r[cs.w_o.index(levels[0] - 5)]
    root_var = g.merkle_path(levels[0] - 6, leaf_var, bit_vars, sibling_vars)
    assert root_var == levels[-1] + g.hash_var_offset
    assert [len(l) for l in g.levels()] == [3, 2] and len(g.paths) == 1
    n_vars = len(cs.values)
    assert sum(v == POISON for v in host) == 12 * per + 7 * 6
    d_vars = ctx.alloc(n_vars * 32)
    ctx.upload(d_vars, K.fr_to_mont(cv, host))
    assert g.fill(d_vars, n_vars) == 3
    got_map = K.fr_from_mont(cv, ctx.download(d_vars, (n_vars, 4)))
    assert got_map == cs.values
    # the nullifier and the new leaf are public: the rows that expose them carry the device-made values
    pi_rows = sorted(cs.pi)
    assert [cs.pi[k] for k in pi_rows] == public_inputs
    nullifier_row, new_leaf_row = pi_rows[1], pi_rows[4]
    for row, call in ((nullifier_row, cs.hash_calls[1]), (new_leaf_row, cs.hash_calls[-1])):
        assert cs.w_o[row] == call[0] + g.hash_var_offset
        assert got_map[cs.w_o[row]] == cs.pi[row]
    got = _prove_from_device_witness(ctx, cv, cs, d_vars, blinders, vk.n, vk.commits)
    assert got == want and len(got) == 802
    assert P.verify(cv, tau, vk, P.proof_deserialize(cv, got), P.new_seeded_transcript(cv, vk), public_inputs)
    ctx.free(d_vars)
    g.close()
    ctx.close()
