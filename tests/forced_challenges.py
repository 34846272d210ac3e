"""Proofs at chosen Fiat-Shamir challenges: the cases, and the helpers that drive the oracle and the device through them.

zkt_prove_with takes its transcript as four callbacks, so a transcript that hands out chosen values for named challenges
drives oracle.plonk.prove and the device prover identically.  The cases are the challenge values for which prove.rs takes
a branch of its own -- a refusal (equal challenges, a zero denominator in a grand product, xi = 1, a quotient too short to
split) or an algebraic edge the reference proves through (xi on the domain, xi = 0, eta in {0, 1}, alpha = 1, ...).

tests/test_forced_challenges_oracle.py pins every case's outcome on the CPU oracle against the literal written here;
tests/test_gpu_forced_challenges.py holds the device to the same literal (and, for a proof, to the oracle's bytes).

An expected outcome is "proof", an error code of include/zkt_plonk.h, or a tuple of codes where the reference and the
device notice the same defect at different places:
    ZeroDivisionError                         -> 6  ZKT_ERR_ZERO_DENOMINATOR
    AssertionError "challenges must be ..."   -> 7  ZKT_ERR_EQUAL_CHALLENGES
    IndexError (quotient too short to split)  -> 9  ZKT_ERR_QUOTIENT_TOO_SHORT
    ValueError TooManyCoefficients            -> 5  ZKT_ERR_TOO_MANY_COEFFICIENTS"""
import ctypes
from types import SimpleNamespace

import numpy as np

from oracle import plonk as P, coracle as K
from helpers import field_elems

PROOF = "proof"
CHALLENGES = ("beta", "gamma", "delta", "epsilon", "alpha", "xi", "eta")

# (name, expected outcome) of cases(), in its order.  Literals: what the reference does at these challenges.
EXPECTED = (
    ("plain", PROOF),
    ("xi_w1", PROOF), ("xi_whalf", PROOF), ("xi_wlast", PROOF),      # Z_H(xi) = 0, L_1(xi) = 0; xi_wlast: xi w = 1
    ("xi_0", PROOF),
    ("xi_1", 6),
    ("alpha_0", 9),
    ("alpha_1", PROOF),
    ("beta_0", (5, 9)),          # z1 = 1 trims to one coefficient, its blinders land at X^1..X^3: the quotient is no polynomial;
                                 # the reference fails committing q_hi (5), the device at its own degree check (9)
    ("eta_0", PROOF), ("eta_1", PROOF),
    ("delta_0", PROOF), ("gamma_0", PROOF),
    ("eps_0", 6), ("delta_m1", 6),
    ("den_row0", 6), ("den_rown2", 6),
    ("den_rown1", PROOF),        # row n - 1 is outside the permutation product
    ("beta_eq_gamma", 7), ("beta_eq_delta", 7), ("beta_eq_eps", 7), ("gamma_eq_delta", 7), ("gamma_eq_eps", 7),
    ("delta_eq_eps", 7),
    ("lk_row0", 6), ("lk_rown2", 6),
    # Row n - 1 is outside the lookup product too, but no whole proof can show it: the tails of h1 and h2 are the zeros of the
    # padded table, so rows n - 2 and n - 1 hold the same pair and the epsilon aimed at row n - 1 (it is epsilon = 0) hits
    # row n - 2 as well.  The reference refuses; the row's exclusion is tested on arbitrary vectors through
    # zkt_debug_grand_products.
    ("lk_rown1", 6),
    ("beta_1", PROOF), ("alpha_m1", PROOF), ("eta_m1", PROOF),
)
NAMES = tuple(name for name, _ in EXPECTED)
# the cases whose outcome depends on where in the vectors something happens, for a shape of several scan blocks
POSITION_EXPECTED = (("xi_wlast", PROOF), ("xi_0", PROOF), ("eta_0", PROOF), ("den_rown1", PROOF), ("den_blk2", 6),
                     ("den_rown2", 6))
POSITION_NAMES = tuple(name for name, _ in POSITION_EXPECTED)
SECOND_BLOCK_ROW = 1024 + 317    # inside the second 1024-element block of the scans, on a live gate of the larger shape


def matches(outcome, expected):
    """outcome: "proof" or a code; expected: a literal of EXPECTED."""
    return outcome in expected if isinstance(expected, tuple) else outcome == expected


class ForcedTranscript:
    """Forwards everything to the oracle transcript `inner`.  challenge_scalar(label) always draws from `inner` first, so
    the transcript's state advances as usual, then substitutes forced[label]: a value, or a callable of the dict of the
    challenges already returned.  `drawn` keeps what was returned, by label."""

    def __init__(self, inner, forced):
        self.inner = inner
        self.cv = inner.cv
        self.forced = dict(forced)
        self.drawn = {}

    def append_u64(self, label, item):
        self.inner.append_u64(label, item)

    def append_scalar(self, label, item):
        self.inner.append_scalar(label, item)

    def append_scalars(self, label, items):
        self.inner.append_scalars(label, items)

    def append_commitment(self, label, item):
        self.inner.append_commitment(label, item)

    def challenge_scalar(self, label):
        v = self.inner.challenge_scalar(label)
        if label in self.forced:
            f = self.forced[label]
            v = (f(dict(self.drawn)) if callable(f) else f) % self.cv.fr.p
        self.drawn[label] = v
        return v


def den_gamma(cv, cs, epk, n, row):
    """gamma, as a function of beta, that makes the first factor of the permutation product's denominator vanish at `row`:
    gamma = -(a_row + beta sigma1_row)   (permutation/mod.rs:213-221)."""
    p = cv.fr.p
    a = cs.wire_evals(n)[0][row]
    s1 = epk.sigma1[row]
    return lambda ch: -(a + ch["beta"] * s1) % p


def lk_epsilon(cv, h1, h2, row):
    """epsilon, as a function of delta, that makes the first factor of the lookup product's denominator vanish at `row`:
    epsilon (1 + delta) + h1_row + delta h2_row = 0   (lookup/mod.rs:120-131)."""
    p = cv.fr.p
    return lambda ch: -(h1[row] + ch["delta"] * h2[row]) * pow(1 + ch["delta"], -1, p) % p


def cases(cv, cs, pk, epk, n, trace):
    """[(name, forced, expected)] in the order of EXPECTED.  `trace`: the ProverTrace of an unforced oracle proof of the
    same circuit (h1 / h2 depend on no challenge)."""
    p = cv.fr.p
    w = cv.fr.root_of_unity(n)
    h1, h2 = trace.evals["h1"], trace.evals["h2"]
    same = lambda other: (lambda ch: ch[other])
    forced = {
        "plain": {},
        "xi_w1": {"xi": w}, "xi_whalf": {"xi": pow(w, n // 2, p)}, "xi_wlast": {"xi": pow(w, n - 1, p)},
        "xi_0": {"xi": 0}, "xi_1": {"xi": 1},
        "alpha_0": {"alpha": 0}, "alpha_1": {"alpha": 1},
        "beta_0": {"beta": 0},
        "eta_0": {"eta": 0}, "eta_1": {"eta": 1},
        "delta_0": {"delta": 0}, "gamma_0": {"gamma": 0},
        "eps_0": {"epsilon": 0}, "delta_m1": {"delta": p - 1},
        "den_row0": {"gamma": den_gamma(cv, cs, epk, n, 0)},
        "den_rown2": {"gamma": den_gamma(cv, cs, epk, n, n - 2)},
        "den_rown1": {"gamma": den_gamma(cv, cs, epk, n, n - 1)},
        "beta_eq_gamma": {"gamma": same("beta")}, "beta_eq_delta": {"delta": same("beta")},
        "beta_eq_eps": {"epsilon": same("beta")}, "gamma_eq_delta": {"delta": same("gamma")},
        "gamma_eq_eps": {"epsilon": same("gamma")}, "delta_eq_eps": {"epsilon": same("delta")},
        "lk_row0": {"epsilon": lk_epsilon(cv, h1, h2, 0)},
        "lk_rown2": {"epsilon": lk_epsilon(cv, h1, h2, n - 2)},
        "lk_rown1": {"epsilon": lk_epsilon(cv, h1, h2, n - 1)},
        "beta_1": {"beta": 1}, "alpha_m1": {"alpha": p - 1}, "eta_m1": {"eta": p - 1},
    }
    assert tuple(forced) == NAMES
    return [(name, forced[name], exp) for name, exp in EXPECTED]


def position_cases(cv, cs, pk, epk, n, trace):
    """The position-dependent subset for a shape of more than one scan block (n >= 2048), in the order of
    POSITION_EXPECTED."""
    assert n >= 2048 and SECOND_BLOCK_ROW < cs.n_gates
    by_name = {name: f for name, f, _ in cases(cv, cs, pk, epk, n, trace)}
    by_name["den_blk2"] = {"gamma": den_gamma(cv, cs, epk, n, SECOND_BLOCK_ROW)}
    return [(name, by_name[name], exp) for name, exp in POSITION_EXPECTED]


def grand_product_case(cv, epk, n, product, row, seed=0):
    """Inputs of the two grand products on their own (zkt_debug_grand_products, K.z1_evals / K.z2_evals): arbitrary vectors
    a b c f t h1 h2 and challenges (beta, gamma, delta, epsilon), integers, with the first factor of the denominator of
    `product` (1: permutation, 2: lookup) vanishing at `row` and nowhere else."""
    p = cv.fr.p
    beta, gamma, delta, epsilon = field_elems(p, 9100 + seed, 4)
    vec = [field_elems(p, 9200 + 7 * seed + i, n) for i in range(7)]
    if product == 1:
        gamma = -(vec[0][row] + beta * epk.sigma1[row]) % p
    else:
        epsilon = -(vec[5][row] + delta * vec[6][row]) * pow(1 + delta, -1, p) % p
    return (beta, gamma, delta, epsilon), vec


def world(cv, gates, table_size, seed, tau, blinder_seed):
    """Everything one circuit's forced-challenge tests share: the circuit, its keys under the SRS of `tau`, the blinders,
    and the unforced oracle proof with its trace."""
    cs = P.synthetic_circuit(cv, gates, table_size, seed=seed)
    n = cs.circuit_bound()
    srs_arr = K.srs_mont(cv, tau, n + 8)
    be = K.CBackend(cv, srs_arr)
    pk, epk, vk = P.setup(be, [None] * (n + 8), cs, True)
    blinders = field_elems(cv.fr.p, blinder_seed, P.NUM_BLINDERS)
    w = SimpleNamespace(cv=cv, cs=cs, n=n, tau=tau, srs_arr=srs_arr, be=be, pk=pk, epk=epk, vk=vk, blinders=blinders)
    w.trace = P.ProverTrace()
    w.plain = P.prove(be, [None] * (n + 8), pk, epk, vk, cs, P.new_seeded_transcript(cv, vk), blinders, w.trace).serialize(cv)
    return w


def transcript(w, forced):
    return ForcedTranscript(P.new_seeded_transcript(w.cv, w.vk), forced)


def oracle_outcome(w, forced):
    """-> ("proof", bytes, challenges) or (code, None, challenges): oracle.plonk.prove under the forced transcript, its
    exceptions mapped to the codes of include/zkt_plonk.h as the module's docstring says."""
    tr = transcript(w, forced)
    try:
        proof = P.prove(w.be, [None] * (w.n + 8), w.pk, w.epk, w.vk, w.cs, tr, w.blinders)
    except ZeroDivisionError:
        return 6, None, tr.drawn
    except AssertionError as e:
        assert "challenges must be different" in str(e)
        return 7, None, tr.drawn
    except IndexError:
        return 9, None, tr.drawn
    except ValueError as e:
        assert "TooManyCoefficients" in str(e)
        return 5, None, tr.drawn
    return PROOF, proof.serialize(w.cv), tr.drawn


# ---- the device side: zkt_transcript_vtable over any transcript object ---------------------------------------------
_U64 = ctypes.POINTER(ctypes.c_uint64)
_CB_U64 = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint64)
_CB_SC = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_char_p, _U64, ctypes.c_size_t, ctypes.c_int)
_CB_CM = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_char_p, _U64, ctypes.c_int)
_CB_CH = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_char_p, _U64)


class TranscriptVtable(ctypes.Structure):
    """zkt_transcript_vtable (include/zkt_plonk.h)"""
    _fields_ = [("user", ctypes.c_void_p), ("append_u64", _CB_U64), ("append_scalars", _CB_SC),
                ("append_commitment", _CB_CM), ("challenge_scalar", _CB_CH)]


def vtable(cv, tr):
    """The ctypes zkt_transcript_vtable whose four callbacks drive `tr` (append_u64 / append_scalar / append_scalars /
    append_commitment / challenge_scalar on integers and affine points).  Values cross as Montgomery limbs: scalars
    cv.fr.limbs64 limbs with R = 2^(64 limbs), commitments cv.fq.limbs64 limbs per coordinate.  The returned struct keeps
    its callback objects alive; an exception raised inside a callback (ctypes would only print it) is kept in
    `.errors`."""
    p, q = cv.fr.p, cv.fq.p
    lr, lq = cv.fr.limbs64, cv.fq.limbs64
    R_r = (1 << (64 * lr)) % p
    rinv_r, rinv_q = pow(1 << (64 * lr), -1, p), pow(1 << (64 * lq), -1, q)
    errors = []

    def limbs(ptr, k, width):
        return sum(int(ptr[width * k + i]) << (64 * i) for i in range(width))

    def guarded(fn):
        def call(*args):
            try:
                fn(*args)
            except BaseException as e:      # noqa: B902 -- nothing may propagate into the C caller
                errors.append(e)
        return call

    def cb_u64(user, label, v):
        tr.append_u64(label.decode(), v)

    def cb_sc(user, label, ptr, count, single):
        vals = [limbs(ptr, k, lr) * rinv_r % p for k in range(count)]
        if single:
            tr.append_scalar(label.decode(), vals[0])
        else:
            tr.append_scalars(label.decode(), vals)

    def cb_cm(user, label, ptr, inf):
        pt = None if inf else (limbs(ptr, 0, lq) * rinv_q % q, limbs(ptr, 1, lq) * rinv_q % q)
        tr.append_commitment(label.decode(), pt)

    def cb_ch(user, label, out):
        v = tr.challenge_scalar(label.decode()) * R_r % p
        for i in range(lr):
            out[i] = (v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF

    cbs = (_CB_U64(guarded(cb_u64)), _CB_SC(guarded(cb_sc)), _CB_CM(guarded(cb_cm)), _CB_CH(guarded(cb_ch)))
    vt = TranscriptVtable(None, *cbs)
    vt.keep = cbs
    vt.errors = errors
    return vt


def prove_with(ctx, prep, tr):
    """zkt_prove_with alone on prepared inputs -> (rc, proof bytes).  No zkt_prove_set_next call: an announcement that a
    failed proof left armed must not be overwritten by the helper."""
    import zkt_plonk_amd as z
    from zkt_plonk_amd._lib import ProveInputs
    L = z.lib()
    L.zkt_prove_with.argtypes = [ctypes.c_void_p, ctypes.POINTER(ProveInputs), ctypes.POINTER(TranscriptVtable),
                                 ctypes.POINTER(ctypes.c_uint8), ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]
    vt = vtable(tr.cv, tr)
    out = (ctypes.c_uint8 * 2048)()
    ln = ctypes.c_size_t(0)
    rc = L.zkt_prove_with(ctx.handle, ctypes.byref(prep.struct), ctypes.byref(vt), out, 2048, ctypes.byref(ln))
    assert not vt.errors, vt.errors
    if rc == 3:      # ZKT_ERR_HIP: the device may have faulted; nothing more is started on it in this session
        import pytest
        pytest.exit("zkt_prove_with: HIP error: %s" % L.zkt_last_error(ctx.handle).decode(), returncode=3)
    return rc, (bytes(out[:ln.value]) if rc == 0 else b"")


def load(z, ctx, w):
    """Loads w's SRS and circuit into ctx and returns the prepared inputs of its witness (host vectors)."""
    cv = w.cv
    ctx.srs_load(w.srs_arr)
    z.GpuProver(ctx, w.n.bit_length() - 1, {k: K.fr_to_mont(cv, w.pk.polys[k]) if w.pk.polys[k] else np.zeros((0, 4), dtype=np.uint64)
                                            for k in z.PK_ORDER})
    return prepare(ctx, w)


def prepare(ctx, w):
    cv, cs = w.cv, w.cs
    a, b, c = (K.fr_to_mont(cv, x) for x in cs.wire_evals(cs.n_gates))
    pos = sorted(cs.pi)
    return ctx.prepare_host(a, b, c, K.fr_to_mont(cv, cs.table), pos, K.fr_to_mont(cv, [cs.pi[k] for k in pos]),
                            K.fr_to_mont(cv, w.blinders))
