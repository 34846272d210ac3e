// Verifier, everything but the pairings: plonk-core/src/proof_system/proof.rs:285-503 up to the two
// SonicKZG10::check calls.  This comment describes the SINGLE-PROOF case, which is host-only code: one proof is
// 13 + 9 + 4 short scalar multiplications (~4 ms of host time on the 64-bit-limb arithmetic of hostec.hpp); a GPU has
// nothing to add at that size.  (A batch of many proofs under one SRS is another matter: zkt_verify_batch_dev further
// down moves the decompressions and the combinations, the two costs that grow with the batch, to the device.)  The
// result is, for each of the two openings, the pair (L, W) with
//     L = sum_i eta^i C_i - (sum_i eta^i v_i) G + z W
// so that the opening is valid iff e(L, h) == e(W, beta h) -- the two pairings stay with the caller (arkworks'
// `PairingEngine::product_of_pairings`), which also holds h and beta h (SonicKZG10's VerifierKey).
#include "ctx.hpp"
#include "ec.hpp"
#include "hostec.hpp"
#include "g1decomp.hpp"
#include "hostinv.hpp"
#include "linearisation.hpp"
#include "msm.hpp"
#include "pairing.hpp"
#include "transcript.hpp"
#include "verify_leaves.hpp"
#include "verify_terms.hpp"

#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

namespace zkt {

template <class P>
static Fe<P> pow_words(const Fe<P>& a, const uint32_t* e, int nwords) {
    Fe<P> r = fe_one<P>();
    bool started = false;
    for (int i = nwords * 32 - 1; i >= 0; --i) {
        if (started) r = fe_sqr<P>(r);
        if ((e[i / 32] >> (i % 32)) & 1u) {
            r = fe_mul<P>(r, a);
            started = true;
        }
    }
    return r;
}

template <class P>
static bool canonical_from_bytes(const uint8_t* b, uint32_t strip_top_bits, Fe<P>* out_mont, Fe<P>* out_canon = nullptr) {
    Fe<P> v;
    memcpy(v.v, b, P::N * 4);
    if (strip_top_bits) v.v[P::N - 1] &= (0xFFFFFFFFu >> strip_top_bits);
    for (int i = P::N - 1; i >= 0; --i) {
        if (v.v[i] < P::mod(i)) break;
        if (v.v[i] > P::mod(i) || i == 0) return false;
    }
    if (out_canon) *out_canon = v;
    *out_mont = fe_to_mont<P>(v);
    return true;
}

// a > -a as canonical integers (ark-serialize SWFlags: bit 7 = "y is the larger root")
template <class Q>
static bool is_larger_root(const Fe<Q>& y_mont) {
    const Fe<Q> y = fe_from_mont<Q>(y_mont), ny = fe_from_mont<Q>(fe_neg<Q>(y_mont));
    for (int i = Q::N - 1; i >= 0; --i)
        if (y.v[i] != ny.v[i]) return y.v[i] > ny.v[i];
    return false;
}

// a^e on 64-bit limbs, fixed 4-bit window (e: little-endian words)
template <class Q>
static hostec::HF<Q> hf_pow(const hostec::HF<Q>& a, const uint64_t* e, int nwords) {
    using hostec::HF;
    HF<Q> tab[16];
    tab[0] = hostec::hf_from<Q>(fe_one<Q>());
    for (int i = 1; i < 16; ++i) tab[i] = hostec::hf_mul<Q>(tab[i - 1], a);
    HF<Q> r = tab[0];
    bool started = false;
    for (int i = nwords * 16 - 1; i >= 0; --i) {
        const unsigned d = (unsigned)(e[i / 16] >> (4 * (i % 16))) & 15u;
        if (started)
            for (int k = 0; k < 4; ++k) r = hostec::hf_mul<Q>(r, r);
        if (d) {
            r = started ? hostec::hf_mul<Q>(r, tab[d]) : tab[d];
            started = true;
        }
    }
    return r;
}

// G1 = E(Fq)[r].  BN254 has cofactor one.  On BLS12-381 the curve has the endomorphism sigma(x, y) = (beta x, y) with
// sigma^2 + sigma + 1 = 0, acting on G1 as lambda = -x^2 (x the curve parameter; lambda^2 + lambda + 1 = r).  As
// endomorphisms (sigma - lambda)(sigma - lambda') = sigma^2 + sigma + 1 - r = -r for lambda' = x^2 - 1, so
// sigma(P) = [lambda] P implies [r] P = 0: two multiplications by the 64-bit |x| replace the 255-bit one of ark-ec's
// is_in_correct_subgroup_assuming_on_curve, with the same answer on every point of the curve.
template <class C>
static bool g1_in_subgroup(const Affine<typename C::Fq>& p) {
    using Q = typename C::Fq;
    if (C::ID == 0 || aff_is_inf<Q>(p)) return true;
    using namespace hostec;
    // beta = 2^((p - 1) / 3): the cube root of unity whose sigma is [-x^2] on G1 (tests/test_verify_host.py pins it)
    static const HF<Q> beta = [] {
        uint64_t e[HF<Q>::N], rem = 0;
        for (int i = HF<Q>::N - 1; i >= 0; --i) {
            const u128 cur = ((u128)rem << 64) | (HParams<Q>::mod(i) - (i == 0 ? 1 : 0));
            e[i] = (uint64_t)(cur / 3);
            rem = (uint64_t)(cur % 3);
        }
        return hf_pow<Q>(hf_from<Q>(fe_from_u32<Q>(2)), e, HF<Q>::N);
    }();
    const uint64_t xabs = 0xd201000000010000ULL;
    auto mul_x = [&](const HX<Q>& a) {
        HX<Q> acc = a;
        for (int i = 62; i >= 0; --i) {
            acc = hx_double<Q>(acc);
            if ((xabs >> i) & 1) acc = hx_add<Q>(acc, a);
        }
        return acc;
    };
    const HX<Q> P = hx_from<Q>(xyzz_from_affine<Q>(p));
    const HX<Q> x2p = mul_x(mul_x(P));                       // [x^2] P
    if (hf_is_zero<Q>(x2p.zz)) return false;                 // sigma(P) is never the identity
    // sigma(P) == -[x^2] P, compared projectively: X = beta x ZZ, Y = -y ZZZ
    const HF<Q> lx = hf_mul<Q>(hf_mul<Q>(beta, hf_from<Q>(p.x)), x2p.zz);
    const HF<Q> ly = hf_mul<Q>(hf_from<Q>(fe_neg<Q>(p.y)), x2p.zzz);
    return memcmp(lx.v, x2p.x.v, sizeof(lx.v)) == 0 && memcmp(ly.v, x2p.y.v, sizeof(ly.v)) == 0;
}

// compressed short-Weierstrass point of ark-serialize 0.3 (proof.rs:98-155 wire format) -> affine (Montgomery);
// both base fields have p = 3 mod 4, so sqrt(a) = a^((p + 1) / 4).  Checked deserialisation, as the reference's
// verifier relies on it (proof.rs:308 "subgroup checks are done when the proof is deserialised"): SWFlags::from_u8
// refuses both flag bits at once, x must be a canonical field element, the point must lie on the curve and in the
// prime-order subgroup.  Under the infinity flag the x bytes are parsed like any field element (so they must be below the
// modulus) and then ignored: GroupAffine::deserialize of ark-ec 0.3 reads (x, flags) with deserialize_with_flags and returns
// zero() when flags.is_infinity() -- as recalled, the crate is not in this image ("parity unpinned"; r03 refused a non-zero x
// there, which was stricter than the reference).
template <class C>
static bool decompress(const uint8_t* b, Affine<typename C::Fq>* out, bool* is_inf) {
    using Q = typename C::Fq;
    using hostec::HF;
    const size_t nb = Q::N * 4;
    const uint8_t flags = b[nb - 1];
    if ((flags & 0xC0) == 0xC0) return false;
    if (flags & 0x40) {
        Fe<Q> ignored;
        if (!canonical_from_bytes<Q>(b, 2, &ignored)) return false;
        *is_inf = true;
        out->x = fe_zero<Q>();
        out->y = fe_zero<Q>();
        return true;
    }
    *is_inf = false;
    Fe<Q> x;
    if (!canonical_from_bytes<Q>(b, 2, &x)) return false;
    const HF<Q> hx = hostec::hf_from<Q>(x);
    const HF<Q> rhs = hostec::hf_add<Q>(hostec::hf_mul<Q>(hostec::hf_mul<Q>(hx, hx), hx), hostec::hf_from<Q>(fe_from_u32<Q>(C::B)));
    static const std::vector<uint64_t> e = [] {   // (p + 1) / 4
        std::vector<uint64_t> w(HF<Q>::N + 1, 0);
        hostec::u128 carry = 1;
        for (int i = 0; i < HF<Q>::N; ++i) {
            carry += hostec::HParams<Q>::mod(i);
            w[i] = (uint64_t)carry;
            carry >>= 64;
        }
        w[HF<Q>::N] = (uint64_t)carry;
        for (int i = 0; i < HF<Q>::N; ++i) w[i] = (w[i] >> 2) | (w[i + 1] << 62);
        w.pop_back();
        return w;
    }();
    const HF<Q> hy = hf_pow<Q>(rhs, e.data(), HF<Q>::N);
    if (memcmp(hostec::hf_mul<Q>(hy, hy).v, rhs.v, sizeof(rhs.v)) != 0) return false;   // x is not on the curve
    Fe<Q> y = hostec::hf_to<Q>(hy);
    if (is_larger_root<Q>(y) != ((flags & 0x80) != 0)) y = fe_neg<Q>(y);
    out->x = x;
    out->y = y;
    return g1_in_subgroup<C>(*out);
}

// sum_i s_i P_i for a handful of points: interleaved width-5 NAFs over one doubling chain (the verifier's ~25-term
// combinations; double-and-add per term cost four times as much)
template <class C>
static hostec::HX<typename C::Fq> msm_wnaf(const hostec::HX<typename C::Fq>* pts, const Fe<typename C::Fr>* scalars_mont, int n) {
    using Q = typename C::Fq;
    using R = typename C::Fr;
    using namespace hostec;
    constexpr int BITS = R::N * 32 + 1;
    std::vector<int8_t> naf((size_t)n * BITS, 0);
    std::vector<HX<Q>> tab((size_t)n * 8);
    int top = 0;
    for (int t = 0; t < n; ++t) {
        Fe<R> s = fe_from_mont<R>(scalars_mont[t]);
        uint32_t k[R::N + 1];
        for (int i = 0; i < R::N; ++i) k[i] = s.v[i];
        k[R::N] = 0;
        auto is_zero = [&] { uint32_t o = 0; for (int i = 0; i <= R::N; ++i) o |= k[i]; return o == 0; };
        int pos = 0;
        while (!is_zero()) {
            int d = 0;
            if (k[0] & 1u) {
                d = (int)(k[0] & 31u);
                if (d >= 16) d -= 32;
                // k -= d
                int64_t carry = -(int64_t)d;
                for (int i = 0; i <= R::N && carry; ++i) {
                    const int64_t v = (int64_t)k[i] + carry;
                    k[i] = (uint32_t)v;
                    carry = v >> 32;
                }
            }
            naf[(size_t)t * BITS + pos] = (int8_t)d;
            for (int i = 0; i < R::N; ++i) k[i] = (k[i] >> 1) | (k[i + 1] << 31);
            k[R::N] >>= 1;
            ++pos;
        }
        if (pos > top) top = pos;
        // odd multiples P, 3P, ..., 15P
        const HX<Q> p2 = hx_double<Q>(pts[t]);
        tab[(size_t)t * 8] = pts[t];
        for (int j = 1; j < 8; ++j) tab[(size_t)t * 8 + j] = hx_add<Q>(tab[(size_t)t * 8 + j - 1], p2);
    }
    HX<Q> acc = hx_identity<Q>();
    for (int i = top - 1; i >= 0; --i) {
        acc = hx_double<Q>(acc);
        for (int t = 0; t < n; ++t) {
            const int d = naf[(size_t)t * BITS + i];
            if (!d) continue;
            HX<Q> e = tab[(size_t)t * 8 + (size_t)((d > 0 ? d : -d) >> 1)];
            if (d < 0) e.y = hf_sub<Q>(HF<Q>{}, e.y);
            acc = hx_add<Q>(acc, e);
        }
    }
    return acc;
}

// the ten verifier-key points and g of one proof: sources SRC_VK .. SRC_G
template <class C>
static void verifier_key_points(const zkt_verify_inputs& in, Affine<typename C::Fq>* out11) {
    using Q = typename C::Fq;
    const size_t nb = Q::N * 4;
    const int L64 = Q::N / 2;
    for (int k = 0; k < 10; ++k) {
        if (in.vk_is_infinity && in.vk_is_infinity[k]) {
            out11[k].x = fe_zero<Q>();
            out11[k].y = fe_zero<Q>();
        } else {
            memcpy(out11[k].x.v, in.vk_commitments + (size_t)k * 2 * L64, nb);
            memcpy(out11[k].y.v, in.vk_commitments + (size_t)k * 2 * L64 + L64, nb);
        }
    }
    memcpy(out11[10].x.v, in.g, nb);
    memcpy(out11[10].y.v, in.g + L64, nb);
}

// verifier_replay's transcript over a HostTranscript: a built-in one through its virtual calls, or a caller's callbacks
template <class C>
struct VtHostTr {
    using R = typename C::Fr;
    using Q = typename C::Fq;
    HostTranscript& tr;
    void scalars(const char* label, const Fe<R>* mont, uint64_t count, bool single) {
        std::vector<uint8_t> b(count * 32);
        for (uint64_t i = 0; i < count; ++i) {
            const Fe<R> c = fe_from_mont<R>(mont[i]);
            memcpy(b.data() + 32 * i, c.v, 32);
        }
        tr.append_scalars(label, b.data(), count, 32, single);
    }
    void commit(const char* label, const Affine<Q>* p) {
        uint8_t x[64] = {0}, y[64] = {0};
        const bool inf = aff_is_inf<Q>(*p);
        if (!inf) {
            const Fe<Q> cx = fe_from_mont<Q>(p->x), cy = fe_from_mont<Q>(p->y);
            memcpy(x, cx.v, Q::N * 4);
            memcpy(y, cy.v, Q::N * 4);
        }
        tr.append_commitment(label, x, y, Q::N * 4, inf);
    }
    Fe<R> challenge(const char* label) {
        uint8_t b[32];
        tr.challenge_scalar(label, R::BITS, b);
        Fe<R> c;
        memcpy(c.v, b, 32);
        return fe_to_mont<R>(c);
    }
    static Fe<R> inv(const Fe<R>& a) { return fe_inv_host<R>(a); }
};

// One proof's data for verifier_replay from the caller's inputs.  The public inputs and their roots are copied (an Fe is
// 16-byte aligned, the caller's words need not be); rho = (1, 1), nothing forced, no sums and no trace until a caller sets them.
template <class C>
struct HostProof {
    using R = typename C::Fr;
    std::vector<Fe<R>> pi;              // roots, values and compute_r0's scratch: n_pi each
    VtProof<C> p;
    HostProof(const zkt_verify_inputs& in, int log_n, const Affine<typename C::Fq>* cm, const Fe<R>* ev) : pi(3 * in.n_pi) {
        if (in.n_pi) {
            memcpy((void*)pi.data(), in.pi_roots, in.n_pi * 32);
            memcpy((void*)(pi.data() + in.n_pi), in.pub_inputs, in.n_pi * 32);
        }
        p.n = in.n;
        p.n_pi = in.n_pi;
        p.w = root_of_unity<R>(log_n);
        p.rho[0] = p.rho[1] = fe_one<R>();
        p.cm = cm;
        p.ev = ev;
        p.roots = pi.data();
        p.vals = pi.data() + in.n_pi;
        p.before = pi.data() + 2 * in.n_pi;
        p.forced = nullptr;
        p.acc = nullptr;
        p.dbg = nullptr;
    }
};

template <class C>
struct Verifier {
    using R = typename C::Fr;
    using Q = typename C::Fq;
    using F = Fe<R>;
    using HX = hostec::HX<Q>;

    static HX to_hx(const Affine<Q>& a) { return hostec::hx_from<Q>(xyzz_from_affine<Q>(a)); }
    static HX mul(const HX& p, const F& s_mont) {   // double-and-add on the canonical scalar
        const F s = fe_from_mont<R>(s_mont);
        HX acc = hostec::hx_identity<Q>();
        bool started = false;
        for (int i = R::N * 32 - 1; i >= 0; --i) {
            if (started) acc = hostec::hx_double<Q>(acc);
            if ((s.v[i / 32] >> (i % 32)) & 1u) {
                acc = hostec::hx_add<Q>(acc, p);
                started = true;
            }
        }
        return acc;
    }
    static constexpr int MAX_TERMS = 13 + 8 + 2;
    // Step 2's result, a sink of verifier_replay: opening o is L_o = sum_k sc[o][k] * base[src[o][k]], checked against
    // W_o = base[SRC_CM + CM_AW + o]
    struct Terms {
        Affine<Q> base[SRC_COUNT];
        int n[2] = {0, 0};
        int src[2][MAX_TERMS];
        F sc[2][MAX_TERMS];
        void term(int o, int s, const F& v) {
            src[o][n[o]] = s;
            sc[o][n[o]] = v;
            ++n[o];
        }
    };

    static int shape(const zkt_verify_inputs& in, int* out_log_n) {
        const size_t nb = Q::N * 4;
        if (in.proof_len != 13 * nb + 2 + 12 * 32) return ZKT_ERR_INVALID_ARGUMENT;
        if (in.n == 0 || (in.n & (in.n - 1))) return ZKT_ERR_INVALID_DOMAIN_SIZE;
        int log_n = 0;
        while (((uint64_t)1 << log_n) < in.n) ++log_n;
        if (log_n > R::TWO_ADICITY) return ZKT_ERR_INVALID_DOMAIN_SIZE;
        *out_log_n = log_n;
        return ZKT_OK;
    }

    // ---- Proof::deserialize (proof.rs:98-155): 11 commitments, 2 x (opening, Option::None), 12 evaluations ----
    // points_done: the commitments were decompressed and checked elsewhere (cm is filled); only the other bytes are looked at
    static int parse(const zkt_verify_inputs& in, Affine<Q>* cm, F* ev, bool points_done) {
        const size_t nb = Q::N * 4;
        size_t pos = 0;
        for (int k = 0; k < 13; ++k) {
            bool inf = false;
            if (!points_done && !decompress<C>(in.proof + pos, &cm[k], &inf)) return ZKT_ERR_INVALID_ARGUMENT;
            pos += nb;
            if (k >= 11) {
                if (in.proof[pos] != 0) return ZKT_ERR_INVALID_ARGUMENT;   // kzg10::Proof::random_v must be None
                pos += 1;
            }
        }
        for (int k = 0; k < 12; ++k) {
            if (!canonical_from_bytes<R>(in.proof + pos, 0, &ev[k])) return ZKT_ERR_INVALID_ARGUMENT;
            pos += 32;
        }
        return ZKT_OK;
    }

    // Steps 1 to 3 for one proof: the pairs (L, W) of both openings
    static int run(const zkt_verify_inputs& in, HostTranscript& tr, uint64_t* out_pairs, int* out_inf) {
        const size_t nb = Q::N * 4;
        const int L64 = Q::N / 2;
        int log_n = 0;
        int rc = shape(in, &log_n);
        if (rc) return rc;
        Affine<Q> cm[13];
        F ev[12];
        if ((rc = parse(in, cm, ev, false))) return rc;
        // Step 2: the transcript, r0 and the scalars of both openings; no group arithmetic
        auto t = std::make_unique<Terms>();
        HostProof<C> hp(in, log_n, cm, ev);
        VtHostTr<C> htr{tr};
        if ((rc = verifier_replay<C>(htr, hp.p, *t))) return rc;
        for (int k = 0; k < 13; ++k) t->base[SRC_CM + k] = cm[k];
        verifier_key_points<C>(in, &t->base[SRC_VK]);
        // Step 3: each list as ONE short multi-scalar multiplication
        for (int o = 0; o < 2; ++o) {
            std::vector<HX> pts;
            std::vector<F> scs;
            for (int k = 0; k < t->n[o]; ++k) {
                pts.push_back(to_hx(t->base[t->src[o][k]]));
                scs.push_back(t->sc[o][k]);
            }
            const HX L = msm_wnaf<C>(pts.data(), scs.data(), (int)pts.size());
            const Affine<Q> la = xyzz_to_affine_host<Q>(hostec::hx_to<Q>(L));
            const Affine<Q>& wit = t->base[SRC_CM + CM_AW + o];
            uint64_t* o_ = out_pairs + (size_t)o * 4 * L64;
            memcpy(o_, la.x.v, nb);
            memcpy(o_ + L64, la.y.v, nb);
            memcpy(o_ + 2 * L64, wit.x.v, nb);
            memcpy(o_ + 3 * L64, wit.y.v, nb);
            if (out_inf) {
                out_inf[2 * o] = aff_is_inf<Q>(la) ? 1 : 0;
                out_inf[2 * o + 1] = aff_is_inf<Q>(wit) ? 1 : 0;
            }
        }
        return ZKT_OK;
    }
};

}  // namespace zkt

using namespace zkt;

template <class C>
static void g1_msm_host_t(const uint64_t* pts, const uint64_t* scalars, size_t n, int scalars_mont, uint64_t* out, int* out_inf) {
    using Q = typename C::Fq;
    using R = typename C::Fr;
    constexpr int L64 = Q::N / 2;
    typename Verifier<C>::HX acc = hostec::hx_identity<Q>();
    for (size_t i = 0; i < n; ++i) {
        Affine<Q> a;
        memcpy(a.x.v, pts + i * 2 * L64, Q::N * 4);
        memcpy(a.y.v, pts + i * 2 * L64 + L64, Q::N * 4);
        if (aff_is_inf<Q>(a)) continue;
        Fe<R> s;
        memcpy(s.v, scalars + 4 * i, 32);
        if (!scalars_mont) s = fe_to_mont<R>(s);
        acc = hostec::hx_add<Q>(acc, Verifier<C>::mul(Verifier<C>::to_hx(a), s));
    }
    const Affine<Q> r = xyzz_to_affine_host<Q>(hostec::hx_to<Q>(acc));
    memcpy(out, r.x.v, Q::N * 4);
    memcpy(out + L64, r.y.v, Q::N * 4);
    if (out_inf) *out_inf = aff_is_inf<Q>(r) ? 1 : 0;
}

extern "C" int zkt_g1_msm_host(int curve_id, const uint64_t* points_xy_mont, const uint64_t* scalars, size_t n,
                               int scalars_montgomery, uint64_t* out_xy_mont, int* out_is_infinity) {
    if ((n && (!points_xy_mont || !scalars)) || !out_xy_mont) return ZKT_ERR_INVALID_ARGUMENT;
    if (curve_id == ZKT_CURVE_BN254) g1_msm_host_t<Bn254Curve>(points_xy_mont, scalars, n, scalars_montgomery, out_xy_mont, out_is_infinity);
    else if (curve_id == ZKT_CURVE_BLS12_381) g1_msm_host_t<Bls381Curve>(points_xy_mont, scalars, n, scalars_montgomery, out_xy_mont, out_is_infinity);
    else return ZKT_ERR_INVALID_ARGUMENT;
    return ZKT_OK;
}

template <class C>
static int pairing_inputs(const uint64_t* g1, const uint64_t* g2, size_t n, std::vector<typename pairing::Tower<C>::G1>& ps,
                          std::vector<typename pairing::Tower<C>::G2>& qs) {
    using Q = typename C::Fq;
    using T = pairing::Tower<C>;
    constexpr int L64 = Q::N / 2;
    ps.resize(n);
    qs.resize(n);
    for (size_t i = 0; i < n; ++i) {
        Fe<Q> c[6];
        memcpy(c[0].v, g1 + i * 2 * L64, Q::N * 4);
        memcpy(c[1].v, g1 + i * 2 * L64 + L64, Q::N * 4);
        for (int k = 0; k < 4; ++k) memcpy(c[2 + k].v, g2 + i * 4 * L64 + (size_t)k * L64, Q::N * 4);
        ps[i].inf = fe_is_zero<Q>(c[0]) && fe_is_zero<Q>(c[1]);
        ps[i].x = hostec::hf_from<Q>(c[0]);
        ps[i].y = hostec::hf_from<Q>(c[1]);
        qs[i].inf = fe_is_zero<Q>(c[2]) && fe_is_zero<Q>(c[3]) && fe_is_zero<Q>(c[4]) && fe_is_zero<Q>(c[5]);
        qs[i].x = typename T::E2{hostec::hf_from<Q>(c[2]), hostec::hf_from<Q>(c[3])};
        qs[i].y = typename T::E2{hostec::hf_from<Q>(c[4]), hostec::hf_from<Q>(c[5])};
        if (!T::g1_on_curve(ps[i]) || !T::g2_on_twist(qs[i])) return ZKT_ERR_INVALID_ARGUMENT;
        // the pairing is bilinear on G1 x G2 only: a point of the curve outside the prime-order subgroup is refused
        Affine<Q> pa;
        pa.x = c[0];
        pa.y = c[1];
        if (!ps[i].inf && !g1_in_subgroup<C>(pa)) return ZKT_ERR_INVALID_ARGUMENT;
    }
    return ZKT_OK;
}

template <class C>
static int pairing_check_t(const uint64_t* g1, const uint64_t* g2, size_t n, int* is_one) {
    std::vector<typename pairing::Tower<C>::G1> ps;
    std::vector<typename pairing::Tower<C>::G2> qs;
    int rc = pairing_inputs<C>(g1, g2, n, ps, qs);
    if (rc) return rc;
    bool valid = true;
    *is_one = pairing::Tower<C>::product_is_one(ps.data(), qs.data(), n, &valid) ? 1 : 0;
    return valid ? ZKT_OK : ZKT_ERR_INVALID_ARGUMENT;   // a G2 argument of small order
}

// every shortcut of csrc/pairing.hpp against its plain definition; 0 = all good, else the number of the failing check
extern "C" int zkt_debug_pairing_selftest(int curve_id) {
    if (curve_id == ZKT_CURVE_BN254) return pairing::Tower<Bn254Curve>::selftest();
    if (curve_id == ZKT_CURVE_BLS12_381) return pairing::Tower<Bls381Curve>::selftest();
    return -1;
}

extern "C" int zkt_pairing_product_is_one(int curve_id, const uint64_t* g1_xy_mont, const uint64_t* g2_xy_mont, size_t n,
                                          int* is_one) {
    if (!is_one || (n && (!g1_xy_mont || !g2_xy_mont))) return ZKT_ERR_INVALID_ARGUMENT;
    if (curve_id == ZKT_CURVE_BN254) return pairing_check_t<Bn254Curve>(g1_xy_mont, g2_xy_mont, n, is_one);
    if (curve_id == ZKT_CURVE_BLS12_381) return pairing_check_t<Bls381Curve>(g1_xy_mont, g2_xy_mont, n, is_one);
    return ZKT_ERR_INVALID_ARGUMENT;
}

extern "C" int zkt_verify_prepare(int curve_id, const zkt_verify_inputs* in, zkt_transcript* transcript, uint64_t* out_pairs,
                                  int* out_is_infinity);

// The whole of Proof::verify (proof.rs:285-503): zkt_verify_prepare, then the two SonicKZG10::check calls
// (proof.rs:441,479), e(L_k, h) e(-W_k, beta h) == 1 for k = 1, 2, folded into ONE product of two pairings the way
// ark-poly-commit's batch_check folds openings: with rho = the low 128 bits of Keccak-256 over (L1, W1, L2, W2, h, beta h),
//     e(L1 + rho L2, h) e(-(W1 + rho W2), beta h) == 1.
// Both checks hold => the folded one holds; if one of them fails, the folded one holds for at most one value of rho
// (the exponent is linear in it), i.e. with probability 2^-128 over the hash: the accept set is the reference's.
template <class C>
static int verify_t(int curve_id, const zkt_verify_inputs* in, zkt_transcript* tr, const uint64_t* h, const uint64_t* beta_h,
                    int* accepted) {
    using Q = typename C::Fq;
    using R = typename C::Fr;
    using HX = hostec::HX<Q>;
    constexpr int L64 = Q::N / 2;
    uint64_t pairs[4 * 12];
    int inf[4];
    int rc = zkt_verify_prepare(curve_id, in, tr, pairs, inf);
    if (rc) return rc;
    Fe<R> rho = fe_zero<R>();
    {
        std::vector<uint8_t> buf(4 + (size_t)(8 * L64 + 8 * L64) * 8);
        const uint32_t cid = (uint32_t)curve_id;
        memcpy(buf.data(), &cid, 4);
        memcpy(buf.data() + 4, pairs, (size_t)8 * L64 * 8);
        memcpy(buf.data() + 4 + (size_t)8 * L64 * 8, h, (size_t)4 * L64 * 8);
        memcpy(buf.data() + 4 + (size_t)12 * L64 * 8, beta_h, (size_t)4 * L64 * 8);
        uint8_t dg[32];
        keccak256(buf.data(), buf.size(), dg);
        memcpy(rho.v, dg, 16);                      // 128 bits: below both scalar moduli
        rho = fe_to_mont<R>(rho);
    }
    auto point = [&](int idx) {
        Affine<Q> a;
        memcpy(a.x.v, pairs + (size_t)idx * 2 * L64, L64 * 8);
        memcpy(a.y.v, pairs + (size_t)idx * 2 * L64 + L64, L64 * 8);
        return hostec::hx_from<Q>(xyzz_from_affine<Q>(a));
    };
    const Fe<R> sc[2] = {fe_one<R>(), rho};
    const HX lp[2] = {point(0), point(2)}, wp[2] = {point(1), point(3)};
    const Affine<Q> lc = xyzz_to_affine_host<Q>(hostec::hx_to<Q>(msm_wnaf<C>(lp, sc, 2)));
    Affine<Q> wc = xyzz_to_affine_host<Q>(hostec::hx_to<Q>(msm_wnaf<C>(wp, sc, 2)));
    if (!aff_is_inf<Q>(wc)) wc.y = fe_neg<Q>(wc.y);
    uint64_t g1[2 * 12], g2[2 * 4 * 6];
    memcpy(g1, lc.x.v, L64 * 8);
    memcpy(g1 + L64, lc.y.v, L64 * 8);
    memcpy(g1 + 2 * L64, wc.x.v, L64 * 8);
    memcpy(g1 + 3 * L64, wc.y.v, L64 * 8);
    memcpy(g2, h, 4 * L64 * 8);
    memcpy(g2 + 4 * L64, beta_h, 4 * L64 * 8);
    int one = 0;
    if ((rc = pairing_check_t<C>(g1, g2, 2, &one))) return rc;
    *accepted = one ? 1 : 0;    // 0: Error::ProofVerificationError
    return ZKT_OK;
}

// k proofs under the SAME structured reference string (h, beta h; the circuits and verifier keys may differ), ONE product of
// two pairings for all of them: every proof contributes its two folded openings (L_2i, W_2i), (L_2i+1, W_2i+1), and
//     e(sum_j rho_j L_j, h) e(-sum_j rho_j W_j, beta h) == 1,   rho_0 = 1, rho_j = low 128 bits of Keccak-256(seed || j),
// seed = Keccak-256 over the curve, k, every (L, W) and (h, beta h).  All 2k checks hold => the product is one; if any
// fails, the product is one for at most a 2^-128 fraction of the seeds.  A rejected batch says nothing about WHICH proof
// is bad: the caller falls back to zkt_verify per proof.  The reference has no such entry (its PC::check folds the two
// openings of one proof only, proof.rs:441,479); this is the service-side extension SURVEY.md 8f.4 asks for.
template <class C>
static int verify_batch_t(int curve_id, const zkt_verify_inputs* ins, zkt_transcript* const* trs, size_t k, const uint64_t* h,
                          const uint64_t* beta_h, int* accepted) {
    using Q = typename C::Fq;
    using R = typename C::Fr;
    using HX = hostec::HX<Q>;
    constexpr int L64 = Q::N / 2;
    const size_t pair_words = (size_t)8 * L64;               // L1, W1, L2, W2 of one proof
    std::vector<uint64_t> pairs(k * pair_words);
    for (size_t i = 0; i < k; ++i) {
        if (!trs[i]) return ZKT_ERR_INVALID_ARGUMENT;
        int inf[4];
        int rc = zkt_verify_prepare(curve_id, &ins[i], trs[i], pairs.data() + i * pair_words, inf);
        if (rc) return rc;
    }
    uint8_t seed[32];
    {
        std::vector<uint8_t> buf(4 + 8 + pairs.size() * 8 + (size_t)8 * L64 * 8);
        const uint32_t cid = (uint32_t)curve_id;
        const uint64_t kk = (uint64_t)k;
        size_t at = 0;
        memcpy(buf.data() + at, &cid, 4); at += 4;
        memcpy(buf.data() + at, &kk, 8); at += 8;
        memcpy(buf.data() + at, pairs.data(), pairs.size() * 8); at += pairs.size() * 8;
        memcpy(buf.data() + at, h, (size_t)4 * L64 * 8); at += (size_t)4 * L64 * 8;
        memcpy(buf.data() + at, beta_h, (size_t)4 * L64 * 8);
        keccak256(buf.data(), buf.size(), seed);
    }
    const size_t m = 2 * k;
    std::vector<Fe<R>> rho(m);
    std::vector<HX> lp(m), wp(m);
    for (size_t j = 0; j < m; ++j) {
        if (j == 0) {
            rho[j] = fe_one<R>();
        } else {
            uint8_t msg[40], dg[32];
            const uint64_t jj = (uint64_t)j;
            memcpy(msg, seed, 32);
            memcpy(msg + 32, &jj, 8);
            keccak256(msg, sizeof msg, dg);
            Fe<R> r = fe_zero<R>();
            memcpy(r.v, dg, 16);                       // 128 bits: below both scalar moduli
            rho[j] = fe_to_mont<R>(r);
        }
        auto point = [&](size_t idx) {
            Affine<Q> a;
            memcpy(a.x.v, pairs.data() + idx * 2 * L64, L64 * 8);
            memcpy(a.y.v, pairs.data() + idx * 2 * L64 + L64, L64 * 8);
            return hostec::hx_from<Q>(xyzz_from_affine<Q>(a));
        };
        lp[j] = point(2 * j);          // pairs are laid out L, W, L, W, ...
        wp[j] = point(2 * j + 1);
    }
    const Affine<Q> lc = xyzz_to_affine_host<Q>(hostec::hx_to<Q>(msm_wnaf<C>(lp.data(), rho.data(), (int)m)));
    Affine<Q> wc = xyzz_to_affine_host<Q>(hostec::hx_to<Q>(msm_wnaf<C>(wp.data(), rho.data(), (int)m)));
    if (!aff_is_inf<Q>(wc)) wc.y = fe_neg<Q>(wc.y);
    uint64_t g1[2 * 12], g2[2 * 4 * 6];
    memcpy(g1, lc.x.v, L64 * 8);
    memcpy(g1 + L64, lc.y.v, L64 * 8);
    memcpy(g1 + 2 * L64, wc.x.v, L64 * 8);
    memcpy(g1 + 3 * L64, wc.y.v, L64 * 8);
    memcpy(g2, h, 4 * L64 * 8);
    memcpy(g2 + 4 * L64, beta_h, 4 * L64 * 8);
    int one = 0;
    int rc = pairing_check_t<C>(g1, g2, 2, &one);
    if (rc) return rc;
    *accepted = one ? 1 : 0;
    return ZKT_OK;
}

// What the stages leave behind for one batch.  zkt_verify_batch_locate reads the per-proof results again when the
// batch is rejected: the leaves of its tree are made of them (verify_leaves.hpp).
template <class C>
struct BatchPrep {
    using Q = typename C::Fq;
    using F = Fe<typename C::Fr>;
    std::vector<int> log_n;
    std::vector<F> ev;                  // 12 evaluations per proof
    std::vector<uint8_t> comp;          // 13 compressed commitments per proof
    std::vector<Affine<Q>> cm;          // ... decompressed
    std::vector<F> rho;                 // 2 per proof, Montgomery
    std::vector<uint64_t> rho_c;        // ... as 4 canonical words: B's scalars, out_rho
    std::vector<F> acc;                 // SRC_COUNT per proof, Montgomery: sum over both openings of rho * scalar, by source
    std::vector<Affine<Q>> other;       // 11 per proof: the ten verifier-key points and g (sources SRC_VK ..)
    size_t points_offset = 0, stage1_end = 0;   // device route: where verify_scratch holds cm, and where stage 1's region ends
    size_t err_proof = 0;               // a refusal: the proof and the reason
    std::string err_what;
    int refuse(int rc, size_t i, const std::string& what) {
        err_proof = i;
        err_what = what;
        return rc;
    }
    const Affine<Q>& base(size_t i, int s) const {
        return s < SRC_VK ? cm[13 * i + s] : other[11 * i + (s - SRC_VK)];
    }
};

// Stage 1, the host's half: lengths, the Option::None bytes, canonical evaluations; the compressed commitments are collected
template <class C>
static int batch_bytes(const zkt_verify_inputs* ins, zkt_transcript* const* trs, size_t k, BatchPrep<C>& bp) {
    using V = Verifier<C>;
    const size_t nb = C::Fq::N * 4;
    bp.log_n.resize(k);
    bp.ev.resize(12 * k);
    bp.comp.resize(13 * k * nb);
    for (size_t i = 0; i < k; ++i) {
        const zkt_verify_inputs& in = ins[i];
        if (!trs[i] || !in.proof || !in.vk_commitments || !in.g || (in.n_pi && (!in.pi_roots || !in.pub_inputs)))
            return bp.refuse(ZKT_ERR_INVALID_ARGUMENT, i, "null pointer");
        int rc = V::shape(in, &bp.log_n[i]);
        if (rc) return bp.refuse(rc, i, rc == ZKT_ERR_INVALID_DOMAIN_SIZE ? "n is not a supported power of two" : "wrong proof length");
        if ((rc = V::parse(in, nullptr, &bp.ev[12 * i], true)))
            return bp.refuse(rc, i, "malformed bytes (an Option that is not None, or an evaluation that is not canonical)");
        size_t pos = 0;
        for (int j = 0; j < 13; ++j) {
            memcpy(bp.comp.data() + (13 * i + j) * nb, in.proof + pos, nb);
            pos += nb + (j >= 11 ? 1 : 0);
        }
    }
    return ZKT_OK;
}

// Stage 3: the seed (it depends on the inputs alone) and the 2 k coefficients
template <class C>
static void batch_coefficients(const zkt_verify_inputs* ins, size_t k, const uint64_t* h, const uint64_t* beta_h, BatchPrep<C>& bp) {
    using Q = typename C::Fq;
    using R = typename C::Fr;
    using F = Fe<R>;
    constexpr int L64 = Q::N / 2;
    const size_t nb = Q::N * 4;
    uint8_t seed[32];
    {
        std::vector<uint8_t> buf;
        auto put = [&](const void* p, size_t bytes) {
            const uint8_t* b = (const uint8_t*)p;
            buf.insert(buf.end(), b, b + bytes);
        };
        auto put64 = [&](uint64_t v) { put(&v, 8); };
        const uint32_t cid = (uint32_t)C::ID;
        put(&cid, 4);
        put64((uint64_t)k);
        for (size_t i = 0; i < k; ++i) {
            const zkt_verify_inputs& in = ins[i];
            put64((uint64_t)in.proof_len);
            put(in.proof, in.proof_len);
            put64(in.n);
            for (int j = 0; j < 10; ++j) {
                const uint8_t inf = in.vk_is_infinity && in.vk_is_infinity[j] ? 1 : 0;
                uint64_t w[2 * 6] = {0};
                if (!inf) memcpy(w, in.vk_commitments + (size_t)j * 2 * L64, 2 * nb);
                put(w, 2 * nb);
                put(&inf, 1);
            }
            put64((uint64_t)in.n_pi);
            if (in.n_pi) {
                put(in.pi_roots, in.n_pi * 32);
                put(in.pub_inputs, in.n_pi * 32);
            }
            put(in.g, 2 * nb);
        }
        put(h, 4 * nb);
        put(beta_h, 4 * nb);
        keccak256(buf.data(), buf.size(), seed);
    }
    const size_t m = 2 * k;
    bp.rho.resize(m);
    bp.rho_c.assign(4 * m, 0);
    for (size_t j = 0; j < m; ++j) {
        F r = fe_zero<R>();
        if (j == 0) {
            r.v[0] = 1;
        } else {
            uint8_t msg[40], dg[32];
            const uint64_t jj = (uint64_t)j;
            memcpy(msg, seed, 32);
            memcpy(msg + 32, &jj, 8);
            keccak256(msg, sizeof msg, dg);
            memcpy(r.v, dg, 16);                       // 128 bits: below both scalar moduli
        }
        memcpy(&bp.rho_c[4 * j], r.v, 32);
        bp.rho[j] = fe_to_mont<R>(r);
    }
}

// Stage 2 and the per-proof half of stage 4: the replay through each handle's own calls, both openings' scalars times their
// rho added up by source
template <class C>
static int batch_terms(const zkt_verify_inputs* ins, zkt_transcript* const* trs, size_t k, BatchPrep<C>& bp) {
    bp.acc.resize(SRC_COUNT * k);
    bp.other.resize(11 * k);
    for (size_t i = 0; i < k; ++i) {
        HostProof<C> hp(ins[i], bp.log_n[i], &bp.cm[13 * i], &bp.ev[12 * i]);
        hp.p.rho[0] = bp.rho[2 * i];
        hp.p.rho[1] = bp.rho[2 * i + 1];
        hp.p.acc = &bp.acc[SRC_COUNT * i];
        if (int rc = vt_terms<C>(VtHostTr<C>{*trs[i]->impl}, hp.p))
            return bp.refuse(rc, i, rc == ZKT_ERR_EQUAL_CHALLENGES ? "two challenges are equal" : "a Lagrange denominator is zero");
        verifier_key_points<C>(ins[i], &bp.other[11 * i]);
    }
    return ZKT_OK;
}

// ---- stage 2 and the per-proof sums of stage 4 on the device (zkt_ctx_set_verify_terms(ctx, 1); verify_terms.hpp) ----
// hipMemcpyAsync on the context's stream unless an earlier step failed: every step records its error in rc and falls
// through to the ONE synchronise of its caller, since an upload may still be reading host memory
static void copy_step(zkt_ctx* c, int& rc, void* dst, const void* src, size_t bytes, hipMemcpyKind kind, const char* what) {
    if (rc) return;
    const hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, c->stream);
    if (e != hipSuccess) rc = hip_fail(c, e, what);
}

// where stage 1 keeps its data in verify_scratch: the compressed commitments at 0, the points, a status byte per point
struct DecompLayout {
    size_t out, status, end;
};
static DecompLayout decomp_layout(size_t npts, size_t nb) {
    auto up = [](size_t b) { return (b + 255) / 256 * 256; };
    DecompLayout l;
    l.out = up(npts * nb);
    l.status = l.out + up(npts * 2 * nb);
    l.end = l.status + up(npts);
    return l;
}

// Stage 1's staging: verify_scratch grown to `bytes` (>= the layout's end), the 13 k compressed commitments up, ONE
// k_g1_decompress launch, behind() -- what else reads the points on the device, enqueued on the same stream: (base) ->
// code -- then the points into bp.cm and the statuses down, and the stream synchronised ONCE.
template <class C, class Behind>
static int decompress_stage(zkt_ctx* c, BatchPrep<C>& bp, size_t k, size_t bytes, std::vector<uint8_t>& status, Behind behind) {
    const size_t nb = C::Fq::N * 4, npts = 13 * k;
    const DecompLayout l = decomp_layout(npts, nb);
    bp.points_offset = l.out;
    int rc = grow(c, c->verify_scratch, bytes);
    if (rc) return rc;
    char* const base = (char*)c->verify_scratch.p;
    bp.cm.resize(npts);
    status.resize(npts);
    {
        ProfScope prof(c, "verify_decompress");
        copy_step(c, rc, base, bp.comp.data(), npts * nb, hipMemcpyHostToDevice, "verify batch: commitments upload");
        if (!rc) rc = g1_decompress_enqueue(c, base, npts, base + l.out, base + l.status);
    }
    if (!rc) rc = behind(base);
    copy_step(c, rc, bp.cm.data(), base + l.out, npts * 2 * nb, hipMemcpyDeviceToHost, "verify batch: points download");
    copy_step(c, rc, status.data(), base + l.status, npts, hipMemcpyDeviceToHost, "verify batch: statuses download");
    const hipError_t e = hipStreamSynchronize(c->stream);
    if (!rc && e != hipSuccess) rc = hip_fail(c, e, "verify batch: decompression");
    return rc;
}

// What stages 1 and 2 on the device bring down: the status of every commitment and the image of the kernel's region
struct TermsDev {
    VtLayout lay;
    std::vector<uint8_t> host;          // the region from lay.desc on, as uploaded and, from lay.states on, as downloaded
    std::vector<uint8_t> point_status;
    uint8_t* at(size_t off) { return host.data() + (off - lay.desc); }
};

// Stage 1's launch and, directly behind it on the stream, the kernel of verify_terms.hip; statuses, points, sums and
// transcript states come down together and the stream is synchronised ONCE.  In: batch_bytes has run, bp.rho is set.
// forced_mont: NULL or 7 k values; dbg: the kernel also returns challenges and r0.  *refused: the error is bp's (a proof
// and a reason), not the runtime's.
template <class C>
static int stages12_dev(zkt_ctx* c, const zkt_verify_inputs* ins, zkt_transcript* const* trs, size_t k, BatchPrep<C>& bp,
                        const uint64_t* forced_mont, bool dbg, TermsDev& td, bool* refused) {
    using Q = typename C::Fq;
    using R = typename C::Fr;
    using F = Fe<R>;
    *refused = false;
    size_t total_pi = 0;
    for (size_t i = 0; i < k; ++i) total_pi += ins[i].n_pi;
    const DecompLayout dl = decomp_layout(13 * k, Q::N * 4);
    const VtLayout lay = vt_layout(dl.end, k, total_pi, forced_mont != nullptr, dbg);
    td.lay = lay;
    td.host.assign(lay.end - lay.desc, 0);
    auto* desc = (VtDesc<R>*)td.at(lay.desc);
    auto* states = (TranscriptState*)td.at(lay.states);
    size_t pi_at = 0;
    F w_of[R::TWO_ADICITY + 1];          // a domain generator costs an exponentiation: once per size, not per proof
    bool have_w[R::TWO_ADICITY + 1] = {false};
    for (size_t i = 0; i < k; ++i) {
        const zkt_verify_inputs& in = ins[i];
        const int lg = bp.log_n[i];
        if (!have_w[lg]) {
            w_of[lg] = root_of_unity<R>(lg);
            have_w[lg] = true;
        }
        desc[i].n = in.n;
        desc[i].n_pi = in.n_pi;
        desc[i].pi_off = pi_at;
        desc[i].reserved = 0;
        desc[i].w = w_of[lg];
        desc[i].rho[0] = bp.rho[2 * i];
        desc[i].rho[1] = bp.rho[2 * i + 1];
        if (in.n_pi) {
            memcpy(td.at(lay.roots) + pi_at * 32, in.pi_roots, in.n_pi * 32);
            memcpy(td.at(lay.vals) + pi_at * 32, in.pub_inputs, in.n_pi * 32);
        }
        pi_at += in.n_pi;
        states[i] = TranscriptState();
        if (!trs[i]->impl->export_state(states[i])) {
            *refused = true;
            return bp.refuse(ZKT_ERR_INVALID_ARGUMENT, i, "a transcript that zkt_transcript_new did not make");
        }
    }
    memcpy(td.at(lay.ev), bp.ev.data(), k * 12 * sizeof(F));
    if (forced_mont) memcpy(td.at(lay.forced), forced_mont, k * 7 * 32);
    bp.stage1_end = lay.end;             // zkt_verify_batch_locate's own region starts behind this stage's
    const size_t down_end = dbg ? lay.before : lay.dbg;
    return decompress_stage<C>(c, bp, k, lay.end, td.point_status, [&](char* base) {
        ProfScope prof(c, "verify_terms");
        int rc = ZKT_OK;
        copy_step(c, rc, base + lay.desc, td.at(lay.desc), lay.status - lay.desc, hipMemcpyHostToDevice, "verify terms: upload");
        if (!rc) rc = verify_terms_enqueue(c, base, lay, base + dl.out, k, forced_mont != nullptr, dbg);
        copy_step(c, rc, td.at(lay.states), base + lay.states, down_end - lay.states, hipMemcpyDeviceToHost, "verify terms: download");
        return rc;
    });
}

// the first commitment the decompression refused: its index, or npts
static size_t first_refused_point(const std::vector<uint8_t>& status) {
    for (size_t p = 0; p < status.size(); ++p)
        if (status[p] > ZKT_G1_IDENTITY) return p;
    return status.size();
}

// ---- zkt_verify_batch_dev: the batch above with its two per-proof costs on the device ------------------------------
// Stage 1: the 13 k compressed commitments go up in one copy and through ONE k_g1_decompress launch (g1decomp.hip); the
//          other bytes of a proof (length, Option::None, evaluations) are checked here.
// Stage 2: verifier_replay per proof, on the host through the handle's calls: transcript, r0, the scalars of both openings
//          -- no group arithmetic.
//          (zkt_ctx_set_verify_terms(ctx, 1): in one kernel behind stage 1's, with the per-proof sums of stage 4 --
//          stages12_dev above; stage 3 then runs first, since the kernel takes each proof's rho.)
// Stage 3: rho_0 = 1, rho_j = low 128 bits of Keccak-256(seed || j); the seed is hashed from everything that determines the
//          pairs (L_j, W_j), which this route never forms (verify_batch_t hashes the pairs: other coefficients, the same
//          soundness argument).
// Stage 4: the 2 k term lists, scaled by their rho_j, are added up per point: inside a proof by source, across proofs for
//          verifier-key points and g of equal CONTENT (a caller may pass one array or a copy per proof).
// Stage 5: A = sum s_k P_k and B = sum rho_j W_j as two variable-base MSMs (msm_bases), canonical scalars.
// The host keeps what is serial and small per proof (a Strobe / Keccak transcript and ~150 Fr products); the device takes
// what is wide: 13 k square roots and subgroup checks, and a (<= 24 k)-point and a 2 k-point MSM.
// `who` names the entry point in an error; bp keeps the per-proof results (zkt_verify_batch_locate goes on from them).
template <class C>
static int batch_fold_dev(zkt_ctx* c, const char* who, const zkt_verify_inputs* ins, zkt_transcript* const* trs, size_t k,
                          const uint64_t* h, const uint64_t* beta_h, BatchPrep<C>& bp, uint64_t* out_ab, int* out_inf) {
    using Q = typename C::Fq;
    using R = typename C::Fr;
    using F = Fe<R>;
    constexpr int L64 = Q::N / 2;
    const size_t nb = Q::N * 4, npts = 13 * k;
    static const char* const CM_NAME[13] = {"a", "b", "c", "t", "h1", "h2", "z1", "z2", "q_lo", "q_mid", "q_hi", "aw", "saw"};
    auto fail = [&](int rc, size_t i, const std::string& what) {
        return set_err(c, rc, std::string(who) + ": proof " + std::to_string(i) + ": " + what);
    };
    auto refused_commitment = [&](size_t p, uint8_t st) {
        static const char* const WHY[6] = {"", "", "x is not below the modulus", "both flag bits set", "not on the curve",
                                           "outside the prime-order subgroup"};
        return fail(ZKT_ERR_INVALID_ARGUMENT, p / 13,
                    std::string("commitment ") + std::to_string(p % 13) + " (" + CM_NAME[p % 13] + ") refused: " +
                        (st < 6 ? WHY[st] : "unknown status"));
    };
    // ---- stage 1 ----
    int rc = batch_bytes<C>(ins, trs, k, bp);
    if (rc) return fail(rc, bp.err_proof, bp.err_what);
    if (c->verify_terms_mode == 1) {
        // ---- stage 3 first (the kernel takes each proof's rho), stages 1 and 2 in one pass over the stream ----
        batch_coefficients<C>(ins, k, h, beta_h, bp);
        TermsDev td;
        bool refused = false;
        if ((rc = stages12_dev<C>(c, ins, trs, k, bp, nullptr, false, td, &refused)))
            return refused ? fail(rc, bp.err_proof, bp.err_what) : rc;
        // refusals in the serial loop's order: the first refused commitment, then the lowest proof the term stage refused
        const size_t p = first_refused_point(td.point_status);
        if (p < npts) return refused_commitment(p, td.point_status[p]);
        const int32_t* tstat = (const int32_t*)td.at(td.lay.status);
        for (size_t i = 0; i < k; ++i)
            if (tstat[i])
                return fail(tstat[i], i, tstat[i] == ZKT_ERR_EQUAL_CHALLENGES ? "two challenges are equal" : "a Lagrange denominator is zero");
        // every proof went through: the handles take the states the host route would have left
        const TranscriptState* states = (const TranscriptState*)td.at(td.lay.states);
        for (size_t i = 0; i < k; ++i)
            if (!trs[i]->impl->import_state(states[i])) return fail(ZKT_ERR_INVALID_ARGUMENT, i, "the transcript refused its state");
        bp.acc.resize(SRC_COUNT * k);
        memcpy((void*)bp.acc.data(), td.at(td.lay.acc), bp.acc.size() * sizeof(F));
        bp.other.resize(11 * k);
        for (size_t i = 0; i < k; ++i) verifier_key_points<C>(ins[i], &bp.other[11 * i]);
    } else {
        bp.stage1_end = decomp_layout(npts, nb).end;
        std::vector<uint8_t> status;
        if ((rc = decompress_stage<C>(c, bp, k, bp.stage1_end, status, [](char*) { return (int)ZKT_OK; }))) return rc;
        for (size_t p = 0; p < npts; ++p)
            if (status[p] > ZKT_G1_IDENTITY) return refused_commitment(p, status[p]);
        // ---- stage 3 (before the transcripts are consumed), stage 2 and the per-proof sums of stage 4 ----
        batch_coefficients<C>(ins, k, h, beta_h, bp);
        if ((rc = batch_terms<C>(ins, trs, k, bp))) return fail(rc, bp.err_proof, bp.err_what);
    }
    // ---- stage 4 across proofs ----
    const size_t m = 2 * k;
    std::vector<Affine<Q>> a_bases, b_bases(m);
    std::vector<F> a_acc;                              // Montgomery sums, one per entry of a_bases
    std::map<std::string, size_t> shared;              // verifier-key points and g, by content
    a_bases.reserve(SRC_COUNT * (k < 64 ? k : 64) + 13 * k);
    for (size_t i = 0; i < k; ++i) {
        for (int o = 0; o < 2; ++o) b_bases[2 * i + o] = bp.cm[13 * i + VL_WITNESS0 + o];
        for (int s = 0; s < SRC_COUNT; ++s) {
            const Affine<Q>& pt = bp.base(i, s);
            const F& sc = bp.acc[SRC_COUNT * i + s];
            if (aff_is_inf<Q>(pt)) continue;
            if (s >= SRC_VK) {
                auto ins_ = shared.emplace(std::string((const char*)&pt, sizeof(pt)), a_bases.size());
                if (!ins_.second) {
                    a_acc[ins_.first->second] = fe_add<R>(a_acc[ins_.first->second], sc);
                    continue;
                }
            }
            a_bases.push_back(pt);
            a_acc.push_back(sc);
        }
    }
    std::vector<uint64_t> a_sc(4 * a_bases.size());
    for (size_t q = 0; q < a_acc.size(); ++q) {
        const F s = fe_from_mont<R>(a_acc[q]);
        memcpy(&a_sc[4 * q], s.v, 32);
    }
    // ---- stage 5 ----
    int inf[2] = {0, 0};
    {
        ProfScope prof(c, "verify_msm");
        if ((rc = msm_bases(c, a_bases.data(), false, a_sc.data(), false, a_bases.size(), 0, out_ab, &inf[0])) ||
            (rc = msm_bases(c, b_bases.data(), false, bp.rho_c.data(), false, m, 0, out_ab + 2 * L64, &inf[1])))
            return rc;
    }
    if (out_inf) {
        out_inf[0] = inf[0];
        out_inf[1] = inf[1];
    }
    return ZKT_OK;
}

template <class C>
static int verify_batch_prepare_dev_t(zkt_ctx* c, const zkt_verify_inputs* ins, zkt_transcript* const* trs, size_t k,
                                      const uint64_t* h, const uint64_t* beta_h, uint64_t* out_ab, int* out_inf, uint64_t* out_rho) {
    BatchPrep<C> bp;
    int rc = batch_fold_dev<C>(c, "verify_batch_dev", ins, trs, k, h, beta_h, bp, out_ab, out_inf);
    if (rc) return rc;
    if (out_rho) memcpy(out_rho, bp.rho_c.data(), 2 * k * 32);
    return ZKT_OK;
}

// ---- zkt_debug_verify_terms / zkt_debug_verify_terms_host: the term stage alone, by any of its three routes ----------
// A built-in handle's state in a core transcript of its own (a stride of one in place of the kernel's LDS), and back
struct CoreCopy {
    TranscriptState st;
    uint64_t words[VT_LANE_WORDS] = {0};
    VtTr tr;
    bool load(HostTranscript& h) {
        if (!h.export_state(st)) return false;
        tr.s = VtSponge{words, words + VT_ST_WORDS, words + VT_ST_WORDS + VT_MSG_WORDS, 1};
        vt_load_state(tr, &st);
        return true;
    }
    bool store(HostTranscript& h) {
        vt_store_state(tr, &st);
        return h.import_state(st);
    }
};

// c == nullptr: no device (routes 0 and 1, the host's own decompression); route 2 needs a context
template <class C>
static int debug_terms_t(zkt_ctx* c, const zkt_verify_inputs* ins, zkt_transcript* const* trs, size_t k, const uint64_t* rho_c4,
                         const uint64_t* forced_mont, int route, uint64_t* out_ch, uint64_t* out_r0, uint64_t* out_acc,
                         int* out_status) {
    using Q = typename C::Fq;
    using R = typename C::Fr;
    using F = Fe<R>;
    const size_t nb = Q::N * 4, npts = 13 * k;
    auto err = [&](int rc, const std::string& what) { return c ? set_err(c, rc, "debug_verify_terms: " + what) : rc; };
    BatchPrep<C> bp;
    int rc = batch_bytes<C>(ins, trs, k, bp);
    if (rc) return err(rc, "proof " + std::to_string(bp.err_proof) + ": " + bp.err_what);
    bp.rho.resize(2 * k);
    for (size_t j = 0; j < 2 * k; ++j) {
        F r = fe_zero<R>();
        r.v[0] = 1;
        if (rho_c4) memcpy(r.v, rho_c4 + 4 * j, 32);
        bp.rho[j] = fe_to_mont<R>(r);
    }
    memset(out_ch, 0, k * 7 * 32);
    memset(out_r0, 0, k * 32);
    memset(out_acc, 0, k * SRC_COUNT * 32);
    if (route == 2) {
        TermsDev td;
        bool refused = false;
        if ((rc = stages12_dev<C>(c, ins, trs, k, bp, forced_mont, true, td, &refused)))
            return refused ? err(rc, "proof " + std::to_string(bp.err_proof) + ": " + bp.err_what) : rc;
        if (first_refused_point(td.point_status) < npts) return err(ZKT_ERR_INVALID_ARGUMENT, "a commitment was refused");
        const TranscriptState* states = (const TranscriptState*)td.at(td.lay.states);
        const int32_t* tstat = (const int32_t*)td.at(td.lay.status);
        for (size_t i = 0; i < k; ++i) {
            if (!trs[i]->impl->import_state(states[i])) return err(ZKT_ERR_INVALID_ARGUMENT, "the transcript refused its state");
            out_status[i] = tstat[i];
            memcpy(out_ch + 28 * i, td.at(td.lay.dbg) + i * 8 * 32, 7 * 32);
            memcpy(out_r0 + 4 * i, td.at(td.lay.dbg) + (i * 8 + 7) * 32, 32);
        }
        memcpy(out_acc, td.at(td.lay.acc), k * SRC_COUNT * 32);
        return ZKT_OK;
    }
    // ---- the commitments: through the device's decompression where there is a device ----
    if (c) {
        std::vector<uint8_t> status;
        if ((rc = decompress_stage<C>(c, bp, k, decomp_layout(npts, nb).end, status, [](char*) { return (int)ZKT_OK; }))) return rc;
        if (first_refused_point(status) < npts) return err(ZKT_ERR_INVALID_ARGUMENT, "a commitment was refused");
    } else {
        bp.cm.resize(npts);
        for (size_t p = 0; p < npts; ++p) {
            bool inf = false;
            if (!decompress<C>(bp.comp.data() + p * nb, &bp.cm[p], &inf)) return ZKT_ERR_INVALID_ARGUMENT;
        }
    }
    // ---- route 0: through the handle's virtual calls, as the batch verifier's host route and a caller's callbacks go;
    // ---- route 1: on the core's state directly, as the kernel goes
    for (size_t i = 0; i < k; ++i) {
        HostProof<C> hp(ins[i], bp.log_n[i], &bp.cm[13 * i], &bp.ev[12 * i]);
        F dbg[8];
        hp.p.rho[0] = bp.rho[2 * i];
        hp.p.rho[1] = bp.rho[2 * i + 1];
        hp.p.forced = forced_mont ? (const F*)forced_mont + 7 * i : nullptr;
        hp.p.acc = (F*)(out_acc + 4 * SRC_COUNT * i);
        hp.p.dbg = dbg;
        if (route == 0) {
            out_status[i] = vt_terms<C>(VtHostTr<C>{*trs[i]->impl}, hp.p);
        } else {
            CoreCopy cc;
            if (!cc.load(*trs[i]->impl)) return err(ZKT_ERR_INVALID_ARGUMENT, "a transcript that zkt_transcript_new did not make");
            out_status[i] = vt_terms<C>(VtCoreTr<C>{cc.tr}, hp.p);
            if (!cc.store(*trs[i]->impl)) return err(ZKT_ERR_INVALID_ARGUMENT, "the transcript refused its state");
        }
        memcpy(out_ch + 28 * i, dbg, 7 * 32);
        memcpy(out_r0 + 4 * i, dbg[7].v, 32);
    }
    return ZKT_OK;
}

extern "C" int zkt_debug_verify_terms(zkt_ctx* c, const zkt_verify_inputs* ins, zkt_transcript* const* transcripts, size_t count,
                                      const uint64_t* rho_canonical4, const uint64_t* forced_mont, int route,
                                      uint64_t* out_challenges, uint64_t* out_r0, uint64_t* out_acc, int* out_status) {
    if (!c) return ZKT_ERR_INVALID_ARGUMENT;
    if (!ins || !transcripts || count == 0 || count > ZKT_VERIFY_BATCH_DEV_MAX || !out_challenges || !out_r0 || !out_acc || !out_status)
        return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "debug_verify_terms: null pointer or bad count");
    if (route != 0 && route != 2) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "debug_verify_terms: route 0 (host) or 2 (kernel)");
    (void)hipSetDevice(c->device);
    if (c->curve == ZKT_CURVE_BN254)
        return debug_terms_t<Bn254Curve>(c, ins, transcripts, count, rho_canonical4, forced_mont, route, out_challenges, out_r0,
                                         out_acc, out_status);
    return debug_terms_t<Bls381Curve>(c, ins, transcripts, count, rho_canonical4, forced_mont, route, out_challenges, out_r0, out_acc,
                                      out_status);
}

extern "C" int zkt_debug_verify_terms_host(int curve_id, const zkt_verify_inputs* ins, zkt_transcript* const* transcripts,
                                           size_t count, const uint64_t* rho_canonical4, const uint64_t* forced_mont, int route,
                                           uint64_t* out_challenges, uint64_t* out_r0, uint64_t* out_acc, int* out_status) {
    if (!ins || !transcripts || count == 0 || count > ZKT_VERIFY_BATCH_DEV_MAX || !out_challenges || !out_r0 || !out_acc ||
        !out_status || (route != 0 && route != 1))
        return ZKT_ERR_INVALID_ARGUMENT;
    if (curve_id == ZKT_CURVE_BN254)
        return debug_terms_t<Bn254Curve>(nullptr, ins, transcripts, count, rho_canonical4, forced_mont, route, out_challenges,
                                         out_r0, out_acc, out_status);
    if (curve_id == ZKT_CURVE_BLS12_381)
        return debug_terms_t<Bls381Curve>(nullptr, ins, transcripts, count, rho_canonical4, forced_mont, route, out_challenges,
                                          out_r0, out_acc, out_status);
    return ZKT_ERR_INVALID_ARGUMENT;
}

// One transcript call on the core's state directly (transcript_core.hpp): the handle's state out, the call, the state in again
extern "C" int zkt_debug_verify_terms_transcript(zkt_transcript* t, int op, const char* label, const uint8_t* data, size_t len,
                                                 uint8_t out32[32]) {
    if (!t || !label || op < 0 || op > 2) return ZKT_ERR_INVALID_ARGUMENT;
    CoreCopy cc;
    if (!cc.load(*t->impl)) return ZKT_ERR_INVALID_ARGUMENT;
    VtTr& tr = cc.tr;
    if (op == 2) {
        if (!out32 || len < 16 || len > 264) return ZKT_ERR_INVALID_ARGUMENT;
        uint32_t w[8];
        vt_tr_challenge(tr, label, (uint32_t)len, w);
        memcpy(out32, w, 32);
    } else {
        if (!data || len > (op == 1 ? 96u : 8u * VT_MSG_WORDS) || (op == 1 && (len & 1))) return ZKT_ERR_INVALID_ARGUMENT;
        if (tr.kind != 0 && len > 68) return ZKT_ERR_INVALID_ARGUMENT;   // one Keccak-256 block: 65 + len + padding <= 136
        memcpy(cc.words + VT_ST_WORDS, data, len);
        if (op == 1) {
            vt_tr_commit_msg(tr, label, (uint32_t)(len / 2));             // the infinity byte behind x || y stays zero
        } else if (tr.kind == 0) {
            vt_merlin_header(tr, label, (uint32_t)len);
            vt_begin_op(tr, VT_FLAG_A);
            vt_absorb_msg(tr, (uint32_t)len);
        } else {
            vt_eth_append(tr, 0, (uint32_t)len);
        }
    }
    return cc.store(*t->impl) ? ZKT_OK : ZKT_ERR_INVALID_ARGUMENT;
}

extern "C" int zkt_ctx_set_verify_terms(zkt_ctx* c, int mode) {
    if (!c) return ZKT_ERR_INVALID_ARGUMENT;
    if (mode != 0 && mode != 1) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "mode: 0 on the host, 1 on the device");
    c->verify_terms_mode = mode;
    return ZKT_OK;
}

// e(P, h) e(-Q, beta h) == 1 for P, Q as (x, y) Montgomery limbs: the check of a batch, of a tree node, of one proof
template <class C>
static int pair_check(const uint64_t* pq, const uint64_t* h, const uint64_t* beta_h, int* one) {
    using Q = typename C::Fq;
    constexpr int L64 = Q::N / 2;
    uint64_t g1[2 * 12], g2[2 * 4 * 6];
    memcpy(g1, pq, 4 * L64 * 8);
    Affine<Q> wc;
    memcpy(wc.x.v, g1 + 2 * L64, L64 * 8);
    memcpy(wc.y.v, g1 + 3 * L64, L64 * 8);
    if (!aff_is_inf<Q>(wc)) wc.y = fe_neg<Q>(wc.y);
    memcpy(g1 + 3 * L64, wc.y.v, L64 * 8);
    memcpy(g2, h, 4 * L64 * 8);
    memcpy(g2 + 4 * L64, beta_h, 4 * L64 * 8);
    return pairing_check_t<C>(g1, g2, 2, one);
}

template <class C>
static int verify_batch_dev_t(zkt_ctx* c, const zkt_verify_inputs* ins, zkt_transcript* const* trs, size_t k, const uint64_t* h,
                              const uint64_t* beta_h, int* accepted) {
    uint64_t ab[2 * 12];
    int rc = verify_batch_prepare_dev_t<C>(c, ins, trs, k, h, beta_h, ab, nullptr, nullptr);
    if (rc) return rc;
    int one = 0;
    if ((rc = pair_check<C>(ab, h, beta_h, &one))) return set_err(c, rc, "verify_batch_dev: the pairing refused its arguments");
    *accepted = one ? 1 : 0;
    return ZKT_OK;
}

// ---- zkt_verify_batch_locate: which proofs of a rejected batch are bad -----------------------------------------
// The batch check is linear in the proofs: proof i has the pair (P_i, Q_i) of verify_leaves.hpp, which passes the check
// iff the proof verifies, and (A, B) is the sum of all pairs.  A rejected batch gets its `count` pairs and their binary
// tree of sums from the device, and the host walks down from the root at one pairing check per node it visits.
template <class C>
struct LocateTree {
    using Q = typename C::Fq;
    size_t count = 0, nodes = 0, sizes[VL_MAX_LEVELS], offs[VL_MAX_LEVELS];
    int levels = 0;
    std::vector<Xyzz<Q>> node;          // P's tree, then Q's; each level by level, leaves first
    void shape(size_t k) {
        count = k;
        levels = vl_levels(k, sizes, offs, &nodes);
        node.resize(2 * nodes);
    }
};

// the canonical scalars of the leaves: SRC_COUNT per proof
template <class C>
static std::vector<uint64_t> leaf_scalars(const BatchPrep<C>& bp) {
    using R = typename C::Fr;
    std::vector<uint64_t> sc(4 * bp.acc.size());
    for (size_t q = 0; q < bp.acc.size(); ++q) {
        const Fe<R> s = fe_from_mont<R>(bp.acc[q]);
        memcpy(&sc[4 * q], s.v, 32);
    }
    return sc;
}

// verify_scratch grown with its first `keep` bytes kept (stage 1's decompressed commitments are read again)
static int verify_scratch_grow(zkt_ctx* c, size_t keep, size_t bytes) {
    if (c->verify_scratch.p && c->verify_scratch.bytes >= bytes) return ZKT_OK;
    void* p = nullptr;
    int rc = dev_alloc(c, &p, bytes);
    if (rc) return rc;
    hipError_t e = hipMemcpyAsync(p, c->verify_scratch.p, keep, hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        dev_free(c, p);
        return hip_fail(c, e, "verify_scratch_grow");
    }
    dev_free(c, c->verify_scratch.p);
    c->verify_scratch = DevBuf{p, bytes};
    return ZKT_OK;
}

// Steps 3 and 4 on the device: the leaves from what batch_fold_dev left in verify_scratch and in bp, the levels, one download
template <class C>
static int locate_tree_dev(zkt_ctx* c, const BatchPrep<C>& bp, size_t k, LocateTree<C>& tree) {
    using Q = typename C::Fq;
    tree.shape(k);
    const VlLayout lay = vl_layout(bp.stage1_end, k, Q::N * 4, vl_raw_bytes(c->curve));
    int rc = verify_scratch_grow(c, bp.stage1_end, lay.end);
    if (rc) return rc;
    char* const base = (char*)c->verify_scratch.p;
    const std::vector<uint64_t> sc = leaf_scalars<C>(bp);
    auto copy = [&](void* dst, const void* src, size_t bytes, hipMemcpyKind kind, const char* what) {
        copy_step(c, rc, dst, src, bytes, kind, what);   // an upload may still be reading sc: one synchronise below
    };
    {
        ProfScope prof(c, "verify_leaves");
        copy(base + lay.other, bp.other.data(), bp.other.size() * sizeof(Affine<Q>), hipMemcpyHostToDevice, "verify leaves: bases upload");
        copy(base + lay.scalars, sc.data(), sc.size() * 8, hipMemcpyHostToDevice, "verify leaves: scalars upload");
        copy(base + lay.rho, bp.rho_c.data(), bp.rho_c.size() * 8, hipMemcpyHostToDevice, "verify leaves: coefficients upload");
        if (!rc)
            rc = verify_leaves_enqueue(c, base + bp.points_offset, base + lay.other, base + lay.scalars, base + lay.rho, k,
                                       base + lay.products, base + lay.tree, tree.nodes);
    }
    if (!rc) {
        ProfScope prof(c, "verify_tree");
        rc = verify_tree_enqueue(c, base + lay.tree, k, tree.nodes);
        copy(tree.node.data(), base + lay.tree, tree.node.size() * sizeof(Xyzz<Q>), hipMemcpyDeviceToHost, "verify tree download");
    }
    const hipError_t e = hipStreamSynchronize(c->stream);
    if (!rc && e != hipSuccess) rc = hip_fail(c, e, "verify tree");
    return rc;
}

// ... and on the host, through the same per-term, per-leaf and per-node code
template <class C>
static void locate_tree_host(const BatchPrep<C>& bp, size_t k, LocateTree<C>& tree) {
    using Q = typename C::Fq;
    tree.shape(k);
    const std::vector<uint64_t> sc = leaf_scalars<C>(bp);
    auto words = [](const uint64_t* w, uint32_t (&out)[8]) { memcpy(out, w, 32); };
    for (size_t i = 0; i < k; ++i) {
        XyzzX<Q> prod[VL_TERMS];
        uint32_t kw[8];
        for (int s = 0; s < VL_SOURCES; ++s) {
            words(&sc[4 * (SRC_COUNT * i + s)], kw);
            prod[s] = vl_mul<Q>(bp.base(i, s), kw);
        }
        for (int o = 0; o < 2; ++o) {
            words(&bp.rho_c[4 * (2 * i + o)], kw);
            prod[VL_SOURCES + o] = vl_mul<Q>(bp.cm[13 * i + VL_WITNESS0 + o], kw);
        }
        tree.node[i] = vl_pack<Q>(vl_sum<Q>(VL_SOURCES, [&](int t) { return prod[t]; }));
        tree.node[tree.nodes + i] = vl_pack<Q>(vl_sum<Q>(2, [&](int t) { return prod[VL_SOURCES + t]; }));
    }
    for (int half = 0; half < 2; ++half)
        for (int l = 0; l + 1 < tree.levels; ++l) {
            const Xyzz<Q>* src = &tree.node[half * tree.nodes + tree.offs[l]];
            Xyzz<Q>* dst = &tree.node[half * tree.nodes + tree.offs[l + 1]];
            for (size_t m = 0; m < tree.sizes[l + 1]; ++m)
                dst[m] = 2 * m + 1 < tree.sizes[l] ? vl_parent<Q>(src[2 * m], src[2 * m + 1]) : src[2 * m];
        }
}

// Step 5: the root is known to fail.  At a failing inner node the left child is checked; if it passes, the right one
// fails without a check, otherwise the right one is checked too: at most 2 ceil(log2 count) checks per bad proof.
template <class C>
static int locate_descend(const LocateTree<C>& tree, const uint64_t* h, const uint64_t* beta_h, std::vector<uint8_t>& bad,
                          size_t* n_checks) {
    using Q = typename C::Fq;
    constexpr int L64 = Q::N / 2;
    bad.assign(tree.count, 0);
    auto passes = [&](int l, size_t m, bool* ok) {
        uint64_t pq[4 * 6];
        for (int half = 0; half < 2; ++half) {
            const Affine<Q> a = xyzz_to_affine_host<Q>(tree.node[half * tree.nodes + tree.offs[l] + m]);
            memcpy(pq + half * 2 * L64, a.x.v, L64 * 8);
            memcpy(pq + half * 2 * L64 + L64, a.y.v, L64 * 8);
        }
        int one = 0;
        int rc = pair_check<C>(pq, h, beta_h, &one);
        ++*n_checks;
        *ok = one != 0;
        return rc;
    };
    std::vector<std::pair<int, size_t>> failing{{tree.levels - 1, 0}};
    while (!failing.empty()) {
        const int l = failing.back().first;
        const size_t m = failing.back().second;
        failing.pop_back();
        if (l == 0) {
            bad[m] = 1;
            continue;
        }
        if (2 * m + 1 >= tree.sizes[l - 1]) {             // the unpaired node moved up unchanged
            failing.push_back({l - 1, 2 * m});
            continue;
        }
        bool left = false, right = false;
        if (int rc = passes(l - 1, 2 * m, &left)) return rc;
        if (!left) {
            failing.push_back({l - 1, 2 * m});
            if (int rc = passes(l - 1, 2 * m + 1, &right)) return rc;
        }
        if (!right) failing.push_back({l - 1, 2 * m + 1});
    }
    return ZKT_OK;
}

// every node as affine (x, y), one field inversion for all of them (Montgomery's trick)
template <class C>
static void tree_affine(const LocateTree<C>& tree, uint64_t* out_xy, int* out_inf) {
    using Q = typename C::Fq;
    constexpr int L64 = Q::N / 2;
    const size_t n = tree.node.size();
    std::vector<Fe<Q>> pre(n + 1);
    pre[0] = fe_one<Q>();
    for (size_t i = 0; i < n; ++i) {
        const Xyzz<Q>& p = tree.node[i];
        pre[i + 1] = xyzz_is_identity<Q>(p) ? pre[i] : fe_mul<Q>(pre[i], fe_mul<Q>(p.zz, p.zzz));
    }
    Fe<Q> inv = fe_inv_host<Q>(pre[n]);
    for (size_t i = n; i-- > 0;) {
        const Xyzz<Q>& p = tree.node[i];
        Affine<Q> a;
        a.x = fe_zero<Q>();
        a.y = fe_zero<Q>();
        const bool is_inf = xyzz_is_identity<Q>(p);
        if (!is_inf) {
            const Fe<Q> d = fe_mul<Q>(inv, pre[i]);       // 1 / (zz zzz)
            inv = fe_mul<Q>(inv, fe_mul<Q>(p.zz, p.zzz));
            a.x = fe_mul<Q>(p.x, fe_mul<Q>(d, p.zzz));    // X / ZZ
            a.y = fe_mul<Q>(p.y, fe_mul<Q>(d, p.zz));     // Y / ZZZ
        }
        if (out_xy) {
            memcpy(out_xy + i * 2 * L64, a.x.v, L64 * 8);
            memcpy(out_xy + i * 2 * L64 + L64, a.y.v, L64 * 8);
        }
        if (out_inf) out_inf[i] = is_inf ? 1 : 0;
    }
}

// The verdict from the root's check on: *accepted, out_bad, the two counters (none of them touched on an error).
// build_tree() fills `tree` when the root fails; it is not called for an accepted batch.  *pairing_refused: the error is a
// pairing check's, not build_tree's.
template <class C, class BuildTree>
static int locate_finish(const uint64_t* root, size_t k, const uint64_t* h, const uint64_t* beta_h, const LocateTree<C>& tree,
                         BuildTree build_tree, int* accepted, uint8_t* out_bad, size_t* n_bad, size_t* n_checks,
                         bool* pairing_refused) {
    int one = 0;
    *pairing_refused = true;
    int rc = pair_check<C>(root, h, beta_h, &one);
    if (rc) return rc;
    size_t checks = 1, b = 0;
    std::vector<uint8_t> bad(k, 0);
    if (!one) {
        *pairing_refused = false;
        if ((rc = build_tree())) return rc;
        *pairing_refused = true;
        if ((rc = locate_descend<C>(tree, h, beta_h, bad, &checks))) return rc;
        for (size_t i = 0; i < k; ++i) b += bad[i];
    }
    *accepted = one ? 1 : 0;
    memcpy(out_bad, bad.data(), k);
    if (n_bad) *n_bad = b;
    if (n_checks) *n_checks = checks;
    return ZKT_OK;
}

template <class C>
static int verify_batch_locate_t(zkt_ctx* c, const zkt_verify_inputs* ins, zkt_transcript* const* trs, size_t k,
                                 const uint64_t* h, const uint64_t* beta_h, int* accepted, uint8_t* out_bad, size_t* n_bad,
                                 size_t* n_checks) {
    BatchPrep<C> bp;
    uint64_t ab[2 * 12];
    int rc = batch_fold_dev<C>(c, "verify_batch_locate", ins, trs, k, h, beta_h, bp, ab, nullptr);
    if (rc) return rc;
    LocateTree<C> tree;
    bool pairing_refused = false;
    rc = locate_finish<C>(ab, k, h, beta_h, tree, [&] { return locate_tree_dev<C>(c, bp, k, tree); }, accepted, out_bad, n_bad,
                          n_checks, &pairing_refused);
    if (rc && pairing_refused) return set_err(c, rc, "verify_batch_locate: the pairing refused its arguments");
    return rc;
}

template <class C>
static int debug_verify_batch_tree_t(zkt_ctx* c, const zkt_verify_inputs* ins, zkt_transcript* const* trs, size_t k,
                                     const uint64_t* h, const uint64_t* beta_h, uint64_t* out_nodes, int* out_inf, uint64_t* out_rho) {
    BatchPrep<C> bp;
    uint64_t ab[2 * 12];
    int rc = batch_fold_dev<C>(c, "debug_verify_batch_tree", ins, trs, k, h, beta_h, bp, ab, nullptr);
    if (rc) return rc;
    LocateTree<C> tree;
    if ((rc = locate_tree_dev<C>(c, bp, k, tree))) return rc;
    tree_affine<C>(tree, out_nodes, out_inf);
    if (out_rho) memcpy(out_rho, bp.rho_c.data(), 2 * k * 32);
    return ZKT_OK;
}

// The whole of zkt_verify_batch_locate without a device: the host's own deserialisation for stage 1, the root from the
// tree, and leaves and levels through the code the kernels run
template <class C>
static int debug_verify_locate_host_t(const zkt_verify_inputs* ins, zkt_transcript* const* trs, size_t k, const uint64_t* h,
                                      const uint64_t* beta_h, int* accepted, uint8_t* out_bad, size_t* n_bad, size_t* n_checks,
                                      uint64_t* out_nodes, int* out_inf, uint64_t* out_rho) {
    using Q = typename C::Fq;
    constexpr int L64 = Q::N / 2;
    const size_t nb = Q::N * 4;
    BatchPrep<C> bp;
    int rc = batch_bytes<C>(ins, trs, k, bp);
    if (rc) return rc;
    bp.cm.resize(13 * k);
    for (size_t p = 0; p < 13 * k; ++p) {
        bool inf = false;
        if (!decompress<C>(bp.comp.data() + p * nb, &bp.cm[p], &inf)) return ZKT_ERR_INVALID_ARGUMENT;
    }
    batch_coefficients<C>(ins, k, h, beta_h, bp);
    if ((rc = batch_terms<C>(ins, trs, k, bp))) return rc;
    LocateTree<C> tree;
    locate_tree_host<C>(bp, k, tree);
    uint64_t root[4 * 6];
    for (int half = 0; half < 2; ++half) {
        const Affine<Q> a = xyzz_to_affine_host<Q>(tree.node[half * tree.nodes + tree.nodes - 1]);
        memcpy(root + half * 2 * L64, a.x.v, L64 * 8);
        memcpy(root + half * 2 * L64 + L64, a.y.v, L64 * 8);
    }
    bool pairing_refused = false;
    if ((rc = locate_finish<C>(root, k, h, beta_h, tree, [] { return (int)ZKT_OK; }, accepted, out_bad, n_bad, n_checks,
                               &pairing_refused)))
        return rc;
    if (out_nodes || out_inf) tree_affine<C>(tree, out_nodes, out_inf);
    if (out_rho) memcpy(out_rho, bp.rho_c.data(), 2 * k * 32);
    return ZKT_OK;
}

static int verify_batch_dev_args(zkt_ctx* c, const void* ins, const void* trs, size_t count, const void* h, const void* bh,
                                 const void* out) {
    if (!c) return ZKT_ERR_INVALID_ARGUMENT;
    if (count == 0) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "verify_batch_dev: an empty batch");
    if (count > ZKT_VERIFY_BATCH_DEV_MAX)
        return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "verify_batch_dev: more proofs than ZKT_VERIFY_BATCH_DEV_MAX");
    if (!ins || !trs || !h || !bh || !out) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    (void)hipSetDevice(c->device);
    return ZKT_OK;
}

extern "C" int zkt_verify_batch_prepare_dev(zkt_ctx* c, const zkt_verify_inputs* ins, zkt_transcript* const* transcripts,
                                            size_t count, const uint64_t* h_g2_mont, const uint64_t* beta_h_g2_mont,
                                            uint64_t* out_ab, int* out_ab_is_infinity, uint64_t* out_rho) {
    if (int rc = verify_batch_dev_args(c, ins, transcripts, count, h_g2_mont, beta_h_g2_mont, out_ab)) return rc;
    if (c->curve == ZKT_CURVE_BN254)
        return verify_batch_prepare_dev_t<Bn254Curve>(c, ins, transcripts, count, h_g2_mont, beta_h_g2_mont, out_ab,
                                                      out_ab_is_infinity, out_rho);
    return verify_batch_prepare_dev_t<Bls381Curve>(c, ins, transcripts, count, h_g2_mont, beta_h_g2_mont, out_ab,
                                                   out_ab_is_infinity, out_rho);
}

extern "C" int zkt_verify_batch_dev(zkt_ctx* c, const zkt_verify_inputs* ins, zkt_transcript* const* transcripts, size_t count,
                                    const uint64_t* h_g2_mont, const uint64_t* beta_h_g2_mont, int* accepted) {
    if (int rc = verify_batch_dev_args(c, ins, transcripts, count, h_g2_mont, beta_h_g2_mont, accepted)) return rc;
    if (c->curve == ZKT_CURVE_BN254)
        return verify_batch_dev_t<Bn254Curve>(c, ins, transcripts, count, h_g2_mont, beta_h_g2_mont, accepted);
    return verify_batch_dev_t<Bls381Curve>(c, ins, transcripts, count, h_g2_mont, beta_h_g2_mont, accepted);
}

extern "C" int zkt_verify_batch_locate(zkt_ctx* c, const zkt_verify_inputs* ins, zkt_transcript* const* transcripts,
                                       size_t count, const uint64_t* h_g2_mont, const uint64_t* beta_h_g2_mont,
                                       int* accepted, uint8_t* out_bad, size_t* n_bad, size_t* n_checks) {
    if (int rc = verify_batch_dev_args(c, ins, transcripts, count, h_g2_mont, beta_h_g2_mont, accepted)) return rc;
    if (!out_bad) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (c->curve == ZKT_CURVE_BN254)
        return verify_batch_locate_t<Bn254Curve>(c, ins, transcripts, count, h_g2_mont, beta_h_g2_mont, accepted, out_bad,
                                                 n_bad, n_checks);
    return verify_batch_locate_t<Bls381Curve>(c, ins, transcripts, count, h_g2_mont, beta_h_g2_mont, accepted, out_bad, n_bad,
                                              n_checks);
}

extern "C" int zkt_debug_verify_batch_tree(zkt_ctx* c, const zkt_verify_inputs* ins, zkt_transcript* const* transcripts,
                                           size_t count, const uint64_t* h_g2_mont, const uint64_t* beta_h_g2_mont,
                                           uint64_t* out_nodes_xy_mont, int* out_is_infinity, uint64_t* out_rho) {
    if (int rc = verify_batch_dev_args(c, ins, transcripts, count, h_g2_mont, beta_h_g2_mont, out_nodes_xy_mont)) return rc;
    if (c->curve == ZKT_CURVE_BN254)
        return debug_verify_batch_tree_t<Bn254Curve>(c, ins, transcripts, count, h_g2_mont, beta_h_g2_mont, out_nodes_xy_mont,
                                                     out_is_infinity, out_rho);
    return debug_verify_batch_tree_t<Bls381Curve>(c, ins, transcripts, count, h_g2_mont, beta_h_g2_mont, out_nodes_xy_mont,
                                                  out_is_infinity, out_rho);
}

extern "C" int zkt_debug_verify_locate_host(int curve_id, const zkt_verify_inputs* ins, zkt_transcript* const* transcripts,
                                            size_t count, const uint64_t* h_g2_mont, const uint64_t* beta_h_g2_mont,
                                            int* accepted, uint8_t* out_bad, size_t* n_bad, size_t* n_checks,
                                            uint64_t* out_nodes_xy_mont, int* out_is_infinity, uint64_t* out_rho) {
    if (!ins || !transcripts || count == 0 || count > ZKT_VERIFY_BATCH_DEV_MAX || !h_g2_mont || !beta_h_g2_mont || !accepted ||
        !out_bad)
        return ZKT_ERR_INVALID_ARGUMENT;
    if (curve_id == ZKT_CURVE_BN254)
        return debug_verify_locate_host_t<Bn254Curve>(ins, transcripts, count, h_g2_mont, beta_h_g2_mont, accepted, out_bad,
                                                      n_bad, n_checks, out_nodes_xy_mont, out_is_infinity, out_rho);
    if (curve_id == ZKT_CURVE_BLS12_381)
        return debug_verify_locate_host_t<Bls381Curve>(ins, transcripts, count, h_g2_mont, beta_h_g2_mont, accepted, out_bad,
                                                       n_bad, n_checks, out_nodes_xy_mont, out_is_infinity, out_rho);
    return ZKT_ERR_INVALID_ARGUMENT;
}

// ---- the G2 half of the test / bench SRS (zkt_srs_generate is the G1 half): h = the G2 generator of ark-bn254 /
// ---- ark-bls12-381 (published constants), beta h = tau h by double-and-add on the twist (one-time, host) ----------
template <class C>
static int srs_g2_t(const uint64_t* tau4, uint64_t* out_h, uint64_t* out_beta_h) {
    using Q = typename C::Fq;
    using R = typename C::Fr;
    using T = pairing::Tower<C>;
    using E2 = typename T::E2;
    constexpr int L64 = Q::N / 2;
    static const uint64_t gen_bn[4][4] = {
        {0x46debd5cd992f6edULL, 0x674322d4f75edaddULL, 0x426a00665e5c4479ULL, 0x1800deef121f1e76ULL},
        {0x97e485b7aef312c2ULL, 0xf1aa493335a9e712ULL, 0x7260bfb731fb5d25ULL, 0x198e9393920d483aULL},
        {0x4ce6cc0166fa7daaULL, 0xe3d1e7690c43d37bULL, 0x4aab71808dcb408fULL, 0x12c85ea5db8c6debULL},
        {0x55acdadcd122975bULL, 0xbc4b313370b38ef3ULL, 0xec9e99ad690c3395ULL, 0x090689d0585ff075ULL}};
    static const uint64_t gen_bls[4][6] = {
        {0xd48056c8c121bdb8ULL, 0x0bac0326a805bbefULL, 0xb4510b647ae3d177ULL, 0xc6e47ad4fa403b02ULL, 0x260805272dc51051ULL, 0x024aa2b2f08f0a91ULL},
        {0xe5ac7d055d042b7eULL, 0x334cf11213945d57ULL, 0xb5da61bbdc7f5049ULL, 0x596bd0d09920b61aULL, 0x7dacd3a088274f65ULL, 0x13e02b6052719f60ULL},
        {0xe193548608b82801ULL, 0x923ac9cc3baca289ULL, 0x6d429a695160d12cULL, 0xadfd9baa8cbdd3a7ULL, 0x8cc9cdc6da2e351aULL, 0x0ce5d527727d6e11ULL},
        {0xaaa9075ff05f79beULL, 0x3f370d275cec1da1ULL, 0x267492ab572e99abULL, 0xcb3e287e85a763afULL, 0x32acd2b02bc28b99ULL, 0x0606c4a02ea734ccULL}};
    hostec::HF<Q> c[4];
    for (int k = 0; k < 4; ++k) {
        Fe<Q> v;
        memcpy(v.v, C::ID == 0 ? (const void*)gen_bn[k] : (const void*)gen_bls[k], L64 * 8);
        c[k] = hostec::hf_from<Q>(fe_to_mont<Q>(v));
    }
    const E2 gx{c[0], c[1]}, gy{c[2], c[3]};
    typename T::G2 gq{gx, gy, false};
    if (!T::g2_on_twist(gq)) return ZKT_ERR_INVALID_ARGUMENT;
    Fe<R> tau;
    memcpy(tau.v, tau4, 32);
    // affine double-and-add; (x, y, inf)
    E2 ax = gx, ay = gy;
    bool ainf = true;
    auto add_pt = [&](const E2& px, const E2& py, bool pinf) {   // acc += p
        if (pinf) return;
        if (ainf) { ax = px; ay = py; ainf = false; return; }
        E2 lam, di;
        if (T::eq2(ax, px)) {
            if (!T::eq2(ay, py) || T::is_zero2(ay)) { ainf = true; return; }
            (void)T::inv2(T::dbl2(ay), &di);
            const E2 xx = T::sqr2(ax);
            lam = T::mul2(T::add2(T::dbl2(xx), xx), di);
        } else {
            (void)T::inv2(T::sub2(px, ax), &di);
            lam = T::mul2(T::sub2(py, ay), di);
        }
        const E2 nx = T::sub2(T::sub2(T::sqr2(lam), ax), px);
        ay = T::sub2(T::mul2(lam, T::sub2(ax, nx)), ay);
        ax = nx;
    };
    for (int i = R::N * 32 - 1; i >= 0; --i) {
        if (!ainf) add_pt(ax, ay, false);                         // double
        if ((tau.v[i / 32] >> (i % 32)) & 1u) add_pt(gx, gy, false);
    }
    memcpy(out_h, &gx, 2 * L64 * 8);
    memcpy(out_h + 2 * L64, &gy, 2 * L64 * 8);
    if (ainf) {
        memset(out_beta_h, 0, 4 * L64 * 8);
    } else {
        memcpy(out_beta_h, &ax, 2 * L64 * 8);
        memcpy(out_beta_h + 2 * L64, &ay, 2 * L64 * 8);
    }
    return ZKT_OK;
}

extern "C" int zkt_srs_generate_g2(int curve_id, const uint64_t* tau_canonical4, uint64_t* out_h, uint64_t* out_beta_h) {
    if (!tau_canonical4 || !out_h || !out_beta_h) return ZKT_ERR_INVALID_ARGUMENT;
    if (curve_id == ZKT_CURVE_BN254) return srs_g2_t<Bn254Curve>(tau_canonical4, out_h, out_beta_h);
    if (curve_id == ZKT_CURVE_BLS12_381) return srs_g2_t<Bls381Curve>(tau_canonical4, out_h, out_beta_h);
    return ZKT_ERR_INVALID_ARGUMENT;
}

extern "C" int zkt_verify(int curve_id, const zkt_verify_inputs* in, zkt_transcript* transcript, const uint64_t* h_g2_mont,
                          const uint64_t* beta_h_g2_mont, int* accepted) {
    if (!in || !transcript || !h_g2_mont || !beta_h_g2_mont || !accepted) return ZKT_ERR_INVALID_ARGUMENT;
    if (curve_id == ZKT_CURVE_BN254) return verify_t<Bn254Curve>(curve_id, in, transcript, h_g2_mont, beta_h_g2_mont, accepted);
    if (curve_id == ZKT_CURVE_BLS12_381) return verify_t<Bls381Curve>(curve_id, in, transcript, h_g2_mont, beta_h_g2_mont, accepted);
    return ZKT_ERR_INVALID_ARGUMENT;
}

extern "C" int zkt_verify_batch(int curve_id, const zkt_verify_inputs* ins, zkt_transcript* const* transcripts, size_t count,
                                const uint64_t* h_g2_mont, const uint64_t* beta_h_g2_mont, int* accepted) {
    if (!ins || !transcripts || count == 0 || count > (1u << 20) || !h_g2_mont || !beta_h_g2_mont || !accepted)
        return ZKT_ERR_INVALID_ARGUMENT;
    if (curve_id == ZKT_CURVE_BN254)
        return verify_batch_t<Bn254Curve>(curve_id, ins, transcripts, count, h_g2_mont, beta_h_g2_mont, accepted);
    if (curve_id == ZKT_CURVE_BLS12_381)
        return verify_batch_t<Bls381Curve>(curve_id, ins, transcripts, count, h_g2_mont, beta_h_g2_mont, accepted);
    return ZKT_ERR_INVALID_ARGUMENT;
}

extern "C" int zkt_verify_prepare(int curve_id, const zkt_verify_inputs* in, zkt_transcript* transcript, uint64_t* out_pairs,
                                  int* out_is_infinity) {
    if (!in || !transcript || !out_pairs || !in->proof || !in->vk_commitments || !in->g || (in->n_pi && (!in->pi_roots || !in->pub_inputs)))
        return ZKT_ERR_INVALID_ARGUMENT;
    if (curve_id == ZKT_CURVE_BN254) return Verifier<Bn254Curve>::run(*in, *transcript->impl, out_pairs, out_is_infinity);
    if (curve_id == ZKT_CURVE_BLS12_381) return Verifier<Bls381Curve>::run(*in, *transcript->impl, out_pairs, out_is_infinity);
    return ZKT_ERR_INVALID_ARGUMENT;
}
