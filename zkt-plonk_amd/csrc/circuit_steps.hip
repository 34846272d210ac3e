// Entries that run single steps of a proof over the loaded circuit's work buffers, without a prover: the commitment of an
// evaluation vector (zkt_commit_evals_dev) and the test hooks of the quotient, the linearisation's kernels and the opening
// division.  Host orchestration only: every launch is another unit's.
#include "circuit.hpp"
#include "msm.hpp"

namespace zkt {

template <class R>
static void debug_quotient_classes_host_t(int log_n, const uint64_t* windows, const uint64_t* challenges, uint64_t* out_u,
                                          uint64_t* out_consts) {
    typedef Fe<R> F;
    const QuotientClassConsts<R> q = quotient_class_consts<R>(log_n);
    for (int k = 0; k < 4; ++k) memcpy(out_consts + 4 * k, q.gamma[k].v, 32);
    for (int k = 0; k < 9; ++k) memcpy(out_consts + 4 * (4 + k), q.vinv[k].v, 32);
    for (int k = 0; k < 3; ++k) memcpy(out_consts + 4 * (13 + k), q.g3[k].v, 32);
    const uint32_t* w = (const uint32_t*)windows;
    QuotientWindows W{};
    const uint32_t** slot[10] = {&W.a, &W.b, &W.c, &W.z1, &W.z2, &W.t, &W.sigma1, &W.sigma2, &W.sigma3, &W.q_lookup};
    for (int k = 0; k < 10; ++k) *slot[k] = w + (size_t)k * QCW * 8;
    F alpha, beta, delta, u[6];
    memcpy(alpha.v, challenges, 32);
    memcpy(beta.v, challenges + 4, 32);
    memcpy(delta.v, challenges + 8, 32);
    quotient_top_coefficients<R>(log_n, W, alpha, beta, delta, u);
    for (int e = 0; e < 6; ++e) memcpy(out_u + 4 * e, u[e].v, 32);
}

}  // namespace zkt

using namespace zkt;

extern "C" {

int zkt_debug_quotient_top(zkt_ctx* c, uint64_t* out_u, int* out_on_classes) {
    if (!c || !out_u) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (int rc = circuit_entry(c, 0)) return rc;
    const CircuitState& S = *c->circuit;
    if (out_on_classes) *out_on_classes = S.use_classes ? 1 : 0;
    memcpy(out_u, S.last_u, sizeof(S.last_u));   // zero until a proof has taken the route
    return ZKT_OK;
}

int zkt_debug_quotient_coeffs(zkt_ctx* c, uint64_t* out, size_t count) {
    if (!c || !out) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (int rc = circuit_entry(c, ENTRY_DEVICE)) return rc;
    const CircuitState& S = *c->circuit;
    if (count > 4 * S.n) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "the quotient vector holds 4n elements");
    ZKT_HIP(c, hipStreamSynchronize(c->stream));
    ZKT_HIP(c, hipMemcpy(out, S.qev, count * 32, hipMemcpyDeviceToHost));
    return ZKT_OK;
}

int zkt_debug_quotient_classes_host(int curve, int log_n, const uint64_t* windows, const uint64_t* challenges, uint64_t* out_u,
                                    uint64_t* out_consts) {
    if (!windows || !challenges || !out_u || !out_consts) return ZKT_ERR_INVALID_ARGUMENT;
    if (curve != ZKT_CURVE_BN254 && curve != ZKT_CURVE_BLS12_381) return ZKT_ERR_INVALID_ARGUMENT;
    return by_curve(curve, [&](auto C) {
        using R = typename decltype(C)::Fr;
        if (log_n < 3 || log_n + 2 > R::TWO_ADICITY) return (int)ZKT_ERR_INVALID_DOMAIN_SIZE;
        debug_quotient_classes_host_t<R>(log_n, windows, challenges, out_u, out_consts);
        return (int)ZKT_OK;
    });
}

// ---- commitments of evaluation vectors (lagrange.hip) --------------------------------------------------
int zkt_lagrange_info(zkt_ctx* c, int* log_n, size_t* bases) {
    if (!c) return ZKT_ERR_INVALID_ARGUMENT;
    const bool ready = c->circuit && lagrange_ready(c, c->circuit->log_n) && !c->lagrange_off;
    if (log_n) *log_n = ready ? c->circuit->log_n : -1;
    if (bases) *bases = ready ? lagrange_bases(c) : 0;
    return ZKT_OK;
}

int zkt_commit_evals_dev(zkt_ctx* c, const void* d_evals, const uint64_t* blinders, int k, int path, uint64_t* out_xy,
                         int* out_is_infinity) {
    if (!c || !d_evals || !out_xy || (k > 0 && !blinders)) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (k < 0 || k > 3) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "0 .. 3 blinders");
    // the work buffer below belongs to round 5 of an announced proof as well
    if (int rc0 = circuit_entry(c, ENTRY_DOMAIN | ENTRY_SRS | ENTRY_WHOLE_KEY | ENTRY_DEVICE | ENTRY_WITHDRAW)) return rc0;
    CircuitState& S = *c->circuit;
    const size_t n = S.n;
    int rc;
    if (path == 1) {
        if ((rc = lagrange_ensure(c, S.log_n))) return rc;
        if (!lagrange_ready(c, S.log_n)) return set_err(c, ZKT_ERR_NOT_LOADED, "the key is too short for the Lagrange-basis table");
    } else if (path != 0) {
        return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "path: 0 coefficients, 1 Lagrange basis");
    }
    uint32_t* d_len = S.status + 8 + 12;
    void* d_bl = (char*)S.lag_scalars + (n + 8) * 32;
    void* poly = S.poly[12];
    ZKT_HIP(c, hipMemsetAsync(d_len, 0, 4, c->stream));
    if (k) ZKT_HIP(c, hipMemcpyAsync(d_bl, blinders, (size_t)k * 32, hipMemcpyHostToDevice, c->stream));
    // poly_from_evals + add_blinders_to_poly (util.rs:63-86, prove.rs:472-483)
    if ((rc = ntt_run(c, S.log_n, 1, 0, d_evals, n, poly))) return rc;
    if (c->fused(4)) {
        const TrimBlindSpec tb{poly, d_bl, d_len, k};
        if ((rc = poly_trim_blind(c, &tb, 1, n, 8))) return rc;
    } else {
        if ((rc = poly_trim_len(c, poly, n, d_len, (char*)poly + n * 32, 8))) return rc;
        if (k && (rc = poly_add_blinders(c, poly, d_len, d_bl, k, n + 8))) return rc;
    }
    if (path == 0) return msm_g1_dev(c, poly, n + (size_t)k, 0, 1, out_xy, out_is_infinity);
    if ((rc = lagrange_scalars(c, d_evals, n, d_len, d_bl, k, S.roots, S.lag_scalars))) return rc;
    if ((rc = msm_begin(c, S.lag_scalars, n + (size_t)k, 0, 1, 0, 1))) return rc;
    uint64_t xy[12] = {};
    if ((rc = msm_end(c, 0, xy))) return rc;
    const size_t words = c->curve == ZKT_CURVE_BN254 ? 8 : 12;
    memcpy(out_xy, xy, words * 8);
    if (out_is_infinity) {
        bool any = false;
        for (size_t i = 0; i < words; ++i) any = any || xy[i] != 0;
        *out_is_infinity = any ? 0 : 1;
    }
    return ZKT_OK;
}

// Test hook: the fused quotient pass on its own (quotient_poly.rs:98-224) over the loaded circuit's key cosets and
// caller-supplied witness cosets, so that the kernel is compared point by point on inputs that satisfy nothing.
int zkt_debug_quotient(zkt_ctx* c, const uint64_t* challenges, const uint64_t* const* wit, const uint64_t* pi_pos,
                       const uint64_t* pi_vals, size_t n_pi, uint64_t* out) {
    if (!c || !challenges || !wit || !out || (n_pi && (!pi_pos || !pi_vals)))
        return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (int rc0 = circuit_entry(c, ENTRY_DEVICE)) return rc0;
    CircuitState& S = *c->circuit;
    if (S.G != 1) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "zkt_debug_quotient: whole-coset circuits only");
    if (n_pi > (size_t)QUOTIENT_PI_DIRECT_MAX) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "too many direct public inputs");
    for (size_t i = 0; i < n_pi; ++i)
        if (pi_pos[i] >= S.n) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "public input position out of range");
    const size_t bytes = 4 * S.n * 32;
    DevSet tmp(c->device);
    void* d[W_COUNT] = {};
    void* d_out = nullptr;
    uint32_t* d_tab = nullptr;
    int rc = ZKT_OK;
    for (int k = 0; k < W_COUNT && !rc; ++k) {
        if (k == W_PI && n_pi) continue;
        if (!wit[k]) rc = set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null witness coset");
        else if (!(rc = tmp.alloc(c, &d[k], bytes)) && hipMemcpy(d[k], wit[k], bytes, hipMemcpyHostToDevice) != hipSuccess)
            rc = set_err(c, ZKT_ERR_HIP, "copy of a witness coset failed");
    }
    if (!rc) rc = tmp.alloc(c, &d_out, bytes);
    if (!rc && n_pi) {
        std::vector<uint32_t> tab(10 * n_pi);
        by_curve(c->curve, [&](auto C) { pi_rows<typename decltype(C)::Fr>(pi_pos, pi_vals, n_pi, 1, tab.data()); });
        if (!(rc = tmp.alloc(c, (void**)&d_tab, tab.size() * 4)) &&
            hipMemcpy(d_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
            rc = set_err(c, ZKT_ERR_HIP, "copy of the public-input rows failed");
    }
    if (!rc) {
        QuotientArgs q = quotient_args(S, d, challenges, challenges + 4, challenges + 8, challenges + 12, challenges + 16);
        q.out = d_out;
        q.n4 = 4 * S.n;
        q.pi_tab = n_pi ? d_tab : nullptr;
        q.n_pi_direct = (uint32_t)n_pi;
        rc = quotient_pointwise(c, q);
        if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = set_err(c, ZKT_ERR_HIP, "quotient kernel failed");
        if (!rc && hipMemcpy(out, d_out, bytes, hipMemcpyDeviceToHost) != hipSuccess) rc = set_err(c, ZKT_ERR_HIP, "copy back failed");
    }
    return rc;
}

// Row a13's two kernels alone (linearization_poly.rs:55-121): k <= 12 polynomials of the prover's lengths, each evaluated at its
// own point (poly_eval_many), and their linear combination sum_j scalars[j] polys[j] (poly_lincomb)
int zkt_debug_eval_lincomb(zkt_ctx* c, const uint64_t* const* polys, const size_t* lens, int k, const uint64_t* points,
                           const uint64_t* scalars, uint64_t* out_evals, uint64_t* out_lincomb, size_t out_len) {
    if (!c || !polys || !lens || !points || !scalars || !out_evals || !out_lincomb) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (int rc0 = circuit_entry(c, ENTRY_DEVICE | ENTRY_WITHDRAW)) return rc0;
    CircuitState& S = *c->circuit;
    const size_t cap = S.n + 8;
    if (k < 1 || k > 12 || out_len < 1 || out_len > cap) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "1 .. 12 polynomials, out_len <= n + 8");
    for (int j = 0; j < k; ++j)
        if (!polys[j] || lens[j] < 1 || lens[j] > cap) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "1 .. n + 8 coefficients each");
    EvalArgs ea{};
    LinCombArgs lc{};
    ea.count = k;
    lc.nterms = k;
    for (int j = 0; j < k; ++j) {
        ZKT_HIP(c, hipMemcpyAsync(S.poly[j], polys[j], lens[j] * 32, hipMemcpyHostToDevice, c->stream));
        ea.poly[j] = lc.poly[j] = S.poly[j];
        ea.len[j] = lc.len[j] = lens[j];
        memcpy(ea.point[j], points + 4 * j, 32);
        memcpy(lc.scalar[j], scalars + 4 * j, 32);
    }
    void* d_partials = (char*)S.small + 64 * 32;
    void* d_results = (char*)S.small + 32 * 32;
    int rc = poly_eval_many(c, ea, d_partials, d_results, S.eval_pw);
    if (rc) return rc;
    if ((rc = poly_lincomb(c, lc, S.sc[0], out_len))) return rc;
    ZKT_HIP(c, hipMemcpyAsync(out_evals, d_results, (size_t)k * 32, hipMemcpyDeviceToHost, c->stream));
    ZKT_HIP(c, hipMemcpyAsync(out_lincomb, S.sc[0], out_len * 32, hipMemcpyDeviceToHost, c->stream));
    ZKT_HIP(c, hipStreamSynchronize(c->stream));
    return ZKT_OK;
}

// kzg10::compute_witness_polynomial alone (row a12: the division of prove.rs:381-451's aggregated polynomial by X - z)
int zkt_debug_open_witness(zkt_ctx* c, const uint64_t* coeffs, size_t len, const uint64_t* z4, uint64_t* out) {
    if (!c || !coeffs || !z4 || !out) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (int rc0 = circuit_entry(c, ENTRY_DEVICE | ENTRY_WITHDRAW)) return rc0;
    CircuitState& S = *c->circuit;
    if (len < 2 || len > S.n + 8) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "2 .. n + 8 coefficients");
    uint32_t z[8], zi[8];
    memcpy(z, z4, 32);
    bool zero = true;
    for (int i = 0; i < 8; ++i) zero = zero && z[i] == 0;
    if (zero) return set_err(c, ZKT_ERR_ZERO_DENOMINATOR, "evaluation point is zero");
    by_curve(c->curve, [&](auto C) {
        using R = typename decltype(C)::Fr;
        memcpy(zi, fe_inv_host<R>(HostF<R>::from_words(z4)).v, 32);
    });
    ZKT_HIP(c, hipMemcpyAsync(S.sc[0], coeffs, len * 32, hipMemcpyHostToDevice, c->stream));
    int rc = open_witness(c, S.sc[0], len, z, zi, S.sc[1], S.sc[2], S.scan_tmp, S.sc[3], S.eval_pw);
    if (rc) return rc;
    ZKT_HIP(c, hipMemcpyAsync(out, S.sc[3], (len - 1) * 32, hipMemcpyDeviceToHost, c->stream));
    ZKT_HIP(c, hipStreamSynchronize(c->stream));
    return ZKT_OK;
}

}  // extern "C"
