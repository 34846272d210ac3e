// Device-side polynomial / evaluation-vector kernels of the prover rounds (launch wrappers).
// Each wrapper cites the reference code it replaces; implementations are in poly.hip.
#pragma once
#include "ctx.hpp"

namespace zkt {

constexpr int LC_MAX_TERMS = 24;   // round 5's first opening: r's 13 terms and 8 more
struct LinCombArgs {            // out[i] = sum_k scalar[k] * poly[k][i]  (poly k read as zero beyond len[k])
    const void* poly[LC_MAX_TERMS];
    uint64_t len[LC_MAX_TERMS];
    uint32_t scalar[LC_MAX_TERMS][8];  // Montgomery
    int nterms;
};

constexpr int EVAL_MAX = 16;
struct EvalArgs {               // result[k] = poly[k](point[k])
    const void* poly[EVAL_MAX];
    uint64_t len[EVAL_MAX];
    uint32_t point[EVAL_MAX][8];
    int count;
    uint8_t table[EVAL_MAX];    // poly_eval_open_tables: which of the two points (point[] is not read there)
};

struct QuotientArgs {           // all vectors hold 4n coset evaluations
    const void *a, *b, *c, *pi, *z1, *z2, *t, *h1, *h2;
    const void *q_m, *q_l, *q_r, *q_o, *q_c, *q_lookup, *q_table, *sigma1, *sigma2, *sigma3, *x, *l1;
    void* out;
    uint32_t alpha[8], beta[8], gamma[8], delta[8], epsilon[8];
    uint32_t zh_inv[4][8];      // 1 / (x^n - 1) on the coset: depends on i mod 4 only
    uint64_t n4;
    // Few public inputs: pi is not transformed at all.  PI(X) = sum_i v_i L_{pos_i}(X) and L_j(x) = L_0(x w^-j), so on
    // the 4n coset PI[k] = sum_i v_i * l1[(k - 4 pos_i) mod 4n].  pi_tab (device): n_pi_direct entries of 10 words,
    // {4 pos_i, nine 29-bit limbs of v_i (arkworks Montgomery form)}; `pi` is ignored when pi_tab is set.
    const uint32_t* pi_tab;
    uint32_t n_pi_direct;
    // Class form (one GPU's share of the 4n coset in a proof sharded over G GPUs, include/zkt_plonk.h): the vectors hold
    // the n4 = 4n / G points of global index cls + G i.  "omega-next" (global index + 4) of point i is entry
    // (i + next_off) mod n4 of the *_next vectors: the same vectors with next_off = 4 / G for G <= 4, the neighbouring
    // class (cls + 4) mod 8 with next_off = (cls + 4) / 8 for G = 8.  zh_inv is indexed by the global index mod 4; the
    // rotations in pi_tab are in class entries (4 pos / G).  G = 0 means the whole coset (G = 1, cls = 0, next_off = 4).
    uint32_t G, cls, next_off;
    const void *z1_next, *z2_next, *t_next, *h1_next;
    // only the points [first, first + count) of the vectors (count = 0: all n4); out[i] is written for those i
    uint64_t first, count;
    // ncls > 1: one launch for the classes cls, cls + 1, .. (the grid's y): class cls + y reads and writes every vector,
    // the *_next ones and `out` included, cls_stride elements further on per y (the classes route's [3][n] arrays)
    uint32_t ncls;
    uint64_t cls_stride;
};
constexpr int QUOTIENT_PI_DIRECT_MAX = 16;

struct ZTermsArgs {
    const void *a, *b, *c, *s1, *s2, *s3, *roots;  // z1
    const void *f, *t, *h1, *h2;                    // z2
    void *num, *den;
    uint32_t beta[8], gamma[8], delta[8], epsilon[8];
    uint64_t n;
};

// elementwise
int poly_mul_vec(zkt_ctx* c, const void* a, const void* b, void* out, size_t n);              // prove.rs:157-161
int poly_set_zero(zkt_ctx* c, void* p, size_t n_elems);
// from_coefficients_vec: *d_len (zero on entry) = number of coefficients after stripping trailing zeros of p[0..n);
// optionally clears zero_count elements at zero_at in the same launch (the slack above a transform's output)
int poly_trim_len(zkt_ctx* c, const void* p, size_t n, uint32_t* d_len, void* zero_at = nullptr, int zero_count = 0);
int poly_copy_pad(zkt_ctx* c, const void* d_in, size_t len, void* out, size_t n);   // prove.rs:39-55 pad_to
// prove.rs:49-55 wire_evals: out[i] = values[idx[i]] (0xFFFFFFFF = Variable::Zero), zero padded to n; d_status |= 16 on
// an index >= n_vars
int poly_gather_pad(zkt_ctx* c, const void* d_values, size_t n_vars, const uint32_t* d_idx, size_t rows, void* out, size_t n,
                    uint32_t* d_status);
int poly_add_blinders(zkt_ctx* c, void* p, const uint32_t* d_len, const void* d_blinders, int k, size_t cap);  // prove.rs:472-483
int poly_lincomb(zkt_ctx* c, const LinCombArgs& a, void* out, size_t n);
// k_trim_len (both launches) and k_add_blinders for up to NTT_MAX_BATCH polynomials of n coefficients in ONE launch, one
// workgroup each: clears zero_count coefficients at poly + n, writes the trimmed length to *d_len and places the k blinders;
// k < 0: only the clearing.
struct TrimBlindSpec {
    void* poly;
    const void* d_blinders;
    uint32_t* d_len;
    int k;
};
int poly_trim_blind(zkt_ctx* c, const TrimBlindSpec* jobs, int nb, size_t n, int zero_count);
// scalars (n + k of them) of a commitment taken against the Lagrange-prefix table (lagrange.hip) for the polynomial with
// evaluations ev[0..n) and, when k > 0, the k blinders of prove.rs:472-483 appended at its trimmed length *d_len
int lagrange_scalars(zkt_ctx* c, const void* ev, size_t n, const uint32_t* d_len, const void* d_blinders, int k, const void* d_roots,
                     void* out);
// d_powers: scratch of EVAL_MAX * (257 + ceil(maxlen / 2048)) elements (powers of each evaluation point)
int poly_eval_many(zkt_ctx* c, const EvalArgs& a, void* d_partials, void* d_results, void* d_powers);         // linearization_poly.rs:55-75
// The fused form for round 5: the polynomials (at most `len` coefficients) are evaluated at z0 (table[k] = 0) or z1 (1), and
// the powers come from the opening tables of both points, built here in ONE launch and left in d_powers for the openings:
// the tables of z0 at d_powers, those of z1 at d_powers + open_witness_powers(len) elements (layout of open_pow_tables).
int poly_eval_open_tables(zkt_ctx* c, const EvalArgs& a, const uint32_t z0[8], const uint32_t z0_inv[8], const uint32_t z1[8],
                          const uint32_t z1_inv[8], size_t len, void* d_partials, void* d_results, void* d_powers);
// grand products (permutation/mod.rs:181-254, lookup/mod.rs:94-151)
int z1_terms(zkt_ctx* c, const ZTermsArgs& a);
int z2_terms(zkt_ctx* c, const ZTermsArgs& a);
int scan_mul(zkt_ctx* c, const void* in, void* out, size_t n, bool reverse, void* d_tmp /* >= 2*(n/1024 + 2048) elems */);
int scan_add(zkt_ctx* c, const void* in, void* out, size_t n, bool reverse, void* d_tmp);
int z_combine(zkt_ctx* c, const void* pn, const void* sd, const uint32_t inv_total[8], void* out, size_t n);
// A grand product in its fused form (which = 1 permutation, 2 lookup; a.num / a.den are not used): one kernel forms the
// terms and scans them within blocks of 1024 into pn_local (forward) and sd_local (reversed), the block totals are scanned
// in d_tmp (grand_product_tmp_elems(n) elements), *d_total_den points at the product of all denominators (device).  After the
// host inverted it, grand_product_combine writes z from the local scans, the block prefixes in d_tmp and the inverse.
size_t grand_product_tmp_elems(size_t n);
int grand_product_scan(zkt_ctx* c, const ZTermsArgs& a, int which, void* pn_local, void* sd_local, void* d_tmp, const void** d_total_den,
                       bool totals_later = false);
// totals_later: the scans of the block totals are left out; grand_product_totals2 then makes those of two grand products
// (their d_tmp) in ONE launch, where each is a single block (grand_product_totals_fit(n))
bool grand_product_totals_fit(size_t n);
int grand_product_totals2(zkt_ctx* c, size_t n, void* d_tmp1, void* d_tmp2);
int grand_product_combine(zkt_ctx* c, const void* pn_local, const void* sd_local, const void* d_tmp, const uint32_t inv_total[8], void* out,
                          size_t n);
// quotient (quotient_poly.rs:98-224)
int quotient_pointwise(zkt_ctx* c, const QuotientArgs& a);
// in place: arkworks Montgomery form -> the quotient kernel's R' = 2^261 form times 32^k32 (k32 in {0, 1}).
// quotient_pointwise expects q_l q_r q_o q_lookup q_table l1 with k32 = 0 and q_m with k32 = 1.
int to_hat_form(zkt_ctx* c, void* v, size_t n, int k32);
// class-major (rank r's n4 / G points at [r * n4 / G, ...)) -> natural order of the 4n coset: out[cls + G i] = in[cls * (n4 / G) + i].
// chunks > 1: the exchange went out in pieces, `in` is [chunk][class][n4 / G / chunks]
int quotient_interleave(zkt_ctx* c, const void* in, void* out, size_t n4, uint32_t G, uint32_t chunks = 1);
// fused: the three trims and the blinders as one launch; closed: quotient_classes_close has made the chunks already
int quotient_split_blind(zkt_ctx* c, const void* q, size_t n, const void* d_b0b1, void* q_lo, void* q_mid, void* q_hi,
                         uint32_t* d_status, bool fused = false, bool closed = false);          // prove.rs:287-300
// The quotient on classes 0, 1, 2 of the 4n coset (prover.hip): [3][n] class arrays of a whole-coset table (4n elements);
// the windows [first, first + QC_WIN) of QC_WIN_POLYS polynomials gathered back to back for one copy to the host; and the
// way back from the three inverse class transforms (q: 4n elements, [3][n] on entry) to the 4n coefficients of t:
// vinv = the inverse of the Vandermonde matrix in gamma_0..2 (row-major), u = the six top coefficients of t, g3 = the
// first three powers of gamma_3 (host words, Montgomery form; quotient_classes.hpp makes them).
constexpr int QC_WIN = 14, QC_WIN_POLYS = 6;
int quotient_classes_of_coset(zkt_ctx* c, const void* in, void* out, size_t n);
int quotient_gather_windows(zkt_ctx* c, const void* const* polys, size_t first, void* out);
int quotient_classes_combine(zkt_ctx* c, void* q, size_t n, const uint32_t* vinv, const uint32_t* u, const uint32_t* g3);
// quotient_classes_combine and the split of quotient_split_blind in one pass: q as above, and the three chunks of n + 2
// coefficients into q_lo, q_mid, q_hi (n + 8 elements each, slack cleared).  [3n + 6, 4n) of q is zero by construction.
int quotient_classes_close(zkt_ctx* c, void* q, size_t n, const uint32_t* vinv, const uint32_t* u, const uint32_t* g3, void* q_lo,
                           void* q_mid, void* q_hi);
// KZG opening witness: w = p / (X - z)  (kzg10::compute_witness_polynomial)
int open_witness(zkt_ctx* c, const void* p, size_t len, const uint32_t z[8], const uint32_t z_inv[8], void* d_tmp_a, void* d_tmp_b,
                 void* d_scan_tmp, void* out, void* d_powers /* open_witness_powers(len) elements of scratch */);
size_t open_witness_powers(size_t maxlen);   // elements: the powers of z and 1/z the two scalings read
// open_witness in stages (kzg.hip runs a first stage of its own).  d_powers (open_witness_powers(len) elements) after
// open_pow_tables: z^0 .. z^256 | zinv^0 .. zinv^256 (OPEN_PW_ROW each), then z^(256 E b) and zinv^(256 E b) for
// b < open_blocks(len), E = open_elems(len).  open_divide: out[j] = zinv^(j+1) sum_{i > j} t_i (j < len - 1), zero at len - 1.
constexpr int OPEN_PW_ROW = 257;
int open_elems(size_t len);
size_t open_blocks(size_t len);
int open_pow_tables(zkt_ctx* c, const uint32_t z[8], const uint32_t z_inv[8], void* d_powers, size_t len);
// d_total (device, one element) given: the fused form -- the scan's block prefixes are added by the kernel that scales, and
// *d_total = sum_i t_i = p(z)
int open_divide(zkt_ctx* c, const void* t, size_t len, void* d_tmp, void* d_scan_tmp, void* out, const void* d_powers,
                void* d_total = nullptr);
// sum_k scalar[k] poly[k][i] times z^i in one pass (i < len; the tables of open_pow_tables for this len): the t of open_divide
int open_combine(zkt_ctx* c, const LinCombArgs& a, void* out, size_t len, const void* d_powers);
// out[r] = sum_b partials[r * nblk + b], r < rows (per-workgroup partial sums of rows evaluations)
int poly_sum_rows(zkt_ctx* c, const void* d_partials, int nblk, int rows, void* d_out);
// sigma.hip: compute_all_sigma_evals (permutation/mod.rs:103-177) from the wiring (device pointers, n_rows indices each) into
// d_sigma[3] of 2^log_n elements; scratch of its own, one synchronisation at the end (the index flag).  "sigma" scope.
int sigma_build(zkt_ctx* c, int log_n, const uint32_t* d_w_l, const uint32_t* d_w_r, const uint32_t* d_w_o, size_t n_rows, size_t n_vars,
                void* const* d_sigma);
// The launches of sigma_build alone, for a caller that brings the memory and waits itself (check.hip): d_scratch holds
// sigma_scratch_bytes(log_n, n_rows) bytes (256-byte aligned); *d_flag, cleared by the caller, is set when an index is
// outside the variable map.  Enqueues on the context's stream, no synchronisation.  Arguments are not checked here.
size_t sigma_scratch_bytes(int log_n, size_t n_rows);
int sigma_enqueue(zkt_ctx* c, int log_n, const uint32_t* d_w_l, const uint32_t* d_w_r, const uint32_t* d_w_o, size_t n_rows, size_t n_vars,
                  void* const* d_sigma, void* d_scratch, uint32_t* d_flag);
// check.hip: zkt_circuit_check_witness on the loaded circuit's keys (all device pointers of 2^log_n elements; pk = the
// coefficients of q_m q_l q_r q_o q_c, zero-padded to 2^log_n).  `in` and `flags` are validated by the caller except for what
// needs the data (table duplicates, indices).  *out is written only on ZKT_OK.
struct WitnessCheckKeys {
    int log_n;
    const void* pk[5];
    const void* q_lookup_ev;
    const void* sigma_ev[3];
};
// the evaluations of q_m q_l q_r q_o q_c over the domain: fft(n) of the key's coefficients pk[0..4] (zero-padded to n) into
// outs[0..4] (n elements each, device), four transforms in one launch per pass and one more.  Enqueues only.
int selector_evals_enqueue(zkt_ctx* c, int log_n, const void* const* pk, void* const* outs);
int witness_check(zkt_ctx* c, const WitnessCheckKeys& keys, const zkt_prove_inputs& in, int flags, zkt_witness_report* out);
// witness_plan.hip: zkt_witness_plan_create on the loaded circuit's selectors (pk as in WitnessCheckKeys).  Validates its
// arguments (rules: ZKT_WITNESS_RULE_* bits), synchronises, *out is written only on ZKT_OK.
struct WitnessPlanKeys {
    int log_n;
    const void* pk[5];
};
int witness_plan_create(zkt_ctx* c, const WitnessPlanKeys& keys, const uint32_t* w_l, const uint32_t* w_r, const uint32_t* w_o,
                        size_t n_rows, size_t n_vars, int wiring_on_device, const size_t* pi_pos, size_t n_pi, uint32_t rules,
                        zkt_witness_plan** out);
// check.hip: zkt_circuit_check_witness_batch on the loaded circuit's keys; `in` and `flags` validated by the caller except for
// what needs the data.  out[0 .. batch) is written only on ZKT_OK.
int witness_check_batch(zkt_ctx* c, const WitnessCheckKeys& keys, const zkt_witness_batch& in, int flags, zkt_witness_report* out);
// table generation
int gen_powers(zkt_ctx* c, void* out, size_t n, const uint32_t base[8], const uint32_t scale[8]);
// Plookup sorted halves h1/h2 (lookup/multiset.rs:103-146)
int lookup_count(zkt_ctx* c, const void* f, size_t n, const void* d_sorted_keys, const uint32_t* d_perm, uint32_t nkeys,
                 uint32_t* d_counts, uint32_t* d_status);
// start offsets of both halves of combine_split (multiset.rs:126-143) from the per-key counts base + hits; nkeys + 1
// entries each.  d_hits is cleared on the way.  d_status |= 8 when a half does not come out at n elements.
int lookup_starts(zkt_ctx* c, const uint32_t* d_base_counts, uint32_t* d_hits, uint32_t nkeys, size_t n, uint32_t* d_even,
                  uint32_t* d_odd, uint32_t* d_status);
int lookup_expand(zkt_ctx* c, const void* d_keys_insertion, const uint32_t* d_starts, uint32_t nkeys, void* out, size_t n);

}  // namespace zkt
