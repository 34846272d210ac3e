// The loaded circuit's device state (ProverKey polynomials, ExtendedProverKey cosets, the per-proof work set) and what the
// units that work on it share: circuit.hip (life cycle), circuit_keys.hip (the keys handed back), circuit_witness.hip
// (witness checks and plans), circuit_steps.hip (single steps over the work buffers) and prover.hip (the five rounds).
#pragma once
#include "ctx.hpp"
#include "ec.hpp"
#include "hostinv.hpp"
#include "poly.hpp"
#include "quotient_classes.hpp"
#include <cstring>

namespace zkt {

enum { PK_QM = 0, PK_QL, PK_QR, PK_QO, PK_QC, PK_S1, PK_S2, PK_S3, PK_QLOOKUP, PK_QTABLE, PK_COUNT };
// coset vectors kept on the device (keys/mod.rs:153-174; x and l_1 are stored, zh is 4 scalars)
enum { CS_QM = 0, CS_QL, CS_QR, CS_QO, CS_QC, CS_QLOOKUP, CS_QTABLE, CS_S1, CS_S2, CS_S3, CS_X, CS_L1, CS_COUNT };
enum { W_A = 0, W_B, W_C, W_PI, W_Z1, W_Z2, W_T, W_H1, W_H2, W_COUNT };  // witness cosets of quotient_poly.rs:52-96

// The keys (ProverKey polynomials, ExtendedProverKey cosets, sigma / q_lookup evaluations, domain roots): read-only for a
// prover, so a fork reads its source's (circuit_fork)
struct CircuitKeys {
    std::shared_ptr<DevShared> keys_mem;   // owns every array below
    void* pk[PK_COUNT] = {};
    size_t pk_len[PK_COUNT] = {};
    void* coset[CS_COUNT] = {};
    void* sigma_ev[3] = {};
    void* q_lookup_ev = nullptr;
    void* roots = nullptr;
    uint32_t zh_inv[4][8] = {};
};
// The tables of the quotient on classes 0, 1, 2 of the 4n coset (quotient_classes.hpp): ccoset[] are coset[] as [3][n]
// class arrays, key_win the windows of sigma1..3 and q_lookup.  Built on first use (ensure_class_tables), keys as well:
// contexts forked afterwards read them.
struct ClassTables {
    std::shared_ptr<DevShared> class_mem;   // owns ccoset[]
    void* ccoset[CS_COUNT] = {};
    bool ccoset_ready = false;
    uint32_t key_win[4][QCW][8] = {};
    uint32_t qc_gamma[4][8] = {}, qc_vinv[9][8] = {}, qc_g3[3][8] = {};
};

struct CircuitState : CircuitKeys, ClassTables {
    // owns everything circuit_alloc_work makes: the per-proof buffers, pinned staging, streams and events below
    DevSet work;
    explicit CircuitState(int device) : work(device) {}
    int log_n = 0;
    size_t n = 0;
    // A proof sharded over G GPUs (zkt_ctx_set_comm): this GPU owns the 4n-coset points of global index cls modulo G,
    // m = 4n / G of them; coset[] and wcos[] hold that class only.  G = 1: the whole coset, as the reference has it.
    int G = 1, cls = 0, log_m = 0;
    size_t m = 0;
    void* wnext[4] = {};       // G = 8: z1, z2, t, h1 on the class (cls + 4) mod 8, where "omega-next" lives
    void* fold = nullptr;      // m elements: a polynomial folded modulo X^m - shift^m before its class transform
    void* qgather = nullptr;   // 4n elements: every rank's quotient evaluations, class-major (the all-gather's target)
    bool have[16] = {};        // commitment slot -> this rank's SRS slice takes part (an MSM was started)
    // per-proof work buffers
    void* ev[8] = {};       // a, b, c, t, f, h1, h2, pi   (n each)
    void* sc[4] = {};       // scan scratch: num, den, PN, SD (n each)
    void* scan_tmp = nullptr;
    void* poly[13] = {};    // a b c t h1 h2 z1 z2 pi q_lo q_mid q_hi work   (n + 8 each)
    void* wcos[W_COUNT] = {};
    void* qev = nullptr;    // 4n
    // scalars of a commitment taken in the Lagrange basis (read by the MSM's level-1 kernels only): n + 16 each; one per
    // commitment that may wait in the queue of a round (t, h1, h2; z2), the last also stages zkt_commit_evals_dev's blinders
    void* lag_scalars = nullptr;
    void* lag_scalars_q[3] = {};
    void* small = nullptr;  // blinders (19), eval partials, eval results
    uint32_t* status = nullptr;  // [0] error bits, [1] len scratch ... [4..7] quotient lens, [8..] poly lens
    uint32_t* lk_u32 = nullptr;  // lookup: perm, base counts, starts of the even half, of the odd half, hit counts
    uint32_t lk_nkeys = 0;       // keys of the resident lookup tables (0 = none)
    std::vector<uint32_t> lk_host_keys, lk_host_sorted, lk_host_counts, lk_host_order;   // host staging (8 words per key)
    // zkt_prove_set_next: rounds 1 and 2 of the NEXT proof depend on no challenge; they are issued behind the last
    // commitments of the current proof, so the GPU never drains between two proofs
    // Round 1 of the next proof goes behind the quotient commitments of round 4, round 2 behind the opening commitments
    // of round 5.  Round 1 overwrites what round 5 of the current proof still reads (the wire polynomials) and both
    // use the status words, so those exist twice; `*_alt` is the set the early work writes.
    bool has_next = false, prefetch_same_table = false;
    int prefetch_stage = 0;        // 0 nothing, 1 round 1 issued, 2 rounds 1 and 2 issued (only then it is usable)
    uint64_t prefetch_epoch = 0;   // zkt_ctx::msm_epoch right after the early work was issued
    zkt_prove_inputs next_in{}, prefetch_in{};
    void* poly_alt[3] = {};
    uint32_t* status_alt = nullptr;
    void* lk_keys = nullptr;     // insertion-order keys then sorted keys
    size_t lk_cap = 0;
    void* pinned = nullptr;
    hipStream_t comm_stream = nullptr;   // sharded proof, asynchronous communicator: the quotient exchange's pieces travel here
    hipEvent_t ev_piece[ZKT_QUOTIENT_CHUNKS] = {}, ev_gathered = nullptr;
    // Round 5: the second opening's polynomial work (a linear combination and a division: memory-bound) runs on this stream
    // beside the first opening's commitment (integer-ALU bound), in buffers of its own
    hipStream_t aux_stream = nullptr;
    hipEvent_t ev_aux_go = nullptr, ev_aux_done = nullptr;
    void* aux_scan_tmp = nullptr;
    void* aux_pw = nullptr;
    hipStream_t copy_stream = nullptr;   // host witness uploads travel beside the main stream's work (cold path)
    hipEvent_t ev_copy[4] = {};          // a, b, c uploaded; [3]: main stream reached the upload point
    void* pinned_pi = nullptr;      // host staging of pi_tab
    uint32_t* pi_tab = nullptr;     // device: QUOTIENT_PI_DIRECT_MAX entries of {rotation, 9 limbs}
    void* eval_pw = nullptr;        // round 5: EVAL_MAX x 257 powers of the evaluation points, or (fused passes) the opening tables of xi and xi w
    // The table polynomial depends on the lookup table only: while consecutive proofs pass the same table its
    // evaluations, coefficients, 4n-coset and commitment are reused (one MSM and two transforms less).
    std::vector<uint64_t> cached_table;
    bool t_cached = false, t_coset_valid = false;
    uint64_t t_srs_generation = 0;   // zkt_ctx::srs_generation the cached commitment was made under
    uint64_t t_commit_xy[12] = {};
    // wire base tables (lagrange.hip): the wires of the round 1 last enqueued that were committed over them; their digest
    // and trimmed lengths are compared when that round is collected (collect_wires)
    bool wire_route[3] = {};
    bool wire_dense_only = false;   // zkt_debug_commit_wires_dev route 0
    int wire_elim_force = -1;       // zkt_debug_commit_wires_dev: 0 = per-variable tables only (route 1), 1 = over free variables (route 2)
    // The quotient on classes 0, 1, 2 of the 4n coset (single GPU, zkt_ctx_set_quotient_route; ClassTables above): wcos[]
    // then hold [3][n] as well.
    bool use_classes = false;       // the route of the proof in flight: layout of wcos[] and of the resident t coset
    void* heads = nullptr;          // 3 x NTT_MAX_BATCH x NTT_HEAD folded head coefficients of the batch being transformed
    void* d_win = nullptr;          // QC_WIN_POLYS windows (a b c z1 z2 t), gathered in round 3 ...
    void* pinned_win = nullptr;     // ... and copied here behind them
    hipEvent_t ev_win = nullptr;
    // zkt_withdraw_prove: the VerifierKey's commitments of this circuit under the SRS of generation vk_srs_generation, as every
    // transcript is seeded from them (kept by zkt_withdraw_setup, else made by the first zkt_withdraw_prove under this circuit),
    // and the table size zkt_withdraw_setup masked q_table for (0: unknown, the circuit was loaded another way)
    bool vk_cached = false;
    uint64_t vk_srs_generation = 0;
    uint64_t vk_commits[10 * 12] = {};
    int vk_inf[10] = {};
    size_t vk_table_size = 0;
    uint32_t last_u[6][8] = {};     // zkt_debug_quotient_top
    bool last_u_valid = false;
};

// ---- host field helpers ------------------------------------------------------------------------------
template <class P>
struct HostF {
    using F = Fe<P>;
    static F from_words(const uint64_t* w) {
        F r;
        memcpy(r.v, w, 32);
        return r;
    }
    static void to_le_bytes(const F& mont, uint8_t out[32]) {
        F c = fe_from_mont<P>(mont);
        memcpy(out, c.v, 32);
    }
    static F from_le_bytes(const uint8_t in[32]) {
        F c;
        memcpy(c.v, in, 32);
        return fe_to_mont<P>(c);
    }
};

template <class Q>
static void fq_to_le(const Fe<Q>& mont, uint8_t* out) {
    Fe<Q> c = fe_from_mont<Q>(mont);
    memcpy(out, c.v, Q::N * 4);
}

// The one curve dispatch: a generic lambda takes the tag and names its type (decltype(C), decltype(C)::Fr for the field alone)
template <class Fn>
static auto by_curve(int curve, Fn&& f) {
    return curve == ZKT_CURVE_BN254 ? f(Bn254Curve{}) : f(Bls381Curve{});
}

// What an entry needs before it touches the loaded circuit, refused in this order (the last two bits refuse nothing);
// `who` names the entry in the messages that carry its name
enum : unsigned {
    ENTRY_DOMAIN = 1u,        // the circuit is wanted for its domain: "no circuit loaded (the domain comes from it)"
    ENTRY_SRS = 2u,           // a committer key as well
    ENTRY_WHOLE_KEY = 4u,     // not on a sharded key
    ENTRY_WHOLE_COSET = 8u,   // not on a sharded context or circuit: the entry reads whole cosets and the whole key
    ENTRY_NO_NEXT = 16u,      // not while a next proof is announced (zkt_prove_set_next)
    ENTRY_DEVICE = 32u,       // the context's device becomes the thread's
    ENTRY_WITHDRAW = 64u,     // the work buffers are shared with an announced proof's early rounds: those are withdrawn
    // an entry that uses the per-proof work buffers (or the MSM's slots) between proofs
    ENTRY_WORK = ENTRY_WHOLE_COSET | ENTRY_NO_NEXT | ENTRY_DEVICE | ENTRY_WITHDRAW,
};
inline int circuit_entry(zkt_ctx* c, unsigned needs, const char* who = "") {
    if (!c->circuit)
        return set_err(c, ZKT_ERR_NOT_LOADED, needs & ENTRY_DOMAIN ? "no circuit loaded (the domain comes from it)" : "no circuit loaded (zkt_circuit_load)");
    if ((needs & ENTRY_SRS) && !c->msm) return set_err(c, ZKT_ERR_NOT_LOADED, "no SRS loaded (zkt_srs_load)");
    if ((needs & ENTRY_WHOLE_KEY) && c->sharded()) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "not available on a sharded key");
    if ((needs & ENTRY_WHOLE_COSET) && (c->sharded() || c->circuit->G != 1))
        return set_err(c, ZKT_ERR_INVALID_ARGUMENT, std::string(who) + ": a sharded context holds one class of every coset and a slice of the key; use an unsharded one");
    if ((needs & ENTRY_NO_NEXT) && c->circuit->has_next) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, std::string(who) + ": a next proof is announced");
    if (needs & ENTRY_DEVICE) (void)hipSetDevice(c->device);
    if (needs & ENTRY_WITHDRAW) c->circuit->prefetch_stage = 0;
    return ZKT_OK;
}

// ---- circuit.hip (circuit_release, circuit_fork, circuit_tables_have_readers: ctx.hpp) -------------------------------------
// keys/mod.rs:98-120 coset_fft of a key polynomial: the whole 4n coset, or this GPU's class of it (a sharded circuit)
int circuit_key_coset(zkt_ctx* c, CircuitState& S, const void* poly, size_t len, void* out);
// setup.rs:104-121: PC::commit of the ten polynomials of the loaded circuit, lens[k] coefficients each
int circuit_commit_keys(zkt_ctx* c, CircuitState& S, const size_t* lens, uint64_t* out_commitments, int* out_is_inf);
// the ten polynomials' lengths with trailing zeros stripped, taken on the device
int circuit_key_lens(zkt_ctx* c, const CircuitState& S, size_t* lens10);
// with a communicator attached: this rank holds exactly its zkt_shard_range of the key, the circuit is that communicator's
int check_sharded_key(zkt_ctx* c);

// ---- derived key values, made once for the load and for the keys handed back -----------------------------------------
// zh_coset takes four values: (g w4n^i)^n - 1 = g^n w4^(i mod 4) - 1 (keys/mod.rs:115-117); it never exists as a vector on
// the device, the load keeps the four inverses
template <class R>
static void circuit_zh4(int log_n, Fe<R> out[4]) {
    const size_t n = (size_t)1 << log_n;
    const Fe<R> one = fe_one<R>(), g = fe_from_u32<R>(R::GENERATOR), w4n = root_of_unity<R>(log_n + 2);
    const Fe<R> w4 = fe_pow_u64<R>(w4n, (uint64_t)n);
    Fe<R> cur = fe_pow_u64<R>(g, (uint64_t)n);
    for (int j = 0; j < 4; ++j) {
        out[j] = fe_sub<R>(cur, one);
        cur = fe_mul<R>(cur, w4);
    }
}
// l_1_coset = coset_fft(L_1), L_1 = ifft(1, 0, ..., 0) = (1/n, ..., 1/n) (keys/mod.rs:119-120): L_1 into S.ev[0], its
// coset into `out`, arkworks' Montgomery form
template <class R>
static int circuit_l1_coset(zkt_ctx* c, CircuitState& S, void* out) {
    const Fe<R> one = fe_one<R>(), ninv = fe_inv_host<R>(fe_from_u64<R>(S.n));
    if (int rc = gen_powers(c, S.ev[0], S.n, one.v, ninv.v)) return rc;
    return circuit_key_coset(c, S, S.ev[0], S.n, out);
}

// ---- the quotient kernel's arguments, for the prover's round 4 and zkt_debug_quotient ---------------------------------
// Public inputs the quotient kernel evaluates itself (poly.hpp): rows of {rotation, nine 29-bit limbs of the value}; the
// rotation 4 pos / G is in entries of a class of a coset split G ways (1: the whole coset)
template <class R>
static void pi_rows(const uint64_t* pi_pos, const uint64_t* pi_vals, size_t n_pi, size_t G, uint32_t* tab) {
    for (size_t i = 0; i < n_pi; ++i) {
        tab[10 * i] = (uint32_t)(4 * pi_pos[i] / G);
        const Fx<R> v = fx_unpack<R>(HostF<R>::from_words(pi_vals + 4 * i));
        for (int w = 0; w < 9; ++w) tab[10 * i + 1 + w] = v.l[w];
    }
}

// The quotient kernel's arguments (quotient_poly.rs:52-224).  _vectors: the twelve coset tables and the nine witness cosets,
// each `off` bytes into its vector (the classes route's [3][n] arrays); quotient_args: the whole-coset keys, the witness,
// the challenges (8 Montgomery words each) and zh_inv.  Output, size and public inputs are the caller's.
static void quotient_vectors(QuotientArgs& q, void* const cs[CS_COUNT], void* const w[W_COUNT], size_t off) {
    auto at = [&](void* const* v, int k) { return (const void*)((const char*)v[k] + off); };
    q.q_m = at(cs, CS_QM); q.q_l = at(cs, CS_QL); q.q_r = at(cs, CS_QR); q.q_o = at(cs, CS_QO); q.q_c = at(cs, CS_QC);
    q.q_lookup = at(cs, CS_QLOOKUP); q.q_table = at(cs, CS_QTABLE); q.x = at(cs, CS_X); q.l1 = at(cs, CS_L1);
    q.sigma1 = at(cs, CS_S1); q.sigma2 = at(cs, CS_S2); q.sigma3 = at(cs, CS_S3);
    q.a = at(w, W_A); q.b = at(w, W_B); q.c = at(w, W_C); q.pi = at(w, W_PI);
    q.z1 = at(w, W_Z1); q.z2 = at(w, W_Z2); q.t = at(w, W_T); q.h1 = at(w, W_H1); q.h2 = at(w, W_H2);
}
static QuotientArgs quotient_args(const CircuitState& S, void* const w[W_COUNT], const void* alpha, const void* beta,
                                  const void* gamma, const void* delta, const void* epsilon) {
    QuotientArgs q{};
    quotient_vectors(q, S.coset, w, 0);
    memcpy(q.alpha, alpha, 32); memcpy(q.beta, beta, 32); memcpy(q.gamma, gamma, 32);
    memcpy(q.delta, delta, 32); memcpy(q.epsilon, epsilon, 32);
    memcpy(q.zh_inv, S.zh_inv, sizeof(q.zh_inv));
    return q;
}

}  // namespace zkt
