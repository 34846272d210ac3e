// Batched Poseidon over the scalar field: the witness-side arithmetic of the reference's hash gadget (SURVEY.md 8f.3;
// plonk-hashing/src/hasher/poseidon/spec.rs:18-111 rounds, :267-316 round schedule, :239-265 input layout).  One thread
// per hash.  Two kernels:
//   k_poseidon_fx      the permutation (hash values, optionally every round's state): what NativePlonkSpecRef computes;
//   k_poseidon_gadget  the WITNESS of the in-circuit gadget PlonkSpecRef (spec.rs:174-219): every value the composer
//                      assigns while it synthesises one hash -- x^2, x^4, x^5 of each s-box (three mul_gates,
//                      spec.rs:107-111) and each of the W^2 running sums of product_mds (one add_gate per term,
//                      spec.rs:73-88) -- in the composer's allocation order, written into the variable map the prover
//                      gathers its wires from (zkt_prove_inputs.variables).
// Constants are the caller's (the reference generates them at run time, constants.rs:27, or parses the BN254 tables of
// gadgets/src/poseidon).
#include "ctx.hpp"
#include "merkle_tree.hpp"
#include <algorithm>
#include <vector>

#include <cstring>
#include <vector>

namespace zkt {

constexpr int POSEIDON_MAX_WIDTH = 8;

// ---- device-resident form ------------------------------------------------------------------------------------------
// Parameters are uploaded ONCE (zkt_poseidon_load) as 29-bit limbs in the kernels' own Montgomery radix R' = 2^261
// ("H" form, fx.hpp): a product of two H values is an H value, so the whole permutation runs on unpacked limbs with no
// conversion, and sum_i m[i][j] state[i] takes its products two at a time under one reduction (fx_mul2_inl).  Inputs are
// converted on load (one product each), the hash / the optional per-round states on store.
// Lazy bounds of k_poseidon_fx, valid for BOTH fields (R' / p is ~170 on BN254 but only ~71 on BLS12-381, so "state < 9p,
// 81 p^2 < R' p" would NOT do there).  Write rho = R' / p >= 64 (static_assert below).  A product returns a b / R' + p'
// with p' < p.  One operand of every MDS product is a canonical matrix entry (< p), the other a state word < S p, so a
// pair product is < (2 S / rho + 1) p; a state word is the sum of at most four of them plus a round constant:
// S <= 4 (2 S / rho + 1) + 1, i.e. S <= 5 / (1 - 8 / rho) <= 5.72.  The s-box squares a state word: S^2 p^2 <= 32.7 p^2 <
// rho p^2 = R' p, and its later products take operands < 2p and < S p.  fx_mul2's contract (a b + c d < R' p) needs
// 2 S p^2 < rho p^2: 11.5 < 64.
template <class P>
constexpr bool poseidon_lazy_bound_ok() {
    // R' = 2^(29 L) >= 64 p  <=>  p < 2^(29 L - 6): the modulus has at most 29 L - 6 bits
    return P::BITS <= 29 * FxP<P>::L - 6;
}

template <class P>
struct PoseidonFxArgs {
    const uint32_t* rc;    // (2 half_full + partial) * W entries of 9 limbs (H form)
    const uint32_t* mds;   // W * W entries of 9 limbs, m[i][j] at (i * W + j)
    uint32_t tag[FxP<P>::L];
    const Fe<P>* inputs;   // batch * arity, arkworks form, device
    Fe<P>* out;            // batch
    Fe<P>* states;         // optional: batch * (rounds + 1) * W
    uint64_t batch;
    int half_full, partial, arity;
};

template <class P>
ZKT_D Fx<P> fx_load_limbs(const uint32_t* p) {
    Fx<P> r;
#pragma unroll
    for (int i = 0; i < FxP<P>::L; ++i) r.l[i] = p[i];
    return r;
}

template <class P, int W>
__global__ __launch_bounds__(128) void k_poseidon_fx(PoseidonFxArgs<P> a) {
    static_assert(FxP<P>::L == 9, "scalar fields use nine limbs");
    static_assert(poseidon_lazy_bound_ok<P>(), "lazy reduction needs R' >= 64 p (state < 5.72 p, its square < R' p)");
    const uint64_t h = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= a.batch) return;
    Fx<P> st[W], nx[W];
    // spec.rs:243-265: element 0 = domain tag, the inputs follow, the rest is zero
#pragma unroll
    for (int i = 0; i < FxP<P>::L; ++i) st[0].l[i] = a.tag[i];
#pragma unroll
    for (int i = 1; i < W; ++i)
        st[i] = (i - 1 < a.arity) ? fx_from_ark<P>(fe_load<P>(a.inputs + h * a.arity + (i - 1))) : fx_zero<P>();
    const int rounds = 2 * a.half_full + a.partial;
    Fe<P>* trace = a.states ? a.states + h * (uint64_t)(rounds + 1) * W : nullptr;
    if (trace) {
#pragma unroll
        for (int i = 0; i < W; ++i) fe_store<P>(trace + i, fx_to_ark<P>(st[i]));
    }
    const uint32_t* rc = a.rc;
#pragma unroll 1
    for (int r = 0; r < rounds; ++r) {
        const bool full = r < a.half_full || r >= a.half_full + a.partial;   // spec.rs:267-316
        // spec.rs:18-37 / 39-71: add the round constants; (x)^5 on every element (full) or on element 0 (partial)
#pragma unroll
        for (int i = 0; i < W; ++i) st[i] = fx_add<P>(st[i], fx_load_limbs<P>(rc + 9 * i));
        rc += 9 * W;
        if (full) {
#pragma unroll
            for (int i = 0; i < W; ++i) {
                const Fx<P> x2 = fx_mul<P>(st[i], st[i]);
                st[i] = fx_mul<P>(fx_mul<P>(x2, x2), st[i]);
            }
        } else {
            const Fx<P> x2 = fx_mul<P>(st[0], st[0]);
            st[0] = fx_mul<P>(fx_mul<P>(x2, x2), st[0]);
        }
        // spec.rs:73-88: result[j] = sum_i m[i][j] * state[i], two products per reduction
#pragma unroll
        for (int j = 0; j < W; ++j) {
            Fx<P> acc;
            bool have = false;
#pragma unroll
            for (int i = 0; i + 1 < W; i += 2) {
                const Fx<P> t = fx_mul2_inl<P>(st[i], fx_load_limbs<P>(a.mds + 9 * (i * W + j)), st[i + 1],
                                               fx_load_limbs<P>(a.mds + 9 * ((i + 1) * W + j)));
                acc = have ? fx_add<P>(acc, t) : t;
                have = true;
            }
            if (W & 1) {
                const Fx<P> t = fx_mul<P>(st[W - 1], fx_load_limbs<P>(a.mds + 9 * ((W - 1) * W + j)));
                acc = have ? fx_add<P>(acc, t) : t;
            }
            nx[j] = acc;
        }
#pragma unroll
        for (int j = 0; j < W; ++j) st[j] = nx[j];
        if (trace) {
#pragma unroll
            for (int i = 0; i < W; ++i) fe_store<P>(trace + (uint64_t)(r + 1) * W + i, fx_to_ark<P>(st[i]));
        }
    }
    fe_store<P>(a.out + h, fx_to_ark<P>(st[1]));   // spec.rs:315: elements[1]
}

// ---- the gadget's witness -------------------------------------------------------------------------------------------
// Everything here stays in arkworks' own Montgomery form ("A": x R, R = 2^256), the form the variable map is stored in,
// so no value is converted on its way out: products against an MDS entry take the entry in H form (A x H -> A), and a
// product of two variables takes one of them shifted up by SH = 5 bits (A x 32 A / R' = A; the shift is two
// instructions per limb, a conversion would be a product).  Every variable is canonical when it is stored, hence
// < p when it is next used: p x 32 p < R' p on both fields.
template <class P>
struct PoseidonGadgetArgs {
    const uint32_t* rc_a;      // round constants as A-form limbs (canonical)
    const uint32_t* mds;       // H form, m[i][j] at (i * W + j)
    uint32_t tag_a[FxP<P>::L];
    const Fe<P>* inputs;       // batch * arity values, or null
    const uint32_t* input_vars;// batch * arity indices into vars, or null
    Fe<P>* vars;               // the variable map
    uint64_t n_vars;
    const uint32_t* trace_base;// per hash, or null: base0 + h * per_hash
    uint64_t base0;
    Fe<P>* out;                // optional: batch hash values
    uint32_t* status;          // set to 1 when a hash was skipped (an index outside the map)
    uint64_t batch;
    int half_full, partial, arity;
};

// value * 2^SH on normalised limbs of a canonical value (32 p < 2^(29 L)); result normalised
template <class P>
ZKT_D Fx<P> fx_shl_sh(const Fx<P>& a) {
    constexpr int L = FxP<P>::L, SH = FxP<P>::SH;
    Fx<P> r;
    r.l[0] = (a.l[0] << SH) & FxP<P>::MASK;
#pragma unroll
    for (int i = 1; i < L - 1; ++i) r.l[i] = ((a.l[i] << SH) | (a.l[i - 1] >> (29 - SH))) & FxP<P>::MASK;
    r.l[L - 1] = (a.l[L - 1] << SH) | (a.l[L - 2] >> (29 - SH));
    return r;
}

// a, b canonical A values -> a b as a canonical A value (mul_gate's assigned value, arithmetic.rs:95-99)
template <class P>
ZKT_D Fx<P> gadget_mul(const Fx<P>& a, const Fx<P>& b_shifted) {
    return fx_cond_sub_p<P>(fx_mul<P>(a, b_shifted));
}

// Stores.  A thread's variables are consecutive in memory, the 64 threads of a wavefront are vars_per_hash x 32 B apart:
// written directly, every store instruction touches 64 different cache lines with 16 bytes each, and the kernel is bound by
// the request rate of that (r04 first version: 1.5-1.7 TB/s of variables, half the issue rate of its own instruction stream).
// So a wavefront stages GADGET_STAGE variables per hash in LDS ([k][lane]: conflict-free writes) and flushes them so that
// 2 GADGET_STAGE consecutive lanes write one hash's GADGET_STAGE x 32 contiguous bytes (two full 128-byte lines at 8):
// 2.4 TB/s on x3 / x4 / x5 alike (4 gives 2.6 / 2.6 / 2.1; profiles/poseidon_r04_v2.txt).
constexpr int GADGET_STAGE = 8;

template <class P, int W>
__global__ __launch_bounds__(128) void k_poseidon_gadget(PoseidonGadgetArgs<P> a) {
    static_assert(FxP<P>::L == 9 && FxP<P>::SH == 5, "scalar fields: nine limbs, R' = 32 R");
    static_assert(P::BITS + FxP<P>::SH < 29 * FxP<P>::L, "p * 2^SH * p < R' p");
    static_assert(sizeof(Fe<P>) == 32, "a variable is two 16-byte words");
    constexpr int K = GADGET_STAGE;
    __shared__ uint4 stage[2][K * 64 * 2];       // per wavefront: [k][lane] x two 16-byte halves
    __shared__ uint64_t sbase[2][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t h = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool have = h < a.batch;
    const uint64_t hh = have ? h : 0;            // lanes without a hash run along (barriers below) and write nothing
    const int rounds = 2 * a.half_full + a.partial;
    const uint64_t per_hash = (uint64_t)2 * a.half_full * (3 * W + W * W) + (uint64_t)a.partial * (3 + W * W);
    const uint64_t base = a.trace_base ? (uint64_t)a.trace_base[hh] : a.base0 + hh * per_hash;
    bool ok = base <= a.n_vars && per_hash <= a.n_vars - base;
    Fx<P> st[W], nx[W];
    // reset + input (spec.rs:239-263): LTVariable::constant(domain_tag), the inputs, LTVariable::zero()
#pragma unroll
    for (int i = 0; i < FxP<P>::L; ++i) st[0].l[i] = a.tag_a[i];
#pragma unroll
    for (int i = 1; i < W; ++i) {
        st[i] = fx_zero<P>();
        if (i - 1 < a.arity) {
            if (a.input_vars) {
                const uint32_t v = a.input_vars[hh * a.arity + (i - 1)];
                if (v != ZKT_VARIABLE_ZERO) {
                    if (v < a.n_vars) st[i] = fx_unpack<P>(fe_load<P>(a.vars + v));
                    else ok = false;
                }
            } else {
                st[i] = fx_unpack<P>(fe_load<P>(a.inputs + hh * a.arity + (i - 1)));
            }
        }
    }
    const bool run = have && ok;
    if (have && !ok) atomicOr(a.status, 1u);
    sbase[wv][lane] = run ? base : ~(uint64_t)0;
    uint4* mystage = stage[wv];
    uint32_t cnt = 0;          // variables staged since the last flush (the same in every thread: the schedule is uniform)
    uint64_t pos = 0;          // variables flushed so far
    auto flush = [&](uint32_t k_count) {
        __syncthreads();
        // 16-byte chunk c of the wavefront's k_count x 64 variables: hash c / (2 k_count), then variable, then half
        const uint32_t per = 2u * k_count;
        for (uint32_t c = lane; c < 64u * per; c += 64u) {
            const uint32_t hsh = c / per, part = c - hsh * per, k = part >> 1, half = part & 1u;
            const uint64_t b = sbase[wv][hsh];
            if (b != ~(uint64_t)0)
                reinterpret_cast<uint4*>(a.vars + b + pos + k)[half] = mystage[(k * 64u + hsh) * 2u + half];
        }
        __syncthreads();
        pos += k_count;
        cnt = 0;
    };
    auto emit = [&](const Fx<P>& x) {
        const Fe<P> v = fx_pack<P>(x);
        mystage[(cnt * 64u + lane) * 2u] = make_uint4(v.v[0], v.v[1], v.v[2], v.v[3]);
        mystage[(cnt * 64u + lane) * 2u + 1u] = make_uint4(v.v[4], v.v[5], v.v[6], v.v[7]);
        if (++cnt == (uint32_t)K) flush(K);
    };
    const uint32_t* rc = a.rc_a;
#pragma unroll 1
    for (int r = 0; r < rounds; ++r) {
        const bool full = r < a.half_full || r >= a.half_full + a.partial;   // output_hash, spec.rs:267-316
        // add_constant (spec.rs:194-200) is a lazy LTVariable transform: no gate, no variable; its value enters the
        // gates that follow
#pragma unroll
        for (int i = 0; i < W; ++i) st[i] = fx_cond_sub_p<P>(fx_add<P>(st[i], fx_load_limbs<P>(rc + 9 * i)));
        rc += 9 * W;
        // power_of_5 (spec.rs:107-111): x^2 = mul(x, x), x^4 = mul(x^2, x^2), x^5 = mul(x^4, x): three variables
#pragma unroll
        for (int i = 0; i < W; ++i) {
            if (i == 0 || full) {
                const Fx<P> xs = fx_shl_sh<P>(st[i]);
                const Fx<P> x2 = gadget_mul<P>(st[i], xs);
                emit(x2);
                const Fx<P> x4 = gadget_mul<P>(x2, fx_shl_sh<P>(x2));
                emit(x4);
                st[i] = gadget_mul<P>(x4, xs);
                emit(st[i]);
            }
        }
        // product_mds (spec.rs:73-88): for j, for i: val = add_gate(val, mul_constant(state[i], m[i][j])): W^2 variables
#pragma unroll
        for (int j = 0; j < W; ++j) {
            Fx<P> acc = fx_zero<P>();
#pragma unroll
            for (int i = 0; i < W; ++i) {
                const Fx<P> t = fx_cond_sub_p<P>(fx_mul<P>(st[i], fx_load_limbs<P>(a.mds + 9 * (i * W + j))));
                acc = fx_cond_sub_p<P>(fx_add<P>(acc, t));
                emit(acc);
            }
            nx[j] = acc;
        }
#pragma unroll
        for (int j = 0; j < W; ++j) st[j] = nx[j];
    }
    if (cnt) flush(cnt);
    if (a.out && run) fe_store<P>(a.out + h, fx_pack<P>(st[1]));   // spec.rs:315: elements[1]
}


// ---- the same witness with W^2 lanes per hash (small batches) --------------------------------------------------------
// One thread per hash walks a dependency chain of 3W + W^2 (full) / 3 + W^2 (partial) products per round: a single
// proof's few hundred hashes (538 in the withdraw circuit at n = 2^20) then take as long as that chain, ~1.7 ms per launch,
// whatever the size of the chip.  Here a hash is spread over LPH >= W^2 lanes of one wavefront: lane (j, i) = j W + i
// holds element i of the state, every lane runs the s-box of its element (three dependent products, redundantly across
// j), multiplies by its own matrix entry m[i][j] (kept in registers for the whole permutation), and the W^2 running sums
// of product_mds are an inclusive scan over i inside each segment j (log2 W shuffle steps).  Depth per round: four products
// instead of 28 - 40, and a round's W^2 sums leave as consecutive 32-byte stores.  Throughput per hash is ~4 x worse than
// k_poseidon_gadget's (lanes idle or redundant in the s-box phase): the host picks this kernel for batches that cannot
// fill the chip with one thread per hash (POSEIDON_LANES_MAX_BATCH).
constexpr uint64_t POSEIDON_LANES_MAX_BATCH = 16384;

template <int W>
struct PoseidonLanes {
    static constexpr int LPH = W * W <= 4 ? 4 : W * W <= 16 ? 16 : W * W <= 32 ? 32 : 64;   // lanes per hash
    static constexpr int PER_WAVE = 64 / LPH;
};

template <class P>
ZKT_D Fx<P> fx_shfl(const Fx<P>& a, int src_lane) {
    Fx<P> r;
#pragma unroll
    for (int i = 0; i < FxP<P>::L; ++i) r.l[i] = (uint32_t)__shfl((int)a.l[i], src_lane);
    return r;
}

// The rounds of one permutation in that layout, shared by k_poseidon_gadget_lanes and k_poseidon_merkle_path.  Lane
// l = j W + i of the segment starting at lane seg0 enters with element i of the initial state in x and leaves with element
// i of the final one; m is its matrix entry m[i][j] (H form), rc points at ITS round constant of the first round
// (rc_a + 9 i).  With store set (the hash runs and the lane is live) the variables go to out[0 .. vars_per_hash) in
// allocation order.  Every lane of the wavefront must call it: the shuffles are wave-wide.
template <class P, int W>
ZKT_D Fx<P> poseidon_lanes_rounds(Fx<P> x, const Fx<P>& m, const uint32_t* rc, Fe<P>* out, bool store, int half_full, int partial,
                                  int lane, int seg0, int l, int i, int j) {
    const int rounds = 2 * half_full + partial;
#pragma unroll 1
    for (int r = 0; r < rounds; ++r) {
        const bool full = r < half_full || r >= half_full + partial;
        x = fx_cond_sub_p<P>(fx_add<P>(x, fx_load_limbs<P>(rc)));     // add_constant: no gate
        rc += 9 * W;
        // power_of_5 of my element; kept where the round has an s-box for it
        const Fx<P> xs = fx_shl_sh<P>(x);
        const Fx<P> x2 = gadget_mul<P>(x, xs);
        const Fx<P> x4 = gadget_mul<P>(x2, fx_shl_sh<P>(x2));
        const Fx<P> x5 = gadget_mul<P>(x4, xs);
        const bool boxed = full || i == 0;
        if (store && j == 0 && boxed) {
            Fe<P>* o = out + 3 * i;
            fe_store<P>(o, fx_pack<P>(x2));
            fe_store<P>(o + 1, fx_pack<P>(x4));
            fe_store<P>(o + 2, fx_pack<P>(x5));
        }
        out += full ? 3 * W : 3;
        Fx<P> s;
#pragma unroll
        for (int k = 0; k < FxP<P>::L; ++k) s.l[k] = boxed ? x5.l[k] : x.l[k];
        // product_mds: my term, then the running sums over i inside segment j (inclusive scan, log2 W steps)
        Fx<P> t = fx_cond_sub_p<P>(fx_mul<P>(s, m));
#pragma unroll
        for (int d = 1; d < W; d <<= 1) {
            const Fx<P> o = fx_shfl<P>(t, lane - d);      // lane - d >= 0 whenever it is used (i >= d)
            if (i >= d) t = fx_cond_sub_p<P>(fx_add<P>(t, o));
        }
        if (store) fe_store<P>(out + l, fx_pack<P>(t));
        out += W * W;
        // next state: element i = the last running sum of segment i
        x = fx_shfl<P>(t, seg0 + i * W + (W - 1));
    }
    return x;
}

template <class P, int W>
__global__ __launch_bounds__(256) void k_poseidon_gadget_lanes(PoseidonGadgetArgs<P> a) {
    static_assert(FxP<P>::L == 9 && FxP<P>::SH == 5, "scalar fields: nine limbs, R' = 32 R");
    constexpr int LPH = PoseidonLanes<W>::LPH, PER_WAVE = PoseidonLanes<W>::PER_WAVE;
    const int lane = threadIdx.x & 63;
    const int sub = lane / LPH;                 // which hash of this wavefront
    const int l = lane % LPH;                   // lane inside the hash
    const int seg0 = lane - l;                  // first lane of the hash
    const bool live = l < W * W;
    const int i = live ? l % W : 0, j = live ? l / W : 0;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t h = wave * PER_WAVE + sub;
    const bool have = h < a.batch;              // lanes without a hash run along (shuffles are wave-wide) and store nothing
    const uint64_t hh = have ? h : 0;
    const uint64_t per_hash = (uint64_t)2 * a.half_full * (3 * W + W * W) + (uint64_t)a.partial * (3 + W * W);
    const uint64_t base = a.trace_base ? (uint64_t)a.trace_base[hh] : a.base0 + hh * per_hash;
    bool ok = base <= a.n_vars && per_hash <= a.n_vars - base;
    // element i of the initial state (spec.rs:239-263)
    Fx<P> x = fx_zero<P>();
    if (i == 0) {
#pragma unroll
        for (int k = 0; k < FxP<P>::L; ++k) x.l[k] = a.tag_a[k];
    } else if (i - 1 < a.arity) {
        if (a.input_vars) {
            const uint32_t v = a.input_vars[hh * a.arity + (i - 1)];
            if (v != ZKT_VARIABLE_ZERO) {
                if (v < a.n_vars) x = fx_unpack<P>(fe_load<P>(a.vars + v));
                else ok = false;
            }
        } else {
            x = fx_unpack<P>(fe_load<P>(a.inputs + hh * a.arity + (i - 1)));
        }
    }
    // a hash is skipped as a whole: every lane of it must agree
    const unsigned long long bad = __ballot(have && live && !ok);
    const unsigned long long mine = (LPH == 64) ? ~0ull : (((1ull << LPH) - 1ull) << seg0);
    const bool run = have && (bad & mine) == 0;
    if (have && l == 0 && !run) atomicOr(a.status, 1u);
    const Fx<P> m = fx_load_limbs<P>(a.mds + 9 * (i * W + j));    // my matrix entry, H form, for every round
    x = poseidon_lanes_rounds<P, W>(x, m, a.rc_a + 9 * i, a.vars + base, run && live, a.half_full, a.partial, lane, seg0, l, i, j);
    if (a.out && run && l == 1 % W) {   // spec.rs:315: elements[1] (W >= 2: lane 1 holds element 1)
        fe_store<P>(a.out + h, fx_pack<P>(x));
    }
}

// ---- the Merkle-path gadget's witness ----------------------------------------------------------------------------------
// merkle_proof (plonk-hashing/src/merkle/binary.rs:8-30) is a CHAIN: level k hashes the two conditional_selects of the
// running hash of level k - 1 and the sibling.  One path per LPH lanes, in the layout above; the levels are walked inside
// the kernel and the running hash stays in registers (element 1 of the final state, broadcast to the segment), so the
// kernel never reads a variable it wrote.  Per level, in the proving composer's allocation order
// (constraint_system/mod.rs:339-354 for each select, binary.rs:23-24 for their order):
//     x_l = b s, y_l = (1 - b) cur, z_l = x_l + y_l,   x_r = b cur, y_r = (1 - b) s, z_r = x_r + y_r,
// then the vars_per_hash variables of hash_two(z_l, z_r) (hasher/mod.rs:26-33: arity 2, state [tag, z_l, z_r, 0 ...]).
// With b in {0, 1} the six are copies and zeros.  A path whose range, indices or bit values are not valid is skipped as a
// whole, before its first store, and raises the status word.
template <class P>
struct MerklePathArgs {
    const uint32_t* rc_a;      // round constants as A-form limbs (canonical)
    const uint32_t* mds;       // H form, m[i][j] at (i * W + j)
    uint32_t tag_a[FxP<P>::L];
    Fe<P>* vars;               // the variable map
    uint64_t n_vars;
    const uint32_t* leaf_var;  // batch
    const uint32_t* bit_vars;  // batch x height
    const uint32_t* sibling_vars;
    const uint32_t* path_base; // per path, or null: base0 + p * height * per_level
    uint64_t base0;
    Fe<P>* out;                // optional: batch roots
    uint32_t* status;
    uint64_t batch;
    int half_full, partial, height;
};

// a plain variable's value; Variable::Zero reads as 0.  The index was validated (or the path does not run).
template <class P>
ZKT_D Fe<P> merkle_read(const Fe<P>* vars, uint32_t v, bool run) {
    Fe<P> r;
#pragma unroll
    for (int k = 0; k < 8; ++k) r.v[k] = 0;
    if (run && v != ZKT_VARIABLE_ZERO) r = fe_load<P>(vars + v);
    return r;
}

template <class P>
ZKT_D bool fe_is_zero_words(const Fe<P>& a) {
    uint32_t acc = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) acc |= a.v[k];
    return acc == 0;
}

template <class P>
ZKT_D bool fe_is_one_words(const Fe<P>& a) {   // R mod p: the canonical 1 of the map's form
    uint32_t acc = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) acc |= a.v[k] ^ P::one(k);
    return acc == 0;
}

template <class P, int W>
__global__ __launch_bounds__(256) void k_poseidon_merkle_path(MerklePathArgs<P> a) {
    static_assert(FxP<P>::L == 9 && FxP<P>::SH == 5, "scalar fields: nine limbs, R' = 32 R");
    static_assert(W >= 3, "hash_two needs two input elements behind the tag");
    static_assert(sizeof(Fe<P>) == 32, "a variable is eight 32-bit words");
    constexpr int LPH = PoseidonLanes<W>::LPH, PER_WAVE = PoseidonLanes<W>::PER_WAVE;
    static_assert(LPH >= 6, "one lane per select variable");
    const int lane = threadIdx.x & 63;
    const int sub = lane / LPH;                 // which path of this wavefront
    const int l = lane % LPH;                   // lane inside the path
    const int seg0 = lane - l;
    const bool live = l < W * W;
    const int i = live ? l % W : 0, j = live ? l / W : 0;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t pth = wave * PER_WAVE + sub;
    const bool have = pth < a.batch;            // lanes without a path run along (shuffles are wave-wide) and store nothing
    const uint64_t pp = have ? pth : 0;
    const uint64_t per_hash = (uint64_t)2 * a.half_full * (3 * W + W * W) + (uint64_t)a.partial * (3 + W * W);
    const uint64_t per_level = 6 + per_hash, span = (uint64_t)a.height * per_level;
    const uint64_t base = a.path_base ? (uint64_t)a.path_base[pp] : a.base0 + pp * span;
    const uint32_t* bit_idx = a.bit_vars + pp * (uint64_t)a.height;
    const uint32_t* sib_idx = a.sibling_vars + pp * (uint64_t)a.height;
    const uint32_t leaf_idx = a.leaf_var[pp];
    // validation, all of it before the first store: the range, every index, every bit's value (the levels are dealt out
    // to the lanes of the segment)
    bool ok = base <= a.n_vars && span <= a.n_vars - base;
    ok = ok && (leaf_idx == ZKT_VARIABLE_ZERO || leaf_idx < a.n_vars);
    for (int k = l; k < a.height; k += LPH) {
        const uint32_t bv = bit_idx[k], sv = sib_idx[k];
        if (sv != ZKT_VARIABLE_ZERO && sv >= a.n_vars) ok = false;
        if (bv != ZKT_VARIABLE_ZERO) {
            if (bv >= a.n_vars) {
                ok = false;
            } else {
                const Fe<P> b = fe_load<P>(a.vars + bv);
                if (!fe_is_zero_words<P>(b) && !fe_is_one_words<P>(b)) ok = false;   // conditional_select asserts a bit
            }
        }
    }
    const unsigned long long bad = __ballot(have && !ok);
    const unsigned long long mine = (LPH == 64) ? ~0ull : (((1ull << LPH) - 1ull) << seg0);
    const bool run = have && (bad & mine) == 0;
    if (have && l == 0 && !run) atomicOr(a.status, 1u);
    const bool store = run && live;
    const Fx<P> m = fx_load_limbs<P>(a.mds + 9 * (i * W + j));
    Fx<P> tag;
#pragma unroll
    for (int k = 0; k < FxP<P>::L; ++k) tag.l[k] = a.tag_a[k];
    Fe<P> cur = merkle_read<P>(a.vars, leaf_idx, run);            // the running hash, the same in every lane of the path
    Fe<P>* out = a.vars + base;
    // the bit and the sibling of the level ahead are fetched while the level in hand runs its rounds
    Fe<P> sib = a.height > 0 ? merkle_read<P>(a.vars, sib_idx[0], run) : cur;
    bool bit = a.height > 0 && !fe_is_zero_words<P>(merkle_read<P>(a.vars, bit_idx[0], run));
#pragma unroll 1
    for (int k = 0; k < a.height; ++k) {
        const Fe<P> s = sib;
        const bool b = bit;
        if (k + 1 < a.height) {
            sib = merkle_read<P>(a.vars, sib_idx[k + 1], run);
            bit = !fe_is_zero_words<P>(merkle_read<P>(a.vars, bit_idx[k + 1], run));
        }
        // lanes 0 .. 5 hold x_l, y_l, z_l, x_r, y_r, z_r: each is s, cur or 0
        const bool left = l < 3;
        const int q = left ? l : l - 3;                       // 0: x = b * first, 1: y = (1 - b) * second, 2: z
        const bool first_is_s = left;                         // select(b, s, cur) on the left, select(b, cur, s) on the right
        const bool take_first = b ? q != 1 : false, take_second = b ? false : q != 0;
        const bool take_s = first_is_s ? take_first : take_second, take_cur = first_is_s ? take_second : take_first;
        Fe<P> sel, zl, zr;
#pragma unroll
        for (int w = 0; w < 8; ++w) {
            sel.v[w] = take_s ? s.v[w] : take_cur ? cur.v[w] : 0u;
            zl.v[w] = b ? s.v[w] : cur.v[w];
            zr.v[w] = b ? cur.v[w] : s.v[w];
        }
        if (run && l < 6) fe_store<P>(out + l, sel);
        // hash_two(z_l, z_r): state [tag, z_l, z_r, 0 ...]
        Fx<P> x = fx_zero<P>();
        if (i == 0) x = tag;
        else if (i == 1) x = fx_unpack<P>(zl);
        else if (i == 2) x = fx_unpack<P>(zr);
        x = poseidon_lanes_rounds<P, W>(x, m, a.rc_a + 9 * i, out + 6, store, a.half_full, a.partial, lane, seg0, l, i, j);
        cur = fx_pack<P>(fx_shfl<P>(x, seg0 + 1));            // elements[1] (spec.rs:315): lane 1 of the segment holds it
        out += per_level;
    }
    if (a.out && run && l == 0) fe_store<P>(a.out + pth, cur);
}

// ---- the note tree (gadgets/src/merkle_tree.rs:57-111) ------------------------------------------------------------------
// Layer L (0 <= L < height) is a dense array in HBM; the root (the "layer" above the last) has a slot of its own.  After
// add_leaf of leaves 0 .. n - 1 the stored node (L, idx), idx < ceil(n / 2^L), is hash_two of its children, the empty value
// nodes[L - 1] standing in for a right child that does not exist yet (pinned on the CPU by
// tests/test_merkle_tree_cases_oracle.py).  Appending m leaves at s therefore recomputes, per level L, the parents
// (s >> (L + 1)) .. ((s + m - 1) >> (L + 1)): level by level, one launch per WIDE level (k_merkle_level, one thread per
// parent) and ONE launch of one workgroup for all the narrow ones (k_merkle_tail, PoseidonLanes<W>::LPH lanes per parent).
// Native hashes, H form throughout: nothing of the gadget's per-step canonical variables is needed here.
constexpr int MERKLE_TAIL_THREADS = 256;
constexpr int MERKLE_TAIL_MAX_PARENTS = 512;    // a level the tail hashes stays in LDS for the next one: 16 + 8 KiB

template <class P>
struct MerkleHashConsts {
    const uint32_t* rc;        // H form
    const uint32_t* mds;       // H form, m[i][j] at (i * W + j)
    uint32_t tag[FxP<P>::L];   // H form
    int half_full, partial;
};

ZKT_D uint64_t merkle_shr(uint64_t x, int k) { return k >= 64 ? 0 : x >> k; }

template <class P>
struct MerkleLevelArgs {
    MerkleHashConsts<P> h;
    const Fe<P>* child;        // layer L
    Fe<P>* parent;             // layer L + 1, or the root slot (its only parent is 0)
    const Fe<P>* empty;        // nodes[L]
    uint64_t p_lo, n_parents;  // the parents p_lo .. p_lo + n_parents - 1
    uint64_t n_child;          // nodes of layer L after this append
};

// The permutation of k_poseidon_fx on a state held by one thread, without its optional trace: H-form limbs, the same lazy
// bounds (state < 5.72 p on entry to every round, see the top of this file).  Kernels that hash natively with one thread per
// hash call this; k_poseidon_fx keeps its own loop because it stores the round states in between.
template <class P, int W>
ZKT_D void poseidon_fx_rounds(Fx<P> (&st)[W], const uint32_t* rc, const uint32_t* mds, int half_full, int partial) {
    static_assert(FxP<P>::L == 9, "scalar fields use nine limbs");
    static_assert(poseidon_lazy_bound_ok<P>(), "lazy reduction needs R' >= 64 p (state < 5.72 p, its square < R' p)");
    Fx<P> nx[W];
    const int rounds = 2 * half_full + partial;
#pragma unroll 1
    for (int r = 0; r < rounds; ++r) {
        const bool full = r < half_full || r >= half_full + partial;   // spec.rs:267-316
#pragma unroll
        for (int i = 0; i < W; ++i) st[i] = fx_add<P>(st[i], fx_load_limbs<P>(rc + 9 * i));
        rc += 9 * W;
        if (full) {
#pragma unroll
            for (int i = 0; i < W; ++i) {
                const Fx<P> x2 = fx_mul<P>(st[i], st[i]);
                st[i] = fx_mul<P>(fx_mul<P>(x2, x2), st[i]);
            }
        } else {
            const Fx<P> x2 = fx_mul<P>(st[0], st[0]);
            st[0] = fx_mul<P>(fx_mul<P>(x2, x2), st[0]);
        }
        // spec.rs:73-88: result[j] = sum_i m[i][j] * state[i], two products per reduction
#pragma unroll
        for (int j = 0; j < W; ++j) {
            Fx<P> acc;
            bool have = false;
#pragma unroll
            for (int i = 0; i + 1 < W; i += 2) {
                const Fx<P> t = fx_mul2_inl<P>(st[i], fx_load_limbs<P>(mds + 9 * (i * W + j)), st[i + 1],
                                               fx_load_limbs<P>(mds + 9 * ((i + 1) * W + j)));
                acc = have ? fx_add<P>(acc, t) : t;
                have = true;
            }
            if (W & 1) {
                const Fx<P> t = fx_mul<P>(st[W - 1], fx_load_limbs<P>(mds + 9 * ((W - 1) * W + j)));
                acc = have ? fx_add<P>(acc, t) : t;
            }
            nx[j] = acc;
        }
#pragma unroll
        for (int j = 0; j < W; ++j) st[j] = nx[j];
    }
}

// One thread per parent: hash_two on state [tag, left, right, 0 ...].  The two children are one contiguous 64-byte pair; a
// right child past the end of the layer is the empty value.
template <class P, int W>
__global__ __launch_bounds__(128) void k_merkle_level(MerkleLevelArgs<P> a) {
    static_assert(W >= 3, "hash_two needs two input elements behind the tag");
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.n_parents) return;
    const uint64_t p = a.p_lo + t;
    Fx<P> st[W];
#pragma unroll
    for (int i = 0; i < FxP<P>::L; ++i) st[0].l[i] = a.h.tag[i];
    st[1] = fx_from_ark<P>(fe_load<P>(a.child + 2 * p));
    st[2] = fx_from_ark<P>(fe_load<P>(2 * p + 1 < a.n_child ? a.child + 2 * p + 1 : a.empty));
#pragma unroll
    for (int i = 3; i < W; ++i) st[i] = fx_zero<P>();
    poseidon_fx_rounds<P, W>(st, a.h.rc, a.h.mds, a.h.half_full, a.h.partial);
    fe_store<P>(a.parent + p, fx_to_ark<P>(st[1]));   // spec.rs:315: elements[1]
}

// hash_two(left, right) spread over the LPH lanes of a segment (the layout of poseidon_lanes_rounds), natively: H-form
// limbs, no variable leaves, so the only canonical values are the terms of the matrix product (a sum of up to eight of
// them would otherwise reach 10 p, and (10 p)^2 > R' p on BLS12-381).  Bounds: a term is cond_sub(product) < p, the running
// sums stay < p, the state entering a round is < 2p (first round < 3p: from_ark gives < 2p), plus its constant < 3p (< 4p);
// the s-box squares that: 16 p^2 < 64 p^2 <= R' p; its later products take operands < 2p and < 4p.  Every lane of the
// wavefront must call it.  Returns the hash (canonical, arkworks form) in EVERY lane of the segment.
template <class P, int W>
ZKT_D Fe<P> merkle_hash_two_lanes(const MerkleHashConsts<P>& h, const Fx<P>& m, const Fe<P>& left, const Fe<P>& right, int lane,
                                  int seg0, int i) {
    Fx<P> x = fx_from_ark<P>(i == 1 ? left : right);
    if (i == 0) {
#pragma unroll
        for (int k = 0; k < FxP<P>::L; ++k) x.l[k] = h.tag[k];
    } else if (i > 2) {
        x = fx_zero<P>();
    }
    const uint32_t* rc = h.rc + 9 * i;
    const int rounds = 2 * h.half_full + h.partial;
#pragma unroll 1
    for (int r = 0; r < rounds; ++r) {
        const bool full = r < h.half_full || r >= h.half_full + h.partial;
        x = fx_add<P>(x, fx_load_limbs<P>(rc));
        rc += 9 * W;
        const Fx<P> x2 = fx_mul<P>(x, x);
        const Fx<P> x5 = fx_mul<P>(fx_mul<P>(x2, x2), x);
        const bool boxed = full || i == 0;
        Fx<P> s;
#pragma unroll
        for (int k = 0; k < FxP<P>::L; ++k) s.l[k] = boxed ? x5.l[k] : x.l[k];
        Fx<P> t = fx_cond_sub_p<P>(fx_mul<P>(s, m));
#pragma unroll
        for (int d = 1; d < W; d <<= 1) {
            const Fx<P> o = fx_shfl<P>(t, lane - d);      // lane - d >= 0 whenever it is used (i >= d)
            if (i >= d) t = fx_cond_sub_p<P>(fx_add<P>(t, o));
        }
        x = fx_shfl<P>(t, seg0 + i * W + (W - 1));
    }
    return fx_to_ark<P>(fx_shfl<P>(x, seg0 + 1));          // elements[1] (spec.rs:315)
}

template <class P>
struct MerkleTailArgs {
    MerkleHashConsts<P> h;
    Fe<P>* const* layers;      // height device pointers
    Fe<P>* root;
    const Fe<P>* empties;      // nodes[0 .. height)
    uint64_t s, m;             // the append: leaves s .. s + m - 1 (m >= 1)
    int level0, height;        // levels level0 .. height - 1; at most MERKLE_TAIL_MAX_PARENTS parents at level0
};

// All the narrow levels of one append in one workgroup.  Per level the parents are dealt out to the workgroup's
// 4 PER_WAVE lane groups, round after round when there are more.  A parent goes to its layer in HBM and to LDS, where
// the next level finds it after the barrier: the kernel never reads from HBM a node it wrote.  What it does read from
// there: both children at level0 (an earlier launch wrote them), the left neighbour of the first new child (an earlier
// append), the empty values.
template <class P, int W>
__global__ __launch_bounds__(MERKLE_TAIL_THREADS) void k_merkle_tail(MerkleTailArgs<P> a) {
    static_assert(FxP<P>::L == 9 && poseidon_lazy_bound_ok<P>(), "scalar fields: nine limbs, R' >= 64 p");
    static_assert(W >= 3, "hash_two needs two input elements behind the tag");
    constexpr int LPH = PoseidonLanes<W>::LPH, PER_WAVE = PoseidonLanes<W>::PER_WAVE;
    constexpr int GROUPS = MERKLE_TAIL_THREADS / 64 * PER_WAVE;
    __shared__ Fe<P> lds_a[MERKLE_TAIL_MAX_PARENTS], lds_b[MERKLE_TAIL_MAX_PARENTS / 2 + 1];
    const int lane = threadIdx.x & 63;
    const int l = lane % LPH, seg0 = lane - l;
    const int group = (threadIdx.x >> 6) * PER_WAVE + lane / LPH;
    const bool live = l < W * W;
    const int i = live ? l % W : 0, j = live ? l / W : 0;
    const Fx<P> m = fx_load_limbs<P>(a.h.mds + 9 * (i * W + j));
    const Fe<P>* cur = nullptr;      // the nodes lo_c .. hi_c of layer L made by this launch (L > level0)
    Fe<P>* nxt = lds_a;
    const uint64_t last = a.s + (a.m - 1);
#pragma unroll 1
    for (int L = a.level0; L < a.height; ++L) {
        const uint64_t lo_c = merkle_shr(a.s, L), hi_c = merkle_shr(last, L);
        const uint64_t p_lo = lo_c >> 1, n_parents = (hi_c >> 1) - p_lo + 1;
        const Fe<P>* child = a.layers[L];
        Fe<P>* parent = L + 1 < a.height ? a.layers[L + 1] : a.root;
        const Fe<P>* empty = a.empties + L;
#pragma unroll 1
        for (uint64_t base = 0; base < n_parents; base += GROUPS) {
            const bool have = base + group < n_parents;   // groups without a parent run along (the shuffles are wave-wide)
            const uint64_t p = p_lo + (have ? base + group : 0);
            const uint64_t cl = 2 * p, cr = 2 * p + 1;
            const Fe<P> left = (cur && cl >= lo_c) ? cur[cl - lo_c] : fe_load<P>(child + cl);
            const Fe<P> right = cr > hi_c ? fe_load<P>(empty) : cur ? cur[cr - lo_c] : fe_load<P>(child + cr);
            const Fe<P> hsh = merkle_hash_two_lanes<P, W>(a.h, m, left, right, lane, seg0, i);
            if (have && l == 0) {
                fe_store<P>(parent + p, hsh);
                nxt[p - p_lo] = hsh;
            }
        }
        __syncthreads();
        cur = nxt;
        nxt = nxt == lds_a ? lds_b : lds_a;
    }
}

// The empty-subtree values at create time (merkle_tree.rs:57-67): nodes[0] = 0, nodes[L + 1] = hash_two(nodes[L], nodes[L]).
// One wavefront, the chain in the registers of its first lane group (the other groups run along).
template <class P, int W>
__global__ __launch_bounds__(64) void k_merkle_empty(MerkleHashConsts<P> h, Fe<P>* empties, int height) {
    constexpr int LPH = PoseidonLanes<W>::LPH;
    const int lane = threadIdx.x & 63;
    const int l = lane % LPH, seg0 = lane - l;
    const bool live = l < W * W;
    const int i = live ? l % W : 0, j = live ? l / W : 0;
    const Fx<P> m = fx_load_limbs<P>(h.mds + 9 * (i * W + j));
    Fe<P> cur;
#pragma unroll
    for (int k = 0; k < 8; ++k) cur.v[k] = 0;
#pragma unroll 1
    for (int L = 0; L < height; ++L) {
        if (lane == 0) fe_store<P>(empties + L, cur);
        if (L + 1 < height) cur = merkle_hash_two_lanes<P, W>(h, m, cur, cur, lane, seg0, i);
    }
}

template <class P>
struct MerklePathsArgs {
    const Fe<P>* const* layers;
    const Fe<P>* empties;
    const uint64_t* index;     // k leaf indices
    const uint32_t* sib0;      // per path, or null: p * height
    const uint32_t* bit0;      // per path, or null: no bits
    Fe<P>* dst;                // the variable map, or k x height siblings
    uint64_t count, total;     // leaves in the tree; k * height threads
    int height;
};

// merkle_path (merkle_tree.rs:77-87): one thread per (path, layer) moves one 32-byte element -- the stored sibling, or
// nodes[layer] when the tree has none there -- and, optionally, writes the position bit as the Montgomery 0 or 1.
template <class P>
__global__ __launch_bounds__(256) void k_merkle_paths(MerklePathsArgs<P> a) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.total) return;
    const uint64_t p = t / (uint64_t)a.height;
    const int layer = (int)(t - p * (uint64_t)a.height);
    const uint64_t idx = a.index[p] >> layer;                       // layer < height <= 64
    const uint64_t sib = idx ^ 1;
    const uint64_t n_layer = a.count ? ((a.count - 1) >> layer) + 1 : 0;
    const Fe<P> v = fe_load<P>(sib < n_layer ? a.layers[layer] + sib : a.empties + layer);
    fe_store<P>(a.dst + (a.sib0 ? (uint64_t)a.sib0[p] : p * (uint64_t)a.height) + layer, v);
    if (a.bit0) {
        Fe<P> b;
#pragma unroll
        for (int k = 0; k < 8; ++k) b.v[k] = (idx & 1) ? P::one(k) : 0u;
        fe_store<P>(a.dst + (uint64_t)a.bit0[p] + layer, b);
    }
}

}  // namespace zkt

// the opaque handle of include/zkt_plonk.h: PoseidonConstants resident in HBM
struct zkt_poseidon {
    int curve = 0, width = 0, half_full = 0, partial = 0;
    void* d_rc = nullptr;    // limbs, H form
    void* d_mds = nullptr;
    void* d_rc_a = nullptr;  // limbs, arkworks form (the gadget kernel's)
    void* d_status = nullptr;// one word: a gadget launch skipped a hash (index outside the variable map)
    uint32_t tag[16] = {};
    uint32_t tag_a[16] = {};
};

namespace zkt {

template <class P>
static void to_h_limbs(const uint64_t* src_mont, size_t count, std::vector<uint32_t>& out) {
    out.resize(count * 9);
    for (size_t k = 0; k < count; ++k) {
        Fe<P> v;
        memcpy(v.v, src_mont + 4 * k, 32);
        const Fx<P> x = fx_cond_sub_p<P>(fx_from_ark<P>(v));   // canonical H form
        for (int i = 0; i < 9; ++i) out[9 * k + i] = x.l[i];
    }
}

// arkworks-form words -> canonical A-form limbs (no conversion: the same residue x R, unpacked)
template <class P>
static int to_a_limbs(const uint64_t* src_mont, size_t count, std::vector<uint32_t>& out) {
    out.resize(count * 9);
    for (size_t k = 0; k < count; ++k) {
        Fe<P> v;
        memcpy(v.v, src_mont + 4 * k, 32);
        const Fx<P> x = fx_unpack<P>(v);
        const Fx<P> cx = fx_cond_sub_p<P>(x);
        for (int i = 0; i < 9; ++i) {
            if (cx.l[i] != x.l[i]) return 1;   // not below the modulus
            out[9 * k + i] = x.l[i];
        }
    }
    return 0;
}

template <class P>
static int poseidon_load_t(zkt_ctx* c, const zkt_poseidon_params& p, zkt_poseidon* h) {
    const int W = p.width, rounds = 2 * p.half_full_rounds + p.partial_rounds;
    std::vector<uint32_t> rc, mds, tag, rc_a, tag_a;
    to_h_limbs<P>(p.round_constants, (size_t)rounds * W, rc);
    to_h_limbs<P>(p.mds, (size_t)W * W, mds);
    to_h_limbs<P>(p.domain_tag, 1, tag);
    if (to_a_limbs<P>(p.round_constants, (size_t)rounds * W, rc_a) || to_a_limbs<P>(p.domain_tag, 1, tag_a))
        return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "poseidon: a constant is not below the field modulus");
    for (int i = 0; i < 9; ++i) h->tag[i] = tag[i];
    for (int i = 0; i < 9; ++i) h->tag_a[i] = tag_a[i];
    int rcode;
    if ((rcode = dev_alloc(c, &h->d_rc, rc.size() * 4))) return rcode;
    if ((rcode = dev_alloc(c, &h->d_mds, mds.size() * 4))) return rcode;
    if ((rcode = dev_alloc(c, &h->d_rc_a, rc_a.size() * 4))) return rcode;
    if ((rcode = dev_alloc(c, &h->d_status, 4))) return rcode;
    ZKT_HIP(c, hipMemsetAsync(h->d_status, 0, 4, c->stream));
    ZKT_HIP(c, hipMemcpyAsync(h->d_rc, rc.data(), rc.size() * 4, hipMemcpyHostToDevice, c->stream));
    ZKT_HIP(c, hipMemcpyAsync(h->d_mds, mds.data(), mds.size() * 4, hipMemcpyHostToDevice, c->stream));
    ZKT_HIP(c, hipMemcpyAsync(h->d_rc_a, rc_a.data(), rc_a.size() * 4, hipMemcpyHostToDevice, c->stream));
    ZKT_HIP(c, hipStreamSynchronize(c->stream));   // the staging vectors die with this call
    return ZKT_OK;
}

template <class P, int W>
static void poseidon_launch_w(zkt_ctx* c, const PoseidonFxArgs<P>& a) {
    hipLaunchKernelGGL((k_poseidon_fx<P, W>), dim3((unsigned)((a.batch + 127) / 128)), dim3(128), 0, c->stream, a);
}

template <class P>
static int poseidon_enqueue_t(zkt_ctx* c, const zkt_poseidon* h, const void* d_inputs, size_t batch, int arity, void* d_out,
                              void* d_states) {
    PoseidonFxArgs<P> a{};
    a.rc = (const uint32_t*)h->d_rc;
    a.mds = (const uint32_t*)h->d_mds;
    for (int i = 0; i < 9; ++i) a.tag[i] = h->tag[i];
    a.inputs = (const Fe<P>*)d_inputs;
    a.out = (Fe<P>*)d_out;
    a.states = (Fe<P>*)d_states;
    a.batch = batch;
    a.half_full = h->half_full;
    a.partial = h->partial;
    a.arity = arity;
    switch (h->width) {
        case 2: poseidon_launch_w<P, 2>(c, a); break;
        case 3: poseidon_launch_w<P, 3>(c, a); break;
        case 4: poseidon_launch_w<P, 4>(c, a); break;
        case 5: poseidon_launch_w<P, 5>(c, a); break;
        case 6: poseidon_launch_w<P, 6>(c, a); break;
        case 7: poseidon_launch_w<P, 7>(c, a); break;
        default: poseidon_launch_w<P, 8>(c, a); break;
    }
    ZKT_HIP(c, hipGetLastError());
    return ZKT_OK;
}

template <class P, int W>
static void poseidon_gadget_launch_w(zkt_ctx* c, const PoseidonGadgetArgs<P>& a, int mode) {
    const bool lanes = mode == 2 || (mode == 0 && a.batch <= POSEIDON_LANES_MAX_BATCH);
    if (lanes) {
        constexpr uint64_t per_block = 4 * PoseidonLanes<W>::PER_WAVE;    // 256 threads = 4 wavefronts
        hipLaunchKernelGGL((k_poseidon_gadget_lanes<P, W>), dim3((unsigned)((a.batch + per_block - 1) / per_block)), dim3(256), 0,
                           c->stream, a);
    } else {
        hipLaunchKernelGGL((k_poseidon_gadget<P, W>), dim3((unsigned)((a.batch + 127) / 128)), dim3(128), 0, c->stream, a);
    }
}

template <class P>
static int poseidon_gadget_enqueue_t(zkt_ctx* c, const zkt_poseidon* h, const zkt_poseidon_gadget_args& g) {
    PoseidonGadgetArgs<P> a{};
    a.rc_a = (const uint32_t*)h->d_rc_a;
    a.mds = (const uint32_t*)h->d_mds;
    for (int i = 0; i < 9; ++i) a.tag_a[i] = h->tag_a[i];
    a.inputs = (const Fe<P>*)g.d_inputs;
    a.input_vars = g.d_input_vars;
    a.vars = (Fe<P>*)g.d_variables;
    a.n_vars = g.n_vars;
    a.trace_base = g.d_trace_base;
    a.base0 = g.trace_base0;
    a.out = (Fe<P>*)g.d_out_hashes;
    a.status = (uint32_t*)h->d_status;
    a.batch = g.batch;
    a.half_full = h->half_full;
    a.partial = h->partial;
    a.arity = g.arity;
    const int mode = g.kernel;   // 0: by batch size; 1: one thread per hash; 2: W^2 lanes per hash
    switch (h->width) {
        case 2: poseidon_gadget_launch_w<P, 2>(c, a, mode); break;
        case 3: poseidon_gadget_launch_w<P, 3>(c, a, mode); break;
        case 4: poseidon_gadget_launch_w<P, 4>(c, a, mode); break;
        case 5: poseidon_gadget_launch_w<P, 5>(c, a, mode); break;
        case 6: poseidon_gadget_launch_w<P, 6>(c, a, mode); break;
        case 7: poseidon_gadget_launch_w<P, 7>(c, a, mode); break;
        default: poseidon_gadget_launch_w<P, 8>(c, a, mode); break;
    }
    ZKT_HIP(c, hipGetLastError());
    return ZKT_OK;
}

template <class P, int W>
static void merkle_path_launch_w(zkt_ctx* c, const MerklePathArgs<P>& a) {
    if constexpr (W >= 3) {
        constexpr uint64_t per_block = 4 * PoseidonLanes<W>::PER_WAVE;    // 256 threads = 4 wavefronts
        hipLaunchKernelGGL((k_poseidon_merkle_path<P, W>), dim3((unsigned)((a.batch + per_block - 1) / per_block)), dim3(256), 0,
                           c->stream, a);
    }
}

template <class P>
static int merkle_path_enqueue_t(zkt_ctx* c, const zkt_poseidon* h, const zkt_merkle_path_args& g) {
    MerklePathArgs<P> a{};
    a.rc_a = (const uint32_t*)h->d_rc_a;
    a.mds = (const uint32_t*)h->d_mds;
    for (int i = 0; i < 9; ++i) a.tag_a[i] = h->tag_a[i];
    a.vars = (Fe<P>*)g.d_variables;
    a.n_vars = g.n_vars;
    a.leaf_var = g.d_leaf_var;
    a.bit_vars = g.d_bit_vars;
    a.sibling_vars = g.d_sibling_vars;
    a.path_base = g.d_path_base;
    a.base0 = g.path_base0;
    a.out = (Fe<P>*)g.d_out_roots;
    a.status = (uint32_t*)h->d_status;
    a.batch = g.batch;
    a.half_full = h->half_full;
    a.partial = h->partial;
    a.height = g.height;
    switch (h->width) {
        case 3: merkle_path_launch_w<P, 3>(c, a); break;
        case 4: merkle_path_launch_w<P, 4>(c, a); break;
        case 5: merkle_path_launch_w<P, 5>(c, a); break;
        case 6: merkle_path_launch_w<P, 6>(c, a); break;
        case 7: merkle_path_launch_w<P, 7>(c, a); break;
        default: merkle_path_launch_w<P, 8>(c, a); break;
    }
    ZKT_HIP(c, hipGetLastError());
    return ZKT_OK;
}

// the argument rules zkt_poseidon_merkle_path_witness_dev and _validate share; *enqueue = 0 when there is nothing to do
static int merkle_path_check_args(zkt_ctx* c, const zkt_poseidon* h, const zkt_merkle_path_args* g, bool* enqueue) {
    *enqueue = false;
    if (!c || !h || !g) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (h->curve != c->curve) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "poseidon parameters belong to another curve");
    if (h->width < 3)
        return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "merkle path: hash_two needs width >= 3 (spec.rs:253-257 FullBuffer)");
    if (g->height < 0) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "merkle path: height >= 0");
    if (g->batch == 0 || g->height == 0) return ZKT_OK;
    if (!g->d_variables) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null variable map");
    if (!g->d_leaf_var || !g->d_bit_vars || !g->d_sibling_vars)
        return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "merkle path: null leaf, bit or sibling index vector");
    if (g->n_vars > 0xFFFFFFFFull) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "variable indices are 32 bits wide");
    *enqueue = true;
    return ZKT_OK;
}

}  // namespace zkt

// the handle of the note tree (zkt_merkle_tree): merkle_tree.hpp

namespace zkt {

// Levels with at least this many parents get a launch of their own (one thread per parent: a permutation's full serial
// latency, whatever the count); narrower ones share the tail's single workgroup (a W-th of that latency per 4 PER_WAVE
// parents).  64 is the minimum of the sweep 2 .. 512 on an MI355X at x5, m = 2^10 and 2^16 (32 within 1 %, 128 4 - 5 % worse):
// docs/EXPERIMENTS.md, "note tree on the device".  Other widths were not swept.
constexpr int MERKLE_WIDE_MIN_PARENTS = 64;

static uint64_t merkle_shr_h(uint64_t x, int k) { return k >= 64 ? 0 : x >> k; }

template <class P>
static MerkleHashConsts<P> merkle_consts(const zkt_poseidon* h) {
    MerkleHashConsts<P> k{};
    k.rc = (const uint32_t*)h->d_rc;
    k.mds = (const uint32_t*)h->d_mds;
    for (int i = 0; i < 9; ++i) k.tag[i] = h->tag[i];
    k.half_full = h->half_full;
    k.partial = h->partial;
    return k;
}

template <class P>
static Fe<P>* merkle_layer(const zkt_merkle_tree* t, int L) {
    size_t off = 0;
    for (int k = 0; k < L; ++k) off += t->layer_len[k];
    return (Fe<P>*)t->d_nodes + off;
}

template <class P, int W>
static void merkle_launch_w(zkt_ctx* c, const MerkleLevelArgs<P>* lv, const MerkleTailArgs<P>* tail, const MerkleHashConsts<P>* empty,
                            Fe<P>* empties, int height) {
    if constexpr (W >= 3) {
        if (lv)
            hipLaunchKernelGGL((k_merkle_level<P, W>), dim3((unsigned)((lv->n_parents + 127) / 128)), dim3(128), 0, c->stream, *lv);
        if (tail) hipLaunchKernelGGL((k_merkle_tail<P, W>), dim3(1), dim3(MERKLE_TAIL_THREADS), 0, c->stream, *tail);
        if (empty) hipLaunchKernelGGL((k_merkle_empty<P, W>), dim3(1), dim3(64), 0, c->stream, *empty, empties, height);
    }
}

template <class P>
static void merkle_launch(zkt_ctx* c, int width, const MerkleLevelArgs<P>* lv, const MerkleTailArgs<P>* tail,
                          const MerkleHashConsts<P>* empty = nullptr, Fe<P>* empties = nullptr, int height = 0) {
    switch (width) {
        case 3: merkle_launch_w<P, 3>(c, lv, tail, empty, empties, height); break;
        case 4: merkle_launch_w<P, 4>(c, lv, tail, empty, empties, height); break;
        case 5: merkle_launch_w<P, 5>(c, lv, tail, empty, empties, height); break;
        case 6: merkle_launch_w<P, 6>(c, lv, tail, empty, empties, height); break;
        case 7: merkle_launch_w<P, 7>(c, lv, tail, empty, empties, height); break;
        default: merkle_launch_w<P, 8>(c, lv, tail, empty, empties, height); break;
    }
}

// the launches of one append after the leaves are in layer 0: leaves s .. s + m - 1, m >= 1
template <class P>
static int merkle_append_levels_t(zkt_ctx* c, zkt_merkle_tree* t, uint64_t s, uint64_t m) {
    const uint64_t last = s + (m - 1);
    const uint64_t thr = t->wide_min_parents ? (uint64_t)t->wide_min_parents : (uint64_t)MERKLE_WIDE_MIN_PARENTS;
    const MerkleHashConsts<P> k = merkle_consts<P>(t->pos);
    int L = 0;
    for (; L < t->height; ++L) {
        const uint64_t p_lo = merkle_shr_h(s, L + 1), n_parents = merkle_shr_h(last, L + 1) - p_lo + 1;
        // the tail keeps a level in LDS: a level it cannot hold is a launch of its own whatever the threshold says
        if (n_parents < thr && n_parents <= (uint64_t)MERKLE_TAIL_MAX_PARENTS) break;
        MerkleLevelArgs<P> a{};
        a.h = k;
        a.child = merkle_layer<P>(t, L);
        a.parent = L + 1 < t->height ? merkle_layer<P>(t, L + 1) : (Fe<P>*)t->d_root;
        a.empty = (const Fe<P>*)t->d_empties + L;
        a.p_lo = p_lo;
        a.n_parents = n_parents;
        a.n_child = merkle_shr_h(last, L) + 1;
        merkle_launch<P>(c, t->pos->width, &a, nullptr);
    }
    if (L < t->height) {
        MerkleTailArgs<P> a{};
        a.h = k;
        a.layers = (Fe<P>* const*)t->d_layers;
        a.root = (Fe<P>*)t->d_root;
        a.empties = (const Fe<P>*)t->d_empties;
        a.s = s;
        a.m = m;
        a.level0 = L;
        a.height = t->height;
        merkle_launch<P>(c, t->pos->width, nullptr, &a);
    }
    ZKT_HIP(c, hipGetLastError());
    return ZKT_OK;
}

template <class P>
static int merkle_create_t(zkt_ctx* c, zkt_merkle_tree* t) {
    std::vector<Fe<P>*> ptrs(t->height);
    for (int L = 0; L < t->height; ++L) ptrs[L] = merkle_layer<P>(t, L);
    ZKT_HIP(c, hipMemcpyAsync(t->d_layers, ptrs.data(), ptrs.size() * sizeof(void*), hipMemcpyHostToDevice, c->stream));
    ZKT_HIP(c, hipMemsetAsync(t->d_root, 0, 32, c->stream));
    const MerkleHashConsts<P> k = merkle_consts<P>(t->pos);
    merkle_launch<P>(c, t->pos->width, nullptr, nullptr, &k, (Fe<P>*)t->d_empties, t->height);
    ZKT_HIP(c, hipGetLastError());
    ZKT_HIP(c, hipStreamSynchronize(c->stream));   // the pointer table dies with this call
    return ZKT_OK;
}

template <class P>
static int merkle_paths_enqueue_t(zkt_ctx* c, zkt_merkle_tree* t, size_t k, bool scattered, bool bits, void* dst) {
    MerklePathsArgs<P> a{};
    a.layers = (const Fe<P>* const*)t->d_layers;
    a.empties = (const Fe<P>*)t->d_empties;
    a.index = (const uint64_t*)t->d_table;
    a.sib0 = scattered ? (const uint32_t*)((const char*)t->d_table + 8 * k) : nullptr;
    a.bit0 = bits ? (const uint32_t*)((const char*)t->d_table + 12 * k) : nullptr;
    a.dst = (Fe<P>*)dst;
    a.count = t->count;
    a.total = (uint64_t)k * (uint64_t)t->height;
    a.height = t->height;
    hipLaunchKernelGGL((k_merkle_paths<P>), dim3((unsigned)((a.total + 255) / 256)), dim3(256), 0, c->stream, a);
    ZKT_HIP(c, hipGetLastError());
    return ZKT_OK;
}

static int merkle_check(zkt_ctx* c, const zkt_merkle_tree* t) {
    if (!c || !t) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (t->curve != c->curve) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "merkle tree: the tree belongs to another curve");
    return ZKT_OK;
}

// the index table of one paths call goes up from the tree's pinned buffer; a table still on its way (the previous call's) is
// waited for first -- the only wait of the enqueue-only entry, and only when two calls follow each other that closely
static int merkle_table_upload(zkt_ctx* c, zkt_merkle_tree* t, const uint64_t* indices, size_t k, const uint32_t* sib0,
                               const uint32_t* bit0) {
    if (t->table_busy) {
        ZKT_HIP(c, hipEventSynchronize(t->table_up));
        t->table_busy = false;
    }
    char* h = (char*)t->h_table;
    memcpy(h, indices, 8 * k);
    if (sib0) memcpy(h + 8 * k, sib0, 4 * k);
    if (bit0) memcpy(h + 12 * k, bit0, 4 * k);
    ZKT_HIP(c, hipMemcpyAsync(t->d_table, h, 16 * k, hipMemcpyHostToDevice, c->stream));
    ZKT_HIP(c, hipEventRecord(t->table_up, c->stream));
    t->table_busy = true;
    return ZKT_OK;
}

static int merkle_check_indices(zkt_ctx* c, const zkt_merkle_tree* t, const uint64_t* indices, size_t k) {
    if (k > ZKT_MERKLE_TREE_PATHS_MAX) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "merkle tree: at most ZKT_MERKLE_TREE_PATHS_MAX paths a call");
    if (k && !indices) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (t->height < 64)
        for (size_t i = 0; i < k; ++i)
            if (indices[i] >> t->height) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "merkle tree: a leaf index is not below 2^height");
    return ZKT_OK;
}

static int poseidon_check_params(zkt_ctx* c, const zkt_poseidon_params* p) {
    if (!p || !p->round_constants || !p->mds || !p->domain_tag) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    // output_hash (spec.rs:267-316) always runs one full and one partial round before its `1..n` loops: a schedule with
    // no partial round does not exist in the reference
    if (p->width < 2 || p->width > POSEIDON_MAX_WIDTH || p->half_full_rounds < 1 || p->partial_rounds < 1)
        return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "poseidon: width in [2, 8], half_full_rounds >= 1, partial_rounds >= 1");
    return ZKT_OK;
}

}  // namespace zkt

using namespace zkt;

extern "C" {

int zkt_poseidon_load(zkt_ctx* c, const zkt_poseidon_params* p, zkt_poseidon** out) {
    if (!c || !out) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (int rc = poseidon_check_params(c, p)) return rc;
    (void)hipSetDevice(c->device);
    zkt_poseidon* h = new zkt_poseidon();
    h->curve = c->curve;
    h->width = p->width;
    h->half_full = p->half_full_rounds;
    h->partial = p->partial_rounds;
    const int rc = c->curve == ZKT_CURVE_BN254 ? poseidon_load_t<Bn254Fr>(c, *p, h) : poseidon_load_t<Bls381Fr>(c, *p, h);
    if (rc) {
        dev_free(c, h->d_rc);
        dev_free(c, h->d_mds);
        dev_free(c, h->d_rc_a);
        dev_free(c, h->d_status);
        delete h;
        return rc;
    }
    *out = h;
    return ZKT_OK;
}

void zkt_poseidon_free(zkt_ctx* c, zkt_poseidon* h) {
    if (!h) return;
    if (c) {
        (void)hipStreamSynchronize(c->stream);
        dev_free(c, h->d_rc);
        dev_free(c, h->d_mds);
        dev_free(c, h->d_rc_a);
        dev_free(c, h->d_status);
    }
    delete h;
}

int zkt_poseidon_hash_batch_dev(zkt_ctx* c, const zkt_poseidon* h, const void* d_inputs, size_t batch, int arity,
                                void* d_out_hashes, void* d_out_states) {
    if (!c || !h || !d_out_hashes || (!d_inputs && batch && arity)) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (h->curve != c->curve) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "poseidon parameters belong to another curve");
    if (arity < 0 || arity > h->width - 1)
        return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "poseidon: arity <= width - 1 (spec.rs:253-257 FullBuffer)");
    if (batch == 0) return ZKT_OK;
    (void)hipSetDevice(c->device);
    if (c->curve == ZKT_CURVE_BN254) return poseidon_enqueue_t<Bn254Fr>(c, h, d_inputs, batch, arity, d_out_hashes, d_out_states);
    return poseidon_enqueue_t<Bls381Fr>(c, h, d_inputs, batch, arity, d_out_hashes, d_out_states);
}

size_t zkt_poseidon_gadget_vars_per_hash(const zkt_poseidon* h) {
    if (!h) return 0;
    const size_t W = (size_t)h->width;
    return (size_t)2 * h->half_full * (3 * W + W * W) + (size_t)h->partial * (3 + W * W);
}

int zkt_poseidon_gadget_witness_dev(zkt_ctx* c, const zkt_poseidon* h, const zkt_poseidon_gadget_args* g) {
    if (!c || !h || !g) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (h->curve != c->curve) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "poseidon parameters belong to another curve");
    if (g->arity < 0 || g->arity > h->width - 1)
        return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "poseidon: arity <= width - 1 (spec.rs:253-257 FullBuffer)");
    if (g->batch == 0) return ZKT_OK;
    if (!g->d_variables) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null variable map");
    if (g->arity && !g->d_inputs == !g->d_input_vars)
        return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "poseidon gadget: exactly one of d_inputs / d_input_vars");
    if (g->n_vars > 0xFFFFFFFFull) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "variable indices are 32 bits wide");
    if (g->kernel < 0 || g->kernel > 2) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "poseidon gadget: kernel = 0 (auto), 1 or 2");
    const size_t per = zkt_poseidon_gadget_vars_per_hash(h);
    if (!g->d_trace_base && (g->trace_base0 > g->n_vars || g->batch > (g->n_vars - g->trace_base0) / per))
        return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "poseidon gadget: the traces do not fit the variable map");
    (void)hipSetDevice(c->device);
    if (c->curve == ZKT_CURVE_BN254) return poseidon_gadget_enqueue_t<Bn254Fr>(c, h, *g);
    return poseidon_gadget_enqueue_t<Bls381Fr>(c, h, *g);
}

// Debug validation of one launch's structure (host side; synchronises): the traces [base, base + vars_per_hash) must be
// pairwise disjoint and inside the map, and no input index may lie inside a trace of the SAME launch (the kernel's hashes
// are independent: such an input would be read before, while or after it is written).  A caller that schedules its own
// launches (the Python mirror does it in PoseidonGadget.levels) runs this once per circuit, not per proof.
int zkt_poseidon_gadget_validate(zkt_ctx* c, const zkt_poseidon* h, const zkt_poseidon_gadget_args* g) {
    if (!c || !h || !g) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (g->arity < 0 || g->arity > h->width - 1)
        return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "poseidon: arity <= width - 1 (spec.rs:253-257 FullBuffer)");
    if (g->batch == 0) return ZKT_OK;
    (void)hipSetDevice(c->device);
    const size_t per = zkt_poseidon_gadget_vars_per_hash(h);
    std::vector<uint64_t> base(g->batch);
    if (g->d_trace_base) {
        std::vector<uint32_t> b32(g->batch);
        ZKT_HIP(c, hipMemcpyAsync(b32.data(), g->d_trace_base, g->batch * 4, hipMemcpyDeviceToHost, c->stream));
        ZKT_HIP(c, hipStreamSynchronize(c->stream));
        for (size_t i = 0; i < g->batch; ++i) base[i] = b32[i];
    } else {
        for (size_t i = 0; i < g->batch; ++i) base[i] = g->trace_base0 + i * per;
    }
    std::vector<uint64_t> sorted(base);
    std::sort(sorted.begin(), sorted.end());
    for (size_t i = 0; i < sorted.size(); ++i) {
        if (sorted[i] > g->n_vars || per > g->n_vars - sorted[i])
            return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "poseidon gadget: a trace lies outside the variable map");
        if (i && sorted[i] < sorted[i - 1] + per)
            return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "poseidon gadget: two traces of one launch overlap");
    }
    if (g->arity && g->d_input_vars) {
        std::vector<uint32_t> idx(g->batch * (size_t)g->arity);
        ZKT_HIP(c, hipMemcpyAsync(idx.data(), g->d_input_vars, idx.size() * 4, hipMemcpyDeviceToHost, c->stream));
        ZKT_HIP(c, hipStreamSynchronize(c->stream));
        for (uint32_t v : idx) {
            if (v == 0xFFFFFFFFu) continue;   // Variable::Zero
            if (v >= g->n_vars) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "poseidon gadget: an input index lies outside the variable map");
            auto it = std::upper_bound(sorted.begin(), sorted.end(), (uint64_t)v);
            if (it != sorted.begin() && (uint64_t)v < *(it - 1) + per)
                return set_err(c, ZKT_ERR_INVALID_ARGUMENT,
                               "poseidon gadget: an input is a variable the same launch writes (run it in a later launch)");
        }
    }
    return ZKT_OK;
}

size_t zkt_merkle_path_vars_per_level(const zkt_poseidon* h) {
    return h ? 6 + zkt_poseidon_gadget_vars_per_hash(h) : 0;
}

int zkt_poseidon_merkle_path_witness_dev(zkt_ctx* c, const zkt_poseidon* h, const zkt_merkle_path_args* g) {
    bool enqueue;
    if (int rc = merkle_path_check_args(c, h, g, &enqueue)) return rc;
    if (!enqueue) return ZKT_OK;
    const size_t span = (size_t)g->height * zkt_merkle_path_vars_per_level(h);
    if (!g->d_path_base && (g->path_base0 > g->n_vars || g->batch > (g->n_vars - g->path_base0) / span))
        return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "merkle path: the paths do not fit the variable map");
    (void)hipSetDevice(c->device);
    if (c->curve == ZKT_CURVE_BN254) return merkle_path_enqueue_t<Bn254Fr>(c, h, *g);
    return merkle_path_enqueue_t<Bls381Fr>(c, h, *g);
}

// Host-side validation of one launch's structure (downloads the index vectors; synchronises): the ranges
// [base, base + height * vars_per_level) must be pairwise disjoint and inside the map, and no leaf, bit or sibling index may
// lie inside a range of the SAME launch (the kernel reads its inputs while other paths are being written).
int zkt_poseidon_merkle_path_validate(zkt_ctx* c, const zkt_poseidon* h, const zkt_merkle_path_args* g) {
    bool enqueue;
    if (int rc = merkle_path_check_args(c, h, g, &enqueue)) return rc;
    if (!enqueue) return ZKT_OK;
    (void)hipSetDevice(c->device);
    const size_t span = (size_t)g->height * zkt_merkle_path_vars_per_level(h), levels = g->batch * (size_t)g->height;
    std::vector<uint64_t> base(g->batch);
    std::vector<uint32_t> leaf(g->batch), bits(levels), sibs(levels);
    if (g->d_path_base) {
        std::vector<uint32_t> b32(g->batch);
        ZKT_HIP(c, hipMemcpyAsync(b32.data(), g->d_path_base, g->batch * 4, hipMemcpyDeviceToHost, c->stream));
        ZKT_HIP(c, hipStreamSynchronize(c->stream));
        for (size_t i = 0; i < g->batch; ++i) base[i] = b32[i];
    } else {
        for (size_t i = 0; i < g->batch; ++i) base[i] = g->path_base0 + i * span;
    }
    ZKT_HIP(c, hipMemcpyAsync(leaf.data(), g->d_leaf_var, g->batch * 4, hipMemcpyDeviceToHost, c->stream));
    ZKT_HIP(c, hipMemcpyAsync(bits.data(), g->d_bit_vars, levels * 4, hipMemcpyDeviceToHost, c->stream));
    ZKT_HIP(c, hipMemcpyAsync(sibs.data(), g->d_sibling_vars, levels * 4, hipMemcpyDeviceToHost, c->stream));
    ZKT_HIP(c, hipStreamSynchronize(c->stream));
    std::sort(base.begin(), base.end());
    for (size_t i = 0; i < base.size(); ++i) {
        if (base[i] > g->n_vars || span > g->n_vars - base[i])
            return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "merkle path: a path's range lies outside the variable map");
        if (i && base[i] < base[i - 1] + span)
            return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "merkle path: two paths' ranges of one launch overlap");
    }
    for (const std::vector<uint32_t>* idx : {&leaf, &bits, &sibs}) {
        for (uint32_t v : *idx) {
            if (v == 0xFFFFFFFFu) continue;   // Variable::Zero
            if (v >= g->n_vars) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "merkle path: an input index lies outside the variable map");
            auto it = std::upper_bound(base.begin(), base.end(), (uint64_t)v);
            if (it != base.begin() && (uint64_t)v < *(it - 1) + span)
                return set_err(c, ZKT_ERR_INVALID_ARGUMENT,
                               "merkle path: an input is a variable the same launch writes (run it in a later launch)");
        }
    }
    return ZKT_OK;
}

int zkt_poseidon_gadget_check(zkt_ctx* c, const zkt_poseidon* h) {
    if (!c || !h) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    (void)hipSetDevice(c->device);
    uint32_t st = 0;
    ZKT_HIP(c, hipMemcpyAsync(&st, h->d_status, 4, hipMemcpyDeviceToHost, c->stream));
    ZKT_HIP(c, hipStreamSynchronize(c->stream));
    if (st) {
        ZKT_HIP(c, hipMemsetAsync(h->d_status, 0, 4, c->stream));
        return set_err(c, ZKT_ERR_INVALID_ARGUMENT,
                       "poseidon gadget: a trace base or an input index lies outside the variable map, or a path's bit is not 0 or 1");
    }
    return ZKT_OK;
}

// host-pointer convenience form: load, stage, run, download; the staging goes with `tmp`
int zkt_poseidon_hash_batch(zkt_ctx* c, const zkt_poseidon_params* p, const uint64_t* inputs, size_t batch, int arity,
                            uint64_t* out_hashes, uint64_t* out_states) {
    if (!c || !out_hashes || (!inputs && batch && arity)) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (int rc0 = poseidon_check_params(c, p)) return rc0;
    if (arity < 0 || arity > p->width - 1)
        return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "poseidon: width in [2, 8], arity <= width - 1 (spec.rs:253-257 FullBuffer)");
    if (batch == 0) return ZKT_OK;
    (void)hipSetDevice(c->device);
    const int W = p->width, rounds = 2 * p->half_full_rounds + p->partial_rounds;
    const size_t n_in = batch * (size_t)arity, n_st = out_states ? batch * (size_t)(rounds + 1) * W : 0;
    zkt_poseidon* h = nullptr;
    DevSet tmp(c->device);
    void *d_in = nullptr, *d_out = nullptr, *d_st = nullptr;
    auto run = [&]() -> int {
        int rc;
        if ((rc = zkt_poseidon_load(c, p, &h))) return rc;
        if ((rc = tmp.alloc(c, &d_in, (n_in ? n_in : 1) * 32))) return rc;
        if ((rc = tmp.alloc(c, &d_out, batch * 32))) return rc;
        if (n_st && (rc = tmp.alloc(c, &d_st, n_st * 32))) return rc;
        if (n_in) ZKT_HIP(c, hipMemcpyAsync(d_in, inputs, n_in * 32, hipMemcpyHostToDevice, c->stream));
        if ((rc = zkt_poseidon_hash_batch_dev(c, h, d_in, batch, arity, d_out, d_st))) return rc;
        ZKT_HIP(c, hipMemcpyAsync(out_hashes, d_out, batch * 32, hipMemcpyDeviceToHost, c->stream));
        if (n_st) ZKT_HIP(c, hipMemcpyAsync(out_states, d_st, n_st * 32, hipMemcpyDeviceToHost, c->stream));
        ZKT_HIP(c, hipStreamSynchronize(c->stream));
        return ZKT_OK;
    };
    const int rc = run();
    if (rc) (void)hipStreamSynchronize(c->stream);
    zkt_poseidon_free(c, h);
    return rc;
}

// ---- the note tree -------------------------------------------------------------------------------------------------------
int zkt_merkle_tree_create(zkt_ctx* c, const zkt_poseidon* h, int height, size_t capacity, zkt_merkle_tree** out) {
    if (!c || !h || !out) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (h->curve != c->curve) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "poseidon parameters belong to another curve");
    if (h->width < 3)
        return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "merkle tree: hash_two needs width >= 3 (spec.rs:253-257 FullBuffer)");
    if (height < 1 || height > 64) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "merkle tree: 1 <= height <= 64");
    if (capacity < 1 || capacity > ZKT_MERKLE_TREE_MAX || (height < 64 && (capacity >> height) && capacity != ((size_t)1 << height)))
        return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "merkle tree: 1 <= capacity <= min(2^height, ZKT_MERKLE_TREE_MAX)");
    (void)hipSetDevice(c->device);
    zkt_merkle_tree* t = new zkt_merkle_tree();
    t->curve = c->curve;
    t->height = height;
    t->pos = h;
    t->capacity = capacity;
    size_t total = 0;
    for (int L = 0; L < height; ++L) {
        const size_t len = std::max<size_t>(1, (size_t)merkle_shr_h(capacity - 1, L) + 1);
        t->layer_len.push_back(len);
        total += len;
    }
    auto make = [&]() -> int {
        int rc;
        if ((rc = dev_alloc(c, &t->d_nodes, total * 32))) return rc;
        if ((rc = dev_alloc(c, &t->d_layers, (size_t)height * sizeof(void*)))) return rc;
        if ((rc = dev_alloc(c, &t->d_empties, (size_t)height * 32))) return rc;
        if ((rc = dev_alloc(c, &t->d_root, 32))) return rc;
        if ((rc = dev_alloc(c, &t->d_table, (size_t)ZKT_MERKLE_TREE_PATHS_MAX * 16))) return rc;
        ZKT_HIP(c, hipHostMalloc(&t->h_table, (size_t)ZKT_MERKLE_TREE_PATHS_MAX * 16));
        ZKT_HIP(c, hipEventCreateWithFlags(&t->table_up, hipEventDisableTiming));
        return c->curve == ZKT_CURVE_BN254 ? merkle_create_t<Bn254Fr>(c, t) : merkle_create_t<Bls381Fr>(c, t);
    };
    if (const int rc = make()) {
        zkt_merkle_tree_free(c, t);
        return rc;
    }
    *out = t;
    return ZKT_OK;
}

void zkt_merkle_tree_free(zkt_ctx* c, zkt_merkle_tree* t) {
    if (!t) return;
    if (c) {
        (void)hipStreamSynchronize(c->stream);
        dev_free(c, t->d_nodes);
        dev_free(c, t->d_layers);
        dev_free(c, t->d_empties);
        dev_free(c, t->d_root);
        dev_free(c, t->d_table);
    }
    if (t->h_table) (void)hipHostFree(t->h_table);
    if (t->table_up) (void)hipEventDestroy(t->table_up);
    delete t;
}

int zkt_merkle_tree_info(const zkt_merkle_tree* t, int* height, uint64_t* count, uint64_t* capacity) {
    if (!t) return ZKT_ERR_INVALID_ARGUMENT;
    if (height) *height = t->height;
    if (count) *count = t->count;
    if (capacity) *capacity = t->capacity;
    return ZKT_OK;
}

// host = the leaves are in host memory: they go straight into layer 0 and the call synchronises
static int merkle_append(zkt_ctx* c, zkt_merkle_tree* t, const void* leaves, size_t m, uint64_t* first_index, bool host) {
    if (int rc = merkle_check(c, t)) return rc;
    if (first_index) *first_index = t->count;
    if (m == 0) return ZKT_OK;
    if (!leaves) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (m > t->capacity - t->count) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "merkle tree: the leaves do not fit the tree's capacity");
    (void)hipSetDevice(c->device);
    const uint64_t s = t->count;
    {
        ProfScope ps(c, "merkle_append");
        ZKT_HIP(c, hipMemcpyAsync((char*)t->d_nodes + s * 32, leaves, m * 32, host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice,
                                  c->stream));
        const int rc = c->curve == ZKT_CURVE_BN254 ? merkle_append_levels_t<Bn254Fr>(c, t, s, m) : merkle_append_levels_t<Bls381Fr>(c, t, s, m);
        if (rc) return rc;   // a launch was refused: the count stays, but layers above 0 may be half made (see the header)
        t->count = s + m;
    }
    if (host) ZKT_HIP(c, hipStreamSynchronize(c->stream));
    return ZKT_OK;
}

int zkt_merkle_tree_append_dev(zkt_ctx* c, zkt_merkle_tree* t, const void* d_leaves, size_t m, uint64_t* first_index) {
    return merkle_append(c, t, d_leaves, m, first_index, false);
}

int zkt_merkle_tree_append(zkt_ctx* c, zkt_merkle_tree* t, const uint64_t* leaves, size_t m, uint64_t* first_index) {
    return merkle_append(c, t, leaves, m, first_index, true);
}

int zkt_merkle_tree_root(zkt_ctx* c, zkt_merkle_tree* t, uint64_t* out4) {
    if (int rc = merkle_check(c, t)) return rc;
    if (!out4) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    (void)hipSetDevice(c->device);
    ZKT_HIP(c, hipMemcpyAsync(out4, t->d_root, 32, hipMemcpyDeviceToHost, c->stream));
    ZKT_HIP(c, hipStreamSynchronize(c->stream));
    return ZKT_OK;
}

int zkt_merkle_tree_layer(zkt_ctx* c, zkt_merkle_tree* t, int layer, uint64_t first, size_t n, uint64_t* out) {
    if (int rc = merkle_check(c, t)) return rc;
    if (layer < 0 || layer >= t->height) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "merkle tree: 0 <= layer < height (the root has its own call)");
    const uint64_t have = t->count ? merkle_shr_h(t->count - 1, layer) + 1 : 0;
    if (first > have || n > have - first) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "merkle tree: the range reaches past the layer's stored nodes");
    if (n == 0) return ZKT_OK;
    if (!out) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    (void)hipSetDevice(c->device);
    size_t off = first;
    for (int k = 0; k < layer; ++k) off += t->layer_len[k];
    ZKT_HIP(c, hipMemcpyAsync(out, (const char*)t->d_nodes + off * 32, n * 32, hipMemcpyDeviceToHost, c->stream));
    ZKT_HIP(c, hipStreamSynchronize(c->stream));
    return ZKT_OK;
}

int zkt_merkle_tree_paths(zkt_ctx* c, zkt_merkle_tree* t, const uint64_t* indices, size_t k, uint64_t* out_siblings) {
    if (int rc = merkle_check(c, t)) return rc;
    if (int rc = merkle_check_indices(c, t, indices, k)) return rc;
    if (k == 0) return ZKT_OK;
    if (!out_siblings) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    (void)hipSetDevice(c->device);
    const size_t bytes = k * (size_t)t->height * 32;
    DevSet tmp(c->device);
    void* d_out = nullptr;
    auto run = [&]() -> int {
        int rc;
        if ((rc = tmp.alloc(c, &d_out, bytes))) return rc;
        {
            ProfScope ps(c, "merkle_paths");
            if ((rc = merkle_table_upload(c, t, indices, k, nullptr, nullptr))) return rc;
            rc = c->curve == ZKT_CURVE_BN254 ? merkle_paths_enqueue_t<Bn254Fr>(c, t, k, false, false, d_out)
                                             : merkle_paths_enqueue_t<Bls381Fr>(c, t, k, false, false, d_out);
            if (rc) return rc;
        }
        ZKT_HIP(c, hipMemcpyAsync(out_siblings, d_out, bytes, hipMemcpyDeviceToHost, c->stream));
        ZKT_HIP(c, hipStreamSynchronize(c->stream));
        return ZKT_OK;
    };
    const int rc = run();
    if (rc) (void)hipStreamSynchronize(c->stream);
    return rc;
}

int zkt_merkle_tree_paths_to_variables_dev(zkt_ctx* c, zkt_merkle_tree* t, const uint64_t* indices, size_t k, void* d_variables,
                                           size_t n_vars, const uint32_t* bit_var0, const uint32_t* sibling_var0) {
    if (int rc = merkle_check(c, t)) return rc;
    if (int rc = merkle_check_indices(c, t, indices, k)) return rc;
    if (k == 0) return ZKT_OK;
    if (!d_variables || !sibling_var0) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    // every range inside the map, no two of them overlapping: sorted by their first variable, neighbours are >= height apart
    const uint64_t H = (uint64_t)t->height;
    std::vector<uint64_t> starts(sibling_var0, sibling_var0 + k);
    if (bit_var0) starts.insert(starts.end(), bit_var0, bit_var0 + k);
    std::sort(starts.begin(), starts.end());
    for (size_t i = 0; i < starts.size(); ++i) {
        if (starts[i] > n_vars || H > n_vars - starts[i])
            return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "merkle tree: a sibling or bit range lies outside the variable map");
        if (i && starts[i] < starts[i - 1] + H)
            return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "merkle tree: two sibling or bit ranges overlap");
    }
    (void)hipSetDevice(c->device);
    ProfScope ps(c, "merkle_paths");
    if (int rc = merkle_table_upload(c, t, indices, k, sibling_var0, bit_var0)) return rc;
    return c->curve == ZKT_CURVE_BN254 ? merkle_paths_enqueue_t<Bn254Fr>(c, t, k, true, bit_var0 != nullptr, d_variables)
                                       : merkle_paths_enqueue_t<Bls381Fr>(c, t, k, true, bit_var0 != nullptr, d_variables);
}

int zkt_debug_merkle_tree_split(zkt_merkle_tree* t, int wide_min_parents) {
    if (!t || wide_min_parents < 0) return ZKT_ERR_INVALID_ARGUMENT;
    t->wide_min_parents = wide_min_parents;
    return ZKT_OK;
}

}  // extern "C"
