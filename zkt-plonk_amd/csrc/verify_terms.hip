// The batch verifier's transcripts and scalar stage on the device (the replay and the layout: verify_terms.hpp; the
// transcripts: transcript_core.hpp; the arithmetic: linearisation.hpp -- each the code the host runs too).
//   k_verify_terms   one lane per proof: verifier_replay from the proof's exported transcript state into the 24 sums by
//                    source -- the Fiat-Shamir replay, xi_point, compute_r0, the linearisation scalars, both fold lists.
// 64-thread workgroups, so a batch of a few thousand proofs spreads over every CU.  Each lane owns VT_LANE_WORDS 64-bit
// words of LDS laid out [word][lane] (23.0 KB per workgroup): the sponge, the message buffer and the Ethereum states are
// addressed by byte there and never sit in a register array.  Lanes diverge -- positions differ with n_pi, so they
// permute at different times -- which this stage can afford.  Nothing is indexed by proof data beyond the per-proof
// offsets the host wrote; every lane checks its index against the count it was given.
//
// Resources (gfx950, docs/EXPERIMENTS.md "one verifier replay and one transcript core"): 256 VGPRs, 6896 bytes of scratch
// per lane for the call frames of the non-inlined field and transcript functions, no spills.
#include "verify_terms.hpp"

namespace zkt {

template <class C>
__global__ __launch_bounds__(VT_THREADS) void k_verify_terms(const VtDesc<typename C::Fr>* __restrict__ desc,
                                                             TranscriptState* __restrict__ states,
                                                             const Affine<typename C::Fq>* __restrict__ points,
                                                             const Fe<typename C::Fr>* __restrict__ ev,
                                                             const Fe<typename C::Fr>* __restrict__ roots,
                                                             const Fe<typename C::Fr>* __restrict__ vals,
                                                             const Fe<typename C::Fr>* __restrict__ forced,
                                                             Fe<typename C::Fr>* __restrict__ before, int32_t* __restrict__ status,
                                                             Fe<typename C::Fr>* __restrict__ acc, Fe<typename C::Fr>* __restrict__ dbg,
                                                             uint32_t count) {
    __shared__ uint64_t lds[VT_LANE_WORDS * VT_THREADS];
    const uint32_t i = blockIdx.x * VT_THREADS + threadIdx.x;
    if (i >= count) return;
    VtTr t;
    t.s.st = lds + threadIdx.x;
    t.s.msg = lds + VT_ST_WORDS * VT_THREADS + threadIdx.x;
    t.s.eth = lds + (VT_ST_WORDS + VT_MSG_WORDS) * VT_THREADS + threadIdx.x;
    t.s.stride = VT_THREADS;
    vt_load_state(t, &states[i]);
    const VtDesc<typename C::Fr> d = desc[i];
    VtProof<C> p;
    p.n = d.n;
    p.n_pi = d.n_pi;
    p.w = d.w;
    p.rho[0] = d.rho[0];
    p.rho[1] = d.rho[1];
    p.cm = points + (size_t)i * 13;
    p.ev = ev + (size_t)i * 12;
    p.roots = roots + d.pi_off;
    p.vals = vals + d.pi_off;
    p.forced = forced ? forced + (size_t)i * 7 : nullptr;
    p.before = before + d.pi_off;
    p.acc = acc + (size_t)i * 24;
    p.dbg = dbg ? dbg + (size_t)i * 8 : nullptr;
    status[i] = vt_terms<C>(VtCoreTr<C>{t}, p);
    vt_store_state(t, &states[i]);
}

template <class C>
static int terms_launch(zkt_ctx* c, char* base, const VtLayout& lay, const void* d_points, size_t count, bool forced, bool dbg) {
    using R = typename C::Fr;
    hipLaunchKernelGGL(k_verify_terms<C>, dim3((unsigned)((count + VT_THREADS - 1) / VT_THREADS)), dim3(VT_THREADS), 0, c->stream,
                       (const VtDesc<R>*)(base + lay.desc), (TranscriptState*)(base + lay.states),
                       (const Affine<typename C::Fq>*)d_points, (const Fe<R>*)(base + lay.ev), (const Fe<R>*)(base + lay.roots),
                       (const Fe<R>*)(base + lay.vals), forced ? (const Fe<R>*)(base + lay.forced) : nullptr,
                       (Fe<R>*)(base + lay.before), (int32_t*)(base + lay.status), (Fe<R>*)(base + lay.acc),
                       dbg ? (Fe<R>*)(base + lay.dbg) : nullptr, (uint32_t)count);
    ZKT_HIP(c, hipGetLastError());
    return ZKT_OK;
}

int verify_terms_enqueue(zkt_ctx* c, void* d_base, const VtLayout& lay, const void* d_points, size_t count, bool forced, bool dbg) {
    if (count == 0 || count > ZKT_VERIFY_BATCH_DEV_MAX) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "verify terms: bad count");
    if (c->curve == ZKT_CURVE_BN254) return terms_launch<Bn254Curve>(c, (char*)d_base, lay, d_points, count, forced, dbg);
    return terms_launch<Bls381Curve>(c, (char*)d_base, lay, d_points, count, forced, dbg);
}

}  // namespace zkt
