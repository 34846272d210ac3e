/*
 * zkt_plonk.h -- C-ABI of the MI355X (gfx950) prover hot path for ZKTLabs/zkt-plonk.
 *
 * The reference is pure Rust and has no FFI; the two generic seams of
 * ZKTPlonk<F, D, PC, T, C, TABLE_SIZE> (plonk-core/src/plonk.rs:39-52) are where a replacement
 * plugs in.  Each entry point below names the reference interface it replaces (file:line relative to
 * /root/reference).  INTEGRATION.md shows the Rust shim (GpuDomain<F>, GpuKZG10<E>, prove_gpu)
 * that binds them.
 *
 * Conventions:
 *  - Field elements cross as little-endian u64 limbs in MONTGOMERY form, exactly arkworks'
 *    in-memory representation (ark-ff 0.3 Fp256 / Fp384): Fr = 4 limbs for both curves,
 *    Fq = 4 limbs (BN254) or 6 limbs (BLS12-381).
 *  - A G1 affine point crosses as x limbs || y limbs; the all-zero pair (0, 0) encodes the point at
 *    infinity (GroupAffine is repr(Rust): the shim repacks explicitly, it never transmutes).
 *  - The caller owns every host buffer; pointers are borrowed for the duration of the call.
 *    Entry points with the _dev suffix take DEVICE pointers (HBM resident, same layout) and enqueue
 *    on the context's stream without synchronising.
 *  - Every call returns ZKT_OK or an error code; zkt_last_error() gives the message.  Nothing
 *    aborts: where the reference panics (zero denominators, equal challenges, short quotient) the
 *    library reports an error.
 *  - A context is used by one thread at a time; several contexts may coexist.
 */
#ifndef ZKT_PLONK_H
#define ZKT_PLONK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct zkt_ctx zkt_ctx;

enum {
    ZKT_CURVE_BN254 = 0,     /* ark-bn254 0.3    (bin/src/instance.rs:7-10)  */
    ZKT_CURVE_BLS12_381 = 1  /* ark-bls12-381 0.3 (bin/src/instance.rs:12-15) */
};

enum {
    ZKT_OK = 0,
    ZKT_ERR_INVALID_ARGUMENT = 1,
    ZKT_ERR_INVALID_DOMAIN_SIZE = 2,   /* Error::InvalidEvalDomainSize, plonk-core/src/error.rs */
    ZKT_ERR_HIP = 3,
    ZKT_ERR_NO_DEVICE = 4,
    ZKT_ERR_TOO_MANY_COEFFICIENTS = 5, /* kzg10 Error::TooManyCoefficients -> Error::PCError     */
    ZKT_ERR_ZERO_DENOMINATOR = 6,      /* reference: .inverse().unwrap() panics                   */
    ZKT_ERR_EQUAL_CHALLENGES = 7,      /* reference: assert_ne! at prove.rs:202-207               */
    ZKT_ERR_NOT_IN_TABLE = 8,          /* Error::ElementNotIndexedInTable, multiset.rs:121        */
    ZKT_ERR_QUOTIENT_TOO_SHORT = 9,    /* reference: slice panic at prove.rs:287-300              */
    ZKT_ERR_NOT_LOADED = 10,
    ZKT_ERR_COMM = 11                  /* the caller's communicator reported a failure */
};

/* ---- context ------------------------------------------------------------------------------ */
/* Creates a context on HIP device `device_id` for `curve_id`.  Fails with ZKT_ERR_NO_DEVICE when no
 * GPU is present: there is no CPU fallback. */
int zkt_ctx_create(int curve_id, int device_id, zkt_ctx** out);
void zkt_ctx_destroy(zkt_ctx* ctx);
/* A second context on the same GPU that SHARES `ctx`'s read-only tables -- the SRS window table and the Lagrange-basis
 * table, the circuit's keys (ProverKey polynomials, ExtendedProverKey cosets), the transform twiddles -- and owns only
 * what a proof writes: its stream, work buffers and MSM slots (about 3 of the ~7 GiB a context holds at n = 2^20).  For a
 * service that keeps several proofs in flight on one GPU (one host thread per context), which is what hides the latency
 * chain of the reference's real circuit sizes: n = 2^14 385 -> 587 proofs/s with two contexts, n = 2^18 156 -> 186 with
 * three.  The fork proves exactly as `ctx` would (same bytes), and a fork may be forked in turn.  Rules: no communicator
 * on either side; while a context forked from `ctx` (or from one of those) still reads one of its key or circuit tables,
 * `ctx` refuses zkt_srs_* / zkt_circuit_* / zkt_ctx_set_comm (its tables are in use); a fork that loads a key or circuit
 * of its own simply stops sharing that part, so a context whose forks have all loaded a key and a circuit of their own is
 * refused nothing.  Contexts may be destroyed in any order: the shared tables belong to no context and are freed when
 * the last context that reads them is destroyed or lets go of them.
 * Create and destroy contexts from one thread (or serialise those calls); prove on them concurrently. */
int zkt_ctx_fork(zkt_ctx* ctx, zkt_ctx** out);
const char* zkt_last_error(const zkt_ctx* ctx);
/* Use an existing hipStream_t (e.g. PyTorch's current stream; NULL is the device's default stream) for every launch of
 * this context.  The stream stays the caller's, and the caller may have work of its own on it when it calls the
 * library (tests/test_gpu_caller_stream.py pins the four rules):
 *  1. Everything that reads caller memory -- a _dev entry's device pointers, the device witness of zkt_prove /
 *     zkt_prove_set_next / zkt_circuit_check_witness -- is ordered behind the work already on the stream at the time of
 *     the call: a buffer the caller's own kernel on this stream is still to write is read after that kernel.  The
 *     library's internal streams (MSM tails, the prover's copy / aux / comm streams, the KZG seam's copy stream) are
 *     ordered against the context's stream with events; none of them reads caller memory ahead of it.
 *  2. Results that an enqueue-only entry leaves in device memory are visible to whatever the caller enqueues on the
 *     stream afterwards, without a synchronisation.  Entries that hand a result to HOST memory synchronise and say so.
 *  3. zkt_ctx_set_stream synchronises the OLD stream before it switches.  MSMs begun with zkt_msm_enqueue_dev and a
 *     proof announced with zkt_prove_set_next carry over: their tails are ordered by events, not by the stream's
 *     identity, and the next call on the new stream collects or continues them with the same results.
 *  4. The library never destroys a caller's stream: zkt_ctx_set_stream to another stream and zkt_ctx_destroy leave it
 *     usable (only the stream zkt_ctx_create made is the library's to destroy). */
int zkt_ctx_set_stream(zkt_ctx* ctx, void* hip_stream);
int zkt_ctx_synchronize(zkt_ctx* ctx);
/* Timing with HIP events on the stream the kernels run on (each event pair costs a few microseconds of stream time,
 * so only these scopes exist).  Names: "ntt_<log2 size>" (whole transform), "msm_main" (grouping, accumulation and
 * bucket fold of one MSM), "msm_accumulate" (the accumulation kernel alone), "msm_fold" / "msm_tail" (bucket fold and
 * reduction, on the side stream), "quotient", and the prover's rounds as stream time between their first and last
 * launch: "round1", "round2" (prove.rs:116-185; issued early when announced by zkt_prove_set_next), "round3"
 * (:190-255), "round4" (:258-313), "round5" (:318-451); "msm_lag_main" / "msm_lag_accumulate": the same two scopes for
 * commitments taken in the Lagrange basis -- t, h1, h2, z2 over the prefix table and the wires committed over their
 * base tables (see "Commitments of evaluation vectors"): they have fewer pairs than the n + 3 points "msm_accumulate" is
 * priced at and would dilute the dense kernel's average;
 * "host_wait": idle time of the context's stream across the prover's host round trips (from the moment the stream
 * drains while the host waits for a round's commitments or evaluations to the next launch; six per proof).
 * The KZG seam (zkt_kzg_commit_batch / zkt_kzg_open): "kzg_commit_batch" (the whole batch of MSMs on the stream),
 * "kzg_open_upload" (the coefficients' copy to HBM), "kzg_open_combine" (power tables and the fused combination /
 * evaluation pass), "kzg_open_divide" (division by X - z) and "kzg_open_msm" (the witness commitment).
 * "sigma": the key, sort, link and evaluation launches of zkt_circuit_sigma_dev / zkt_circuit_setup_wiring (not the
 * domain table they read).
 * "check_witness": every launch of zkt_circuit_check_witness (selector transforms, the sigma launches when the wiring
 * is checked, the gate, residual and comparison kernels), not its uploads.
 * "check_witness_batch": the same launches of zkt_circuit_check_witness_batch, once for the whole batch.
 * "merkle_append": the copy of the leaves into layer 0 and every level launch of one zkt_merkle_tree_append(_dev);
 * "merkle_paths": the table upload and the gather launch of zkt_merkle_tree_paths / _paths_to_variables_dev.
 * "withdraw_layout": the two row launches of zkt_withdraw_create / zkt_withdraw_rows / zkt_withdraw_setup;
 * "withdraw_witness": everything zkt_withdraw_witness enqueues, from the staged requests' copy to the closing kernel.
 * A scope that covers a batch counts its units in `calls` (the three commitments of a round grouped and accumulated as one
 * batch of launches: 3); "<name>#launches" returns the number of recorded scopes instead.
 * on = 0: off; 1: every scope; 2: only "msm_accumulate" and "host_wait" -- the level for timing the dominant kernel
 * and the stream's idle time live inside a throughput measurement (~18 event pairs per proof instead of ~80). */
int zkt_profile_enable(zkt_ctx* ctx, int on);
int zkt_profile_get(zkt_ctx* ctx, const char* name, uint64_t* calls, double* total_ms);
const char* zkt_version(void);

/* ---- one proof across the GPUs of a node (BASELINE.json configs[4]) -------------------------
 * One process (and one context) per GPU; the same calls are made on every rank with the same inputs.  What shards:
 *   - every KZG commitment (commitment.rs:24-46): rank r keeps the SRS slice zkt_shard_range(total, r, world) and sums
 *     over it; the partial sums of a prover round travel in ONE all-gather as raw bytes (world x k x 128|192 B) and are
 *     added on every rank (a collective cannot reduce curve points);
 *   - the 4n-coset work of round 4 (quotient_poly.rs:52-224): rank r owns the coset points whose index is r modulo
 *     world -- a coset of 4n / world points on which it transforms the nine witness polynomials (keys: once, at load)
 *     and runs the fused quotient pass with no communication ("omega-next" = index + 4 stays in the class for world
 *     <= 4; with 8 ranks the four shifted vectors are transformed on the neighbouring class as well).  ONE all-gather
 *     of 4n x 32 B in total brings the quotient evaluations together before the inverse transform.
 * Everything else (the n-point inverse transforms, grand products, evaluations, openings' polynomials, Fiat-Shamir) is
 * replicated: every rank produces the same proof bytes, equal to the single-GPU bytes.
 * The communicator is supplied by the caller: libzkt_comm_rccl.so (zkt_comm_rccl.h) is that communicator over RCCL as a C
 * library of its own, for hosts that have none (a Rust binary); zkt-plonk_amd/parallel.py has the same over
 * torch.distributed.  This library links no transport.  With more than one GPU the device exchange -- an in-place
 * all-gather on the library's own HBM buffer -- is UNVERIFIED ON HARDWARE: no multi-GPU node was available; it runs with
 * world-of-one RCCL communicators under 2 / 4 thread-ranks on one GPU, and the sharded prover itself is byte-checked with
 * thread and gloo ranks on one GPU up to BLS12-381 n = 2^22 x 8 ranks.
 * all_gather: `bytes` per rank, results in rank order; on_device = 0: host pointers;
 * on_device = 1 (only if device_buffers != 0): device pointers, the library has synchronised `hip_stream` before the
 * call and the exchange must be complete when the callback returns.  Returns 0 on success.
 * all_gather_async (optional, may be NULL; needs device_buffers != 0): device pointers; the collective is ENQUEUED on
 * `hip_stream` behind the work already there and the callback returns without waiting for it -- the library never
 * synchronises the host around it.  With it the quotient exchange of round 4 goes out in ZKT_QUOTIENT_CHUNKS pieces on a
 * stream of its own, each behind the kernel that produced the piece, so that the collective of one piece travels while
 * the next is computed, and the host is not blocked at any exchange of device data.  Without it the library falls back
 * to the blocking callback (one whole exchange after the quotient pass). */
typedef struct {
    void* user;
    int rank;
    int world;               /* 1, 2, 4 or 8 */
    int device_buffers;      /* 0: device exchanges are staged through pinned host memory by the library */
    int (*all_gather)(void* user, const void* send, void* recv, size_t bytes, int on_device, void* hip_stream);
    int (*all_gather_async)(void* user, const void* d_send, void* d_recv, size_t bytes, void* hip_stream);
} zkt_comm_vtable;
#define ZKT_QUOTIENT_CHUNKS 4
/* Attach (or, with NULL / world = 1, detach) the communicator.  Must precede zkt_srs_load_slice / zkt_circuit_load /
 * zkt_circuit_setup of the sharded proof: keys are laid out for the rank's share. */
int zkt_ctx_set_comm(zkt_ctx* ctx, const zkt_comm_vtable* comm);
/* Contiguous share [*lo, *hi) of `total` units for `rank` (sizes differ by at most one). */
int zkt_shard_range(size_t total, int rank, int world, size_t* lo, size_t* hi);
/* Exchanged bytes and collective calls since the communicator was attached (this rank's send side). */
int zkt_comm_stats(zkt_ctx* ctx, uint64_t* calls, uint64_t* bytes_sent);
/* Plumbing check without a GPU: gathers `bytes` from every rank through the vtable (host buffers). */
int zkt_comm_selftest(const zkt_comm_vtable* comm, const void* send, void* recv, size_t bytes);

/* ---- device memory helpers (plumbing for callers without their own allocator) -------------- */
int zkt_dev_alloc(zkt_ctx* ctx, size_t bytes, void** dptr);
int zkt_dev_free(zkt_ctx* ctx, void* dptr);
int zkt_dev_upload(zkt_ctx* ctx, void* dptr, const void* host, size_t bytes);
int zkt_dev_download(zkt_ctx* ctx, void* host, const void* dptr, size_t bytes);

/* ---- Domain seam: D: EvaluationDomain<F> + EvaluationDomainExt<F> (prove.rs:70) ------------ */
/* Radix-2 transform of size 2^log_n over Fr, natural order in and out.
 *   inverse = 0, coset = 0 : D::fft            (util.rs:104-113)  out[i] = sum_j in[j] w^(ij)
 *   inverse = 1, coset = 0 : D::ifft(_in_place) (util.rs:63-86)   inverse, scaled by 1/n
 *   inverse = 0, coset = 1 : D::coset_fft(_in_place) (util.rs:117-140)  in[j] *= g^j first
 *   inverse = 1, coset = 1 : D::coset_ifft_in_place (util.rs:90-100)    then out[j] *= g^-j
 * `in` holds in_len <= 2^log_n elements and is zero-padded (ark-poly resizes the coefficient vector);
 * `out` receives 2^log_n elements.  in == out is allowed.  log_n > TWO_ADICITY (28 / 32) or
 * in_len > 2^log_n -> ZKT_ERR_INVALID_DOMAIN_SIZE. */
int zkt_ntt(zkt_ctx* ctx, int log_n, int inverse, int coset, const uint64_t* in, size_t in_len, uint64_t* out);
int zkt_ntt_dev(zkt_ctx* ctx, int log_n, int inverse, int coset, const void* d_in, size_t in_len, void* d_out);
/* One GPU's share of D::coset_fft on the domain of size 2^log_big (util.rs:117-140) sharded by output index over
 * G = 2^(log_big - log_n) GPUs: out[i] = p(g w_big^(cls + G i)), i < 2^log_n -- the evaluations whose index is cls
 * modulo G, a coset of their own, obtained by one 2^log_n-point transform with no exchange.  in_len may exceed 2^log_n
 * (the polynomial is folded modulo X^(2^log_n) - shift^(2^log_n) first).  Host pointers. */
int zkt_ntt_class(zkt_ctx* ctx, int log_n, int log_big, int cls, const uint64_t* in, size_t in_len, uint64_t* out);
/* EvaluationDomainExt::group_gen (util.rs:52-58): writes the 2^log_n-th root of unity (4 limbs). */
int zkt_domain_group_gen(zkt_ctx* ctx, int log_n, uint64_t* out4);

/* ---- Commitment seam: PC: HomomorphicCommitment<F> = KZG10<E> (commitment.rs:10-46) --------- */
/* Loads `count` G1 powers (ck.powers_of_g of SonicKZG10's CommitterKey, produced by PC::trim at
 * plonk.rs:79-85) and precomputes the window multiples used by the MSM.  One-time per key.  The
 * prover never commits to more than n + 7 coefficients (the opening witnesses), so loading n + 8 of the 4n + 1 powers the reference keeps is
 * enough.  Replaces nothing at run time: it is the device-resident form of `ck`.
 * _dev: the powers already in HBM, read behind the work already on the context's stream.  Both forms release the
 * previous key and allocate the new tables, which waits for the device: unlike the other _dev entries this one is no
 * enqueue.  Synchronises the stream.  The points are taken as they come, unchecked (as the reference's CLI reads them): for a
 * key from outside, zkt_srs_check validates it first. */
int zkt_srs_load(zkt_ctx* ctx, const uint64_t* g1_xy_mont, size_t count);
int zkt_srs_load_dev(zkt_ctx* ctx, const void* d_g1_xy_mont, size_t count);
/* Test/bench SRS with a KNOWN trapdoor: powers_of_g[i] = tau^i * G (tau: 4 canonical limbs).
 * Stands in for PC::setup (ark-poly-commit kzg10 setup), which is out of scope; insecure by design. */
int zkt_srs_generate(zkt_ctx* ctx, const uint64_t* tau_canonical4, size_t count);
int zkt_srs_download(zkt_ctx* ctx, size_t offset, size_t count, uint64_t* out_xy_mont);
/* The G2 half of that test SRS, i.e. SonicKZG10's VerifierKey::h and ::beta_h for the same trapdoor: h = the G2
 * generator of ark-bn254 / ark-bls12-381, beta_h = tau h (arkworks' Fp2 layout x.c0, x.c1, y.c0, y.c1, Montgomery
 * limbs).  Host-only; what zkt_verify takes next to the proof.  Insecure by design, like zkt_srs_generate. */
int zkt_srs_generate_g2(int curve_id, const uint64_t* tau_canonical4, uint64_t* out_h, uint64_t* out_beta_h);
/* Sharded committer key: this rank keeps powers [offset, offset + count) of a key of `total` powers -- its
 * zkt_shard_range(total, rank, world).  The window table shrinks by the number of ranks.  zkt_msm_g1* then index into the
 * slice; zkt_prove / zkt_circuit_setup combine the ranks' partial sums through the communicator. */
int zkt_srs_load_slice(zkt_ctx* ctx, const uint64_t* g1_xy_mont_slice, size_t offset, size_t count, size_t total);
int zkt_srs_generate_slice(zkt_ctx* ctx, const uint64_t* tau_canonical4, size_t offset, size_t count, size_t total);
/* sum_i scalars[i] * powers_of_g[base_offset + i], affine result (x || y Montgomery limbs, (0,0) and
 * *out_is_infinity = 1 for the identity).  This is VariableBaseMSM::multi_scalar_mul as called by
 * kzg10::commit / open_with_witness_polynomial (prove.rs:133-135,178-180,249-251,306-308,373-375,
 * 381-451): scalars_montgomery = 1 takes polynomial coefficients as they sit in a DensePolynomial
 * (the into_repr() conversion happens on the device), 0 takes canonical bigints (commitment.rs:36-42).
 * base_offset mirrors skip_leading_zeros_and_convert_to_bigints (powers_of_g[num_leading_zeros..]).
 * len + base_offset > loaded powers -> ZKT_ERR_TOO_MANY_COEFFICIENTS; len = 0 -> identity. */
int zkt_msm_g1(zkt_ctx* ctx, const uint64_t* scalars, size_t len, size_t base_offset, int scalars_montgomery,
               uint64_t* out_xy_mont, int* out_is_infinity);
/* Same with the scalars already resident in HBM; the affine result is written to HOST memory
 * (it feeds the host-side transcript).  Synchronises the stream. */
int zkt_msm_g1_dev(zkt_ctx* ctx, const void* d_scalars, size_t len, size_t base_offset, int scalars_montgomery,
                   void* out_xy_mont_host);
/* Enqueue-only form for benchmarking the device part under HIP events (no host finish, no sync). */
int zkt_msm_enqueue_dev(zkt_ctx* ctx, const void* d_scalars, size_t len, size_t base_offset, int scalars_montgomery);
/* Window size c, number of windows and loaded powers of the current SRS (0s when none). */
int zkt_msm_info(zkt_ctx* ctx, int* window_bits, int* windows, size_t* srs_count);

/* VariableBaseMSM::multi_scalar_mul (ark-ec 0.3) on the device for ARBITRARY affine bases, the seam of
 * HomomorphicCommitment::multi_scalar_mul (commitment.rs:31-45): sum_i scalars[i] * bases[i].
 * bases: n x (x, y) Montgomery limbs in arkworks' layout (8 / 12 u64 per point), (0,0) = identity.
 * scalars: n x 4 u64, Montgomery (scalars_montgomery = 1) or canonical 256-bit integers (0).  Canonical scalars are used
 * as full integers: every bit counts, values >= r included (for a point of the prime-order subgroup the result is then
 * sum (s_i mod r) P_i).  Bases may repeat, appear negated, be the identity or carry a zero scalar.  Bases are NOT checked
 * for being on the curve or in the subgroup (as arkworks does not); an invalid point gives an unspecified point, never a
 * fault.  (zkt_g1_check tests them.)  Result: affine, host memory, (0,0) and *out_is_infinity = 1 for the identity (out_is_infinity may be NULL).
 * n = 0 -> the identity; 1 <= n <= ZKT_MSM_BASES_MAX on either curve; a larger n -> ZKT_ERR_INVALID_ARGUMENT, a failed
 * allocation -> ZKT_ERR_HIP.  Needs no SRS: the call works on any context (with or without a key, forked, between proofs)
 * and leaves the loaded SRS, Lagrange-basis table, circuit and the prover's MSM buffers untouched; its scratch memory is
 * its own, allocated on first use, grown as needed and freed by zkt_ctx_destroy.  A proof announced with
 * zkt_prove_set_next keeps its early work: the call only adds its own launches behind it on the context's stream, and that
 * proof's bytes do not change.  Local even on a context with a communicator (no collective).  Synchronises the stream.
 * _dev: bases and scalars already in HBM, same layouts; the result still goes to host memory. */
#define ZKT_MSM_BASES_MAX ((size_t)1 << 22)
int zkt_msm_g1_bases(zkt_ctx* ctx, const uint64_t* bases_xy_mont, const uint64_t* scalars, size_t n,
                     int scalars_montgomery, uint64_t* out_xy_mont, int* out_is_infinity);
int zkt_msm_g1_bases_dev(zkt_ctx* ctx, const void* d_bases_xy_mont, const void* d_scalars, size_t n,
                         int scalars_montgomery, uint64_t* out_xy_mont_host, int* out_is_infinity);
/* Digit width c and number of windows zkt_msm_g1_bases uses for n points (0s for n = 0); n > ZKT_MSM_BASES_MAX ->
 * ZKT_ERR_INVALID_ARGUMENT. */
int zkt_msm_bases_info(zkt_ctx* ctx, size_t n, int scalars_montgomery, int* window_bits, int* windows);

/* ---- KZG commitment seam (PC::commit / PC::open of a KZG10 wrapper that keeps the host prover) ----------
 * zkt_kzg_commit_batch: PC::commit(ck, [p_0 .. p_(k-1)], None) in ONE call, entry j = sum_i p_j[i] * powers_of_g[i].
 * The k MSMs go out on the prover's schedule (grouped launches where the key size gains from them, the bucket reductions
 * overlapping the next MSM) instead of one blocking zkt_msm_g1 each; the host form uploads polynomial j + 1 on a copy
 * stream while polynomial j's MSM runs.  scalars_montgomery as in zkt_msm_g1.
 * zkt_kzg_open: open_individual_opening_challenges with challenges c_j (opening_challenges(j), j < k):
 * w = commit(floor((sum_j c_j p_j) / (X - z))), and out_evals[j] = p_j(z) when out_evals_mont is not NULL (k x 4 u64).
 * Coefficients, challenges and the point are Montgomery limbs, as they sit in arkworks memory.
 * Output: entry j at out_xy_mont + j * 2L (L = 4 on BN254, 6 on BLS12-381), x limbs then y limbs as zkt_msm_g1; the
 * identity is written as (0,0) with its flag set to 1; out_is_infinity may be NULL.
 * Lengths: lens[j] = 0 is the zero polynomial; k = 0 -> ZKT_OK, nothing written; k > ZKT_KZG_BATCH_MAX ->
 * ZKT_ERR_INVALID_ARGUMENT; any lens[j] above the loaded powers -> ZKT_ERR_TOO_MANY_COEFFICIENTS, checked before any work
 * is enqueued (no output is written then).  Any point z is valid, z = 0 (the witness is the combination shifted down by one
 * coefficient) and roots of unity included; a combination of degree < 1 gives the identity.
 * Needs a loaded SRS (ZKT_ERR_NOT_LOADED otherwise) and no circuit; a key loaded as a slice (zkt_srs_load_slice /
 * _generate_slice) -> ZKT_ERR_INVALID_ARGUMENT.  Local: no collective, even with a communicator set.  The scratch memory
 * is the call's own (allocated on first use, grown as needed, freed by zkt_ctx_destroy; a forked context gets its own); the
 * circuit's buffers are never touched, and a proof announced with zkt_prove_set_next yields the same bytes (its early work
 * is redone when the call took the MSM slots it used).  Synchronises the stream.
 * _dev: the coefficient vectors already in HBM (d_coeffs[j] may be NULL when lens[j] = 0); results still go to host memory. */
#define ZKT_KZG_BATCH_MAX 32
int zkt_kzg_commit_batch(zkt_ctx* ctx, const uint64_t* const* coeffs, const size_t* lens, int k,
                         int scalars_montgomery, uint64_t* out_xy_mont, int* out_is_infinity);
int zkt_kzg_commit_batch_dev(zkt_ctx* ctx, const void* const* d_coeffs, const size_t* lens, int k,
                             int scalars_montgomery, uint64_t* out_xy_mont, int* out_is_infinity);
int zkt_kzg_open(zkt_ctx* ctx, const uint64_t* const* coeffs, const size_t* lens, int k,
                 const uint64_t* challenges_mont, const uint64_t* point_mont,
                 uint64_t* out_w_xy_mont, int* out_w_is_infinity, uint64_t* out_evals_mont);
int zkt_kzg_open_dev(zkt_ctx* ctx, const void* const* d_coeffs, const size_t* lens, int k,
                     const uint64_t* challenges_mont, const uint64_t* point_mont,
                     uint64_t* out_w_xy_mont, int* out_w_is_infinity, uint64_t* out_evals_mont);

/* ---- Commitments of evaluation vectors (Lagrange-basis key) ------------------------------------------
 * The reference commits to t, h1, h2 and z2 through their coefficients (prove.rs:145-180,225-251: poly_from_evals,
 * add_blinders_to_poly, PC::commit -- one dense MSM each).  As EVALUATION vectors they are piecewise constant (table
 * values then zeros, sorted runs, a grand product whose ratio is 1 wherever the lookup stands still), so the library
 * commits to them in the Lagrange basis of the circuit's domain: with S_k = sum_{i<k} [L_i(tau)] G,
 *     commit = sum_k (e_(k-1) - e_k) S_k + sum_j b_j ([tau^(n+j)] G - [tau^j] G),
 * an MSM whose scalars vanish inside every run.  The same group element, so the same proof bytes; a dense vector costs
 * what its coefficients would.  The second base table (prefix sums of the inverse DFT of the powers over G1, plus the
 * blinder points; as large as the first) is built on the first proof after a key or circuit change -- about 0.55 s at
 * n = 2^20 on BN254 -- when the key is whole (not a slice of a sharded key) and holds more than n powers; otherwise,
 * or after zkt_ctx_set_lagrange(ctx, 0), the coefficients are committed as the reference does.
 *
 * Wire polynomials over per-variable bases.  A wire's evaluation vector is a gather of the variable map (prove.rs:49-55:
 * a[i] = variables[w_l[i]]), so  commit(a) = sum_v variables[v] T_v + blinder terms,  T_v = sum_{i : w_l[i] = v} [L_i(tau)] G:
 * one scalar per DISTINCT variable of the wire, not one per row.  The route is taken for a proof that passes the witness
 * as `variables` + w_l / w_r / w_o with wires_on_device != 0, when the Lagrange-basis table above exists and commitments
 * of evaluations are not switched off; per wire, when its distinct variables are fewer than 0.9 n_rows (the withdraw
 * circuit at n = 2^20: the right wire has 0.27 n_rows, the left 0.83, the output wire 1.00 and stays dense).
 * Cached: per wire the sorted distinct variables and the table of their T_v with the two blinder points (window
 * multiples as for the other tables: 64 bytes x windows per base on BN254, 265 MB + 810 MB for the circuit above), built
 * inside the first proof that brings a wiring (one-off; not yet timed on hardware, see docs/EXPERIMENTS.md), keyed on the three vectors'
 * addresses, n_rows, n_vars, the key and the domain.  Forks made afterwards read the same tables; a fork made before
 * builds its own.  A key or circuit reload drops them.
 * Staleness: the build keeps a 128-bit digest of the vectors' contents (sums of position-keyed 64-bit mixes; it guards
 * against reuse of the addresses, not against an adversary).  Every proof on the route computes the digest of the vectors it
 * was given ahead of round 1; the host compares when it collects round 1 (also of a proof announced with
 * zkt_prove_set_next), before a_commit is absorbed.  On a mismatch the affected commitments are taken again from the
 * blinded coefficients, which exist anyway, and the tables are rebuilt by the next proof (a context whose forks read its
 * tables keeps them and commits densely instead).
 * Fallbacks, per wire, to the coefficient route: too many distinct variables; a T_v that is the identity (a degenerate
 * tau); a table that cannot be allocated; a blinded polynomial trimmed below n coefficients (a constant or all-Zero
 * wire: its blinders then sit below X^n; found with the digest, committed again).  Sharded keys and host-resident
 * witnesses keep dense wire commitments.  The proof bytes are the same on either route.
 *
 * Wire polynomials over the circuit's free variables (measured on MI355X: docs/EXPERIMENTS.md; the kernel trace and
 * counter passes of this route have not been run).  Most variables of
 * a circuit are not free.  Walking the rows in ascending order, a row with q_m = 0 and q_o = 1 or -1 that is no
 * public-input position of the proof, whose output is a real variable seen on no wire of an earlier row and on no input
 * wire of this one, DEFINES that output as an affine function of earlier variables; a variable first seen anywhere else
 * is free.  Substituting, x_v = kappa_v + sum_f M[v][f] x_f over free f (at most 16 terms: a longer form makes v free), so
 *     commit(wire k) = sum_f x_f A^k_f + C^k + blinder terms,   A^k_f = sum_v M[v][f] T^k_v,   C^k = sum_v kappa_v T^k_v:
 * one scalar per free variable that reaches the wire (the withdraw circuit at n = 2^20: 0.20 n, 0.11 n and 0.20 n bases
 * on the left, right and output wire, against 0.83 n, 0.27 n and 1.00 n distinct variables; the tables are built inside
 * the first proof that brings a wiring, 5.3 s there, 1.2 s at 2^18).
 * THE ROUTE PRESUMES A WITNESS THAT SATISFIES THE CIRCUIT.  For such a witness the commitments are the same group elements
 * and the proof the same bytes.  For any other witness the round-1 commitments may differ from the reference's; the
 * quotient is still computed from the true wire polynomials, so such a proof is refused exactly as without the route
 * (ZKT_ERR_QUOTIENT_TOO_SHORT).  Nothing is ever proved that the reference would not prove.
 * Taken, per wire, on top of the rules above when the table has fewer than 0.9 of the bases the wire uses otherwise (the
 * constant point counted); a point that has to be a base and is the identity, or a failed allocation, leaves the wire
 * on its other route.  Built with the wire tables (host pass over the rows, then T^k_v of every variable and one
 * double-and-add per non-zero of M on the device), keyed additionally on the proof's public-input positions, which
 * every proof compares on the host: other positions rebuild the tables (a context whose forks read its tables commits
 * densely instead).  Digest, trimmed-length fallback and fork rules are those of the wire tables.
 * zkt_ctx_set_wire_elimination(ctx, mode): 0 = off, 1 = automatic (the default): circuits of 2^17 rows and more, where an
 * MSM's time is its additions, 2 = whenever a table can be built.  Forks inherit the mode. */
int zkt_ctx_set_lagrange(zkt_ctx* ctx, int on);
int zkt_ctx_set_wire_elimination(zkt_ctx* ctx, int mode);
/* The quotient of round 4 on three classes of the 4n coset (single GPU).  The quotient has 3n + 6 coefficients, six of
 * them fixed by the blinded polynomials' top coefficients alone, so its values on the classes 0, 1, 2 of g <w_4n> (the
 * points g w_4n^(j + 4i)) determine it: seven witness polynomials go through three n-point class transforms instead of
 * one of 4n points, the quotient kernel covers 3n points, and three inverse class transforms, one 3 x 3 combination and
 * the six top coefficients (formed on the host from windows of 14 coefficients) give the same 4n coefficients.  The
 * proof bytes are those of the whole-coset route.  An unsatisfied circuit, which the whole coset shows as coefficients
 * above 3n + 5, is refused through the verifier's identity at xi instead (r(xi) against the constant of compute_r0), with
 * the same code, ZKT_ERR_QUOTIENT_TOO_SHORT.  Costs [3][n] class copies of the twelve coset tables (36 n elements of
 * device memory, made by the first proof that takes the route; forks made afterwards share them).
 * zkt_ctx_set_quotient_route(ctx, mode): 0 = automatic (the default): three classes for single-GPU circuits of 2^18 rows
 * and more, 1 = three classes, 2 = the whole coset.  A sharded context always uses the whole coset (each GPU its class).
 * Forks inherit the mode. */
int zkt_ctx_set_quotient_route(zkt_ctx* ctx, int mode);
/* Fused streaming passes of the prover (single launches where the reference sequence makes several and stores vectors
 * that the next kernel reads back).  Round 5: each opening's linear combination, r included, is one pass that also scales
 * by xi^i; r(xi) of the three-classes route is the total of the division's suffix sums minus the evaluations the host
 * holds, not a second evaluation; the scan's block prefixes are added by the kernel that scales by xi^-(j+1).  Round 3:
 * each grand product is one kernel that forms the terms and scans them within blocks, the scan of the block totals,
 * and one kernel that applies prefixes and inverted total (the four scans of the block totals of both grand products are
 * one launch where each is a single block).  Blinding: one launch per batch of polynomials finds the trimmed lengths and
 * places the blinders.  Round 4 on the three-classes route: the three class transforms of a batch are one launch per
 * pass and the quotient kernel one launch (the class is a dimension of the grid), and one closing pass turns the three
 * inverse transforms into the quotient's 4n coefficients and its three chunks (the combination, the split and the zeros
 * above 3n + 5, which are then not scanned).  The proof bytes, the error codes and the trimmed-length slots are the
 * same in every mode.
 * zkt_ctx_set_fused_passes(ctx, mode): 0 = automatic (the default: fused), 1 = fused, 2 = one launch per step, the
 * sequence the fused one is tested against.  zkt_debug_grand_products follows the mode.  Sharded contexts honour it like
 * any other context.  Forks inherit the mode. */
int zkt_ctx_set_fused_passes(zkt_ctx* ctx, int mode);
/* *log_n = domain the table serves (-1: none, evaluations go through their coefficients), *bases = its points */
int zkt_lagrange_info(zkt_ctx* ctx, int* log_n, size_t* bases);
/* PC::commit of poly_from_evals(domain, evals) (util.rs:63-86) with k in 0..3 blinders added as add_blinders_to_poly
 * does (prove.rs:472-483); the domain is the loaded circuit's.  d_evals: n elements in HBM; blinders: k x 4 words,
 * host.  path 0 = through the coefficients (the reference's route), 1 = through the Lagrange-basis table (built if
 * need be; ZKT_ERR_NOT_LOADED when the key cannot carry one).  Both give the same affine point (x || y Montgomery
 * limbs on the host, (0,0) and *out_is_infinity = 1 for the identity).  Synchronises the stream. */
int zkt_commit_evals_dev(zkt_ctx* ctx, const void* d_evals, const uint64_t* blinders, int k, int path, uint64_t* out_xy_mont,
                         int* out_is_infinity);

/* ---- Fiat-Shamir transcripts (host side; T: TranscriptProtocol, plonk-core/src/transcript.rs:16-45) */
enum {
    ZKT_TRANSCRIPT_MERLIN = 0,   /* MerlinTranscript, plonk-core/src/transcript.rs:46-109 (merlin 3.0) */
    ZKT_TRANSCRIPT_ETHEREUM = 1  /* EthereumTranscript, gadgets/src/transcript.rs:8-90 (BN254 only)   */
};
typedef struct zkt_transcript zkt_transcript;
/* T::new(label) (plonk.rs:105).  Scalars/coordinates are canonical little-endian bytes here. */
zkt_transcript* zkt_transcript_new(int kind, const char* label);
void zkt_transcript_free(zkt_transcript* t);
void zkt_transcript_append_u64(zkt_transcript* t, const char* label, uint64_t v);            /* transcript.rs:58-60 */
/* count scalars of 32 bytes; single != 0 mirrors append_scalar, 0 mirrors append_scalars (transcript.rs:62-79) */
void zkt_transcript_append_scalars(zkt_transcript* t, const char* label, const uint8_t* le32, size_t count, int single);
void zkt_transcript_append_commitment(zkt_transcript* t, const char* label, const uint8_t* x_le, const uint8_t* y_le,
                                      size_t fq_bytes, int is_infinity);                      /* transcript.rs:81-86 */
void zkt_transcript_challenge_scalar(zkt_transcript* t, const char* label, int fr_bits, uint8_t out_le32[32]); /* :101-108 */
/* VerifierKey::seed_transcript (proof_system/keys/mod.rs:260-275) in one call: circuit_size, then the ten commitments
 * q_m q_l q_r q_o q_c sigma1 sigma2 sigma3 q_lookup q_table under their "<name>_commit" labels.  xy_le: 10 x (x, y),
 * fq_bytes little-endian canonical bytes per coordinate; is_infinity: 10 flags (may be NULL = none). */
void zkt_transcript_seed(zkt_transcript* t, uint64_t circuit_size, const uint8_t* xy_le, const uint8_t* is_infinity,
                         size_t fq_bytes);
/* raw merlin access (conformance vectors); ZKT_ERR_INVALID_ARGUMENT on a non-merlin transcript */
int zkt_transcript_append_message(zkt_transcript* t, const char* label, const uint8_t* msg, size_t len);
int zkt_transcript_challenge_bytes(zkt_transcript* t, const char* label, uint8_t* out, size_t len);

/* Foreign transcript: the Rust shim implements these four callbacks on top of its own
 * `T: TranscriptProtocol<F, PC::Commitment>`; values cross as arkworks Montgomery limbs. */
typedef struct {
    void* user;
    void (*append_u64)(void* user, const char* label, uint64_t v);
    void (*append_scalars)(void* user, const char* label, const uint64_t* fr_mont, size_t count, int single);
    void (*append_commitment)(void* user, const char* label, const uint64_t* g1_xy_mont, int is_infinity);
    void (*challenge_scalar)(void* user, const char* label, uint64_t* fr_mont_out4);
} zkt_transcript_vtable;

/* ---- Prover: proof_system::prove (plonk-core/src/proof_system/prove.rs:59-470) ---------------- */
/* Loads the preprocessed circuit: the ten ProverKey polynomials in coefficient form
 * (keys/mod.rs:29-77), order q_m, q_l, q_r, q_o, q_c, sigma1, sigma2, sigma3, q_lookup, q_table, each
 * pk_lens[k] <= n = 2^log_n coefficients (trailing zeros stripped or not).  The ExtendedProverKey
 * (keys/mod.rs:78-174: 13 coset vectors on the 4n domain, sigma / q_lookup evaluations) is derived on
 * the device and stays resident in HBM; it never crosses PCIe. */
int zkt_circuit_load(zkt_ctx* ctx, int log_n, const uint64_t* const* pk_polys, const size_t* pk_lens);

/* proof_system::setup on the device (plonk-core/src/proof_system/setup.rs:42-166): the ten padded evaluation vectors
 * of the SetupComposer in ProverKey order (q_m, q_l, q_r, q_o, q_c, sigma1, sigma2, sigma3, q_lookup, q_table;
 * eval_lens[k] <= n values each, the rest zero - setup.rs:28-35 pad_to) become the ProverKey polynomials (iNTT), the
 * ExtendedProverKey (as in zkt_circuit_load) and the ten VerifierKey commitments (PC::commit, setup.rs:104-121).
 * out_commitments: 10 x (x, y) in arkworks Montgomery limbs (2 x 4 u64 on BN254, 2 x 6 on BLS12-381), (0, 0) and
 * out_is_infinity[k] = 1 for the identity (an all-zero selector).  The circuit is left loaded: zkt_prove can follow.
 * Needs zkt_srs_load with >= n powers.  evals_on_device != 0: the ten entries are device pointers.  The sigma
 * evaluations are the caller's here (permutation/mod.rs compute_all_sigma_evals); zkt_circuit_setup_wiring below makes
 * them on the device from the composer's wiring. */
int zkt_circuit_setup(zkt_ctx* ctx, int log_n, const uint64_t* const* evals, const size_t* eval_lens, int evals_on_device,
                      uint64_t* out_commitments, int* out_is_infinity);

/* compute_all_sigma_evals (permutation/mod.rs:103-177) from the wiring: d_w_l / d_w_r / d_w_o = n_rows variable indices
 * each (ZKT_VARIABLE_ZERO = Variable::Zero), device pointers; d_sigma[3] receive n = 2^log_n Montgomery elements each.
 * Number the wires p = 3 gate + column (Left, Right, Output): a wire maps to the next p of the same variable, the last
 * to the first (the reference's per-variable lists in insertion order, permutation/mod.rs:76-137); wires of rows >=
 * n_rows map to themselves; the value of a target (col, i) is k_col w^i, k = (1, 7, 13) (permutation/constants.rs).
 * On the device: a stable radix sort of the 3 n_rows positions by variable (8 bits a pass, only the passes n_vars
 * needs; deterministic, no result depends on the order of atomics), a neighbour lookup, one evaluation pass.  Scratch
 * (about 16 bytes a wire plus a table of n elements, ~80 MB at n = 2^20) is the call's own and is freed before it
 * returns.  Needs no SRS and no loaded circuit and touches neither (nor the Lagrange tables, nor an announced next
 * proof); works on a forked context; enqueues on the context's stream and synchronises once, at the end.
 * ZKT_ERR_INVALID_DOMAIN_SIZE unless 0 <= log_n <= 25 (positions are 32-bit); ZKT_ERR_INVALID_ARGUMENT for n_rows > n, a
 * null pointer (the wiring may be null when n_rows = 0: the identity permutation) and for an index that is neither
 * < n_vars nor ZKT_VARIABLE_ZERO. */
int zkt_circuit_sigma_dev(zkt_ctx* ctx, int log_n, const uint32_t* d_w_l, const uint32_t* d_w_r, const uint32_t* d_w_o,
                          size_t n_rows, size_t n_vars, void* const* d_sigma);
/* zkt_circuit_setup with sigma1..3 made on the device: evals / eval_lens as there, entries 5, 6, 7 must be NULL / 0.
 * w_l / w_r / w_o: the composer's wiring as in zkt_prove_inputs, host pointers (uploaded here) or, with
 * wiring_on_device != 0, device pointers; the other seven entries are host or device as evals_on_device says.  So
 * setup takes the composer's own data and nothing derived: selectors, table mask, wiring.  Everything else is
 * zkt_circuit_setup: the circuit left loaded, the ten commitments in ProverKey order, the refusal on a context with
 * live forks, sharded contexts (every rank computes the whole sigma vectors; they are replicated like all n-domain
 * work).  ZKT_ERR_INVALID_DOMAIN_SIZE unless 3 <= log_n <= 25; ZKT_ERR_INVALID_ARGUMENT for n_rows > n, a non-NULL
 * entry 5 / 6 / 7, a NULL wiring pointer with n_rows > 0 and an index outside the variable map -- after any of these
 * no circuit is loaded (the previous one is released, as by a failing zkt_circuit_setup).
 * Cost: see docs/EXPERIMENTS.md "sigma from the wiring". */
int zkt_circuit_setup_wiring(zkt_ctx* ctx, int log_n, const uint64_t* const* evals, const size_t* eval_lens,
                             int evals_on_device, const uint32_t* w_l, const uint32_t* w_r, const uint32_t* w_o,
                             size_t n_rows, size_t n_vars, int wiring_on_device,
                             uint64_t* out_commitments, int* out_is_infinity);

typedef struct {
    /* wire_evals() of the proving composer (prove.rs:49-55,116): n_rows <= n values each, zero padded */
    const uint64_t* a_evals;
    const uint64_t* b_evals;
    const uint64_t* c_evals;
    size_t n_rows;
    /* the lookup table as a LookupTable IndexSet (lookup/table.rs:19): distinct values, insertion order.  A value
     * that appears twice -> ZKT_ERR_INVALID_ARGUMENT ("lookup table holds a repeated value"). */
    const uint64_t* table;
    size_t table_len;
    /* PublicInputs BTreeMap (constraint_system/pi.rs:52-105): ascending positions and their values */
    const size_t* pi_pos;
    const uint64_t* pi_vals;
    size_t n_pi;
    /* the 19 F::rand(rng) draws of prove.rs in reference order:
     * a(2) b(2) c(2) h1(3) h2(2) z1(3) z2(3) b0 b1   (prove.rs:125-127,170-171,225,244,296) */
    const uint64_t* blinders;
    /* non-zero: a_evals / b_evals / c_evals are DEVICE pointers (witness already resident in HBM) */
    int wires_on_device;
    /* Alternative to the three evaluation vectors, used when a_evals is NULL: the witness as the composer holds it
     * (prove.rs:49-55 wire_evals runs on the device).  `variables`: n_vars assigned values (var_map, Montgomery
     * form); w_l / w_r / w_o: n_rows variable indices per gate, ZKT_VARIABLE_ZERO = Variable::Zero (value 0,
     * constraint_system/variable.rs:10-15).  An index >= n_vars -> ZKT_ERR_INVALID_ARGUMENT.  wires_on_device
     * applies to these four arrays as well. */
    const uint64_t* variables;
    size_t n_vars;
    const uint32_t* w_l;
    const uint32_t* w_r;
    const uint32_t* w_o;
} zkt_prove_inputs;
#define ZKT_VARIABLE_ZERO 0xFFFFFFFFu

/* Runs the five prover rounds on the device and writes the CanonicalSerialize bytes of
 * Proof<F, D, KZG10<E>> (proof.rs:106-155): 802 bytes on BN254, 1010 on BLS12-381.  The transcript must
 * already be seeded by VerifierKey::seed_transcript (keys/mod.rs:260-275), as in plonk.rs:105-108.
 * Needs zkt_srs_load (>= n + 8 powers) and zkt_circuit_load.  Errors mirror the reference's Err / panics:
 * ZKT_ERR_NOT_IN_TABLE, ZKT_ERR_EQUAL_CHALLENGES, ZKT_ERR_ZERO_DENOMINATOR, ZKT_ERR_QUOTIENT_TOO_SHORT.
 * Challenge values that are refused, as the reference refuses them (tests/forced_challenges.py holds the table):
 *  - two of beta, gamma, delta, epsilon equal (any of the six pairs): ZKT_ERR_EQUAL_CHALLENGES, in round 3
 *    (assert_ne!, prove.rs:202-207);
 *  - a denominator of the permutation or the lookup grand product that vanishes at a row 0 .. n - 2 -- for one of the
 *    three factors beta sigma_k(w^i) + wire_i + gamma, or for epsilon (1 + delta) + h1_i + delta h2_i or its neighbour;
 *    epsilon = 0 and delta = -1 do wherever h1_i = h2_i = 0 resp. h1_i = h2_i, which the zeros of the padded table bring
 *    about: ZKT_ERR_ZERO_DENOMINATOR, after the scans of round 3.  Row n - 1 enters no product: a zero there proves;
 *  - alpha = 0, and beta = 0 with blinders (z1 = 1 is trimmed and its blinders land at X^1..X^3): the quotient is too short
 *    or no polynomial, ZKT_ERR_QUOTIENT_TOO_SHORT, reported with the evaluations of round 5 (for beta = 0 the reference
 *    fails later, committing q_hi, with TooManyCoefficients);
 *  - xi = 1 (L_1(xi) divides by n (xi - 1)): ZKT_ERR_ZERO_DENOMINATOR, in round 5.
 * Everything else is proved, in particular xi on the domain (Z_H(xi) = 0), xi w = 1, xi = 0 (the opening witnesses are then
 * the combinations shifted down by one coefficient), eta in {0, 1}, alpha = 1, gamma = 0, delta = 0.  A refusal withdraws
 * an announced successor (zkt_prove_set_next) and leaves the context ready for the next proof.
 * A device witness (wires_on_device != 0) is read behind the work already on the context's stream.  The proof goes to
 * host memory and the transcript is fed on the host between the rounds.  Synchronises the stream. */
int zkt_prove(zkt_ctx* ctx, const zkt_prove_inputs* in, zkt_transcript* transcript, uint8_t* proof_out,
              size_t proof_cap, size_t* proof_len);
/* Optional, for back-to-back proofs on one context: announces the inputs of the proof that will follow the next
 * zkt_prove / zkt_prove_with call.  Rounds 1 and 2 (prove.rs:116-185) need no challenge, so that call issues them for
 * `next` behind its own quotient commitments (round 1) and opening commitments (round 2): their bucket reductions
 * are latency-bound and leave the GPU nearly empty otherwise, and it no longer drains between the two proofs.  The following zkt_prove must
 * be given the same inputs (same pointers and sizes; the data they point to must stay unchanged meanwhile) - otherwise
 * the early work is simply redone.  NULL withdraws the announcement.  Proof bytes are the same either way.
 * The call itself only records the announcement: nothing is enqueued, no synchronisation; the announced device
 * witness is first read by that next zkt_prove, behind the work on the context's stream at that time. */
int zkt_prove_set_next(zkt_ctx* ctx, const zkt_prove_inputs* next);
int zkt_prove_with(zkt_ctx* ctx, const zkt_prove_inputs* in, const zkt_transcript_vtable* transcript,
                   uint8_t* proof_out, size_t proof_cap, size_t* proof_len);

/* check_gate of the reference's circuit debugger (plonk-core/src/constraint_system/helper.rs:13-75, the
 * check_circuit_satisfied of its README and gate tests) on the device: which rows of a witness break the loaded circuit,
 * by which rule, and how many.  zkt_prove only reports THAT a witness is bad (ZKT_ERR_QUOTIENT_TOO_SHORT after four
 * rounds, ZKT_ERR_NOT_IN_TABLE), never where.  One deliberate difference: the reference's loop is zipped with
 * setup.pp.get_pos() and so stops after as many rows as there are public inputs; this call checks every row.
 * `in` is what zkt_prove takes, in either witness form (a_evals / b_evals / c_evals, or variables + w_l / w_r / w_o when
 * a_evals is NULL; wires_on_device selects host or device pointers); blinders is ignored and may be NULL.  All
 * n = 2^log_n rows of the loaded circuit are checked; rows >= n_rows carry zero wires, as the prover pads them.
 *   arithmetic (bit 0): q_m a b + q_l a + q_r b + q_o c + q_c + pi != 0, pi = pi_vals[k] at row pi_pos[k], 0 elsewhere
 *                       (a wrong public input shows up as a failure at its row);
 *   lookup (bit 1):     q_lookup c is non-zero and not among table[0 .. table_len) (zero always passes: the prover pads
 *                       the table with zeros; table_len = 0 is allowed);
 *   wiring (bit 2):     only with ZKT_CHECK_WIRING, only for the variables form (ZKT_ERR_INVALID_ARGUMENT with a_evals
 *                       set): the sigma evaluations made from w_l / w_r / w_o (the launches of zkt_circuit_sigma_dev)
 *                       against the loaded key's, element by element over the 3n wires -- "is this the wiring the key
 *                       was made from".  The bare evaluation form has no wiring to check: `checked` then lacks bit 2,
 *                       and copy constraints between its rows are NOT verified.
 * Returns ZKT_OK whenever the check ran: an unsatisfied witness is a result, not an error.  Errors:
 * ZKT_ERR_NOT_LOADED without a circuit; ZKT_ERR_INVALID_ARGUMENT for NULL in / out, unknown flag bits, n_rows > n,
 * table_len >= n, a repeated table value, a public-input position >= n, and an index that is neither < n_vars nor
 * ZKT_VARIABLE_ZERO.  On any error *out is left untouched.
 * Needs no SRS; works on a forked context and on one with a communicator (local and replicated, no collective).  Leaves
 * the circuit's work buffers, the resident lookup keys, the Lagrange and wire tables and a proof announced with
 * zkt_prove_set_next untouched (that proof's bytes do not change).  The selector evaluations are made per call from the
 * key's coefficients (five n-point transforms) into the call's own scratch: 5 n x 32 B for them, plus the sorted table,
 * a host witness's copy and, with ZKT_CHECK_WIRING, 3 n x 32 B and the sort's ~16 B a wire and n x 32 B; grown on demand,
 * freed by zkt_ctx_destroy.  Enqueues on the context's stream and synchronises once, at the end. */
enum {                              /* flags */
    ZKT_CHECK_WIRING = 1            /* also compare the given wiring with the loaded key's permutation */
};
#define ZKT_CHECK_NONE ((uint64_t)-1)
typedef struct {
    int satisfied;                  /* 1 iff every count below is 0 */
    int checked;                    /* bit 0 arithmetic, bit 1 lookup, bit 2 wiring: which rules ran */
    uint64_t n_arithmetic;          /* rows whose gate equation is not 0 */
    uint64_t first_arithmetic;      /* smallest such row, ZKT_CHECK_NONE when there is none */
    uint64_t residual[4];           /* the gate equation's value at first_arithmetic, Montgomery limbs (0 when none) */
    uint64_t n_lookup;              /* rows with q_lookup c != 0 and not in the table */
    uint64_t first_lookup;
    uint64_t n_wiring;              /* wires (column, row) whose sigma differs from the key's */
    uint64_t first_wiring_row;      /* smallest wire in the order p = 3 row + column; ZKT_CHECK_NONE when none */
    int first_wiring_column;        /* 0 Left, 1 Right, 2 Output; -1 when none */
} zkt_witness_report;
int zkt_circuit_check_witness(zkt_ctx* ctx, const zkt_prove_inputs* in, int flags, zkt_witness_report* out);

/* The same check over a batch of variable maps that share one wiring -- what one zkt_witness_complete_enqueue leaves in
 * HBM.  A completion satisfies every defining row by construction; whether a witness is good is decided by the rows that
 * define nothing (equal_constrain, boolean rows, public rows, the lookup), and this call judges all of them for the whole
 * batch: one set of selector transforms and one synchronisation, where a loop of the single call makes `batch` of each.
 * out[w] equals, field for field (counts, first rows, residual, checked, satisfied), what zkt_circuit_check_witness reports
 * for witness w alone, given w's map, its public inputs, its table and the same flags.  Errors and refusals are those of
 * the single call, applied to the whole batch (a repeated value in any table, an index outside the map, ...); in addition
 * ZKT_ERR_INVALID_ARGUMENT for batch = 0, batch > ZKT_WITNESS_BATCH_MAX, stride < n_vars, n_tables not 0, 1 or batch, and
 * a NULL d_pi_vals with n_pi > 0.  On an error no report is written.  ZKT_CHECK_WIRING concerns the shared wiring: it is
 * checked once and its three fields are copied into every report.
 * Kernels (csrc/check.hip): a thread loads its row's selectors, wire indices and public-input slot once and walks a tile of
 * witnesses (the batch is the launch's second dimension); one status block per witness, filled with sums and minima
 * (vector atomics), so no result depends on an order.  Enqueues on the context's stream behind whatever is there -- a
 * completion in particular, without a wait in between -- and synchronises once, at the end.  Works on a fork and under a
 * communicator (local, no collective); leaves an announced proof (zkt_prove_set_next) untouched, as the single call does.
 * The name carries no _dev suffix although the maps are device pointers: the call synchronises and returns host reports. */
typedef struct {
    const void* d_variables;        /* DEVICE: witness w = d_variables + w * stride scalars, as the completion leaves them */
    size_t stride, batch, n_vars;   /* 1 <= batch <= ZKT_WITNESS_BATCH_MAX, stride >= n_vars */
    const uint32_t *w_l, *w_r, *w_o; size_t n_rows; int wiring_on_device;   /* one wiring for the whole batch */
    const size_t* pi_pos; size_t n_pi;
    const void* d_pi_vals;          /* DEVICE: batch x n_pi, in the order of pi_pos: what zkt_witness_complete_enqueue writes */
    const uint64_t* const* tables; const size_t* table_lens; size_t n_tables;   /* HOST; 0, 1 (shared) or batch (one each) */
} zkt_witness_batch;
int zkt_circuit_check_witness_batch(zkt_ctx* ctx, const zkt_witness_batch* in, int flags, zkt_witness_report* out /* batch */);

/* ---- Witness completion from the circuit's free variables: the solving half of the check above ----------------------
 * The caller uploads the values of the free variables (for a circuit written against the reference's composer: its direct
 * assign_variable calls, less the two that should_be_zero_with_output makes when the plan is created with
 * ZKT_WITNESS_RULE_IS_ZERO); the device fills in every variable that a gate defines and returns the public inputs the
 * witness implies.  Nothing is assumed about the circuit beyond the rule below, which is part of this interface.
 *
 * THE RULE.  Row i asserts q_m a b + q_l a + q_r b + q_o c + q_c + PI_i = 0 (composer.rs:170-199), a, b, c the values of
 * w_l[i], w_r[i], w_o[i].  The rows are walked in ascending order.  A variable is "unseen" at row i if it stands on no wire of
 * a row before i.  ZKT_VARIABLE_ZERO and rows >= n_rows define nothing.
 *  - A public-input row (i among pi_pos) defines nothing.  Its public input is an output:
 *        PI_i = -(q_m a b + q_l a + q_r b + q_o c + q_c)                       (set_variable_public, mod.rs:216-240).
 *  - Rule Z (the is-zero pair), only for a plan made with ZKT_WITNESS_RULE_IS_ZERO (zkt_witness_plan_create_ex), tried at
 *    row i before rule O.  It fires when neither row i nor row i + 1 is a public-input row, i + 1 < n_rows; row i has wires
 *    (x, y, z) with q_m != 0, q_o != 0, q_l = q_r = 0 (q_c arbitrary); y and z are real variables, unseen at row i, distinct
 *    from each other and from x; x is any real variable or ZKT_VARIABLE_ZERO; and row i + 1 has wires
 *    (x, z, ZKT_VARIABLE_ZERO) with q_m != 0 and q_l = q_r = q_o = q_c = 0 (it asserts x z = 0).  Row i then defines both:
 *        x = 0:   y = 0,  z = -q_c / q_o;          x != 0:   z = 0,  y = -q_c / (q_m x).
 *    With the reference's selectors (q_m = 1, q_o = 1, q_c = -1) this is should_be_zero_with_output and should_eq_with_output
 *    (mod.rs:243-289): y = x^-1 or 0 (inverse().unwrap_or_default()), z = (x == 0).  The two equations admit no other z, and
 *    another y only at x = 0, where the reference's own choice, 0, is taken: the rule is never unsolvable.  Row i + 1 defines
 *    nothing; level(y) = level(z) = 1 + level(x).  If any clause fails, the rows fall through to rules O and R as without the
 *    bit.  The rule is opt-in because a mul_gate on a first-seen right operand followed by a row asserting x out = 0 has the
 *    same shape: without the bit that right operand is the caller's to supply, with it the device chooses it.
 *  - Rule O.  Otherwise, if q_o[i] != 0 and v = w_o[i] is a real variable, unseen, and different from w_l[i] and w_r[i], the
 *    row defines   v = -(q_m a b + q_l a + q_r b + q_c) / q_o.   This covers add, sub, mul, square and linear_transform
 *    (arithmetic.rs:15-104, :138-200), the three rows of conditional_select (mod.rs:318-373), bits_le (mod.rs:175-213) and
 *    the lookup copy (mod.rs:140-160).
 *  - Rule R.  Otherwise, if v = w_r[i] is a real variable, unseen, and different from w_l[i] and w_o[i], and w_l[i] and
 *    w_o[i] are each ZKT_VARIABLE_ZERO or already seen, the row defines   v = -(q_l a + q_o c + q_c) / (q_m a + q_r).
 *    This is the div_gate (arithmetic.rs:104-130).  A zero denominator is a property of the witness, not an error of the
 *    call: v is written as 0 and the row is reported (zkt_witness_complete_status).
 *  - Everything else is free: every other variable first seen on some wire is the caller's to supply.  A boolean row
 *    (x, x, x) (boolean.rs:26-34) defines nothing, by the "different from" clauses.  A variable on no wire is never touched.
 *  - There is no left-wire rule: no gate of the reference needs one.
 * The level of a defined variable is 1 + the largest level of the two other wires of its row; free variables and
 * ZKT_VARIABLE_ZERO have level 0.  Lookup-table membership is not looked at (that is zkt_circuit_check_witness's job).
 *
 * Schedule and launches (csrc/witness_plan.hpp, csrc/witness_plan.hip): the defining rows sorted by level; a level with
 * many rows is one launch with a thread per (witness, row), a run of narrower levels is one launch of one 256-thread
 * workgroup per witness that walks the levels behind a workgroup barrier; more than 64 such launches fall back to a single
 * narrow one.  Inside a launch a value written is read only by the workgroup that wrote it: no grid barrier, no flags, no
 * atomics on values.  A closing launch computes the public inputs.  Measured on an MI355X (docs/EXPERIMENTS.md, "witness
 * completion from the free variables"): the BN254 2^20 withdrawal (depth 33 853) in 78.9 ms at batch 1, 85.2 ms at batch 64;
 * the time follows the depth (2.3 us a level), hardly the batch.  Scope "witness_complete" of zkt_profile_get.
 * Everything in canonical Montgomery words, as the prover requires them. */
#define ZKT_WITNESS_BATCH_MAX 256                  /* most witnesses one completion takes */
typedef struct zkt_witness_plan zkt_witness_plan;
typedef struct {
    uint64_t n_free;                /* variables the caller supplies */
    uint64_t n_out;                 /* defined by rule O */
    uint64_t n_right;               /* defined by rule R */
    uint64_t n_unused;              /* on no wire */
    uint32_t depth;                 /* the largest level */
    uint32_t max_level_rows;        /* rows of the widest level */
    uint32_t launches;              /* launches that fill the map under the current split (the closing one not counted) */
    uint32_t reserved;              /* the number of rule-Z pairs (two variables each); 0 for every plan made without the bit */
    uint64_t device_bytes;          /* 32 B a scheduled row + 160 B a distinct coefficient tuple + 4 B a level + 192 B a
                                     * public input + 16 B x ZKT_WITNESS_BATCH_MAX of status, each rounded up to 256 B */
} zkt_witness_plan_report;
typedef struct {
    uint64_t n_unsolvable;          /* rule-R rows whose denominator was 0 */
    uint64_t first_unsolvable;      /* the smallest such row, ZKT_CHECK_NONE when there is none */
} zkt_witness_status;
/* Plans the circuit loaded in `ctx` (its selectors: the evaluations are made from the key's coefficients as
 * zkt_circuit_check_witness makes them) under the wiring w_l / w_r / w_o (n_rows indices each, host pointers, or device
 * pointers with wiring_on_device != 0: what zkt_prove_inputs carries) and the ascending public-input positions pi_pos.
 * The plan copies all it needs and owns its device memory: a later zkt_circuit_load does not affect it, and any context of
 * the same curve and device may complete with it -- a fork, a context with a communicator (the call is local, no
 * collective).  Synchronises.  ZKT_ERR_NOT_LOADED without a circuit; ZKT_ERR_INVALID_ARGUMENT for n_rows > n, an index that
 * is neither < n_vars nor ZKT_VARIABLE_ZERO, a position >= n, unsorted or repeated positions, NULL wiring with n_rows > 0. */
int zkt_witness_plan_create(zkt_ctx* ctx, const uint32_t* w_l, const uint32_t* w_r, const uint32_t* w_o, size_t n_rows,
                            size_t n_vars, int wiring_on_device, const size_t* pi_pos, size_t n_pi, zkt_witness_plan** out);
/* The same with a choice of rules: rules = 0 is zkt_witness_plan_create, bit for bit; ZKT_WITNESS_RULE_IS_ZERO adds rule Z
 * above.  Unknown bits: ZKT_ERR_INVALID_ARGUMENT. */
enum { ZKT_WITNESS_RULE_IS_ZERO = 1 };   /* rules */
int zkt_witness_plan_create_ex(zkt_ctx* ctx, const uint32_t* w_l, const uint32_t* w_r, const uint32_t* w_o, size_t n_rows,
                               size_t n_vars, int wiring_on_device, const size_t* pi_pos, size_t n_pi, uint32_t rules,
                               zkt_witness_plan** out);
/* Waits for ctx's stream (NULL: no wait), then frees the plan and its device memory. */
void zkt_witness_plan_free(zkt_ctx* ctx, zkt_witness_plan* plan);
int zkt_witness_plan_info(const zkt_witness_plan* plan, zkt_witness_plan_report* info);
/* Per variable: 0 on no wire, 1 free, 2 defined by rule O, 3 defined by rule R, 4 rule Z's inverse y, 5 rule Z's flag z.
 * n_vars bytes. */
int zkt_witness_plan_kinds(const zkt_witness_plan* plan, uint8_t* out_kind);
/* Completes `batch` witnesses in DEVICE memory: witness w is d_variables + w * stride scalars, stride >= n_vars; only the
 * defined variables are written, free ones, those on no wire and the padding up to stride stay as they are.  d_out_pi
 * (optional, DEVICE): batch x n_pi scalars in position order.  1 <= batch <= ZKT_WITNESS_BATCH_MAX.  Enqueue only: no
 * allocation, no synchronisation, on the context's stream, so zkt_prove with wires_on_device follows without a wait. */
int zkt_witness_complete_enqueue(zkt_ctx* ctx, const zkt_witness_plan* plan, void* d_variables, size_t stride, size_t batch,
                             void* d_out_pi);
/* Synchronises and returns, per witness of the completions enqueued since the last such call, the rule-R rows with a zero
 * denominator; clears the block.  Completions on several contexts share the plan's one block. */
int zkt_witness_complete_status(zkt_ctx* ctx, const zkt_witness_plan* plan, size_t batch, zkt_witness_status* out);
/* The host-pointer form: uploads batch x stride scalars, completes, downloads them (and out_pi, out_status when not NULL),
 * synchronises. */
int zkt_witness_complete(zkt_ctx* ctx, const zkt_witness_plan* plan, uint64_t* variables, size_t stride, size_t batch,
                         uint64_t* out_pi, zkt_witness_status* out_status);

/* ---- Witness synthesis for Poseidon-heavy circuits as batched field kernels ----------------------
 * (1) The permutation of plonk-hashing/src/hasher/poseidon/spec.rs (rounds :18-111, schedule :267-316, input layout
 * :239-265: state[0] = domain_tag, the inputs follow, output = state[1]) for `batch` independent hashes, one thread per
 * hash: what NativePlonkSpecRef computes.  out_states (optional) receives every round's state, batch x (rounds + 1) x
 * width scalars -- ROUND STATES ONLY: they are not the variables of the in-circuit gadget (that is (2) below).
 * Constants are the caller's PoseidonConstants (the reference generates them at run time, constants.rs:27, or parses the
 * BN254 tables of gadgets/src/poseidon).  Everything in Montgomery limbs; host pointers. */
typedef struct {
    int width;                       /* 2 .. 8 */
    int half_full_rounds;            /* full rounds before and after the partial ones */
    int partial_rounds;
    const uint64_t* round_constants; /* (2 half_full + partial) x width */
    const uint64_t* mds;             /* width x width, row major: m[i][j] */
    const uint64_t* domain_tag;      /* one scalar */
} zkt_poseidon_params;
int zkt_poseidon_hash_batch(zkt_ctx* ctx, const zkt_poseidon_params* params, const uint64_t* inputs, size_t batch, int arity,
                            uint64_t* out_hashes, uint64_t* out_states);
/* The same with everything resident in HBM: zkt_poseidon_load uploads the parameters once (as the kernel's own 29-bit
 * limbs), zkt_poseidon_hash_batch_dev takes DEVICE pointers, allocates nothing and enqueues on the context's stream
 * without synchronising.  d_out_states: optional, batch x (rounds + 1) x width scalars (round states, see above).
 * half_full_rounds >= 1 and partial_rounds >= 1 (output_hash, spec.rs:267-316, always runs one of each before its loops). */
typedef struct zkt_poseidon zkt_poseidon;
int zkt_poseidon_load(zkt_ctx* ctx, const zkt_poseidon_params* params, zkt_poseidon** out);
void zkt_poseidon_free(zkt_ctx* ctx, zkt_poseidon* params);
int zkt_poseidon_hash_batch_dev(zkt_ctx* ctx, const zkt_poseidon* params, const void* d_inputs, size_t batch, int arity,
                                void* d_out_hashes, void* d_out_states);

/* (2) The WITNESS of the in-circuit gadget PoseidonRef<ConstraintSystem, PlonkSpecRef, _, WIDTH>::hash (spec.rs:174-219,
 * 343-375).  While the reference's composer synthesises one hash it assigns a fresh variable per gate
 * (constraint_system/arithmetic.rs:19,79; variable.rs:117-126): power_of_5 is three mul_gates (x^2, x^4, x^5;
 * spec.rs:107-111), every term of product_mds an add_gate (the W^2 running sums, j outer, i inner; spec.rs:73-88);
 * add_constant / mul_constant allocate nothing (lazy LTVariable transforms, variable.rs:77-86).  That is
 *     zkt_poseidon_gadget_vars_per_hash = 2 half_full (3 W + W^2) + partial (3 + W^2)      (804 / 1288 / 1888 for x3 / x4 / x5)
 * variables per hash, consecutive in VariableMap::values.  This entry point computes exactly those values for `batch`
 * independent hashes and writes them, in allocation order, into the variable map the prover gathers its wires from
 * (zkt_prove_inputs.variables with wires_on_device = 1): hash h fills d_variables[base .. base + vars_per_hash) with
 * base = d_trace_base[h], or trace_base0 + h * vars_per_hash when d_trace_base is NULL.  The hash value (elements[1] after
 * the last round, spec.rs:315) is the variable at base + vars_per_hash - 1 - (W - 2) W; d_out_hashes (optional) receives
 * it as well.  Inputs are plain variables (coeff 1, offset 0: every call site of circuits/src/withdraw.rs and
 * plonk-hashing/src/merkle/binary.rs): their VALUES in d_inputs (batch x arity), or their INDICES into d_variables in
 * d_input_vars (ZKT_VARIABLE_ZERO = Variable::Zero) -- exactly one of the two.  Hashes of one launch are independent:
 * an input may not be a variable the same launch writes.  Device pointers, no allocation, no synchronisation; a trace
 * base or input index outside [0, n_vars) makes the kernel skip that hash and raise a flag that
 * zkt_poseidon_gadget_check (which synchronises the stream) turns into ZKT_ERR_INVALID_ARGUMENT.
 * "Parity unpinned": the reference holds no known answer for the gadget; tests compare with the oracle's gate-by-gate
 * restatement of the composer. */
typedef struct {
    size_t batch;
    int arity;                      /* inputs per hash, <= width - 1 */
    const void* d_inputs;           /* batch x arity scalars, or NULL */
    const uint32_t* d_input_vars;   /* batch x arity variable indices, or NULL */
    void* d_variables;              /* VariableMap::values, n_vars scalars */
    size_t n_vars;
    const uint32_t* d_trace_base;   /* per hash, or NULL */
    size_t trace_base0;
    void* d_out_hashes;             /* optional: batch scalars */
    int kernel;                     /* 0: chosen by batch size; 1: one thread per hash (throughput: large batches);
                                     * 2: width^2 lanes per hash (latency: a single proof's few hundred hashes) */
} zkt_poseidon_gadget_args;
size_t zkt_poseidon_gadget_vars_per_hash(const zkt_poseidon* params);
int zkt_poseidon_gadget_witness_dev(zkt_ctx* ctx, const zkt_poseidon* params, const zkt_poseidon_gadget_args* args);
int zkt_poseidon_gadget_check(zkt_ctx* ctx, const zkt_poseidon* params);
/* Optional validation of ONE launch's arguments on the host (downloads the index vectors, synchronises): the traces must
 * be pairwise disjoint and inside the map and no input index may be a variable the same launch writes -- the two rules
 * zkt_poseidon_gadget_witness_dev cannot afford to check per proof and whose violation yields a stale or racy witness
 * (the proof then fails to verify).  ZKT_ERR_INVALID_ARGUMENT names the rule.  Run it once per circuit layout. */
int zkt_poseidon_gadget_validate(zkt_ctx* ctx, const zkt_poseidon* params, const zkt_poseidon_gadget_args* args);

/* (3) The WITNESS of the Merkle-path gadget merkle_proof (plonk-hashing/src/merkle/binary.rs:8-30) for `batch` paths of
 * `height` levels, ONE launch: a chain in which each level hashes two conditional_selects of the level below, so it cannot
 * be a launch of independent hashes unless the host walks every path first.  Per level, for the bit b, the sibling s and
 * the running hash cur (the leaf at level 0), the composer allocates, in this order (constraint_system/mod.rs:339-354 for
 * one select, binary.rs:23-24 for the two),
 *     x_l = b s, y_l = (1 - b) cur, z_l = x_l + y_l,   x_r = b cur, y_r = (1 - b) s, z_r = x_r + y_r,
 * and then the zkt_poseidon_gadget_vars_per_hash variables of hash_two(z_l, z_r) (hasher/mod.rs:26-33: arity 2).  A level is
 *     zkt_merkle_path_vars_per_level = 6 + zkt_poseidon_gadget_vars_per_hash
 * consecutive variables, a path `height` consecutive levels: path p fills d_variables[base .. base + height *
 * vars_per_level) with base = d_path_base[p], or path_base0 + p * height * vars_per_level when d_path_base is NULL.  The
 * root is the hash variable of the last level, base + (height - 1) * vars_per_level + 6 + (vars_per_hash - 1 - (W - 2) W);
 * d_out_roots (optional) receives it as well.  The running hash stays in registers: the kernel reads no variable it wrote.
 * Inputs are plain variables (coeff 1, offset 0: binary.rs:42-78 assigns the bits and the siblings itself, and every caller
 * in circuits/src/withdraw.rs passes a hash variable as the leaf), given as INDICES into d_variables
 * (ZKT_VARIABLE_ZERO = Variable::Zero reads as 0).  A leaf, bit or sibling may not be a variable the same launch writes.
 * width >= 3 (hash_two on width 2 is FullBuffer, spec.rs:253-257) and height >= 0, else ZKT_ERR_INVALID_ARGUMENT; batch =
 * 0 or height = 0 enqueues nothing.  Device pointers, no allocation, no synchronisation.  A path whose range leaves
 * [0, n_vars), one of whose indices is neither < n_vars nor ZKT_VARIABLE_ZERO, or one of whose bits holds a value other
 * than 0 or 1 (conditional_select asserts that; the library never aborts) is skipped as a whole -- nothing of it is
 * written, the other paths of the launch are unaffected -- and raises the flag zkt_poseidon_gadget_check reports.
 * Cost: the levels of a path are serial, one permutation's latency each whatever the batch -- measured 0.22-0.23 ms per
 * level on an MI355X, 14.8 ms for 8 paths of 64 levels on Bn254x5 (docs/EXPERIMENTS.md, "Merkle path on the device"). */
typedef struct {
    size_t batch;
    int height;
    void* d_variables;               /* VariableMap::values, n_vars scalars */
    size_t n_vars;
    const uint32_t* d_leaf_var;      /* batch */
    const uint32_t* d_bit_vars;      /* batch x height, level 0 first */
    const uint32_t* d_sibling_vars;  /* batch x height */
    const uint32_t* d_path_base;     /* batch, or NULL */
    size_t path_base0;
    void* d_out_roots;               /* optional: batch scalars */
} zkt_merkle_path_args;
size_t zkt_merkle_path_vars_per_level(const zkt_poseidon* params);
int zkt_poseidon_merkle_path_witness_dev(zkt_ctx* ctx, const zkt_poseidon* params, const zkt_merkle_path_args* args);
/* Optional validation of ONE launch's arguments on the host (downloads the index vectors, synchronises): the paths' ranges
 * must be pairwise disjoint and inside the map, and no leaf, bit or sibling index may lie inside a range the launch
 * writes.  ZKT_ERR_INVALID_ARGUMENT names the rule.  Run it once per circuit layout. */
int zkt_poseidon_merkle_path_validate(zkt_ctx* ctx, const zkt_poseidon* params, const zkt_merkle_path_args* args);

/* (4) The note tree itself: MerkleTree<F, G, H, HEIGHT> (gadgets/src/merkle_tree.rs:39-111) kept in HBM and appended to
 * there.  The reference's add_leaf (merkle_tree.rs:89-106) walks HEIGHT hash_two calls per leaf, one after the other; m
 * appended leaves need only ~2 m + HEIGHT hashes, at most HEIGHT of them dependent, because the tree after add_leaf of
 * leaves 0 .. n - 1 is the dense one in which every stored node (layer, idx), idx < ceil(n / 2^layer), is hash_two of its two
 * children with nodes[layer - 1] standing in for a right child that does not exist yet.  Levels with many parents are one
 * launch each (a thread per parent), all the narrow ones are ONE launch of one workgroup that walks them with a lane group
 * per parent and passes each level to the next through LDS; the threshold between the two (64 parents) comes from a sweep
 * on an MI355X with the BN254 x5 tables
 * (docs/EXPERIMENTS.md, "note tree on the device").  The siblings merkle_path returns are exactly what
 * zkt_poseidon_merkle_path_witness_dev reads out of the variable map: zkt_merkle_tree_paths_to_variables_dev writes them
 * there without a trip to the host.
 * The handle is bound to a loaded zkt_poseidon, which is BORROWED and must outlive the tree; width >= 3 (hash_two).  Every
 * call enqueues on the stream of the context it is given -- use one context per tree, or order the streams yourself.  Any
 * context will do: forked, with a communicator (the tree is local, no collective is made), with or without SRS or circuit
 * -- the tree touches none of their memory.  Everything in Montgomery words.
 * The reference's serialised MerkleTreeStore file is written and read by zkt_merkle_tree_save_file / _load_file ("(4b) The
 * store files" below).  Out of scope: deleting or updating leaves (the reference has neither); a tree sharded over ranks. */
#define ZKT_MERKLE_TREE_MAX ((size_t)1 << 24)      /* most leaves a tree holds */
#define ZKT_MERKLE_TREE_PATHS_MAX 4096             /* most paths one zkt_merkle_tree_paths* call takes */
typedef struct zkt_merkle_tree zkt_merkle_tree;
/* MerkleTree::new over an empty store (merkle_tree.rs:57-75).  1 <= height <= 64 and 1 <= capacity <= min(2^height,
 * ZKT_MERKLE_TREE_MAX), else ZKT_ERR_INVALID_ARGUMENT; a failed allocation gives ZKT_ERR_HIP.  Layer L (0 <= L < height) is a
 * dense array of max(1, ceil(capacity / 2^L)) scalars, ~2 x capacity x 32 B in all.  The `height` empty-subtree values are
 * computed on the device: nodes[0] = H::empty_hash() = 0, nodes[L + 1] = hash_two(nodes[L], nodes[L]) (merkle_tree.rs:58-67).
 * Synchronises. */
int zkt_merkle_tree_create(zkt_ctx* ctx, const zkt_poseidon* params, int height, size_t capacity, zkt_merkle_tree** out);
void zkt_merkle_tree_free(zkt_ctx* ctx, zkt_merkle_tree* tree);
/* add_leaf (merkle_tree.rs:89-106) for the m scalars of d_leaves (DEVICE memory) in order; *first_index (optional) receives
 * the index of the first, i.e. the number of leaves before the call.  Enqueue only: no allocation, no synchronisation.
 * m = 0: ZKT_OK, nothing enqueued.  count + m > capacity: ZKT_ERR_INVALID_ARGUMENT, the tree unchanged, nothing enqueued.
 * Afterwards every stored node of every layer and the root equal what the reference holds after the same add_leaf calls,
 * however the leaves were split into batches.  ZKT_ERR_HIP (a copy or a launch the runtime refused) leaves the count as it
 * was, but nodes above layer 0 may be half made: free the tree and rebuild it from its leaves.  Measured on an MI355X: docs/EXPERIMENTS.md, "note tree on the device". */
int zkt_merkle_tree_append_dev(zkt_ctx* ctx, zkt_merkle_tree* tree, const void* d_leaves, size_t m, uint64_t* first_index);
/* The same with HOST leaves: uploads them, enqueues as the _dev form does, synchronises. */
int zkt_merkle_tree_append(zkt_ctx* ctx, zkt_merkle_tree* tree, const uint64_t* leaves, size_t m, uint64_t* first_index);
/* MerkleTree::root (merkle_tree.rs:108-110): synchronises and writes four words.  A tree without a leaf has the root 0, as
 * MerkleTreeStore::default().root is (merkle_tree.rs:8-13) -- NOT the hash of an empty tree. */
int zkt_merkle_tree_root(zkt_ctx* ctx, zkt_merkle_tree* tree, uint64_t* out4);
/* Any of the outputs may be NULL.  count: MerkleTreeStore::next_index. */
int zkt_merkle_tree_info(const zkt_merkle_tree* tree, int* height, uint64_t* count, uint64_t* capacity);
/* Downloads the stored nodes (layer, first .. first + n): the content of the reference's BTreeMap<(usize, usize), F>
 * (merkle_tree.rs:10, :94), for persistence and for tests.  Synchronises.  Layer L holds ceil(count / 2^L) nodes; a range
 * that reaches past them, or a layer outside [0, height), gives ZKT_ERR_INVALID_ARGUMENT (layer = height is not a layer: the
 * root has its own call). */
int zkt_merkle_tree_layer(zkt_ctx* ctx, zkt_merkle_tree* tree, int layer, uint64_t first, size_t n, uint64_t* out);
/* merkle_path(index) (merkle_tree.rs:77-87) for k HOST indices: k x height scalars to HOST memory, level 0 first.  Any index
 * below 2^height is valid, as in the reference: the sibling (layer, idx ^ 1), idx = index >> layer, is the stored node when
 * idx ^ 1 < ceil(count / 2^layer) and nodes[layer] otherwise.  An index >= 2^height or k > ZKT_MERKLE_TREE_PATHS_MAX gives
 * ZKT_ERR_INVALID_ARGUMENT; everything is checked on the host before anything is enqueued.  Synchronises. */
int zkt_merkle_tree_paths(zkt_ctx* ctx, zkt_merkle_tree* tree, const uint64_t* indices, size_t k, uint64_t* out_siblings);
/* The same paths written into the prover's variable map (DEVICE memory, n_vars scalars): path p puts its `height` siblings
 * at d_variables[sibling_var0[p] + layer] and, when bit_var0 is not NULL, its position bits (index >> layer) & 1 at
 * d_variables[bit_var0[p] + layer] as the Montgomery 0 or 1 -- where PoECircuit::synthesize (plonk-hashing/src/merkle/
 * binary.rs:42-78) allocates them: `height` consecutive bits, then `height` consecutive siblings.  indices, bit_var0 and
 * sibling_var0 are HOST arrays of k entries, free on return: the small table goes up on the stream from a pinned buffer the
 * tree owns (a second call waits for the first one's table to have left that buffer, nothing else).  Ranges that leave
 * [0, n_vars) or overlap each other, an index >= 2^height and k > ZKT_MERKLE_TREE_PATHS_MAX give ZKT_ERR_INVALID_ARGUMENT
 * before anything is enqueued.  Enqueue only: no allocation, no synchronisation of the stream. */
int zkt_merkle_tree_paths_to_variables_dev(zkt_ctx* ctx, zkt_merkle_tree* tree, const uint64_t* indices, size_t k,
                                           void* d_variables, size_t n_vars, const uint32_t* bit_var0,
                                           const uint32_t* sibling_var0);

/* (4b) The store files: the two files the reference CLI keeps its state in, --merkle-tree (MerkleTreeStore,
 * gadgets/src/merkle_tree.rs:8-13) and --notes (Notes, gadgets/src/note.rs), read by ProveWithdraw, Deposit, InitStore and
 * ListNotes.  Both are serialize_unchecked output (bin/src/parser.rs); the byte layouts (csrc/storefile.hpp) are DERIVED from
 * ark-serialize 0.3's rules, as the key files' are: usize and u64 are 8 bytes little endian, a scalar is 32 canonical
 * little-endian bytes on both curves, a Vec or BTreeMap is a u64 length and then its items (a map's in ascending key order).
 * The reference holds no such file, so no reference-made file has ever been compared ("parity unpinned").
 *   MerkleTreeStore: u64 E; E entries (u64 layer, u64 idx, scalar) in ascending (layer, idx) order; the scalar root; u64
 *                    next_index.  MerkleTreeStore::default() is 48 bytes.  After add_leaf of `count` leaves the map holds, for
 *                    every layer L in [0, HEIGHT), exactly the indices 0 .. ceil(count / 2^L) - 1 (merkle_tree.rs:92-95): what
 *                    zkt_merkle_tree_layer returns.  HEIGHT is not in the file; it is max layer + 1.
 *   Notes:           u64 count; per note u64 leaf_index, scalar identifier, u64 amount, scalar secret (80 bytes).
 * With the key files (zkt_keyfile_*, zkt_srs_*_file, zkt_circuit_*_file) these are all the files of a reference data directory
 * but one: the --cvk file is NOT read or written.  Its type comes from ark-poly-commit, whose source is not in the reference
 * tree, so its layout cannot be derived here.
 *
 * zkt_merkle_tree_save_file: the tree as a MerkleTreeStore file.  Synchronises; the layers come out in bounded chunks through
 * pinned staging, into a temporary sibling of `path` that is renamed into place (a failed call leaves neither).  An empty
 * tree writes the 48-byte default store.  Errors: ZKT_ERR_INVALID_ARGUMENT with the path in the message (also kept for
 * zkt_keyfile_last_error). */
int zkt_merkle_tree_save_file(zkt_ctx* ctx, zkt_merkle_tree* tree, const char* path);
/* What zkt_merkle_tree_load_file found.  entries: the file's E.  mismatches: stored nodes of the file (the root not among
 * them) that differ from the rebuilt tree's; first_layer / first_idx: the smallest such (layer, idx), -1 / 0 when there is
 * none; root_matches: 1 when the file's root is the rebuilt one. */
typedef struct {
    uint64_t entries, mismatches;
    int first_layer;
    uint64_t first_idx;
    int root_matches;
} zkt_tree_file_report;
/* Reads a MerkleTreeStore file into a new tree of (height, capacity) bound to `poseidon` (as zkt_merkle_tree_create; *out is
 * the caller's to free) and checks the file against it, the way zkt_srs_check treats a committer key.  The file is parsed on
 * the host, in chunks; ZKT_ERR_INVALID_ARGUMENT, with a message naming the path and the byte offset, for: a file that is
 * truncated or has trailing bytes (its size is not 48 + 48 E); a scalar not below the modulus; keys that are not ascending;
 * keys that are not exactly the dense set of next_index leaves under `height` (a key outside it, or too few entries);
 * next_index > capacity.  Nothing is created then.  Otherwise layer 0 is uploaded and appended through
 * zkt_merkle_tree_append_dev, so the tree kept is self-consistent whatever the file says above layer 0, and EVERY stored node
 * of every layer and the root are compared with the rebuilt ones on the device: one launch over all the file's nodes (they go
 * up in the same bounded chunks; the file is never whole in host memory), a lane per node.  A mismatch is a finding, not an
 * error: ZKT_OK with the rebuilt tree, and the caller decides.  report may be NULL.  Scratch (48 B per entry and 32 B per
 * leaf) is the call's own and freed before it returns.  Synchronises. */
int zkt_merkle_tree_load_file(zkt_ctx* ctx, const zkt_poseidon* poseidon, int height, size_t capacity, const char* path,
                              zkt_merkle_tree** out, zkt_tree_file_report* report);
/* The --notes file.  Host-only, no context; errors are ZKT_ERR_INVALID_ARGUMENT with the text (path, offset) in
 * zkt_keyfile_last_error.  Scalars are Montgomery words.  Read is two-call: with any output NULL only *count is written;
 * with all four, `cap` notes fit (a file with more -> ZKT_ERR_INVALID_ARGUMENT).  Truncated files, trailing bytes and scalars
 * not below the modulus are refused.  Write goes through a temporary sibling, as the key-file writers do. */
int zkt_notes_read_file(const char* path, int curve_id, size_t cap, uint64_t* out_leaf_indices, uint64_t* out_identifiers_mont,
                        uint64_t* out_amounts, uint64_t* out_secrets_mont, size_t* count);
int zkt_notes_write_file(const char* path, int curve_id, const uint64_t* leaf_indices, const uint64_t* identifiers_mont,
                         const uint64_t* amounts, const uint64_t* secrets_mont, size_t count);

/* (5) The withdraw circuit as a component: WithdrawCircuit<F, u64, G, H, INPUTS, HEIGHT>::synthesize
 * (circuits/src/withdraw.rs:57-150) -- its rows, its setup (the CLI's Compile, bin/src/main.rs:90-112) and the witness of
 * a batch of withdrawals (ProveWithdraw, bin/src/main.rs:190-300), all made on the device.
 * zkt_withdraw_create plans the circuit on the host from (Poseidon parameters, INPUTS, HEIGHT): variable numbering and row
 * order are the reference composer's allocation order.  4 <= width <= 8 (width 3 cannot hash a leaf: three inputs make it
 * FullBuffer), 1 <= inputs <= 32, 1 <= height <= 64, else ZKT_ERR_INVALID_ARGUMENT.  The plan is one gadget template per
 * arity (the rows of one PoseidonRef::hash relative to its first variable, selectors from the round constants, the MDS
 * entries and the domain tag), the list of hash calls, the glue rows (per note 7 H + 4, 130 + INPUTS global ones) and the
 * INPUTS + 4 public-input positions.  On the device one kernel stamps the hash rows (a thread per hash call and template
 * row) and one scatters the glue rows.  The handle keeps in HBM the wiring (3 x n_gates x 4 B), the templates, the index
 * vectors of the witness launches and the staging of the requests; the selector vectors are scratch of the calls that
 * need them.  It loads and owns a zkt_poseidon of its own: zkt_withdraw_poseidon returns it BORROWED, so that a
 * zkt_merkle_tree can be bound to the same tables.  Create synchronises. */
typedef struct zkt_withdraw zkt_withdraw;
typedef struct {
    int inputs, height, width;
    int log_n_min;                     /* the smallest log_n with n_gates <= 2^log_n */
    size_t n_gates;                    /* inputs ((3 + height) P + 7 height + 4) + 2 P + 130 + inputs, P = vars_per_hash */
    size_t n_vars;
    size_t n_hashes;                   /* inputs (3 + height) + 2 */
    size_t vars_per_hash;
    size_t n_pi;                       /* inputs + 4 */
    size_t device_bytes;               /* what the handle holds in HBM (0 from zkt_debug_withdraw_layout_host); 128 KiB of it
                                          (ZKT_WITHDRAW_PROVE_MAX scalars) is the staging of zkt_withdraw_prove's new leaves */
} zkt_withdraw_info;
int zkt_withdraw_create(zkt_ctx* ctx, const zkt_poseidon_params* params, int inputs, int height, zkt_withdraw** out);
void zkt_withdraw_free(zkt_ctx* ctx, zkt_withdraw* w);
const zkt_poseidon* zkt_withdraw_poseidon(const zkt_withdraw* w);
int zkt_withdraw_get_info(const zkt_withdraw* w, zkt_withdraw_info* out);
/* The n_pi public-input rows, ascending: root, nullifiers, withdraw_amount, new_identifier, new_leaf -- the CLI's order
 * (bin/src/main.rs:266-271). */
int zkt_withdraw_pi_pos(const zkt_withdraw* w, size_t* out);
/* Regenerates the rows on the device and downloads them to HOST memory, n_gates entries each: out_selectors6 = q_m, q_l,
 * q_r, q_o, q_c, q_lookup (Montgomery words), out_wires3 = w_l, w_r, w_o (ZKT_VARIABLE_ZERO = Variable::Zero).  Either
 * of the two may be NULL.  Synchronises the stream. */
int zkt_withdraw_rows(zkt_ctx* ctx, const zkt_withdraw* w, uint64_t* const* out_selectors6, uint32_t* const* out_wires3);
/* The same rows expanded by the planner on the HOST, with no context and no device: for tests.  info, the row outputs,
 * out_pi_pos (n_pi) and out_hash_calls (n_hashes x 5 words: first variable, arity, three input variables with
 * ZKT_VARIABLE_ZERO beyond the arity) are each optional: call once for info, then with buffers of those sizes. */
int zkt_debug_withdraw_layout_host(int curve_id, const zkt_poseidon_params* params, int inputs, int height, zkt_withdraw_info* info,
                                   uint64_t* const* out_selectors6, uint32_t* const* out_wires3, size_t* out_pi_pos,
                                   uint32_t* out_hash_calls);
/* proof_system::setup of the circuit: the six selector vectors and the q_table mask (0 for the first table_size rows, 1
 * after, as zkt_circuit_setup documents it) are made on the device and go, with the resident wiring, through
 * zkt_circuit_setup_wiring with evals_on_device and wiring_on_device set; results and refusals are that call's, plus
 * ZKT_ERR_INVALID_ARGUMENT for log_n < log_n_min and table_size >= n.  Afterwards the circuit is loaded and the key-file
 * writers (zkt_circuit_save_files ..) work as after any setup.  Scratch (~200 MB of selectors at n = 2^20) is the call's
 * own.  Synchronises the stream. */
int zkt_withdraw_setup(zkt_ctx* ctx, const zkt_withdraw* w, int log_n, size_t table_size, uint64_t* out_commitments,
                       int* out_is_infinity);
/* One withdrawal as the CLI assembles it (bin/src/main.rs:198-271).  HOST pointers, scalars in Montgomery words. */
typedef struct {
    const uint64_t* secrets;           /* inputs scalars */
    const uint64_t* identifiers;       /* inputs scalars */
    const uint64_t* amounts;           /* inputs words */
    const uint64_t* leaf_indices;      /* inputs words, each below 2^height */
    const uint64_t* siblings;          /* inputs x height scalars, level 0 first; NULL: taken from `tree` */
    const uint64_t* root;              /* one scalar; NULL: the tree's root (costs a synchronisation: zkt_merkle_tree_root) */
    const uint64_t* new_secret;
    const uint64_t* new_identifier;
    uint64_t withdraw_amount;
} zkt_withdraw_request;
typedef struct {
    uint32_t bad_paths;                /* bit k: note k's path does not end in the root variable */
} zkt_withdraw_status;
/* The whole variable map and the public inputs of `batch` withdrawals (1 <= batch <= ZKT_WITNESS_BATCH_MAX), made on the
 * device.  d_variables is DEVICE memory: request b's map is the n_vars scalars at d_variables + b * stride (stride >=
 * n_vars, the layout zkt_circuit_check_witness_batch reads; padding beyond n_vars is never written); batch x stride must
 * fit the 32-bit variable indices of the gadget kernels.  Refused on the host before anything is enqueued: a sum of
 * amounts that overflows u64, withdraw_amount above the sum (withdraw.rs:59), a leaf index >= 2^height, siblings == NULL
 * without a tree or with a tree of another height (ZKT_ERR_INVALID_ARGUMENT); a secret equal to 0
 * (ZKT_ERR_ZERO_DENOMINATOR: the reference panics on 1 / secret, main.rs:257).  A tree must be bound to
 * zkt_withdraw_poseidon(w).
 * Launches, all on the context's stream, their number independent of the batch, no allocation: the staged requests' copy;
 * (1) a kernel that writes every variable that is neither a hash trace nor a select (amounts, identifiers, root, secrets,
 * 1 / secret, position bits, siblings, lookup copies, the 64 bits of amount_out and their 63 recombination sums, the
 * running sums, new_secret, new_identifier) -- with a tree the siblings come from
 * zkt_merkle_tree_paths_to_variables_dev instead (one call per ZKT_MERKLE_TREE_PATHS_MAX paths: two beyond 4096); (2) zkt_poseidon_gadget_witness_dev for the arity-1 hashes
 * (commitments, nullifiers, the new commitment); (3) the same for the arity-3 hashes (leaves, the new leaf); (4)
 * zkt_poseidon_merkle_path_witness_dev for the batch x inputs paths; (5) a kernel that gathers the public inputs and
 * compares every path's root with the root variable.  The launches' index vectors for every batch slot are made by one
 * more small kernel when (stride, batch) differ from the previous call's, and kept.
 * The requests are staged in pinned memory the handle owns: a second call waits for the first one's copy to have left
 * that buffer, nothing else; the requests' arrays are free on return.
 * out_pi (optional): batch x n_pi scalars in position order = the CLI's order.  out_status (optional): per request.  When
 * either is non-NULL the call synchronises; with both NULL it only enqueues (no synchronisation), and zkt_prove with
 * wires_on_device can follow without a wait.  A wrong sibling is a property of the witness, not an error: the map is
 * written, the bit is reported and zkt_circuit_check_witness names the equal_constrain row. */
int zkt_withdraw_witness(zkt_ctx* ctx, zkt_withdraw* w, const zkt_withdraw_request* reqs, size_t batch, zkt_merkle_tree* tree,
                         void* d_variables, size_t stride, uint64_t* out_pi, zkt_withdraw_status* out_status);
/* Fills zkt_prove_inputs for request b of such a map: the device wiring and n_rows, n_vars, wires_on_device = 1, the
 * given public inputs; a_evals .. c_evals are set NULL; table, table_len and blinders are left for the caller. */
int zkt_withdraw_prove_inputs(const zkt_withdraw* w, const void* d_variables, size_t stride, size_t b, const size_t* pi_pos,
                              const uint64_t* pi_vals, zkt_prove_inputs* out);
/* Deposit (bin/src/main.rs:160-163): leaf = H(identifier, amount, H(secret)) for m deposits, DEVICE pointers (m scalars,
 * m scalars, m words, m scalars out), two launches of the hash-batch kernel; the output feeds zkt_merkle_tree_append_dev
 * without the host.  The 3 m scalars of scratch are the call's own, so it synchronises the stream before it returns. */
int zkt_note_leaves(zkt_ctx* ctx, const zkt_poseidon* poseidon, const void* d_secrets, const void* d_identifiers,
                    const void* d_amounts_u64, size_t m, void* d_out_leaves);

/* ProveWithdraw (bin/src/main.rs:190-319) for a batch of requests in ONE call: the identifiers set deduplicated into the
 * lookup table, the witness (zkt_withdraw_witness), one proof per request under a transcript seeded from the loaded circuit's
 * own commitments and n (zkt_prove), the CLI's check of each proof (zkt_verify, main.rs:298) and the new leaves added to the
 * tree (main.rs:302-304).  Needs what zkt_prove needs: an SRS and the withdraw circuit loaded (zkt_withdraw_setup, or
 * zkt_circuit_load / _load_file of its ProverKey). */
#define ZKT_WITHDRAW_PROVE_MAX 4096                /* most requests one zkt_withdraw_prove takes */
typedef struct {
    int transcript_kind; const char* label;          /* T::new("ZKT Plonk"), plonk.rs:107 */
    const uint64_t* identifiers_set; size_t set_len; /* Montgomery; a repeated value is dropped, the first kept
                                                        (IndexSet::from_iter, lookup/table.rs:64-72); > table_size refused */
    const uint64_t* blinders;                        /* batch x 19, the order zkt_prove documents */
    int verify;                                      /* != 0: zkt_verify each proof (main.rs:298); needs the next three */
    const uint64_t* g_xy_mont; const uint64_t* h_g2_mont; const uint64_t* beta_h_g2_mont;
    int append;                                      /* != 0: add the new leaves to `tree` (main.rs:302-304) */
    void* d_variables; size_t stride; size_t slots;  /* caller's workspace: `slots` maps, as zkt_withdraw_witness reads it */
} zkt_withdraw_prove_args;
typedef struct { int code; uint32_t bad_paths; int verified; uint64_t new_leaf_index; } zkt_withdraw_result;
/* proofs: batch x proof_stride bytes (proof_stride >= 802 on BN254, 1010 on BLS12-381), request b's proof at b x proof_stride;
 * out_pi (optional): batch x n_pi scalars, the CLI-order public inputs; results: batch entries.
 * Snapshot.  The whole batch is proved against the tree as it is at the call: one root, like the withdrawals of one block
 *   (nothing is appended before the last proof).  The CLI's one-at-a-time behaviour is batch = 1.  Paths and roots come from
 *   `tree` or from reqs[b].siblings / .root, exactly as in zkt_withdraw_witness.
 * Chunking.  1 <= slots <= ZKT_WITNESS_BATCH_MAX maps of `stride` scalars at d_variables.  The batch is worked in chunks of
 *   `slots` requests: one zkt_withdraw_witness per chunk, whose public inputs and bad_paths come to the host (one
 *   synchronisation a chunk), then the chunk's proofs, each announced to its predecessor with zkt_prove_set_next.  The chain
 *   does not cross a chunk boundary (the next chunk's maps do not exist yet).  Proof bytes depend neither on that nor on
 *   `slots`.  An announcement the caller made before the call is withdrawn.
 * Table.  The deduplicated set is every proof's lookup table.  More values than the table size are refused
 *   (ZKT_ERR_INVALID_ARGUMENT, "table size exceeds max size", lookup/table.rs:57): the size zkt_withdraw_setup was given when
 *   it set the loaded circuit up (kept with the circuit), n - 1 (zkt_prove's own bound) under a circuit loaded another way.
 * Per-request results.  Whatever zkt_withdraw_witness would refuse on the host -- for any request of the batch -- fails the
 *   whole call before anything is enqueued, as do a null pointer, batch outside 1 .. ZKT_WITHDRAW_PROVE_MAX, slots or stride
 *   out of range, a proof_stride too short, an unknown transcript kind and, with append != 0, a missing tree or one without
 *   room for `batch` more leaves.  After that: a request whose bad_paths != 0 is not proved (code = ZKT_ERR_INVALID_ARGUMENT,
 *   its proof bytes zeroed); a request zkt_prove refuses keeps that code (ZKT_ERR_NOT_IN_TABLE for an identifier outside the
 *   set, ZKT_ERR_EQUAL_CHALLENGES, ZKT_ERR_ZERO_DENOMINATOR, ZKT_ERR_QUOTIENT_TOO_SHORT; proof bytes zeroed); the batch goes
 *   on in both cases, and the successor of a refused proof is proved like any other (its early rounds are simply issued
 *   again).  Any other failure of zkt_prove ends the call with that code.  verified: 1 when verify != 0 and zkt_verify
 *   accepted the proof under out_pi, else 0.  The return value is ZKT_OK unless the call as a whole failed.
 * Append.  After the last proof the new leaves of the requests that were proved -- with verify != 0: proved and verified --
 *   are appended in request order through ONE zkt_merkle_tree_append_dev.  They never visit the host: a small kernel gathers
 *   them chunk by chunk from the maps' new-leaf variable into staging the handle owns.  new_leaf_index is the leaf's index
 *   for those requests and UINT64_MAX for all others.  Nothing is appended when there is none.
 * The call allocates no device memory (the first call under a circuit that zkt_withdraw_setup did not make, or after the SRS
 * was loaded again, makes the circuit's commitments once, zkt_circuit_commitments, and keeps them with the circuit),
 * synchronises once more at its end, and leaves the context
 * ready for the next proof on every path: no announcement pending. */
int zkt_withdraw_prove(zkt_ctx* ctx, zkt_withdraw* w, const zkt_withdraw_request* reqs, size_t batch, zkt_merkle_tree* tree,
                       const zkt_withdraw_prove_args* args, uint8_t* proofs, size_t proof_stride, uint64_t* out_pi,
                       zkt_withdraw_result* results);

/* ---- Verifier (proof_system/proof.rs:285-503): zkt_verify_prepare = everything but the pairings,
 * ---- zkt_pairing_product_is_one = the pairings, zkt_verify = both ------------------------------------------------
 * Deserialises the proof (proof.rs:98-155; points are decompressed and checked to be on the curve), replays the
 * transcript, computes r0 (proof.rs:163-217) and the linearisation commitment (proof.rs:220-282, the 13-point
 * multi_scalar_mul of commitment.rs:32-45), and folds each of the two SonicKZG10::check calls (proof.rs:420-500) into
 * ONE pair of G1 points (L, W) with L = sum_i eta^i C_i - (sum_i eta^i v_i) g + z W: the opening is valid iff
 * e(L, h) == e(W, beta h).  The two pairings stay with the caller (arkworks), who holds h and beta h.  Host-only code:
 * a proof is ~30 short scalar multiplications.  `transcript` must be seeded like the prover's.
 * out_pairs: L1, W1, L2, W2 as (x, y) Montgomery limbs; out_is_infinity: 4 flags (may be NULL).
 * Errors: ZKT_ERR_INVALID_ARGUMENT for malformed bytes / points off the curve, ZKT_ERR_EQUAL_CHALLENGES (proof.rs:340-345). */
typedef struct {
    uint64_t n;                         /* VerifierKey::n */
    const uint64_t* vk_commitments;     /* 10 x (x, y), zkt_transcript_seed order */
    const int* vk_is_infinity;          /* 10 flags or NULL */
    const uint64_t* pi_roots;           /* VerifierKey::pi_roots, n_pi Montgomery scalars */
    const uint64_t* pub_inputs;         /* the public inputs, same order */
    size_t n_pi;
    const uint8_t* proof;               /* CanonicalSerialize bytes (802 / 1010) */
    size_t proof_len;
    const uint64_t* g;                  /* SonicKZG10 VerifierKey::g (= powers_of_g[0]), (x, y) */
} zkt_verify_inputs;
int zkt_verify_prepare(int curve_id, const zkt_verify_inputs* in, zkt_transcript* transcript, uint64_t* out_pairs,
                       int* out_is_infinity);

/* The pairing check itself, on the host: prod_i e(P_i, Q_i) == 1 for P_i in G1 ((x, y) Montgomery limbs) and Q_i in G2
 * (arkworks' Fp2 layout: x.c0, x.c1, y.c0, y.c1; all-zero = infinity).  The optimal ate pairing of ark-ec (Miller loop over
 * 6x + 2 plus two Frobenius steps on BN254, over |x| on BLS12-381, csrc/pairing.hpp); the line slopes of a G2 point are
 * computed once and kept, so the fixed h / beta h of a KZG check cost no G2 arithmetic per call; one shared squaring chain
 * and one final exponentiation for the whole product.  ~0.5 ms for the two pairings of one KZG check on BN254.  Points
 * off the curve / twist, G1 points outside the prime-order subgroup (BLS12-381) -> ZKT_ERR_INVALID_ARGUMENT; G2
 * subgroup membership is the caller's business (h and beta h come from the trusted VerifierKey). */
int zkt_pairing_product_is_one(int curve_id, const uint64_t* g1_xy_mont, const uint64_t* g2_xy_mont, size_t n, int* is_one);
/* The whole of Proof::verify (proof_system/proof.rs:285-503): zkt_verify_prepare, then both openings' checks
 * e(L_k, h) e(-W_k, beta h) == 1 (proof.rs:441,479) folded into one product of two pairings with a 128-bit challenge rho
 * hashed from (L1, W1, L2, W2, h, beta h): e(L1 + rho L2, h) e(-(W1 + rho W2), beta h) == 1 -- ark-poly-commit's batch_check
 * folding; a proof failing either check passes with probability 2^-128.  h, beta_h: SonicKZG10 VerifierKey::h and
 * ::beta_h (G2).  *accepted = 1 / 0 (Error::ProofVerificationError).  ~2.3 ms per BN254 proof on one host core. */
int zkt_verify(int curve_id, const zkt_verify_inputs* in, zkt_transcript* transcript, const uint64_t* h_g2_mont,
               const uint64_t* beta_h_g2_mont, int* accepted);

/* `count` proofs under ONE structured reference string (h, beta h), circuits / verifier keys free to differ: each proof is
 * taken through zkt_verify_prepare with its own seeded transcript, and all 2 * count opening checks are folded into ONE
 * product of two pairings with 128-bit coefficients hashed from every (L, W), h and beta h (see csrc/verify.hip).
 * *accepted = 1 iff every proof verifies (a batch holding a bad proof passes with probability 2^-128); a rejected batch
 * does not say which proof failed -- zkt_verify_batch_locate names the bad proofs, or fall back to zkt_verify per
 * proof.  Cost per proof: the transcript, r0 and the two short
 * multi-scalar multiplications; the pairings (~0.5 ms on BN254) are paid once per batch.  The reference verifies proof by
 * proof (proof.rs:285-503); this is the batch form SURVEY.md 8f.4 lists.  Errors as zkt_verify_prepare (a malformed
 * proof fails the call, not just the batch). */
int zkt_verify_batch(int curve_id, const zkt_verify_inputs* ins, zkt_transcript* const* transcripts, size_t count,
                     const uint64_t* h_g2_mont, const uint64_t* beta_h_g2_mont, int* accepted);

/* Checked GroupAffine::deserialize (ark-serialize 0.3, compressed form) of n G1 points on the device, one thread per point
 * on the context's stream (csrc/g1decomp.hip).  compressed: n x nb bytes, nb = ceil((MODULUS_BITS + 2) / 8) = 32 on
 * BN254, 48 on BLS12-381: x little-endian, the top two bits of the last byte are SWFlags (bit 7: y is the larger root,
 * bit 6: infinity).  out_xy_mont: n x (x, y) Montgomery limbs in arkworks' layout, (0,0) for the identity AND for every
 * refused point; out_status: one byte per point,
 *   ZKT_G1_VALID 0            a point of G1
 *   ZKT_G1_IDENTITY 1         the infinity flag; the x bits must still be below the modulus and are then ignored
 *   ZKT_G1_NOT_CANONICAL 2    x >= q after the flag bits are stripped (under the infinity flag too)
 *   ZKT_G1_BOTH_FLAGS 3       both flag bits set (decided before x is looked at)
 *   ZKT_G1_NOT_ON_CURVE 4     x^3 + b is not a square
 *   ZKT_G1_NOT_IN_SUBGROUP 5  on the curve, outside the prime-order subgroup (BLS12-381 only; BN254 has cofactor one)
 * -- the rules of the host verifier's deserialisation, which agrees with this one on every input.  The bytes may come
 * from anyone: a refusal is a status, never an error code or a fault.  n = 0 -> ZKT_OK, nothing touched; n >
 * ZKT_G1_DECOMPRESS_MAX -> ZKT_ERR_INVALID_ARGUMENT; a failed allocation -> ZKT_ERR_HIP.  Needs no SRS and no circuit,
 * works on any context (forked, with a communicator: local, no collective); its scratch memory is shared with
 * zkt_verify_batch_dev only.  The host form synchronises the stream.
 * _dev: all three buffers in HBM (input and points 16-byte aligned, else ZKT_ERR_INVALID_ARGUMENT); only enqueues. */
#define ZKT_G1_DECOMPRESS_MAX ((size_t)1 << 22)
enum {
    ZKT_G1_VALID = 0,
    ZKT_G1_IDENTITY = 1,
    ZKT_G1_NOT_CANONICAL = 2,
    ZKT_G1_BOTH_FLAGS = 3,
    ZKT_G1_NOT_ON_CURVE = 4,
    ZKT_G1_NOT_IN_SUBGROUP = 5
};
int zkt_g1_decompress(zkt_ctx* ctx, const uint8_t* compressed, size_t n, uint64_t* out_xy_mont, uint8_t* out_status);
int zkt_g1_decompress_dev(zkt_ctx* ctx, const void* d_compressed, size_t n, void* d_out_xy_mont, void* d_out_status);

/* zkt_g1_check: the per-point test of zkt_g1_decompress for n UNCOMPRESSED G1 points, one thread per point
 * (csrc/g1check.hip): what a committer key is made of before zkt_srs_load sees it.  points_xy_mont: n x (x, y) as arkworks Montgomery limbs, the layout zkt_srs_load and
 * zkt_msm_g1_bases take (8 u64 per point on BN254, 12 on BLS12-381), (0,0) = the identity; host memory, or with
 * points_on_device = 1 device memory, 16-byte aligned (else ZKT_ERR_INVALID_ARGUMENT), read behind the work already on the
 * context's stream (rule 1 of zkt_ctx_set_stream).  out_status: host, one byte per point, the first that applies of
 *   ZKT_G1_NOT_CANONICAL      the raw limbs of x or of y are >= q
 *   ZKT_G1_IDENTITY           the point is (0,0)
 *   ZKT_G1_NOT_ON_CURVE       y^2 != x^3 + b
 *   ZKT_G1_NOT_IN_SUBGROUP    on the curve, outside the prime-order subgroup (BLS12-381 only)
 *   ZKT_G1_VALID              otherwise
 * (ZKT_G1_BOTH_FLAGS never occurs: there are no flags).  The points may come from anyone: a refusal is a status, never an
 * error code or a fault.  n = 0 -> ZKT_OK, nothing touched; any n is taken (in pieces of ZKT_MSM_BASES_MAX points); a failed
 * allocation -> ZKT_ERR_HIP.  Needs no SRS and no circuit, works on any context (forked, with a communicator: local, no
 * collective); its scratch memory is that of zkt_srs_check.  Synchronises the stream.
 * zkt_debug_g1_check_host: the same function run on the host (one source text for both), no context, no device. */
int zkt_g1_check(zkt_ctx* ctx, const void* points_xy_mont, size_t n, int points_on_device, uint8_t* out_status);
int zkt_debug_g1_check_host(int curve_id, const uint64_t* points, size_t n, uint8_t* out_status);

/* zkt_srs_check: is g1_xy_mont[0 .. count) the powers_of_g of the KZG key whose VerifierKey holds h and beta_h -- is there a tau with
 * P_i = tau^i P_0 for every i and beta_h = tau h?  For a key file before zkt_srs_load (which takes the points as they come,
 * as the reference's deserialize_unchecked does): corrupted, truncated and mixed-up keys are named here instead of failing
 * every proof later.  Two tests, both on the device (csrc/g1check.hip):
 *   points     every P_i gets its zkt_g1_check status; any status but ZKT_G1_VALID is bad (the identity too: tau^i g never
 *              is).  The report counts them and names the first; out_status (host, count bytes, may be NULL) receives
 *              all of them.
 *   structure  only when every point is valid (a combination of invalid points means nothing).  rho = seed32 read as a
 *              little-endian integer, reduced mod r; with S = sum_(i < count) rho^i P_i, one device MSM, the key is accepted
 *              iff e(rho S - rho^count P_(count-1), beta_h) e(P_0 - S, h) == 1, which is sum_i rho^i (P_(i+1) - tau P_i) = 0
 *              in one pairing equation.  A key with the wrong structure passes for at most count values of rho: with
 *              probability at most count / r (below 2^-229 at ZKT_SRS_CHECK_MAX) when the seed is drawn after the key
 *              is fixed.  The CALLER draws the seed, 32 random bytes; the library holds no randomness.  A seed that reduces
 *              to rho = 0 -> ZKT_ERR_INVALID_ARGUMENT.  count = 1 has nothing to relate: structure_ok = 1, S = P_0.
 * h, beta_h: G2, arkworks' Fp2 layout as zkt_verify takes them; they are trusted (off the twist -> ZKT_ERR_INVALID_ARGUMENT).
 * 1 <= count <= ZKT_SRS_CHECK_MAX = 2^24 + 1 (the reference's 4n + 1 powers at n = 2^22), else ZKT_ERR_INVALID_ARGUMENT.
 * points_on_device as zkt_g1_check: with the key in HBM one upload serves this call and zkt_srs_load_dev.  The points go
 * through in chunks of at most ZKT_MSM_BASES_MAX: upload (host points), statuses, their reduction, and -- while no point
 * has been bad -- the powers of rho and the MSM of zkt_msm_g1_bases over the chunk; the chunk sums are added on the host,
 * which finishes with two short scalar multiplications and zkt_pairing_product_is_one.  After the first bad point the later
 * chunks still get statuses and counts, and no MSM.  Scratch: that of zkt_msm_g1_bases plus one chunk of points and status
 * bytes, and that call's rules hold: any context (no key needed, forked, between proofs), the loaded SRS, Lagrange-basis
 * table, circuit and an announced proof untouched, local on a context with a communicator.  Profile scopes
 * "srs_check_points" and "srs_check_msm".  Synchronises the stream.
 * zkt_debug_srs_check_chunk: the chunk size of this context's later calls (tests reach chunk boundaries at small sizes);
 * 0 restores ZKT_MSM_BASES_MAX, more than that -> ZKT_ERR_INVALID_ARGUMENT.
 * zkt_debug_srs_check_finish_host: the host's end alone, no context: S (ignored when S_inf), P_0, P_(count-1) affine
 * Montgomery limbs, rho as four canonical words (non-zero) -> *structure_ok.  S is taken for granted. */
#define ZKT_SRS_CHECK_MAX (((size_t)1 << 24) + 1)
typedef struct {
    uint64_t count, n_bad, first_bad;      /* first_bad = index of the first point whose status is not VALID (count if none) */
    uint64_t by_status[6];                 /* how many points got each ZKT_G1_* status */
    int first_bad_status;
    int points_ok;                         /* n_bad == 0 (an identity among the powers is bad: tau^i g is never the identity) */
    int structure_checked;                 /* 0 when !points_ok (the combination of invalid points means nothing) */
    int structure_ok;
    int ok;                                /* points_ok && structure_ok */
    uint64_t sum_xy_mont[12];              /* S, affine ((0,0) when sum_is_infinity), when structure_checked */
    int sum_is_infinity;
} zkt_srs_report;
int zkt_srs_check(zkt_ctx* ctx, const void* g1_xy_mont, size_t count, int points_on_device, const uint64_t* h_g2_mont,
                  const uint64_t* beta_h_g2_mont, const uint8_t seed32[32], uint8_t* out_status, zkt_srs_report* report);
int zkt_debug_srs_check_chunk(zkt_ctx* ctx, size_t max_points);
int zkt_debug_srs_check_finish_host(int curve_id, const uint64_t* S, int S_inf, const uint64_t* P0, const uint64_t* Plast,
                                    uint64_t count, const uint64_t* rho_canonical4, const uint64_t* h, const uint64_t* beta_h,
                                    int* structure_ok);

/* zkt_verify_batch with the two costs that grow with `count` moved to the device (csrc/verify.hip): the 13 * count
 * compressed commitments are decompressed and checked in ONE zkt_g1_decompress launch, and the 2 * count folded openings
 * are multiplied out as two device MSMs (the machinery of zkt_msm_g1_bases) instead of ~35 host scalar multiplications per
 * proof.  For a verifier of many proofs under one SRS (a relayer, an aggregator); for one proof or a handful use
 * zkt_verify / zkt_verify_batch -- measured on an MI355X (docs/EXPERIMENTS.md "locating the bad proofs of a batch"), the
 * host route is faster for a single proof (1.3 ms against 1.5 ms on BN254, 2.8 against 4.1 on BLS12-381) and the device
 * route from 16 proofs on, the next count measured (3.1x / 4.3x there, 5.7x / 14x at 4096, where the per-proof host stage
 * is all that is left: 0.11 ms / 0.12 ms per proof); there is no automatic fallback: the caller chooses the entry point.
 * Arguments as zkt_verify_batch (every transcript seeded like its prover's, consumed exactly as zkt_verify_prepare
 * consumes it), with a context in place of the curve id (the context's curve is used).  Per proof the host keeps the byte-level checks (length, the two Option::None bytes,
 * canonical evaluations), the transcript, r0 and the scalars of the two openings; it never forms the pairs (L_j, W_j).
 * With rho_0 = 1, rho_j = the low 128 bits of Keccak-256(seed || j) for opening j < 2 * count, and seed = Keccak-256 over
 * the curve id, count, and per proof its bytes, n, the ten verifier-key commitments and flags, pi_roots, the public
 * inputs and g, then h and beta h, the call computes
 *     A = sum_j rho_j L_j  (terms on one point added up: inside a proof, and across proofs for verifier-key points and g
 *                           that are EQUAL BY CONTENT; identities dropped; at most 24 bases per proof),
 *     B = sum_j rho_j W_j,
 * and the batch is accepted iff e(A, h) e(-B, beta h) == 1.  zkt_verify_batch hashes the pairs (L_j, W_j) themselves, so
 * the two entry points draw DIFFERENT coefficients; the inputs hashed here determine every pair, so this binds at least
 * as much, and the two have the same accept set up to 2^-128.
 * zkt_verify_batch_prepare_dev stops before the pairing: out_ab = A, B as (x, y) Montgomery limbs, out_ab_is_infinity 2
 * flags (may be NULL), out_rho (may be NULL) the 2 * count coefficients as 4 canonical u64 words each -- for a caller who
 * keeps arkworks' product_of_pairings.  zkt_verify_batch_dev runs the host pairing of zkt_pairing_product_is_one and
 * sets *accepted; a rejected batch does not say which proof failed: zkt_verify_batch_locate below does.
 * Errors: count = 0 or count > ZKT_VERIFY_BATCH_DEV_MAX (24 * count <= ZKT_MSM_BASES_MAX) -> ZKT_ERR_INVALID_ARGUMENT;
 * malformed bytes, or a commitment whose status is neither ZKT_G1_VALID nor ZKT_G1_IDENTITY -> ZKT_ERR_INVALID_ARGUMENT,
 * zkt_last_error names the proof index and the commitment; otherwise as zkt_verify_prepare.
 * Needs no SRS and no circuit; works on a forked context and on one with a communicator (local, no collective).  Its
 * scratch memory is its own (allocated on first use, grown as needed, freed by zkt_ctx_destroy); the key, the circuit,
 * the Lagrange and wire tables stay untouched, and a proof announced with zkt_prove_set_next yields the same bytes.
 * Synchronises the stream.  Profile scopes: "verify_decompress", "verify_msm".
 * Under zkt_ctx_set_verify_terms(ctx, 1) (below) the transcript, r0 and the scalars of the two openings move to the
 * device as well: one kernel, one lane per proof, enqueued directly behind the decompression, with one synchronisation
 * for both; the host keeps the byte-level checks, the seed hash and the merge across proofs.  A, B, the coefficients, the
 * verdict, the return codes and the proof named by zkt_last_error are the same under both modes (of several refused
 * proofs the lowest index is reported, as the serial loop does).  The scratch grows by one more region behind the
 * decompression's: per proof 128 bytes of description, 12 * 32 of evaluations, 232 of transcript state, 4 of status and
 * 24 * 32 of sums, and 3 * 32 bytes per public input (roots, values, running products); each part rounded up to 256
 * bytes; zkt_verify_batch_locate's own parts then start behind it.  Profile scope: "verify_terms".
 * Measured on an MI355X (docs/EXPERIMENTS.md "the batch verifier's transcripts and scalar stage on the device"): mode 1
 * wins from 256 proofs on, the next count measured after 16 (8.1 ms against 30.0 ms on BN254, 9.4 against 34.2 on
 * BLS12-381; at 4096: 46 against 457 ms and 55 against 481 ms, 0.010 - 0.012 ms of host time per proof left), and loses
 * below: the kernel walks one proof's hash chain per lane and takes 1.6 - 4.2 ms whatever the count (one proof: 3.0
 * against 1.5 ms and 6.1 against 4.4 ms; 16 proofs: 5.5 against 3.5 ms on BN254, level on BLS12-381).  Mode 0 is the
 * default and there is no automatic choice: the caller sets the mode. */
#define ZKT_VERIFY_BATCH_DEV_MAX (ZKT_MSM_BASES_MAX / 24)
int zkt_verify_batch_prepare_dev(zkt_ctx* ctx, const zkt_verify_inputs* ins, zkt_transcript* const* transcripts, size_t count,
                                 const uint64_t* h_g2_mont, const uint64_t* beta_h_g2_mont, uint64_t* out_ab,
                                 int* out_ab_is_infinity, uint64_t* out_rho);
int zkt_verify_batch_dev(zkt_ctx* ctx, const zkt_verify_inputs* ins, zkt_transcript* const* transcripts, size_t count,
                         const uint64_t* h_g2_mont, const uint64_t* beta_h_g2_mont, int* accepted);

/* zkt_ctx_set_verify_terms: where zkt_verify_batch_prepare_dev, zkt_verify_batch_dev, zkt_verify_batch_locate and
 * zkt_debug_verify_batch_tree run the per-proof stage between the decompression and the MSMs -- the Fiat-Shamir replay
 * (Merlin / STROBE-128 or the Keccak-256 Ethereum transcript), zh(xi), L_1(xi), r0, the 13 linearisation scalars, both
 * fold lists and their sums by source.  mode 0 (the default): on the host, one proof after the other.  mode 1: on the
 * device (csrc/verify_terms.hip; the arithmetic is csrc/verify_terms.hpp, shared with a host rehearsal).  Any other value
 * -> ZKT_ERR_INVALID_ARGUMENT.  A fork inherits the mode.  Results do not depend on the mode.
 * Mode 1 takes each transcript's state out of its handle, runs the replay on the device, and puts the final state back:
 * every handle must come from zkt_transcript_new (either kind; a batch may mix kinds), else ZKT_ERR_INVALID_ARGUMENT.
 * After a successful call each handle holds the state the host route would have left (consumed exactly as
 * zkt_verify_prepare consumes it).  On an error NO state is written back under mode 1: every handle is as the caller
 * seeded it (mode 0 leaves the handles in front of the refused proof consumed and that proof's partly consumed).
 * Test hooks of the stage.  Both take the batch as zkt_verify_batch_dev does, rho_canonical4 = 2 * count coefficients as
 * 4 canonical words each (NULL: all ones) and forced_mont = NULL or 7 * count Montgomery values beta, gamma, delta,
 * epsilon, alpha, xi, eta per proof that replace the transcript's answers (the transcript is still fed and asked).  Per
 * proof they return out_status (ZKT_OK, ZKT_ERR_EQUAL_CHALLENGES or ZKT_ERR_ZERO_DENOMINATOR), out_challenges (7 values,
 * as far as they were drawn, the rest zero), out_r0 and out_acc (24 sums by source; zero for a refused proof), 4
 * Montgomery words each, and leave every handle where the route left it, a refused proof's included.  They return ZKT_OK
 * when they ran: a per-proof refusal is a result.  Malformed bytes or a refused commitment -> the error of the real call.
 * zkt_debug_verify_terms: on a context, the commitments through the device's decompression; route 0 = the host route
 * (the replay through the handle's own calls, as mode 0 runs it), route 2 = the kernel.  Synchronises the stream.
 * zkt_debug_verify_terms_host: no context and no device, the host verifier's own decompression; route 0 as above,
 * route 1 = the replay on the transcript's exported state directly, as the kernel runs it, on the host.
 * zkt_debug_verify_terms_transcript: ONE transcript call on the exported state directly, on the host, on a handle of
 * zkt_transcript_new (state out, the call, state in), so that STROBE-128 and Keccak-256 can be held to known answers
 * and to the handle's own calls.  op 0: a message -- Merlin append_message(label, data[0 .. len)), len <= 104; Ethereum one
 * item, data little-endian, hashed big-endian, len <= 68.  op 1: a commitment that is not the identity, data = x || y
 * little-endian, len = both.  op 2: a challenge of len = fr_bits bits (Merlin: (len + 7) / 8 - 1 bytes) -> out32,
 * little-endian.  Anything else -> ZKT_ERR_INVALID_ARGUMENT. */
int zkt_ctx_set_verify_terms(zkt_ctx* ctx, int mode);
int zkt_debug_verify_terms(zkt_ctx* ctx, const zkt_verify_inputs* ins, zkt_transcript* const* transcripts, size_t count,
                           const uint64_t* rho_canonical4, const uint64_t* forced_mont, int route, uint64_t* out_challenges,
                           uint64_t* out_r0, uint64_t* out_acc, int* out_status);
int zkt_debug_verify_terms_host(int curve_id, const zkt_verify_inputs* ins, zkt_transcript* const* transcripts, size_t count,
                                const uint64_t* rho_canonical4, const uint64_t* forced_mont, int route,
                                uint64_t* out_challenges, uint64_t* out_r0, uint64_t* out_acc, int* out_status);
int zkt_debug_verify_terms_transcript(zkt_transcript* transcript, int op, const char* label, const uint8_t* data, size_t len,
                                      uint8_t out32[32]);

/* zkt_verify_batch_dev that also names the bad proofs of a rejected batch.  The batch check is linear in the proofs: with
 * the coefficients rho_j of zkt_verify_batch_dev (same seed), proof i has the pair
 *     P_i = rho_2i L_2i + rho_2i+1 L_2i+1,   Q_i = rho_2i W_2i + rho_2i+1 W_2i+1,
 * which passes e(P_i, h) e(-Q_i, beta h) == 1 iff the proof verifies (up to 2^-128), and (A, B) is the sum of all pairs.
 * The call runs zkt_verify_batch_dev's stages and its one pairing check.  If that passes: *accepted = 1, out_bad all zero,
 * *n_checks = 1, and nothing else ran -- an accepted batch costs what zkt_verify_batch_dev costs.  If it fails, the device
 * forms the `count` pairs (csrc/verify_leaves.hip: per proof at most 24 full-width scalar multiplications for P_i, one per
 * source point, and two by 128-bit coefficients for Q_i) and adds neighbours (2m, 2m + 1) level by level into a binary
 * tree whose root is (A, B), an unpaired last node moving up unchanged; the tree comes down in one copy and the host walks
 * it from the root: at a failing node the left child is checked; if it passes the right child fails without a check,
 * otherwise the right child is checked too.  A failing leaf is a bad proof: out_bad[i] = 1 (count bytes, all written),
 * *accepted = 0, *n_bad = their number b, *n_checks = the pairing checks made, root included:
 *     n_checks <= 1 + 2 * b * ceil(log2(count)),   and exactly 1 for count = 1.
 * The verdicts are those of zkt_verify per proof, at one host stage for the batch plus one pairing check per node visited
 * instead of a whole zkt_verify per proof.  Measured on an MI355X (docs/EXPERIMENTS.md "locating the bad proofs of a
 * batch"), one bad proof among 4096: 485 ms against 5277 ms for the zkt_verify loop on BN254 (24 checks), 562 ms against
 * 11364 ms on BLS12-381; among 256: 44 against 330 ms and 58 against 709 ms; the loop wins only for a single proof.
 * Arguments, limits, errors and context rules are those of zkt_verify_batch_dev (1 <= count <= ZKT_VERIFY_BATCH_DEV_MAX; a
 * malformed proof or a refused commitment fails the call and zkt_last_error names the proof; transcripts are consumed as
 * zkt_verify_prepare consumes them; forked contexts and contexts with a communicator work; no key, circuit or table is
 * touched and an announced proof keeps its bytes).  accepted and out_bad are required, n_bad and n_checks may be NULL; on
 * an error none of the four is written.
 * Scratch: the call's own (shared with zkt_verify_batch_dev and zkt_g1_decompress, grown on demand).  A rejected batch needs,
 * behind the 13 * count * 3 * nb + 13 * count bytes of the decompression (nb = 32 / 48), per proof 11 * 2 * nb bytes of
 * bases, 24 * 32 of scalars, 2 * 32 of coefficients and 26 * 16 * L of products (L = 9 / 14 limbs: 144 / 224 bytes each),
 * and 2 * nodes * 4 * nb bytes of tree, nodes = count + ceil(count / 2) + ... + 1 < 2 * count + 64; each part rounded up to
 * 256 bytes.  That is ~5.8 KB (BN254) / ~8.5 KB (BLS12-381) per proof.
 * Synchronises the stream.  Profile scopes: those of zkt_verify_batch_dev, then "verify_leaves", "verify_tree".
 * Of zkt_verify_batch_dev's family (host arguments, work on the context's stream); its run on a stream the caller
 * keeps busy is tests/test_gpu_verify_locate_stream.py. */
int zkt_verify_batch_locate(zkt_ctx* ctx, const zkt_verify_inputs* ins, zkt_transcript* const* transcripts,
                            size_t count, const uint64_t* h_g2_mont, const uint64_t* beta_h_g2_mont,
                            int* accepted, uint8_t* out_bad, size_t* n_bad, size_t* n_checks);
/* Test hooks of the call above.  Both return the tree: out_nodes_xy_mont = 2 * nodes affine points as (x, y) Montgomery
 * limbs, P's tree then Q's, each level by level with the leaves first ((0, 0) for the identity), out_is_infinity 2 * nodes
 * flags, out_rho the 2 * count coefficients as 4 canonical words each; all normalised with ONE field inversion.
 * zkt_debug_verify_batch_tree builds leaves and levels on the device whatever the verdict (errors as the call above).
 * zkt_debug_verify_locate_host runs the whole call on the host, with no context and no device: the host verifier's own
 * deserialisation, and leaves and levels through the very code the kernels run (csrc/verify_leaves.hpp); the three tree
 * outputs may be NULL.  It returns the error code only. */
int zkt_debug_verify_batch_tree(zkt_ctx* ctx, const zkt_verify_inputs* ins, zkt_transcript* const* transcripts,
                                size_t count, const uint64_t* h_g2_mont, const uint64_t* beta_h_g2_mont,
                                uint64_t* out_nodes_xy_mont, int* out_is_infinity, uint64_t* out_rho);
int zkt_debug_verify_locate_host(int curve_id, const zkt_verify_inputs* ins, zkt_transcript* const* transcripts,
                                 size_t count, const uint64_t* h_g2_mont, const uint64_t* beta_h_g2_mont,
                                 int* accepted, uint8_t* out_bad, size_t* n_bad, size_t* n_checks,
                                 uint64_t* out_nodes_xy_mont, int* out_is_infinity, uint64_t* out_rho);

/* HomomorphicCommitment::multi_scalar_mul (commitment.rs:32-45) for ARBITRARY points: the verifier's 13-point
 * linearisation commitment and similar short combinations.  Host arithmetic (double-and-add on 64-bit limbs): at this
 * size a device launch would cost more than the sum.  scalars: 4 limbs each, Montgomery or canonical. */
int zkt_g1_msm_host(int curve_id, const uint64_t* points_xy_mont, const uint64_t* scalars, size_t n, int scalars_montgomery,
                    uint64_t* out_xy_mont, int* out_is_infinity);

/* ---- key files of the reference CLI ------------------------------------------------------------
 * `serialize_to_file` = CanonicalSerialize::serialize_unchecked (bin/src/parser.rs:14-22).  Layouts restated from
 * ark-serialize / ark-poly-commit 0.3 (see csrc/keyfile.hip); the reference holds no key file, so these readers are
 * pinned only by the round trip against the writer in oracle/keyfile.py ("parity unpinned").  Host-only; values come
 * back as arkworks Montgomery limbs, ready for zkt_srs_load / zkt_circuit_load / zkt_transcript_seed. */
/* --ck (bin/src/main.rs:105): SonicKZG10 CommitterKey -> powers_of_g[0 .. min(count, max_powers)); max_powers = 0: all.
 * out_xy_mont = NULL: only *n_powers.  The prover needs n + 8 of the 4n + 1 powers the file holds. */
int zkt_keyfile_committer_key(const char* path, int curve_id, size_t max_powers, uint64_t* out_xy_mont, size_t* n_powers);
/* --pk (bin/src/main.rs:107): ProverKey<F> (keys/mod.rs:29-41) -> the ten coefficient vectors in zkt_circuit_load
 * order and their lengths; out_polys = NULL (or an entry NULL): lengths only. */
int zkt_keyfile_prover_key(const char* path, int curve_id, uint64_t* const* out_polys, size_t* lens10);
/* --vk (bin/src/main.rs:111): VerifierKey (keys/mod.rs:180-210) -> n, pi_roots, the ten commitments (x, y) in
 * zkt_transcript_seed order with their infinity flags. */
int zkt_keyfile_verifier_key(const char* path, int curve_id, uint64_t* n, uint64_t* pi_roots_mont, size_t pi_cap, size_t* n_pi,
                             uint64_t* commitments_xy_mont, int* is_infinity10);
/* --epk (bin/src/main.rs:34-35,108-109): ExtendedProverKey<F> (keys/mod.rs:148-174) = seventeen Vec<F> in declaration
 * order: arith { q_m_coset q_l_coset q_r_coset q_o_coset q_c_coset }, lookup { q_lookup q_lookup_coset q_table_coset },
 * perm { sigma1 sigma1_coset sigma2 sigma2_coset sigma3 sigma3_coset x_coset }, zh_coset, l_1_coset (4n values each, n
 * for q_lookup and the three sigma vectors).  This library never NEEDS the file: zkt_circuit_load derives the extended
 * key from the ProverKey on the device in milliseconds, where the file of an n = 2^20 circuit holds 1.9 GB.  It is read
 * so that a file the reference wrote can be checked against that derivation.
 * zkt_keyfile_extended_prover_key: the seventeen lengths, and vector `which` (0 .. 16; -1: lengths only) as Montgomery
 * limbs into out_mont (cap elements); streamed, nothing else is held in memory.
 * zkt_circuit_check_epk_file: every vector of the file against the loaded circuit's own extended key, recomputed on the
 * device.  *first_mismatch_vector = -1: identical; otherwise the vector (0 .. 16) and *mismatch_at the first differing
 * element, or (size_t)-1 when the vector's length is not this circuit's.  Unsharded contexts only; not during a proof. */
#define ZKT_EPK_VECTORS 17
int zkt_keyfile_extended_prover_key(const char* path, int curve_id, int which, uint64_t* out_mont, size_t cap, size_t* lens17);
int zkt_circuit_check_epk_file(zkt_ctx* ctx, const char* epk_path, int* first_mismatch_vector, size_t* mismatch_at);
/* the two loads a prover service does at start-up, straight from the CLI's files */
int zkt_srs_load_file(zkt_ctx* ctx, const char* ck_path, size_t max_powers);
int zkt_circuit_load_file(zkt_ctx* ctx, const char* pk_path, int log_n);

/* ---- the keys that setup makes, and the files of the reference CLI's `Compile` ------------------------------------
 * proof_system::setup (setup.rs:42-166) returns a ProverKey, a VerifierKey and an ExtendedProverKey; `Compile`
 * (bin/src/main.rs:105-111) writes them with the CommitterKey to --ck / --pk / --vk / --epk.  zkt_circuit_setup /
 * zkt_circuit_setup_wiring return the VerifierKey's commitments and keep the rest in HBM; the entries below bring all
 * of it out, whichever way the circuit was loaded (zkt_circuit_load, _load_file, _setup, _setup_wiring).  All of them
 * synchronise and write to host memory or files; after any of them the next zkt_prove gives the bytes it would have
 * given.  The file layouts are those of the readers above: restated from ark-serialize / ark-poly-commit 0.3 and
 * pinned to the writer in oracle/keyfile.py and to those readers, not to a file the reference made ("parity
 * unpinned").
 *
 * zkt_circuit_export -- the ProverKey (setup.rs:72-101, keys/mod.rs:29-41): the ten polynomials in zkt_circuit_load
 * order as coefficients in Montgomery limbs.  lens10[k] is the length DensePolynomial::from_coefficients_vec leaves
 * (trailing zeros stripped, the zero polynomial 0), taken on the device, whatever lengths the load was given.
 * out_polys = NULL or an entry NULL: no download for it (lengths only); an entry holds n elements.  Read-only on the
 * keys and free of the work buffers: allowed on forks, on sharded contexts (the polynomials are replicated) and while a
 * next proof is announced.
 * zkt_circuit_commitments -- the VerifierKey's commitments (setup.rs:104-121 PC::commit, keys/mod.rs:196-210) of the
 * loaded circuit under the loaded SRS, in the format of zkt_circuit_setup's outputs ((0, 0) and the flag for the
 * identity): what a context started from a --pk file needs to seed its transcript.  The same commit stage as
 * zkt_circuit_setup, over the trimmed lengths: the SRS must be as long as the longest polynomial
 * (ZKT_ERR_TOO_MANY_COEFFICIENTS otherwise).
 * zkt_circuit_export_epk -- the ExtendedProverKey (keys/mod.rs:78-174): vector `which` (0 .. 16, arkworks' order, see
 * zkt_keyfile_extended_prover_key; -1: lengths only) in Montgomery limbs into out_mont (cap elements; too few ->
 * ZKT_ERR_INVALID_ARGUMENT) and the seventeen lengths.  The derivation is the one zkt_circuit_check_epk_file compares
 * a file with.
 * zkt_circuit_check_vk_file -- a --vk file (bin/src/main.rs:111) against the loaded circuit under the loaded SRS:
 * *first_mismatch = -1 identical, 0 .. 9 the first differing commitment, 10 another n.
 * The last three (and the file writers below that need them) use the per-proof work buffers: unsharded contexts only,
 * refused while a next proof is announced (zkt_prove_set_next); forks are fine. */
int zkt_circuit_export(zkt_ctx* ctx, uint64_t* const* out_polys, size_t* lens10);
int zkt_circuit_commitments(zkt_ctx* ctx, uint64_t* out_commitments, int* out_is_infinity);
int zkt_circuit_export_epk(zkt_ctx* ctx, int which, uint64_t* out_mont, size_t cap, size_t* lens17);
int zkt_circuit_check_vk_file(zkt_ctx* ctx, const char* vk_path, int* first_mismatch);
/* Host-only writers of the three small files, from Montgomery limbs.  Each writes a temporary sibling of `path` and
 * renames it: a failed call leaves neither a truncated key file nor the temporary one.  A limb vector that is not
 * below its modulus -> ZKT_ERR_INVALID_ARGUMENT (our readers refuse such values, so every file written can be read
 * back); so is a file that cannot be written.  zkt_keyfile_last_error: the calling thread's last writer failure, a
 * text that names the path ("" after a success).
 * --ck (bin/src/main.rs:105; plonk.rs:79-85 PC::trim): powers_of_g = the count >= 1 points, an empty powers_of_gamma_g,
 * shifted_powers_of_g / shifted_powers_of_gamma_g / enforced_degree_bounds = None, max_degree = count - 1.  An all-zero
 * (x, y) is the identity, as the reader returns it, written as GroupAffine::zero() = (0, 1) with the infinity flag.
 * --pk (bin/src/main.rs:107; keys/mod.rs:29-41): ten LabeledPolynomial labelled as in setup.rs:92-101, degree_bound and
 * hiding_bound None; lens10[k] coefficients each, written as given (zkt_circuit_export's are trimmed).
 * --vk (bin/src/main.rs:111; keys/mod.rs:180-210): n, pi_roots (n_pi > 0 needs them), the ten commitments;
 * is_infinity10 may be NULL when (0, 0) alone marks the identity. */
const char* zkt_keyfile_last_error(void);
int zkt_keyfile_write_committer_key(const char* path, int curve_id, const uint64_t* g1_xy_mont, size_t count);
int zkt_keyfile_write_prover_key(const char* path, int curve_id, const uint64_t* const* polys, const size_t* lens10);
int zkt_keyfile_write_verifier_key(const char* path, int curve_id, uint64_t n, const uint64_t* pi_roots_mont, size_t n_pi,
                                   const uint64_t* commitments_xy_mont, const int* is_infinity10);
/* Files straight from the device; errors name the path in zkt_last_error.
 * zkt_srs_save_file -- --ck (bin/src/main.rs:105): the first `count` loaded powers (0: all), downloaded a block at a
 * time.  Unsharded contexts only.
 * zkt_circuit_write_epk_file -- --epk (bin/src/main.rs:108-109): the seventeen vectors streamed through two pinned
 * chunks (the next chunk's copy and the next vector's transform run while the current chunk is written); host memory
 * is the two chunks, where the file of an n = 2^20 circuit holds 1.9 GB.
 * zkt_circuit_save_files -- --pk / --vk / --epk (bin/src/main.rs:107-111) of the loaded circuit; a NULL path is
 * skipped.  The vk's pi_roots are w^pos (keys/mod.rs:186-188), w = zkt_domain_group_gen(log_n), for the n_pi
 * public-input positions: ascending, distinct and below n, otherwise ZKT_ERR_INVALID_ARGUMENT and nothing is written.
 * A --pk alone needs neither an SRS nor an unsharded context. */
int zkt_srs_save_file(zkt_ctx* ctx, const char* ck_path, size_t count);
int zkt_circuit_write_epk_file(zkt_ctx* ctx, const char* epk_path);
int zkt_circuit_save_files(zkt_ctx* ctx, const char* pk_path, const char* vk_path, const char* epk_path, const size_t* pi_pos,
                           size_t n_pi);

/* ---- debug / test support ------------------------------------------------------------------ */
/* Dumps the compiled-in parameter tables (modulus, -p^-1 mod 2^32, R, R^2) as u32 words for
 * which = 0 (Fr) or 1 (Fq) of the context's curve; returns the limb count. */
int zkt_debug_params(zkt_ctx* ctx, int which, uint32_t* out, size_t out_words);
/* Runs a field routine on the HOST (the same __host__ __device__ code the kernels execute) so that
 * the arithmetic can be pinned against big integers without a GPU.  which: 0 = Fr, 1 = Fq; a, b, out:
 * packed Montgomery words (8 or 12 x u32).  op 0: product; 1: 32-bit-limb reference product;
 * 2: arkworks form -> 29-bit limbs -> arkworks form; 3: 3*(a^2 - b^2) through the lazy add/sub/mul path;
 * 4: a^-1 (host binary GCD); 5: a^-1 (the kernels' Fermat ladder); 6: a^2 + b^2 through the double product and
 * the squaring kernel; 7: (a - b) * b through the carry-free difference; 8 (nine-limb fields only): 2 (a - b) * y with
 * y the plain value of b, through the NTT butterfly's limb-wise sums, wide carry-free difference and the product by a
 * constant with a precomputed quotient (fx_mul_shoup); 9: 4 (a + b) through limb-wise sums and the lazy reduction. */
int zkt_host_field_op(int curve_id, int which, int op, const uint32_t* a, const uint32_t* b, uint32_t* out);
/* Sum of `count` affine G1 points on the HOST (x, y arkworks Montgomery limbs each; (0, 0) = identity): the combine
 * step of an MSM whose points are sharded across GPUs by index range (the partial sums are
 * all-gathered as raw bytes - no collective can reduce curve points - and added locally).  No context needed. */
int zkt_g1_sum_host(int curve_id, const uint64_t* points_xy_mont, size_t count, uint64_t* out_xy_mont, int* out_is_infinity);
/* Elementwise Fr product on the device (out[i] = a[i]*b[i], Montgomery); test hook for the field
 * kernels. Host pointers. */
int zkt_debug_fr_mul(zkt_ctx* ctx, const uint64_t* a, const uint64_t* b, size_t n, uint64_t* out);
/* Up to four transforms of one plan in one launch per pass, the way the prover's rounds issue them, and nothing else:
 * polynomial y reads in_len[y] <= 2^log_n elements of d_in[y] (the rest is zero) and writes 2^log_n to d_out[y]; the outputs
 * are distinct, d_out[y] == d_in[y] is allowed.  Device pointers, Montgomery words; enqueued on the context's stream.
 * nb outside 1 .. 4 -> ZKT_ERR_INVALID_ARGUMENT. */
int zkt_debug_ntt_batch(zkt_ctx* ctx, int log_n, int inverse, int coset, int nb, const void* const* d_in, const size_t* in_len,
                        void* const* d_out);
/* Overrides the pass radices of every transform above 2^10 that this context runs afterwards: npass = 2 or 3 passes of
 * 2^log_r[i] points, 5 <= log_r[i] <= 9, first pass first.  Tests use it to run every radix in every position at small
 * sizes; the policy alone reaches radix 2^9 only from 2^25.  npass = 0 restores the policy (log_r is ignored).  Plans built
 * under a split are kept apart from the policy's.  The prover's own transforms on this context obey the override too, at
 * sizes it does not fit they fail: do not run a proof under one, restore the policy first.  ZKT_ERR_INVALID_ARGUMENT:
 * another npass, a radix outside 5 .. 9, a forked context (it shares its root's plans); and, from the transform, a domain
 * size that is not the product of the radices.  (A tile that would not fit its pass is refused as well, but no two or
 * three radices of 2^5 and more have one: that check is a guard, not a reachable refusal.) */
int zkt_debug_ntt_split(zkt_ctx* ctx, int npass, const int* log_r);
/* The device allocations the library holds at this moment, over all contexts of the process: their number and their bytes
 * (contexts' buffers and caller allocations of zkt_dev_alloc, shared tables, NTT plans; no pinned host memory).  Leak tests
 * compare it before the first context is created and after the last is destroyed: unlike the card's free memory it does
 * not depend on other processes.  No context needed; null pointer -> ZKT_ERR_INVALID_ARGUMENT. */
int zkt_debug_live_allocations(uint64_t* count, uint64_t* bytes);
/* Overrides where the appends of this tree change from one launch per level to the single-workgroup tail: levels with at
 * least wide_min_parents parents are hashed by the wide kernel, the others by the tail kernel.  1 sends every level to the
 * wide kernel, INT_MAX every level to the tail kernel (up to the 512 parents a level of the tail may have: it keeps the
 * level in LDS, a wider one is a launch of its own whatever is asked), 0 restores the policy.  Tests use it to run both
 * kernels on every level of small trees.  A negative value gives ZKT_ERR_INVALID_ARGUMENT. */
int zkt_debug_merkle_tree_split(zkt_merkle_tree* tree, int wide_min_parents);
/* How many nodes one staging chunk of zkt_merkle_tree_save_file / _load_file holds, on this context: 0 restores the default
 * (2^16).  Tests shrink it so that a small file crosses several chunks.  Null context -> ZKT_ERR_INVALID_ARGUMENT. */
int zkt_debug_store_chunk(zkt_ctx* ctx, size_t nodes);
/* Self-check of the host pairing's shortcuts against their plain definitions (Frobenius maps = powers by p, sparse
 * and cyclotomic products = dense ones, the final exponentiation leaves an element of order r).  0 = all good. */
int zkt_debug_pairing_selftest(int curve_id);
/* The fused quotient pass alone (quotient_poly.rs:98-224), for per-kernel tests: t(x) on the 4n coset from the loaded
 * circuit's ExtendedProverKey and caller-supplied witness cosets.  challenges: alpha beta gamma delta epsilon (5 x 4
 * words); wit: nine HOST vectors of 4n elements in the order a b c pi z1 z2 t h1 h2 (quotient_poly.rs:52-96).  With
 * n_pi > 0 (at most 16) wit[3] is ignored and PI is evaluated the way the prover does for few public inputs, from
 * rotations of the l1 coset (pi_pos: gate indices, pi_vals: 4 words each).  out: 4n elements.  Everything in arkworks
 * Montgomery words.  Whole-coset (single-GPU) circuits only. */
int zkt_debug_quotient(zkt_ctx* ctx, const uint64_t* challenges, const uint64_t* const* wit, const uint64_t* pi_pos,
                       const uint64_t* pi_vals, size_t n_pi, uint64_t* out);
/* The quotient on three classes (zkt_ctx_set_quotient_route).  _top: the six top coefficients u = t_{3n} .. t_{3n+5} the
 * host formed for the last proof that took the route (6 x 4 words, zero before the first); *out_on_classes (may be NULL) = the last proof's
 * route.  _coeffs: the first `count` <= 4n elements of the quotient vector as the last proof left it (the coefficients
 * of t on either route).  _classes_host: the host arithmetic alone, no device and no context: windows = the
 * coefficients n - 6 .. n + 7 of a b c z1 z2 t sigma1 sigma2 sigma3 q_lookup (10 x 14 x 4 words), challenges = alpha
 * beta delta (3 x 4 words); out_u: 6 x 4 words; out_consts: 16 x 4 words: X^n on the classes 0..3, the inverse of the
 * Vandermonde matrix in the first three (row-major), the first three powers of the fourth.  Montgomery words. */
int zkt_debug_quotient_top(zkt_ctx* ctx, uint64_t* out_u, int* out_on_classes);
int zkt_debug_quotient_coeffs(zkt_ctx* ctx, uint64_t* out, size_t count);
int zkt_debug_quotient_classes_host(int curve, int log_n, const uint64_t* windows, const uint64_t* challenges, uint64_t* out_u,
                                    uint64_t* out_consts);
/* The two grand products alone over the loaded circuit's permutation and domain (rows a8 / a9: compute_z1_poly's and
 * compute_z2_poly's evaluation vectors, permutation/mod.rs:181-254, lookup/mod.rs:94-151), through the launches round 3 of
 * the prover makes.  challenges: beta gamma delta epsilon (4 x 4 words); vectors: a b c f t h1 h2, n elements each, host;
 * out_z1 / out_z2: n elements each.  Montgomery words. */
int zkt_debug_grand_products(zkt_ctx* ctx, const uint64_t* challenges, const uint64_t* const* vectors, uint64_t* out_z1,
                             uint64_t* out_z2);
/* Plookup's h1 / h2 alone (lookup/multiset.rs:103-146 combine_split with t = table padded by zeros to n), through
 * the prover's own round-2 code: the loaded circuit fixes n; f: n elements (what round 2 forms as q_lookup . c);
 * table: table_len < n distinct values in insertion order (zkt_prove_inputs.table); h1_out / h2_out: n elements each.
 * fresh = 0 reuses the sorted keys the previous call or proof left on the device, as a proof over an unchanged table
 * does (table is then ignored unless none are resident).  Errors as zkt_prove gives them: a value of f outside the
 * table -> ZKT_ERR_NOT_IN_TABLE, a repeated table value, table_len >= n or halves whose length is not n ->
 * ZKT_ERR_INVALID_ARGUMENT; no circuit -> ZKT_ERR_NOT_LOADED.  Refused while a next proof is announced
 * (zkt_prove_set_next); the next zkt_prove rebuilds its table polynomial and keys.  Host pointers, Montgomery words. */
int zkt_debug_combine_split(zkt_ctx* ctx, const uint64_t* table, size_t table_len, const uint64_t* f, int fresh,
                            uint64_t* h1_out, uint64_t* h2_out);
/* The prover's round-1 code alone (gather, transforms, the three wire commitments and their collection) on a variable
 * map and index vectors in HBM that need satisfy no circuit; the loaded circuit fixes n.  blinders: 6 x 4 words (two per
 * wire, a b c), host.  route 0 = through the coefficients, 1 = over the wire base tables where the rules of "Commitments
 * of evaluation vectors" allow them; out_route[k] = 1 when wire k's commitment is the one taken over its table.
 * out_xy: 3 x (x || y) Montgomery limbs, (0,0) and out_is_infinity[k] = 1 for the identity.  An index >= n_vars ->
 * ZKT_ERR_INVALID_ARGUMENT.  Synchronises the stream; refused while a next proof is announced (zkt_prove_set_next). */
int zkt_debug_commit_wires_dev(zkt_ctx* ctx, const void* d_variables, size_t n_vars, const uint32_t* d_w_l, const uint32_t* d_w_r,
                               const uint32_t* d_w_o, size_t n_rows, const uint64_t* blinders, int route, uint64_t* out_xy_mont,
                               int* out_is_infinity, int* out_route);
/* The same with route 2 as well: over the tables of the circuit's free variables, for a proof whose public inputs stand at
 * pi_pos[0 .. n_pi) (host).  The loaded circuit's selectors define the rows, so the points equal route 0's only for a
 * variable map that satisfies them; out_route[k] = 2 for a wire that went over free variables.  Routes 0 and 1 ignore
 * pi_pos and behave as zkt_debug_commit_wires_dev. */
int zkt_debug_commit_wires_pi_dev(zkt_ctx* ctx, const void* d_variables, size_t n_vars, const uint32_t* d_w_l, const uint32_t* d_w_r,
                                  const uint32_t* d_w_o, size_t n_rows, const uint64_t* blinders, int route, const size_t* pi_pos,
                                  size_t n_pi, uint64_t* out_xy_mont, int* out_is_infinity, int* out_route);
/* The host pass behind the tables over free variables, alone; needs no device and no context.  selectors: q_m q_l q_r q_o
 * q_c, n_rows x 4 Montgomery words each; w_l / w_r / w_o: n_rows indices each (ZKT_VARIABLE_ZERO allowed); pi_pos: the
 * proof's public-input positions; K in 1 .. 64: the support cap (the prover uses 16).  Outputs, caller-allocated:
 * out_kind[n_vars] (0 on no wire, 1 free, 2 defined), out_free[n_vars] (*out_n_free filled, in order of appearance), the
 * terms (v, f, M[v][f]) in out_term_v / out_term_f / out_term_coef (capacity K x n_vars; 4 Montgomery words a
 * coefficient; *out_n_terms filled; grouped by v in defining order, f ascending), out_kappa[n_vars x 4 words]
 * (zero for a variable that is not defined). */
int zkt_debug_wire_elimination(int curve, const uint64_t* const* selectors, const uint32_t* w_l, const uint32_t* w_r, const uint32_t* w_o,
                               size_t n_rows, size_t n_vars, const size_t* pi_pos, size_t n_pi, int K, uint8_t* out_kind,
                               uint32_t* out_free, size_t* out_n_free, uint32_t* out_term_v, uint32_t* out_term_f,
                               uint64_t* out_term_coef, size_t* out_n_terms, uint64_t* out_kappa);
/* The host planner behind zkt_witness_plan_create, alone (csrc/witness_plan.hpp); needs no device and no context.
 * selectors: q_m q_l q_r q_o q_c, n_rows x 4 Montgomery words each; wires: w_l w_r w_o, n_rows indices each (an index
 * >= n_vars is read as ZKT_VARIABLE_ZERO); pi_pos ascending and distinct (positions >= n_rows are ignored).  Outputs,
 * n_vars entries each: out_kind (0 on no wire, 1 free, 2 rule O, 3 rule R), out_def_row (the defining row, 0xFFFFFFFF when
 * none), out_level. */
int zkt_debug_witness_plan_host(int curve_id, const uint64_t* const* selectors, const uint32_t* const* wires, size_t n_rows,
                                size_t n_vars, const size_t* pi_pos, size_t n_pi, uint8_t* out_kind, uint32_t* out_def_row,
                                uint32_t* out_level);
/* The same under a choice of rules (ZKT_WITNESS_RULE_IS_ZERO or 0; 0 is the call above): out_kind also holds 4 and 5, and
 * both variables of a rule-Z pair carry the pair's first row in out_def_row. */
int zkt_debug_witness_plan_host_ex(int curve_id, const uint64_t* const* selectors, const uint32_t* const* wires, size_t n_rows,
                                   size_t n_vars, const size_t* pi_pos, size_t n_pi, uint32_t rules, uint8_t* out_kind,
                                   uint32_t* out_def_row, uint32_t* out_level);
/* Overrides the threshold between the two completion kernels for this plan: a level with at least wide_min_rows rows is a
 * launch of its own, the runs of narrower levels between such are one narrow launch each; a split of more than 64 launches
 * is one narrow launch altogether.  0 restores the policy.  zkt_witness_plan_info's `launches` follows. */
int zkt_debug_witness_plan_split(zkt_witness_plan* plan, uint32_t wide_min_rows);
/* kzg10's witness polynomial alone (row a12): out[0 .. len - 1) = (p(X) - p(z)) / (X - z) for the len <= n + 8 coefficients
 * p, as the prover computes it (scaled suffix sums).  Host pointers, Montgomery words. */
int zkt_debug_open_witness(zkt_ctx* ctx, const uint64_t* coeffs, size_t len, const uint64_t* z4, uint64_t* out);
/* Row a13's kernels alone (linearization_poly.rs:55-121): k <= 12 polynomials (lens[j] <= n + 8 coefficients, Montgomery words),
 * each evaluated at points[j] (out_evals: k x 4 words), and the first out_len coefficients of sum_j scalars[j] polys[j]. */
int zkt_debug_eval_lincomb(zkt_ctx* ctx, const uint64_t* const* polys, const size_t* lens, int k, const uint64_t* points,
                           const uint64_t* scalars, uint64_t* out_evals, uint64_t* out_lincomb, size_t out_len);

/* Raw-limb field and curve routines (csrc/fx.hpp, csrc/ecx.hpp) for tests at their stated bounds.  One dispatcher runs
 * either on the host (zkt_host_*: the C++ loops of the products, no GPU needed) or in a plain kernel, one record per
 * thread, on the context's stream (zkt_debug_*: the device's multiply-add chains).  Limbs are passed as given, never
 * normalised on the way in.  fx records: in = a, b, c, d of L words each (a packed operand in the first N words of its
 * slot), out = 4 L words (a packed result in the first N words, a predicate in word 0, the rest zero).  xyzz records (the
 * curve's base field): in = two points of 4 L + 1 words (x, y, zz, zzz, identity flag; an affine operand in the x, y
 * slots), out = one point.  which: 0 = Fr, 1 = Fq.  An op the field does not support returns ZKT_ERR_INVALID_ARGUMENT. */
enum zkt_fx_op {
    ZKT_FX_UNPACK = 0, ZKT_FX_UNPACK_SHIFT = 1, ZKT_FX_PACK = 2, ZKT_FX_FROM_ARK = 3, ZKT_FX_TO_ARK = 4,
    ZKT_FX_NORMALIZE = 5, ZKT_FX_ADD = 6, ZKT_FX_DBL = 7, ZKT_FX_SUB_1 = 8, ZKT_FX_SUB_2 = 9, ZKT_FX_SUB_4 = 10,
    ZKT_FX_SUB_8 = 11, ZKT_FX_SUB2_6 = 12, ZKT_FX_ADD_LAZY = 13, ZKT_FX_SUB_LAZY_3 = 14, ZKT_FX_SUB_LAZY_4 = 15,
    ZKT_FX_SUB_LAZY_5 = 16, ZKT_FX_SUB_LAZY_9 = 17, ZKT_FX_SUB_LAZY_WIDE_8_30 = 18, ZKT_FX_MUL = 19, ZKT_FX_MUL_INL = 20,
    ZKT_FX_SQR = 21, ZKT_FX_SQR_INL = 22, ZKT_FX_MUL2_INL = 23, ZKT_FX_MUL_SHOUP = 24 /* a x, b w, c wq */,
    ZKT_FX_MUL_LOW = 25, ZKT_FX_REDUCE_SMALL = 26, ZKT_FX_REDUCE_LAZY = 27 /* not on the 381-bit field */,
    ZKT_FX_COND_SUB_P = 28, ZKT_FX_CANON = 29, ZKT_FX_IS_ZERO_CANON = 30, ZKT_FX_IS_ZERO_LT2P = 31, ZKT_FX_OP_COUNT = 32
};
enum zkt_xyzz_op {
    ZKT_XYZZ_ADD_MIXED = 0, ZKT_XYZZ_ADD_MIXED_INL = 1, ZKT_XYZZ_ADD = 2, ZKT_XYZZ_ADD_INL = 3, ZKT_XYZZ_DOUBLE = 4,
    ZKT_XYZZ_DOUBLE_AFFINE = 5, ZKT_XYZZ_OP_COUNT = 6
};
/* limb count L, limb width and SH (R' = 2^(limb_bits L) = 2^(32 N + SH)) of a field's limb form; no context needed */
int zkt_debug_fx_layout(int curve_id, int which, int* limbs, int* limb_bits, int* sh);
int zkt_host_fx_op(int curve_id, int which, int op, const uint32_t* in, size_t n, uint32_t* out);
int zkt_debug_fx_op(zkt_ctx* ctx, int which, int op, const uint32_t* in, size_t n, uint32_t* out);
int zkt_host_xyzz_op(int curve_id, int op, const uint32_t* in, size_t n, uint32_t* out);
int zkt_debug_xyzz_op(zkt_ctx* ctx, int op, const uint32_t* in, size_t n, uint32_t* out);

#ifdef __cplusplus
}
#endif
#endif /* ZKT_PLONK_H */
