// The G1 MSM (msm.hip) and the Lagrange-basis table builder (lagrange.hip): the plan and state of both MSM paths (over the
// key's window table, over caller-supplied bases) and every entry point the other translation units call.
#pragma once
#include "ctx.hpp"

#include <functional>

namespace zkt {

// Grouped pairs per accumulation thread ("chunk").  It is chosen ON THE DEVICE from the number of pairs an MSM really has
// (zero digits are dropped, so a sparse scalar vector -- the differences of a piecewise-constant evaluation vector,
// lagrange.hip -- has few): chunk = max(ceil(pairs / acc_threads), lo), lo = isqrt(2 pairs / buckets) clamped to
// [1, MSM_CHUNK_MIN]: the length of a thread's serial chain and the pieces per bucket the fold has to add are balanced.
constexpr int MSM_CHUNK_MIN = 16;
constexpr int MSM_R2_BLOCKS = 1;     // partial sums per row handed to the host
constexpr int MSM_MAX_Y = 24;

// Window layout: W windows of width c or c-1 covering exactly lambda+1 bits, so that no window
// (in particular not the top one) is left with only a few significant bits: a 2-bit top window
// would pour n entries into 4 buckets.
struct MsmWindows {
    int W;
    uint8_t width[40];
    uint16_t start[40];
};

// What the grouping (two-level counting sort of (key, table index) pairs) and everything behind it is sized by, for
// either MSM path (msm_plan, msm.hip).  Over the key's window table all windows share ONE set of B = 2^(c-1) buckets and a
// pair's index addresses table[W][count]; over caller-supplied bases every window owns Bw = 2^(c-1) buckets of its own
// (keys 1 .. W Bw) and the index addresses the n bases.
struct MsmPlan {
    MsmWindows win{};
    int W = 0, c = 0;        // windows, widest digit
    int dig = 0;             // compile-time window layout of the level-1 kernels (0: generic; always 0 over supplied bases)
    uint32_t Bw = 0;         // buckets per window = 2^(c-1), ids 1..Bw
    uint32_t keys = 0;       // key range of the sort: Bw (shared buckets) or W Bw
    uint32_t lb = 8;         // level-2 key bits: key = (bin << lb) | low
    int lcols = 8;           // log2 columns of the level-2 tables (8, or 10 for more than 2^17 keys)
    bool packed = false;     // (low key, table index, sign) fit ONE 32-bit word: 4-byte pairs
    uint32_t nb1 = 0;        // level-1 bins
    uint32_t l1_scalars = 0; // scalars per level-1 workgroup
    uint32_t l2_items = 0;   // upper bound of level-2 tiles
};

constexpr int MSM_BATCH = 3;         // MSMs whose grouping and accumulation go out as ONE launch per kernel (blockIdx.y = MSM)
// Per-MSM arguments of a batched launch.  The main-stream work buffers (pairs, grouped indices, count tables) exist
// MSM_BATCH times, `s_*` apart; what the side stream reads later (offsets, pieces, params, heavy list) belongs to a slot.
struct MsmBatch {
    const void* scalars[MSM_BATCH];
    uint64_t n[MSM_BATCH];
    uint64_t base_off[MSM_BATCH];
    const void* table[MSM_BATCH];    // the base table each MSM runs against (the key's powers or the Lagrange-prefix table)
    uint64_t tcount[MSM_BATCH];      // ... and its bases per window
    uint32_t* heavy[MSM_BATCH];
    uint32_t* params[MSM_BATCH];
    uint32_t* offsets[MSM_BATCH];
    void* pieces[MSM_BATCH];
    uint64_t s_bin_offs, s_bin_aux, s_bin, s_tile_desc, s_cnt, s_pairs_bytes, s_vals, s_chunk;   // strides, in elements (pairs: bytes)
    uint32_t vb_stride;              // variable-base MSM (zkt_msm_g1_bases): buckets per window; unused by the SRS path
};

constexpr int MSM_TAIL_BATCH = 6;    // bucket folds / reductions that go out as ONE launch per kernel (blockIdx.y = slot)
struct MsmTailBatch {                // per-slot arguments of a batched tail
    const uint32_t* offsets[MSM_TAIL_BATCH];
    const uint32_t* params[MSM_TAIL_BATCH];
    const void* pieces[MSM_TAIL_BATCH];
    void* buckets[MSM_TAIL_BATCH];
    uint32_t* heavy[MSM_TAIL_BATCH];
    void* rowcol[MSM_TAIL_BATCH];
    void* partials[MSM_TAIL_BATCH];
};

constexpr int MSM_HEAVY = 32;       // buckets with more pieces than this are folded by a whole block
constexpr int MSM_HEAVY_BLOCKS = 64;     // grid-stride over the (normally empty) list of crowded buckets

// Wire base tables (lagrange.hip): a wire's evaluation vector is a gather of the variable map, a[i] = variables[w[i]], so
// its commitment is  sum_v variables[v] T_v  with  T_v = sum_{i : w[i] = v} [L_i(tau)] G  -- one scalar per DISTINCT variable
// of the wire.  The tables depend on the key and the wiring only; they are keyed on the index vectors' addresses and
// sizes, the key and the domain, and carry a digest of the vectors' contents that every proof checks.
struct WireBases {
    std::shared_ptr<DevShared> mem;   // owns table[] and u[]; a context forked after the build reads them through it
    void* table[3] = {};       // Affine[W][cnt + 2]: T of every distinct variable (ascending), then the two blinder points
    uint32_t* u[3] = {};       // the cnt distinct variables, ascending
    size_t cnt[3] = {};
    bool use[3] = {};          // false: the wire is committed through its coefficients (too many distinct variables, ...)
    // Tables over the circuit's FREE variables (lagrange.hip): u holds the free variables that reach the wire, the table their
    // points A_f, then the constant point C when has_c, then the two blinder points
    bool elim[3] = {};
    bool has_c[3] = {};
    bool elim_wanted = false;  // part of the key: the build was asked to eliminate, for the public-input positions below
    std::vector<size_t> pi_pos;   // ascending
    bool built = false;        // the key below was examined (use[] says what came of it)
    bool stale = false;        // a proof found other index contents than the digest: rebuild before the next use
    const void* w[3] = {};
    size_t n_rows = 0, n_vars = 0;
    int log_n = -1;
    uint64_t srs_generation = 0;
    uint64_t digest[2] = {};
};
constexpr int MSM_TBL_WIRE = 2;      // msm_begin tbl = MSM_TBL_WIRE + k: the table of wire k (0 left, 1 right, 2 output)

// Second base table (lagrange.hip): prefix sums of the Lagrange-basis key of the domain of size 2^lag_log_n followed by
// the blinder points, same window layout, count2 <= count bases.  Commitments of polynomials given by their
// evaluations go through it (msm_begin table = 1).  Null until a circuit of that size asks for it.
struct LagrangeTable {
    std::shared_ptr<DevShared> lag_mem;   // owns table2
    void* table2 = nullptr;
    size_t count2 = 0;
    int lag_log_n = -1;
    bool lag_failed = false;       // the key is too short (or sharded): evaluations are committed through their coefficients
};

struct MsmState : LagrangeTable {
    // owns everything below that is this context's alone: work buffers, slots, pinned rows, the side stream, events
    DevSet work;
    explicit MsmState(int device) : work(device) {}
    size_t count = 0;      // bases loaded
    // index-range sharding: this GPU holds powers [slice_off, slice_off + count) of a key of `total`
    size_t slice_off = 0, total = 0;
    MsmPlan plan;          // window and sort layout for `count` bases (shared buckets)
    uint32_t* heavy[11] = {};   // per slot: [0] = count, [1..] = heavy bucket ids
    // The key's window table.  It, the Lagrange table and the wire tables are read-only once built: a fork reads its
    // source's through holders of its own (zkt_ctx_fork), everything else below is each context's own.
    std::shared_ptr<DevShared> table_mem;
    void* table = nullptr; // Affine[W][count]
    WireBases wb;
    DevBuf wb_scalars[3];          // per wire: cnt + 2 scalars of the proof being enqueued (read by its grouping launches only)
    uint64_t* wb_dig = nullptr;    // device: the digest kernel's two sums
    uint64_t* wb_pin = nullptr;    // pinned: [0..1] digest of the proof in flight, [2..3] the three trimmed lengths (32-bit)
    // the base table and its bases per window behind a `tbl` selector
    const void* tbl_table(int tbl) const { return tbl >= MSM_TBL_WIRE ? wb.table[tbl - MSM_TBL_WIRE] : tbl ? table2 : table; }
    size_t tbl_count(int tbl) const {
        return tbl >= MSM_TBL_WIRE ? wb.cnt[tbl - MSM_TBL_WIRE] + (wb.has_c[tbl - MSM_TBL_WIRE] ? 1 : 0) + 2 : tbl ? count2 : count;
    }
    uint32_t* params[11] = {};     // per slot, device: [0] chunk, [1] pairs (written by k_msm_scan_aux)
    // work buffers (sized for n = count)
    uint32_t* vals2 = nullptr;                     // table indices grouped by bucket
    void* pairs = nullptr;                         // uint2[m]: after the level-1 split
    uint32_t* bin_offs = nullptr;                  // [nb1][blocks] level-1 counts, scanned per 4096-tile
    uint32_t* bin_aux = nullptr;                   // tile totals, scanned; last = number of pairs
    uint32_t *bin_start = nullptr, *tile_start = nullptr;   // nb1 + 1 each: level-2 work list
    void* tile_desc = nullptr;                     // uint2[l2_items]: pair range of every level-2 tile
    uint32_t *cnt2 = nullptr, *pos2 = nullptr;     // [level-2 tiles][256]
    uint32_t* chunk_bucket = nullptr;              // bucket of the first pair of every accumulation chunk
    MsmBatch strides{};                            // the s_* members: distance between the work buffers of a batch's MSMs
    // per slot, because the bucket fold that reads them runs on the side stream while the next MSM is already grouping
    uint32_t* offsets[11] = {};   // B + 2
    void* pieces[11] = {};        // XyzzRaw[max_chunks + B + 2]
    // The latency-bound tail of an MSM (bucket reduction) runs on a side stream so that it overlaps the
    // next MSM's accumulation; each in-flight MSM owns one slot of tail buffers.
    static constexpr int SLOTS = 11;
    void* buckets[SLOTS] = {};      // Xyzz[B + 1]
    void* rowcol[SLOTS] = {};       // Xyzz[NI + NJ]: row / column sums of the bucket matrix
    void* host_result[SLOTS] = {};  // pinned: the (rows + 1) x R2_BLOCKS partial sums the host finishes
    void* host_result_dev[SLOTS] = {};  // the same memory as the kernels address it
    size_t acc_lds = 0;            // dynamic LDS of k_msm_accumulate (0; ZKT_MSM_ACC_LDS caps its residency in experiments)
    size_t acc_threads = 196608;   // chunks an MSM is cut into: resident threads of k_msm_accumulate (occupancy query) x 2
    hipStream_t side = nullptr;
    hipEvent_t ev_main[SLOTS] = {}, ev_done[SLOTS] = {};
    bool pending[SLOTS] = {};
    // Small keys (count <= MSM_DEFER_MAX): a proof is then a chain of latencies, and the bucket reduction of every
    // commitment of a round is the same ~25 dependent curve operations whether one launch sequence covers one slot or six:
    // the tails are deferred and issued once per round, batched (msm_flush_tails).  Large keys keep a tail per enqueue: it
    // overlaps the next commitment's accumulation instead of the transforms behind the round.
    bool defer_tails = false;
    int tail_wait[SLOTS] = {};     // slots whose accumulation is enqueued and whose tail is not, in order
    int n_tail_wait = 0;
};

// Scratch of zkt_msm_g1_bases (variable-base MSM over the caller's points, msm.hip): buffers of its own, allocated on the
// first call and grown when a call needs more, so that the call never touches the prover's slots, work set or tables.
struct MsmBasesState {
    DevSet mem;   // owns every buffer below and the pinned partial sums
    explicit MsmBasesState(int device) : mem(device) {}
    DevBuf bases;     // the call's points in the accumulation's packed R' form
    DevBuf scalars;   // zkt_msm_g1_bases: the uploaded scalars
    DevBuf vals, pairs, bin_offs, bin_aux, bin_start, tile_start, tile_desc, cnt2, pos2, chunk_bucket;   // grouping
    DevBuf offsets, heavy, params, pieces, buckets, rowcol;                                              // accumulation, tail
    DevBuf check_points, check_status;   // zkt_g1_check / zkt_srs_check (g1check.hip): a chunk uploaded from the host; totals and status bytes
    void* partials = nullptr;      // pinned: W x (c) rows of partial sums the host combines (Horner over the windows)
    void* partials_dev = nullptr;
    size_t acc_lds = 0, acc_threads = 0;   // as MsmState's
};

constexpr size_t MSM_DEFER_MAX = ((size_t)1 << 16) + 64;      // small key: latency regime (tails deferred and batched)
constexpr size_t MSM_TAIL_INL_MAX = ((size_t)1 << 18) + 64;   // up to here the bucket reduction's additions inline their products

// ---- msm.hip ----
// the key: `count` powers from the host or the device / generated from a trapdoor (test, bench); slice_off, total: this
// GPU's index range of a sharded key (total = 0: the whole key)
int srs_load(zkt_ctx* c, const void* src, size_t count, bool on_device, size_t slice_off = 0, size_t total = 0);
int srs_generate(zkt_ctx* c, const uint64_t* tau4, size_t count, size_t slice_off = 0, size_t total = 0);
void msm_release(zkt_ctx* c);
bool msm_tables_have_readers(const zkt_ctx* c);   // a fork still reads the key's, the Lagrange or the wire tables of `c`
// window multiples + R' conversion of an affine base table whose first `count` entries are filled (arkworks R form)
int msm_table_finish(zkt_ctx* c, void* table, size_t count);
// `child` gets an MSM state of its own (work buffers, slots, side stream) over `parent`'s base tables (zkt_ctx_fork)
int msm_fork(zkt_ctx* child, const zkt_ctx* parent);
void msm_slice(zkt_ctx* c, size_t* off, size_t* count, size_t* total);
// one MSM, begun and collected
int msm_g1_dev(zkt_ctx* c, const void* d_scalars, size_t n, size_t base_off, int mont, uint64_t* out_xy, int* out_inf);
// zkt_msm_g1_bases: sum scalars[i] * bases[i] over the caller's affine points (host or device memory each), affine result in
// host memory; n <= ZKT_MSM_BASES_MAX is checked here.  Synchronises the stream.
int msm_bases(zkt_ctx* c, const void* bases, bool bases_on_device, const void* scalars, bool scalars_on_device, size_t n, int mont,
              uint64_t* out_xy, int* out_inf);
// the context's MsmBasesState, made on first use (g1check.hip keeps its chunk buffers and the powers of rho there)
int msm_bases_scratch(zkt_ctx* c, MsmBasesState** out);
// prover-facing batch form: begin up to MsmState::SLOTS commitments, then collect them (tbl = 1: the Lagrange-prefix
// table of lagrange.hip, tbl = MSM_TBL_WIRE + k: the base table of wire k)
int msm_begin(zkt_ctx* c, const void* d_scalars, size_t n, size_t base_off, int mont, int slot, int tbl = 0);
int msm_begin_batch(zkt_ctx* c, int k, const void* const* d_scalars, const size_t* ns, int mont, const int* slots, const int* tbls);
// a round's queued commitments: batches of MSM_BATCH launches-as-one when `grouped`, then the deferred tails; ready(j),
// when given, runs before the MSM of entry j is enqueued
int msm_begin_many(zkt_ctx* c, int k, const void* const* d_scalars, const size_t* ns, int mont, const int* slots, const int* tbls,
                   bool grouped, const std::function<int(int)>& ready = {});
int msm_end(zkt_ctx* c, int slot, uint64_t* out_xy);
int msm_end_sharded(zkt_ctx* c, const int* slots, const bool* have, int k, uint64_t* out_xy /* k x 12 words */);
// issues the deferred tails (no-op when none are waiting); the prover calls it behind the last commitment of a round
int msm_flush_tails(zkt_ctx* c);
bool msm_defers_tails(const zkt_ctx* c);
bool msm_batches_grouping(const zkt_ctx* c);   // a round's commitments are grouped as one batch of launches (small keys, and 2^18)

// ---- lagrange.hip ----
int lagrange_ensure(zkt_ctx* c, int log_n);
bool lagrange_ready(const zkt_ctx* c, int log_n);
size_t lagrange_bases(const zkt_ctx* c);
// Wire base tables.  _prepare makes the tables of these index vectors current (builds them when the key, the vectors'
// addresses or sizes changed or a proof found them stale; synchronises the stream then) -- ZKT_OK also when none can be
// had; wire_bases_use tells per wire.  _digest enqueues the digest of the vectors' present contents (into pinned
// memory), _lens the copy of the three trimmed lengths; _scalars the gather of wire k's scalars; once the stream has
// passed them, _check compares: false = wire k has to be committed again through its coefficients.
// `elim`, when given, asks for tables over the circuit's free variables where they shrink a wire: the key's selector
// coefficients q_m q_l q_r q_o q_c (device, zero-padded to the domain) and the proof's public-input positions (host).  The
// positions are compared in every call; other positions rebuild the tables.  _route: 0 coefficients, 1 the wire's
// per-variable table, 2 its table over free variables.
struct WireElimKeys {
    const void* pk[5];
    const size_t* pi_pos;
    size_t n_pi;
};
int wire_bases_prepare(zkt_ctx* c, int log_n, const uint32_t* const* d_idx, size_t n_rows, size_t n_vars, const WireElimKeys* elim = nullptr);
bool wire_bases_use(const zkt_ctx* c, int k);
int wire_bases_route(const zkt_ctx* c, int k);
int wire_bases_digest(zkt_ctx* c, const uint32_t* const* d_idx, size_t n_rows);
int wire_bases_lens(zkt_ctx* c, const uint32_t* d_lens);
int wire_bases_scalars(zkt_ctx* c, int k, const void* d_vars, const void* d_blinders, size_t n, const void** out, size_t* len);
bool wire_bases_check(zkt_ctx* c, int k, size_t n);
void wire_bases_drop(zkt_ctx* c);

}  // namespace zkt
