// Library context: one per caller thread / proof stream (SURVEY.md section 8b "Threading").
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <map>
#include <string>
#include <tuple>
#include <vector>
#include <memory>

#include "../../include/zkt_plonk.h"
#include "fp.hpp"
#include "fx.hpp"
#include "ntt.hpp"

namespace zkt {

struct MsmState;      // msm.hip
struct MsmBasesState; // msm.hip (zkt_msm_g1_bases)
struct KzgState;      // kzg.hip (zkt_kzg_commit_batch / zkt_kzg_open)
struct CircuitState;  // circuit.hpp

// Everything one owner takes from the runtime and gives back together: device memory, pinned memory, streams, events.
// A state's work set, a function's temporaries and the context's own allocations are each one of these, so nothing is
// released by hand: what the set made goes with the set.
struct DevSet {
    const int device;
    std::vector<std::pair<void*, size_t>> mem;   // device allocations with their sizes (zkt_debug_live_allocations counts them)
    std::vector<void*> host;
    std::vector<hipStream_t> streams;
    std::vector<hipEvent_t> events;
    explicit DevSet(int dev) : device(dev) {}
    DevSet(const DevSet&) = delete;
    DevSet& operator=(const DevSet&) = delete;
    // waits for the streams it made, then: events, streams, pinned memory, device memory.  Work on any other stream that
    // still uses the set is the caller's to wait for.
    ~DevSet() { clear(); }
    void clear();
    // each sets c's error as ZKT_HIP does
    int alloc(zkt_ctx* c, void** p, size_t bytes);
    void release(void* p);                           // one device allocation ahead of the rest
    int pinned(zkt_ctx* c, void** p, size_t bytes, unsigned flags = 0);
    int stream(zkt_ctx* c, hipStream_t* s);          // non-blocking
    int event(zkt_ctx* c, hipEvent_t* e);            // timing disabled
};
// scratch that is allocated on first use and grown when a call needs more (grow), in the set of whoever uses it
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
};

}  // namespace zkt

struct zkt_ctx {
    int curve = 0;
    const int device;
    explicit zkt_ctx(int dev) : device(dev), owned(dev) {}
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string err;

    // NTT plans keyed by (log_n, inverse, coset, split); tables live in HBM for the ctx lifetime.  split: 0 = the policy's
    // radices, otherwise the forced ones of zkt_debug_ntt_split (ntt_split_code), so the two never serve each other.
    // A plan owns its tables (NttPlan::mem), so the pointers a fork copies keep them alive.
    // (A fork copies the map, forced plans included; its own split stays 0, so it never looks one of those up.)
    std::map<std::tuple<int, int, int, int>, std::shared_ptr<void>> ntt_plans;
    int ntt_split_npass = 0;                 // zkt_debug_ntt_split: 0 = policy, else 2 or 3 passes of ntt_split_log_r
    int ntt_split_log_r[3] = {0, 0, 0};
    // scratch (grown on demand, never shrunk)
    zkt::DevBuf ntt_scratch, io_a, io_b;
    zkt::DevBuf check_scratch;    // zkt_circuit_check_witness (check.hip): the call's own, never shared with a fork
    zkt::DevBuf verify_scratch;   // zkt_g1_decompress / zkt_verify_batch_dev (g1decomp.hip, verify.hip): the call's own

    // optional per-kernel HIP-event timing (bench.py's live roofline measurement)
    int prof_on = 0;   // 0 off, 1 every scope, 2 only the dominant kernel's scope ("msm_accumulate")
    struct ProfSlot {
        std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
        double total_ms = 0.0;
        uint64_t calls = 0;      // units (a batched launch of three MSMs counts three)
        uint64_t launches = 0;   // scopes recorded (zkt_profile_get "<name>#launches")
    };
    std::map<std::string, ProfSlot> prof;
    std::vector<hipEvent_t> event_pool;

    // Communicator of a proof sharded across GPUs (zkt_ctx_set_comm); world == 1: single GPU
    struct Comm {
        zkt_comm_vtable vt{};
        void* pinned = nullptr;      // staging of device exchanges when the communicator takes host buffers only
        size_t pinned_bytes = 0;
        uint64_t calls = 0, bytes = 0;
    } comm;
    bool sharded() const { return comm.vt.world > 1; }

    std::shared_ptr<zkt::MsmState> msm;
    std::shared_ptr<zkt::MsmBasesState> msmb;   // zkt_msm_g1_bases scratch (separate from the prover's MSM state)
    std::shared_ptr<zkt::KzgState> kzg;         // KZG seam scratch: copy stream, open buffers (never forked)
    size_t srs_check_chunk = 0;                 // zkt_debug_srs_check_chunk: points per chunk of zkt_srs_check, 0 = ZKT_MSM_BASES_MAX
    size_t store_chunk = 0;                     // zkt_debug_store_chunk: nodes per staging chunk of the tree-file entries, 0 = the default
    uint64_t msm_epoch = 0;   // bumped by every MSM enqueue and SRS (re)load: work issued ahead of time is tied to it
    uint64_t srs_generation = 0;   // bumped by every SRS (re)load: cached commitments are tied to the key they were made under
    bool is_fork = false;     // made by zkt_ctx_fork: no forced NTT split, no communicator
    bool aux_off = false;          // A/B builds: ZKT_NO_AUX keeps round 5's second opening on the main stream
    bool batch_off = false;        // A/B builds: ZKT_MSM_NO_BATCH commits a round's polynomials one launch sequence each
    bool lagrange_off = false;     // zkt_ctx_set_lagrange(ctx, 0): evaluations are committed through their coefficients
    int wire_elim_mode = 1;        // zkt_ctx_set_wire_elimination: 0 off, 1 automatic (large circuits), 2 whenever a table can be built
    int quotient_route = 0;        // zkt_ctx_set_quotient_route: 0 automatic (three classes on large single-GPU circuits), 1 three classes, 2 the whole coset
    int verify_terms_mode = 0;     // zkt_ctx_set_verify_terms: the batch verifier's transcripts and scalar stage, 0 on the host, 1 on the device
    int fused_passes = 0;          // zkt_ctx_set_fused_passes: 0 automatic (fused), 1 fused, 2 one launch per step (the reference sequence)
    // the parts of the fused sequences, one bit each: 1 = round 5's openings, 2 = round 3's grand products, 4 = blinding,
    // 8 = the classes route's three classes in one grid (transforms and quotient kernel), 16 = its closing pass (combine,
    // split and the tail's zeros in one kernel), 32 = round 3's four scans of the block totals in one launch
    // (A/B builds: ZKT_FUSED_PARTS picks the parts that modes 0 and 1 fuse)
    int fused_parts = 63;
    bool fused(int part) const { return fused_passes != 2 && (fused_parts & part); }
    std::shared_ptr<zkt::CircuitState> circuit;
    zkt::DevSet owned;   // every dev_alloc made on behalf of this ctx: scratch, caller buffers, Poseidon / Merkle handles
};

namespace zkt {

// Experiment knobs (A/B runs of tools/ab_*.sh) are read from the environment ONLY by libraries built with
// -DZKT_EXPERIMENTS (zkt-plonk_amd/build.py build_experiments() -> _ab/libzkt_exp.so); the shipped library never looks
// at the environment, so a stray variable cannot change or break a proof.
const char* exp_env(const char* name);

int set_err(zkt_ctx* c, int code, const std::string& msg);
// ZKT_ERR_INVALID_ARGUMENT while a context forked from `c` still reads one of c's key or circuit tables
int refuse_if_forked(zkt_ctx* c, const char* what);
int hip_fail(zkt_ctx* c, hipError_t e, const char* what);

#define ZKT_HIP(c, call)                                        \
    do {                                                        \
        hipError_t _e = (call);                                 \
        if (_e != hipSuccess) return zkt::hip_fail((c), _e, #call); \
    } while (0)

// Records a start/stop HIP event pair on the context's stream around a launch (or a group of
// launches) when profiling is on; durations are resolved lazily by zkt_profile_get.
struct ProfScope {
    zkt_ctx* c;
    zkt_ctx::ProfSlot* slot = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipStream_t stream = nullptr;
    uint64_t count = 1;   // units the scope stands for (a batch of transforms is counted per transform)
    ProfScope(zkt_ctx* ctx, const char* name, hipStream_t on_stream = nullptr, uint64_t units = 1);
    ~ProfScope();
};

// all-gather through the context's communicator: `bytes` per rank, rank order.  _host: host buffers;
// _dev: device buffers, ordered after everything enqueued on the context's stream, complete on return
int comm_all_gather_host(zkt_ctx* c, const void* send, void* recv, size_t bytes);
int comm_all_gather_dev(zkt_ctx* c, const void* d_send, void* d_recv, size_t bytes);
// the communicator's optional stream-ordered entry (zkt_comm_vtable::all_gather_async): enqueued on `st`, no host wait
bool comm_async_available(const zkt_ctx* c);
int comm_all_gather_async(zkt_ctx* c, const void* d_send, void* d_recv, size_t bytes, hipStream_t st);

// grows `b` to at least `bytes`, in the set that owns it (the context's unless named); waits for c's stream before a
// buffer that exists is replaced
int grow(zkt_ctx* c, DevBuf& b, size_t bytes, DevSet* in = nullptr);
inline int dev_alloc(zkt_ctx* c, void** p, size_t bytes) { return c->owned.alloc(c, p, bytes); }
inline void dev_free(zkt_ctx* c, void* p) { c->owned.release(p); }

// Device memory that several contexts may read (zkt_ctx_fork): tables that are complete before a second context sees
// them.  It belongs to no context: it is held through shared_ptr and freed with the last holder, in whatever order the
// contexts go.  A fork does not copy its source's pointer, it reads through a holder of its own that keeps the source's
// alive (dev_shared_reader), so use_count() > 1 on a context's holder means exactly: a context forked from this one, or
// from one forked from it, still reads these tables.
struct DevShared : DevSet {
    using DevSet::DevSet;
    std::shared_ptr<DevShared> from;   // a fork's holder: the tables are this one's
};
inline std::shared_ptr<DevShared> dev_shared_reader(const std::shared_ptr<DevShared>& of) {
    if (!of) return nullptr;
    auto r = std::make_shared<DevShared>(of->device);
    r->from = of;
    return r;
}
inline bool dev_shared_has_readers(const std::shared_ptr<DevShared>& m) { return m && m.use_count() > 1; }

// ntt.hip
template <class P>
Fe<P> root_of_unity(int log_n);
// coset: 0 none, 1 the generator g, ntt_class_code(log_big, cls) a class of a larger coset (see ntt.hip)
int ntt_run(zkt_ctx* c, int log_n, int inverse, int coset, const void* d_in, size_t in_len, void* d_out);
// nb <= NTT_MAX_BATCH transforms of one plan, one launch per pass; distinct outputs, out[y] == in[y] allowed
// d_head (forward only): NTT_HEAD elements per polynomial that stand in for its coefficients 0 .. NTT_HEAD - 1
int ntt_run_batch(zkt_ctx* c, int log_n, int inverse, int coset, int nb, const void* const* d_in, const size_t* in_len,
                  void* const* d_out, const void* d_head = nullptr);
// heads of nb polynomials of n + NTT_HEAD coefficients folded modulo X^n - gammas[j], j < 3 (host, 8 words each), into
// d_out[(j * NTT_MAX_BATCH + y) * NTT_HEAD + i]: what ntt_run_batch takes as d_head for class j
int ntt_fold_heads(zkt_ctx* c, int nb, const void* const* d_in, size_t n, const uint32_t* gammas, void* d_out);
// ntt_run_batch for the three cosets `codes` at once, one launch per pass (the grid's z = class): class j reads
// d_in[y] + j * in_stride and writes d_out[y] + j * out_stride (strides in elements; in_stride = 0 shares the inputs).  In
// place as ntt_run_batch allows, the ranges of different (y, j) disjoint.  d_head: the whole output of ntt_fold_heads.
int ntt_run_classes(zkt_ctx* c, int log_n, int inverse, const int codes[3], int nb, const void* const* d_in, const size_t* in_len,
                    void* const* d_out, size_t in_stride, size_t out_stride, const void* d_head = nullptr);
int ntt_class_code(int log_big, int cls);
// zkt_debug_ntt_split: npass = 0 restores the policy; transforms above 2^10 built afterwards use the given radices
int ntt_force_split(zkt_ctx* c, int npass, const int* log_r);
int ntt_run_class(zkt_ctx* c, int log_n, int log_big, int cls, const void* d_in, size_t in_len, void* d_out, void* d_fold);

// circuit.hip (the state and what else its units share: circuit.hpp)
void circuit_release(zkt_ctx* c);
// a circuit state of its own over the parent's read-only tables (zkt_ctx_fork)
int circuit_fork(zkt_ctx* child, const zkt_ctx* parent);
bool circuit_tables_have_readers(const zkt_ctx* c);

}  // namespace zkt
