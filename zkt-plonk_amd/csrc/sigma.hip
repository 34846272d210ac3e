// The sigma evaluations from the circuit's wiring: permutation/mod.rs:76-177 (add_variables_to_map,
// compute_sigma_permutations, compute_all_sigma_evals) on the device.
//
// Number the wires p = 3 g + col (gate-major: Left, Right, Output of gate 0, then gate 1, ...).  The reference keeps, per
// variable, the list of its wires in insertion order, which is rising p, and maps every wire to the next one of its list,
// the last to the first.  So sigma is "the next p with the same variable, cyclically": a STABLE sort of the 3 n_rows
// positions by variable, then a neighbour lookup in the sorted order.
//
//   k_sigma_keys     key[p] = 0 for Variable::Zero, v + 1 for variable v (so bit_length(n_vars) bits carry information);
//                    an index outside the map raises the flag and is sorted with Variable::Zero, so that every row is
//                    still written
//   LSD radix sort   8 bits per pass, only the passes the key width needs.  Per pass: a digit histogram per workgroup
//                    (k_sigma_hist), one exclusive scan over (digit, workgroup) (k_scan_*), the scatter (k_sigma_scatter).
//                    The first pass takes its values implicitly: the value is the position.
//   k_sigma_link     next[p]: the following slot's position when it holds the same key, else the first of the run
//                    (found by a binary search in the sorted keys, by the run's last slot alone)
//   k_sigma_eval     sigma_col[g] = k_col' * w^g' of the target (col', g'); rows >= n_rows map to themselves
//
// Nothing here depends on scheduling: the histograms are sums, and the scatter ranks an element inside its workgroup by
// wave ballots and a per-wave count table walked in wave order, never by the arrival order of an atomic.
#include "poly.hpp"

#include <algorithm>

namespace zkt {

constexpr int SG_THREADS = 256;
constexpr int SG_ROUNDS = 8;                        // a workgroup's tile: SG_ROUNDS rounds of SG_THREADS consecutive slots
constexpr int SG_TILE = SG_THREADS * SG_ROUNDS;
constexpr int SG_SCAN_CHUNK = SG_THREADS * 8;       // histogram entries one workgroup of the scan takes

__global__ __launch_bounds__(SG_THREADS) void k_sigma_keys(const uint32_t* w_l, const uint32_t* w_r, const uint32_t* w_o, uint32_t rows,
                                                           uint32_t n_vars, uint32_t* keys, uint32_t* flag) {
    const uint32_t g = blockIdx.x * SG_THREADS + threadIdx.x;
    if (g >= rows) return;
    const uint32_t v[3] = {w_l[g], w_r[g], w_o[g]};
#pragma unroll
    for (int col = 0; col < 3; ++col) {
        uint32_t k = 0;
        if (v[col] != ZKT_VARIABLE_ZERO) {
            if (v[col] < n_vars) k = v[col] + 1;
            else atomicOr(flag, 1u);
        }
        keys[3 * g + col] = k;
    }
}

// hist[d * nb + workgroup] = number of the workgroup's keys with digit d
__global__ __launch_bounds__(SG_THREADS) void k_sigma_hist(const uint32_t* keys, uint32_t count, int shift, uint32_t* hist, uint32_t nb) {
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t tile = blockIdx.x * SG_TILE;
#pragma unroll
    for (int r = 0; r < SG_ROUNDS; ++r) {
        const uint32_t i = tile + r * SG_THREADS + threadIdx.x;
        if (i < count) atomicAdd(&h[(keys[i] >> shift) & 255u], 1u);   // a count: the order of the additions is immaterial
    }
    __syncthreads();
    hist[threadIdx.x * nb + blockIdx.x] = h[threadIdx.x];
}

// exclusive scan of x over the workgroup's 256 threads; *total = the sum
__device__ __forceinline__ uint32_t sg_block_scan(uint32_t x, uint32_t* sh, uint32_t* total) {
    const int t = threadIdx.x;
    sh[t] = x;
    __syncthreads();
#pragma unroll
    for (int off = 1; off < SG_THREADS; off <<= 1) {
        const uint32_t y = t >= off ? sh[t - off] : 0u;
        __syncthreads();
        sh[t] += y;
        __syncthreads();
    }
    const uint32_t incl = sh[t];
    *total = sh[SG_THREADS - 1];
    __syncthreads();
    return incl - x;
}
// The scan of `a` (a multiple of SG_SCAN_CHUNK entries) in three launches: chunk sums, their scan by one workgroup, the
// scan inside every chunk on top of its offset.
__global__ __launch_bounds__(SG_THREADS) void k_scan_reduce(const uint32_t* a, uint32_t* sums) {
    __shared__ uint32_t sh[SG_THREADS];
    const uint4* q = reinterpret_cast<const uint4*>(a + (size_t)blockIdx.x * SG_SCAN_CHUNK) + 2 * threadIdx.x;
    const uint4 u = q[0], v = q[1];
    uint32_t total;
    (void)sg_block_scan(u.x + u.y + u.z + u.w + v.x + v.y + v.z + v.w, sh, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}
__global__ __launch_bounds__(SG_THREADS) void k_scan_top(uint32_t* sums, uint32_t count) {
    __shared__ uint32_t sh[SG_THREADS];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < count; base += SG_THREADS) {
        const uint32_t i = base + threadIdx.x;
        uint32_t total;
        const uint32_t ex = sg_block_scan(i < count ? sums[i] : 0u, sh, &total);
        if (i < count) sums[i] = carry + ex;
        carry += total;
    }
}
__global__ __launch_bounds__(SG_THREADS) void k_scan_apply(uint32_t* a, const uint32_t* sums) {
    __shared__ uint32_t sh[SG_THREADS];
    uint4* q = reinterpret_cast<uint4*>(a + (size_t)blockIdx.x * SG_SCAN_CHUNK) + 2 * threadIdx.x;
    const uint4 u = q[0], v = q[1];
    uint32_t total;
    const uint32_t e0 = sums[blockIdx.x] + sg_block_scan(u.x + u.y + u.z + u.w + v.x + v.y + v.z + v.w, sh, &total);
    const uint32_t e1 = e0 + u.x, e2 = e1 + u.y, e3 = e2 + u.z, e4 = e3 + u.w, e5 = e4 + v.x, e6 = e5 + v.y, e7 = e6 + v.z;
    q[0] = make_uint4(e0, e1, e2, e3);
    q[1] = make_uint4(e4, e5, e6, e7);
}

// One pass of the sort.  `start` is the scanned histogram: start[d * nb + workgroup] = first output slot of the workgroup's
// keys with digit d.  The workgroup walks its tile in rounds of 256 consecutive slots; inside a round an element's slot is
//     base[d] + (elements with digit d in the waves before its own) + (lanes with digit d below its own in its wave),
// the last from a ballot per digit bit, the middle from the per-wave counts in LDS: the input order inside each digit is
// kept whatever the waves' timing.  vals_in == nullptr: the value is the position.
__global__ __launch_bounds__(SG_THREADS) void k_sigma_scatter(const uint32_t* keys_in, const uint32_t* vals_in, uint32_t count, int shift,
                                                              const uint32_t* start, uint32_t nb, uint32_t* keys_out,
                                                              uint32_t* vals_out) {
    constexpr int WAVES = SG_THREADS / 64;
    __shared__ uint32_t base[256];
    __shared__ uint32_t wcnt[WAVES][256];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    base[t] = start[(size_t)t * nb + blockIdx.x];
#pragma unroll
    for (int w = 0; w < WAVES; ++w) wcnt[w][t] = 0;
    __syncthreads();
    const uint32_t tile = blockIdx.x * SG_TILE;
#pragma unroll 1
    for (int r = 0; r < SG_ROUNDS; ++r) {
        const uint32_t first = tile + r * SG_THREADS;
        if (first >= count) break;   // the same in every thread
        const uint32_t i = first + t;
        const bool valid = i < count;
        const uint32_t k = valid ? keys_in[i] : 0u;
        const uint32_t v = valid ? (vals_in ? vals_in[i] : i) : 0u;
        const uint32_t d = (k >> shift) & 255u;
        unsigned long long same = __ballot(valid);   // the valid lanes of this wave that hold digit d
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long m = __ballot(bit);
            same &= bit ? m : ~m;
        }
        const uint32_t rank = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
        if (valid && rank == 0) wcnt[wave][d] = (uint32_t)__popcll(same);
        __syncthreads();
        if (valid) {
            uint32_t off = base[d] + rank;
#pragma unroll
            for (int w = 0; w < WAVES; ++w)
                if (w < wave) off += wcnt[w][d];
            if (off < count) {   // always, when `start` is the scan of this pass's own histogram
                keys_out[off] = k;
                vals_out[off] = v;
            }
        }
        __syncthreads();
        uint32_t sum = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            sum += wcnt[w][t];
            wcnt[w][t] = 0;
        }
        base[t] += sum;
        __syncthreads();
    }
}

// next[p] for the position p of sorted slot s: the next slot's position inside a run of equal keys, the run's first
// position from its last slot (vals == nullptr: the order is the identity)
__global__ __launch_bounds__(SG_THREADS) void k_sigma_link(const uint32_t* keys, const uint32_t* vals, uint32_t count, uint32_t* next) {
    const uint32_t s = blockIdx.x * SG_THREADS + threadIdx.x;
    if (s >= count) return;
    const uint32_t k = keys[s];
    const uint32_t p = vals ? vals[s] : s;
    uint32_t to;
    if (s + 1 < count && keys[s + 1] == k) {
        to = s + 1;
    } else if (s == 0 || keys[s - 1] != k) {
        to = s;                              // a run of one
    } else {
        uint32_t lo = 0, hi = s;             // the first slot that holds k: keys[lo - 1] < k <= keys[hi]
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (keys[mid] < k) lo = mid + 1;
            else hi = mid;
        }
        to = lo;
    }
    if (p < count) next[p] = vals ? vals[to] : to;
}

// permutation/mod.rs:139-177: sigma_col[g] = k_c * w^r for the target (c, r) of wire (col, g), k = (1, K1, K2)
template <class P>
__global__ __launch_bounds__(SG_THREADS) void k_sigma_eval(const uint32_t* next, uint32_t rows, const Fe<P>* roots, uint32_t n, Fe<P> k1,
                                                           Fe<P> k2, Fe<P>* s1, Fe<P>* s2, Fe<P>* s3) {
    const uint32_t g = blockIdx.x * SG_THREADS + threadIdx.x;
    if (g >= n) return;
    Fe<P>* const out[3] = {s1, s2, s3};
#pragma unroll
    for (uint32_t col = 0; col < 3; ++col) {
        uint32_t r = g, c = col;
        if (g < rows) {
            const uint32_t q = next[3 * g + col];
            r = q / 3;
            c = q - 3 * r;
        }
        Fe<P> x = fe_load<P>(roots + (r < n ? r : g));
        if (c) x = fe_mul<P>(x, c == 1 ? k1 : k2);
        fe_store<P>(out[col] + g, x);
    }
}

namespace {
// how the launches below carve the caller's block: every part starts on a 256-byte boundary
struct SigmaLayout {
    uint32_t count, nb, nchunks;
    size_t hist_len;
    size_t roots, keys[2], vals[2], hist, sums, total;
    SigmaLayout(int log_n, size_t n_rows) {
        const size_t n = (size_t)1 << log_n;
        count = (uint32_t)(3 * n_rows);                                                 // log_n <= 25: below 2^32
        nb = (count + SG_TILE - 1) / SG_TILE;
        hist_len = ((size_t)256 * nb + SG_SCAN_CHUNK - 1) / SG_SCAN_CHUNK * SG_SCAN_CHUNK;
        nchunks = (uint32_t)(hist_len / SG_SCAN_CHUNK);
        size_t at = 0;
        auto take = [&](size_t bytes) {
            const size_t here = at;
            at += (bytes + 255) / 256 * 256;
            return here;
        };
        roots = take(n * 32);
        for (int k = 0; k < 2; ++k) {
            keys[k] = take((size_t)count * 4);
            vals[k] = take((size_t)count * 4);
        }
        hist = take(hist_len * 4);
        sums = take((size_t)nchunks * 4);
        total = at + 256;
    }
};
}  // namespace

size_t sigma_scratch_bytes(int log_n, size_t n_rows) { return SigmaLayout(log_n, n_rows).total; }

template <class P>
static int sigma_enqueue_t(zkt_ctx* c, int log_n, const uint32_t* d_w_l, const uint32_t* d_w_r, const uint32_t* d_w_o, size_t n_rows,
                           size_t n_vars, void* const* d_sigma, void* d_scratch, uint32_t* flag) {
    const size_t n = (size_t)1 << log_n;
    const SigmaLayout L(log_n, n_rows);
    const uint32_t count = L.count, nb = L.nb, nchunks = L.nchunks;
    const uint32_t vars = (uint32_t)std::min<size_t>(n_vars, 0xFFFFFFFFu);         // keys v + 1 stay 32-bit
    int key_bits = 0;
    while (key_bits < 32 && ((uint64_t)vars >> key_bits)) ++key_bits;               // keys are 0 .. vars
    const int npass = (key_bits + 7) / 8;

    char* const base = (char*)d_scratch;
    Fe<P>* const roots = (Fe<P>*)(base + L.roots);
    uint32_t* const keys[2] = {(uint32_t*)(base + L.keys[0]), (uint32_t*)(base + L.keys[1])};
    uint32_t* const vals[2] = {(uint32_t*)(base + L.vals[0]), (uint32_t*)(base + L.vals[1])};
    uint32_t* const hist = (uint32_t*)(base + L.hist);
    uint32_t* const sums = (uint32_t*)(base + L.sums);
    int rc;
    if (count) {
        // the scan works on whole chunks: the tail behind the 256 nb real entries only has to be defined (what a scan
        // leaves there comes after every real entry, so it reaches none of them in the next pass)
        ZKT_HIP(c, hipMemsetAsync(hist, 0, L.hist_len * 4, c->stream));
    }
    const Fe<P> one = fe_one<P>(), w = root_of_unity<P>(log_n);
    if ((rc = gen_powers(c, roots, n, w.v, one.v))) return rc;                      // domain.elements()
    {
        ProfScope prof(c, "sigma");
        const uint32_t* sorted_keys = nullptr;
        const uint32_t* sorted_vals = nullptr;   // nullptr: the identity order
        uint32_t* next = nullptr;
        if (count) {
            const uint32_t rows = (uint32_t)n_rows;
            hipLaunchKernelGGL(k_sigma_keys, dim3((rows + SG_THREADS - 1) / SG_THREADS), dim3(SG_THREADS), 0, c->stream, d_w_l, d_w_r,
                               d_w_o, rows, vars, keys[0], flag);
            ZKT_HIP(c, hipGetLastError());
            int cur = 0;
            for (int pass = 0; pass < npass; ++pass, cur ^= 1) {
                const int shift = 8 * pass;
                hipLaunchKernelGGL(k_sigma_hist, dim3(nb), dim3(SG_THREADS), 0, c->stream, (const uint32_t*)keys[cur], count, shift,
                                   hist, nb);
                hipLaunchKernelGGL(k_scan_reduce, dim3(nchunks), dim3(SG_THREADS), 0, c->stream, (const uint32_t*)hist, sums);
                hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(SG_THREADS), 0, c->stream, sums, nchunks);
                hipLaunchKernelGGL(k_scan_apply, dim3(nchunks), dim3(SG_THREADS), 0, c->stream, hist, (const uint32_t*)sums);
                hipLaunchKernelGGL(k_sigma_scatter, dim3(nb), dim3(SG_THREADS), 0, c->stream, (const uint32_t*)keys[cur],
                                   pass ? (const uint32_t*)vals[cur] : (const uint32_t*)nullptr, count, shift,
                                   (const uint32_t*)hist, nb, keys[cur ^ 1], vals[cur ^ 1]);
                ZKT_HIP(c, hipGetLastError());
            }
            sorted_keys = keys[cur];
            sorted_vals = npass ? vals[cur] : nullptr;
            next = vals[cur ^ 1];
            hipLaunchKernelGGL(k_sigma_link, dim3((count + SG_THREADS - 1) / SG_THREADS), dim3(SG_THREADS), 0, c->stream, sorted_keys,
                               sorted_vals, count, next);
            ZKT_HIP(c, hipGetLastError());
        }
        hipLaunchKernelGGL(k_sigma_eval<P>, dim3((unsigned)((n + SG_THREADS - 1) / SG_THREADS)), dim3(SG_THREADS), 0, c->stream,
                           (const uint32_t*)next, (uint32_t)n_rows, (const Fe<P>*)roots, (uint32_t)n, fe_from_u32<P>(7),
                           fe_from_u32<P>(13), (Fe<P>*)d_sigma[0], (Fe<P>*)d_sigma[1], (Fe<P>*)d_sigma[2]);   // permutation/constants.rs K1, K2
        ZKT_HIP(c, hipGetLastError());
    }
    return ZKT_OK;
}

int sigma_enqueue(zkt_ctx* c, int log_n, const uint32_t* d_w_l, const uint32_t* d_w_r, const uint32_t* d_w_o, size_t n_rows, size_t n_vars,
                  void* const* d_sigma, void* d_scratch, uint32_t* d_flag) {
    return c->curve == ZKT_CURVE_BN254 ? sigma_enqueue_t<Bn254Fr>(c, log_n, d_w_l, d_w_r, d_w_o, n_rows, n_vars, d_sigma, d_scratch, d_flag)
                                       : sigma_enqueue_t<Bls381Fr>(c, log_n, d_w_l, d_w_r, d_w_o, n_rows, n_vars, d_sigma, d_scratch, d_flag);
}

// zkt_circuit_sigma_dev / zkt_circuit_setup_wiring: scratch of the call's own, released (after the stream has drained)
// when the call returns
static int sigma_build_run(zkt_ctx* c, int log_n, const uint32_t* d_w_l, const uint32_t* d_w_r, const uint32_t* d_w_o, size_t n_rows,
                           size_t n_vars, void* const* d_sigma, bool* bad_index) {
    DevSet tmp(c->device);
    void* block = nullptr;
    int rc = tmp.alloc(c, &block, sigma_scratch_bytes(log_n, n_rows));
    if (rc) return rc;
    struct Drain {   // declared behind `tmp`: it runs first
        zkt_ctx* c;
        ~Drain() { (void)hipStreamSynchronize(c->stream); }
    } drain{c};
    // the flag lives in the block's spare last 256 bytes
    uint32_t* flag = (uint32_t*)((char*)block + sigma_scratch_bytes(log_n, n_rows) - 256);
    ZKT_HIP(c, hipMemsetAsync(flag, 0, 4, c->stream));
    if ((rc = sigma_enqueue(c, log_n, d_w_l, d_w_r, d_w_o, n_rows, n_vars, d_sigma, block, flag))) return rc;
    uint32_t h_flag = 0;
    ZKT_HIP(c, hipMemcpyAsync(&h_flag, flag, 4, hipMemcpyDeviceToHost, c->stream));
    ZKT_HIP(c, hipStreamSynchronize(c->stream));
    *bad_index = h_flag != 0;
    return ZKT_OK;
}

int sigma_build(zkt_ctx* c, int log_n, const uint32_t* d_w_l, const uint32_t* d_w_r, const uint32_t* d_w_o, size_t n_rows, size_t n_vars,
                void* const* d_sigma) {
    if (log_n < 0 || log_n > 25) return set_err(c, ZKT_ERR_INVALID_DOMAIN_SIZE, "InvalidEvalDomainSize: the wiring's positions are 32-bit (log_n <= 25)");
    if (n_rows > ((size_t)1 << log_n)) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "more wiring rows than the domain size");
    if (!d_sigma || !d_sigma[0] || !d_sigma[1] || !d_sigma[2] || (n_rows && (!d_w_l || !d_w_r || !d_w_o)))
        return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    bool bad = false;
    const int rc = sigma_build_run(c, log_n, d_w_l, d_w_r, d_w_o, n_rows, n_vars, d_sigma, &bad);
    if (rc) return rc;
    if (bad) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "wiring index outside the variable map: every entry must be < n_vars or ZKT_VARIABLE_ZERO");
    return ZKT_OK;
}

}  // namespace zkt

using namespace zkt;

extern "C" int zkt_circuit_sigma_dev(zkt_ctx* c, int log_n, const uint32_t* d_w_l, const uint32_t* d_w_r, const uint32_t* d_w_o,
                                     size_t n_rows, size_t n_vars, void* const* d_sigma) {
    if (!c) return ZKT_ERR_INVALID_ARGUMENT;
    (void)hipSetDevice(c->device);
    return sigma_build(c, log_n, d_w_l, d_w_r, d_w_o, n_rows, n_vars, d_sigma);
}
