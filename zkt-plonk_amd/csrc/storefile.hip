// The two store files of the reference CLI (include/zkt_plonk.h, "(4b) The store files"; byte layouts: storefile.hpp): the
// note tree written from and rebuilt into HBM, with every node the file claims compared against the rebuilt tree on the
// device, and the host-only readers and writers of the notes file.
#include "ctx.hpp"
#include "keyfile.hpp"
#include "merkle_tree.hpp"
#include "storefile.hpp"

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

namespace zkt {

constexpr size_t STORE_CHUNK_NODES = (size_t)1 << 16;   // 3 MiB of file entries, 2 MiB of layer nodes a staging buffer

static size_t store_chunk(const zkt_ctx* c) { return c->store_chunk ? c->store_chunk : STORE_CHUNK_NODES; }

// the scalar of file entry t (48 bytes: layer, idx, 32 canonical little-endian bytes), in Montgomery form
template <class P>
ZKT_D Fe<P> store_entry_scalar(const uint64_t* nodes, uint64_t t) {
    Fe<P> x;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint64_t w = nodes[6 * t + 2 + k];
        x.v[2 * k] = (uint32_t)w;
        x.v[2 * k + 1] = (uint32_t)(w >> 32);
    }
    return fe_to_mont<P>(x);
}

// the file's layer 0 (its first `count` entries: the keys ascend) as the leaves of an append
template <class P>
__global__ __launch_bounds__(256) void k_store_leaves(const uint64_t* nodes, uint64_t count, Fe<P>* leaves) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    fe_store<P>(leaves + t, store_entry_scalar<P>(nodes, t));
}

template <class P>
struct StoreCompareArgs {
    const uint64_t* nodes;       // n file entries; the last is the root, given the key (height, 0)
    uint64_t n;
    const Fe<P>* const* layers;  // the rebuilt tree's layers
    const Fe<P>* root;
    uint32_t height;
    unsigned long long* out;     // [0] mismatching nodes, [1] the smallest mismatching key, [2] the root differs
};

constexpr int STORE_KEY_SHIFT = 56;   // a key packs as layer << 56 | idx: layer < 64, idx < ZKT_MERKLE_TREE_MAX = 2^24

// A lane per node of the file: every key was checked on the host to lie inside the rebuilt tree's stored nodes.
template <class P>
__global__ __launch_bounds__(256) void k_store_compare(StoreCompareArgs<P> a) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.n) return;
    const uint64_t layer = a.nodes[6 * t], idx = a.nodes[6 * t + 1];
    const bool is_root = t == a.n - 1;
    if (!is_root && layer >= a.height) return;   // never: the host refuses such a key before anything goes up
    const Fe<P> mine = fe_load<P>(is_root ? a.root : a.layers[layer] + idx);
    if (fe_eq<P>(store_entry_scalar<P>(a.nodes, t), mine)) return;
    if (is_root) {
        a.out[2] = 1;
        return;
    }
    atomicAdd(a.out, 1ull);
    atomicMin(a.out + 1, (unsigned long long)((layer << STORE_KEY_SHIFT) | idx));
}

static int store_tree_check(zkt_ctx* c, const zkt_merkle_tree* t) {
    if (!c || !t) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (t->curve != c->curve) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "merkle tree: the tree belongs to another curve");
    return ZKT_OK;
}

static int store_save(zkt_ctx* c, zkt_merkle_tree* t, const char* path) {
    const kw::Field& fr = kw::field(c->curve, false);
    const size_t chunk = store_chunk(c);
    DevSet tmp(c->device);
    uint64_t* h = nullptr;
    if (int rc = tmp.pinned(c, (void**)&h, std::max<size_t>(chunk, 1) * 32)) return rc;
    kw::File w(path);
    sf::write_tree_head(w, sf::dense_entries(t->count, t->height));
    size_t layer_off = 0;
    for (int L = 0; L < t->height && w.ok(); ++L) {
        const uint64_t len = sf::dense_layer_len(t->count, L);
        for (uint64_t first = 0; first < len && w.ok(); first += chunk) {
            const size_t cnt = (size_t)std::min<uint64_t>(chunk, len - first);
            ZKT_HIP(c, hipMemcpyAsync(h, (const char*)t->d_nodes + (layer_off + first) * 32, cnt * 32, hipMemcpyDeviceToHost, c->stream));
            ZKT_HIP(c, hipStreamSynchronize(c->stream));
            for (size_t i = 0; i < cnt && w.ok(); ++i) sf::write_tree_entry(w, fr, (uint64_t)L, first + i, h + 4 * i);
        }
        layer_off += t->layer_len[L];
    }
    ZKT_HIP(c, hipMemcpyAsync(h, t->d_root, 32, hipMemcpyDeviceToHost, c->stream));
    ZKT_HIP(c, hipStreamSynchronize(c->stream));
    sf::write_tree_tail(w, fr, h, t->count);
    return keyfile_write_done(c, w);
}

template <class P>
static int store_rebuild_and_compare_t(zkt_ctx* c, zkt_merkle_tree* t, const uint64_t* d_nodes, uint64_t entries, uint64_t count, void* d_leaves,
                                       unsigned long long* d_out) {
    if (count) {
        {
            ProfScope ps(c, "store_leaves");
            hipLaunchKernelGGL((k_store_leaves<P>), dim3((unsigned)((count + 255) / 256)), dim3(256), 0, c->stream, d_nodes, count, (Fe<P>*)d_leaves);
            ZKT_HIP(c, hipGetLastError());
        }
        if (int rc = zkt_merkle_tree_append_dev(c, t, d_leaves, (size_t)count, nullptr)) return rc;
    }
    StoreCompareArgs<P> a{};
    a.nodes = d_nodes;
    a.n = entries + 1;
    a.layers = (const Fe<P>* const*)t->d_layers;
    a.root = (const Fe<P>*)t->d_root;
    a.height = (uint32_t)t->height;
    a.out = d_out;
    ProfScope ps(c, "store_compare");
    hipLaunchKernelGGL((k_store_compare<P>), dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, c->stream, a);
    ZKT_HIP(c, hipGetLastError());
    return ZKT_OK;
}

static int store_load(zkt_ctx* c, const zkt_poseidon* pos, int height, size_t capacity, const char* path, zkt_merkle_tree** out,
                      zkt_tree_file_report* report) {
    const kw::Field& fr = kw::field(c->curve, false);
    sf::TreeFile file;
    auto refused = [&]() { return keyfile_refused(c, sf::refusal_message(path, file.kind(), file.offset())); };
    if (!file.open(path, fr, height, capacity)) return refused();
    const uint64_t entries = file.entries(), count = file.next_index();
    const size_t chunk = store_chunk(c);
    // A dense file of next_index <= capacity leaves holds fewer than 2 capacity + height entries.  One that announces more
    // gets no device memory: the same chunked parse names what is wrong with it (at the latest, next_index above the capacity).
    if (entries > 2 * (uint64_t)capacity + (uint64_t)height) {
        std::vector<uint8_t> buf(chunk * sf::TREE_ENTRY_BYTES);
        while (file.next(buf.data(), chunk)) {}
        file.finish();
        return refused();
    }
    DevSet tmp(c->device);
    uint8_t* h[2] = {};
    hipEvent_t up[2] = {};
    uint64_t* d_nodes = nullptr;
    void* d_leaves = nullptr;
    unsigned long long* d_out = nullptr;
    unsigned long long* h_out = nullptr;
    zkt_merkle_tree* t = nullptr;
    auto run = [&]() -> int {
        int rc;
        for (int k = 0; k < 2; ++k) {
            if ((rc = tmp.pinned(c, (void**)&h[k], chunk * sf::TREE_ENTRY_BYTES))) return rc;
            if ((rc = tmp.event(c, &up[k]))) return rc;
        }
        if ((rc = tmp.pinned(c, (void**)&h_out, 3 * sizeof(unsigned long long) + sf::TREE_ENTRY_BYTES))) return rc;
        if ((rc = tmp.alloc(c, (void**)&d_nodes, (size_t)(entries + 1) * sf::TREE_ENTRY_BYTES))) return rc;
        if ((rc = tmp.alloc(c, &d_leaves, std::max<size_t>((size_t)std::min<uint64_t>(count, entries), 1) * 32))) return rc;
        if ((rc = tmp.alloc(c, (void**)&d_out, 3 * sizeof(unsigned long long)))) return rc;
        // the entries, chunk by chunk: read and checked in one pinned buffer while the other one's copy is on its way
        {
            ProfScope ps(c, "store_upload");
            uint64_t done = 0;
            bool busy[2] = {};
            for (int k = 0;; k ^= 1) {
                if (busy[k]) ZKT_HIP(c, hipEventSynchronize(up[k]));
                busy[k] = false;
                const size_t cnt = file.next(h[k], chunk);
                if (cnt == 0) break;
                ZKT_HIP(c, hipMemcpyAsync((char*)d_nodes + done * sf::TREE_ENTRY_BYTES, h[k], cnt * sf::TREE_ENTRY_BYTES, hipMemcpyHostToDevice,
                                          c->stream));
                ZKT_HIP(c, hipEventRecord(up[k], c->stream));
                busy[k] = true;
                done += cnt;
            }
        }
        if (!file.finish()) return refused();
        // the root rides along as one more node, keyed (height, 0)
        uint8_t* h_root = (uint8_t*)(h_out + 3);
        sf::put64(h_root, (uint64_t)height);
        sf::put64(h_root + 8, 0);
        memcpy(h_root + 16, file.root(), 32);
        h_out[0] = 0;
        h_out[1] = ~0ull;
        h_out[2] = 0;
        ZKT_HIP(c, hipMemcpyAsync((char*)d_nodes + entries * sf::TREE_ENTRY_BYTES, h_root, sf::TREE_ENTRY_BYTES, hipMemcpyHostToDevice, c->stream));
        ZKT_HIP(c, hipMemcpyAsync(d_out, h_out, 3 * sizeof(unsigned long long), hipMemcpyHostToDevice, c->stream));
        if ((rc = zkt_merkle_tree_create(c, pos, height, capacity, &t))) return rc;   // waits for the copies above
        rc = c->curve == ZKT_CURVE_BN254 ? store_rebuild_and_compare_t<Bn254Fr>(c, t, d_nodes, entries, count, d_leaves, d_out)
                                         : store_rebuild_and_compare_t<Bls381Fr>(c, t, d_nodes, entries, count, d_leaves, d_out);
        if (rc) return rc;
        ZKT_HIP(c, hipMemcpyAsync(h_out, d_out, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        return ZKT_OK;
    };
    const int rc = run();
    const hipError_t e = hipStreamSynchronize(c->stream);   // before `tmp` goes, whatever happened
    if (rc || e != hipSuccess) {
        if (t) zkt_merkle_tree_free(c, t);
        if (rc) return rc;
        ZKT_HIP(c, e);
    }
    if (report) {
        report->entries = entries;
        report->mismatches = h_out[0];
        report->first_layer = h_out[0] ? (int)(h_out[1] >> STORE_KEY_SHIFT) : -1;
        report->first_idx = h_out[0] ? h_out[1] & (((uint64_t)1 << STORE_KEY_SHIFT) - 1) : 0;
        report->root_matches = h_out[2] ? 0 : 1;
    }
    *out = t;
    return ZKT_OK;
}

}  // namespace zkt

using namespace zkt;

extern "C" {

int zkt_debug_store_chunk(zkt_ctx* c, size_t nodes) {
    if (!c) return ZKT_ERR_INVALID_ARGUMENT;
    c->store_chunk = nodes;
    return ZKT_OK;
}

int zkt_merkle_tree_save_file(zkt_ctx* c, zkt_merkle_tree* t, const char* path) {
    if (int rc = store_tree_check(c, t)) return rc;
    if (!path) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    (void)hipSetDevice(c->device);
    return store_save(c, t, path);
}

int zkt_merkle_tree_load_file(zkt_ctx* c, const zkt_poseidon* pos, int height, size_t capacity, const char* path, zkt_merkle_tree** out,
                              zkt_tree_file_report* report) {
    if (!c || !pos || !path || !out) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (height < 1 || height > 64) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "merkle tree: 1 <= height <= 64");
    if (capacity < 1 || capacity > ZKT_MERKLE_TREE_MAX || (height < 64 && (capacity >> height) && capacity != ((size_t)1 << height)))
        return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "merkle tree: 1 <= capacity <= min(2^height, ZKT_MERKLE_TREE_MAX)");
    (void)hipSetDevice(c->device);
    return store_load(c, pos, height, capacity, path, out, report);
}

int zkt_notes_write_file(const char* path, int curve_id, const uint64_t* leaf_indices, const uint64_t* identifiers_mont, const uint64_t* amounts,
                         const uint64_t* secrets_mont, size_t count) {
    if (!path || (curve_id != ZKT_CURVE_BN254 && curve_id != ZKT_CURVE_BLS12_381) ||
        (count && (!leaf_indices || !identifiers_mont || !amounts || !secrets_mont)))
        return keyfile_refused(nullptr, "zkt_notes_write_file: null pointer or unknown curve");
    kw::File w(path);
    sf::write_notes(w, curve_id, leaf_indices, identifiers_mont, amounts, secrets_mont, count);
    return keyfile_write_done(nullptr, w);
}

int zkt_notes_read_file(const char* path, int curve_id, size_t cap, uint64_t* out_leaf_indices, uint64_t* out_identifiers_mont, uint64_t* out_amounts,
                        uint64_t* out_secrets_mont, size_t* count) {
    if (!path || !count || (curve_id != ZKT_CURVE_BN254 && curve_id != ZKT_CURVE_BLS12_381))
        return keyfile_refused(nullptr, "zkt_notes_read_file: null pointer or unknown curve");
    std::vector<uint8_t> buf;
    if (!sf::read_whole_file(path, buf)) return keyfile_refused(nullptr, sf::refusal_message(path, sf::UNREADABLE, 0));
    uint64_t offset = 0;
    const int kind = sf::parse_notes(buf.data(), buf.size(), curve_id, cap, out_leaf_indices, out_identifiers_mont, out_amounts, out_secrets_mont,
                                     count, &offset);
    if (kind) return keyfile_refused(nullptr, sf::refusal_message(path, kind, offset));
    keyfile_clear_error();
    return ZKT_OK;
}

}  // extern "C"
