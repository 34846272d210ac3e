// The leaves and the tree of zkt_verify_batch_locate on the device (arithmetic and layout: verify_leaves.hpp).
//   k_vl_terms   one thread per (term, proof): a double-and-add scalar multiplication, the product stored as raw limbs.
//                Threads are numbered term-major, so a wave holds one kind of term: the 128-bit coefficients of Q's two
//                terms do not wait for full-width neighbours.
//   k_vl_leaves  one thread per proof: P_i = the sum of its 24 products, Q_i = the sum of its two; level 0 of both trees.
//   k_vl_level   one thread per node of the next level and tree: the sum of its two children, or the unpaired child itself.
// 64-thread workgroups and products through the shared fx_mul, as k_g1_decompress: a batch of a few thousand proofs
// spreads over every CU.  Nothing is indexed by data; every thread checks its index against the count it was given.
//
// Resources (gfx950, docs/EXPERIMENTS.md "locating the bad proofs of a batch").
#include "verify_leaves.hpp"

namespace zkt {

constexpr int VL_THREADS = 64;

template <class Q>
__global__ __launch_bounds__(VL_THREADS) void k_vl_terms(const Affine<Q>* __restrict__ proof_points,
                                                         const Affine<Q>* __restrict__ other,
                                                         const uint4* __restrict__ scalars, const uint4* __restrict__ rho,
                                                         uint32_t count, XyzzRaw<Q>* __restrict__ products) {
    const uint32_t idx = blockIdx.x * VL_THREADS + threadIdx.x;
    if (idx >= (uint32_t)VL_TERMS * count) return;
    const uint32_t term = idx / count, i = idx - term * count;
    const Affine<Q>* bp;
    const uint4* sp;
    if (term < (uint32_t)VL_PROOF_POINTS) {
        bp = proof_points + (size_t)i * VL_PROOF_POINTS + term;
        sp = scalars + ((size_t)i * VL_SOURCES + term) * 2;
    } else if (term < (uint32_t)VL_SOURCES) {
        bp = other + (size_t)i * (VL_SOURCES - VL_PROOF_POINTS) + (term - VL_PROOF_POINTS);
        sp = scalars + ((size_t)i * VL_SOURCES + term) * 2;
    } else {
        bp = proof_points + (size_t)i * VL_PROOF_POINTS + VL_WITNESS0 + (term - VL_SOURCES);
        sp = rho + ((size_t)i * 2 + (term - VL_SOURCES)) * 2;
    }
    const Affine<Q> base = aff_load<Q>(bp);
    const uint4 lo = sp[0], hi = sp[1];
    const uint32_t k[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    xx_store_raw<Q>(&products[idx], vl_mul<Q>(base, k));
}

template <class Q>
__global__ __launch_bounds__(VL_THREADS) void k_vl_leaves(const XyzzRaw<Q>* __restrict__ products, uint32_t count,
                                                          Xyzz<Q>* __restrict__ tree, size_t nodes) {
    const uint32_t i = blockIdx.x * VL_THREADS + threadIdx.x;
    if (i >= count) return;
    const XyzzX<Q> p = vl_sum<Q>(VL_SOURCES, [&](int t) { return xx_load_raw<Q>(&products[(size_t)t * count + i]); });
    const XyzzX<Q> q = vl_sum<Q>(2, [&](int t) { return xx_load_raw<Q>(&products[(size_t)(VL_SOURCES + t) * count + i]); });
    xyzz_store<Q>(&tree[i], vl_pack<Q>(p));
    xyzz_store<Q>(&tree[nodes + i], vl_pack<Q>(q));
}

// src: a level of n_src nodes, dst: the next one of (n_src + 1) / 2; blockIdx.y picks the tree
template <class Q>
__global__ __launch_bounds__(VL_THREADS) void k_vl_level(Xyzz<Q>* __restrict__ tree, size_t nodes, size_t src_off,
                                                         size_t dst_off, uint32_t n_src) {
    const uint32_t m = blockIdx.x * VL_THREADS + threadIdx.x;
    if (m >= (n_src + 1) / 2) return;
    const Xyzz<Q>* src = tree + (size_t)blockIdx.y * nodes + src_off;
    Xyzz<Q>* dst = tree + (size_t)blockIdx.y * nodes + dst_off;
    const Xyzz<Q> l = xyzz_load<Q>(&src[2 * (size_t)m]);
    if (2 * m + 1 < n_src)
        xyzz_store<Q>(&dst[m], vl_parent<Q>(l, xyzz_load<Q>(&src[2 * (size_t)m + 1])));
    else
        xyzz_store<Q>(&dst[m], l);
}

template <class Q>
static int leaves_launch(zkt_ctx* c, const void* d_proof_points, const void* d_other, const void* d_scalars, const void* d_rho,
                         size_t count, void* d_products, void* d_tree, size_t nodes) {
    const size_t threads = count * VL_TERMS;
    hipLaunchKernelGGL(k_vl_terms<Q>, dim3((unsigned)((threads + VL_THREADS - 1) / VL_THREADS)), dim3(VL_THREADS), 0, c->stream,
                       (const Affine<Q>*)d_proof_points, (const Affine<Q>*)d_other, (const uint4*)d_scalars, (const uint4*)d_rho,
                       (uint32_t)count, (XyzzRaw<Q>*)d_products);
    ZKT_HIP(c, hipGetLastError());
    hipLaunchKernelGGL(k_vl_leaves<Q>, dim3((unsigned)((count + VL_THREADS - 1) / VL_THREADS)), dim3(VL_THREADS), 0, c->stream,
                       (const XyzzRaw<Q>*)d_products, (uint32_t)count, (Xyzz<Q>*)d_tree, nodes);
    ZKT_HIP(c, hipGetLastError());
    return ZKT_OK;
}

template <class Q>
static int tree_launch(zkt_ctx* c, void* d_tree, size_t count, size_t nodes) {
    size_t sizes[VL_MAX_LEVELS], offs[VL_MAX_LEVELS], total = 0;
    const int levels = vl_levels(count, sizes, offs, &total);
    if (total != nodes) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "verify tree: node count does not match the batch");
    for (int l = 0; l + 1 < levels; ++l) {
        hipLaunchKernelGGL(k_vl_level<Q>, dim3((unsigned)((sizes[l + 1] + VL_THREADS - 1) / VL_THREADS), 2), dim3(VL_THREADS), 0,
                           c->stream, (Xyzz<Q>*)d_tree, nodes, offs[l], offs[l + 1], (uint32_t)sizes[l]);
        ZKT_HIP(c, hipGetLastError());
    }
    return ZKT_OK;
}

size_t vl_raw_bytes(int curve) {
    return curve == ZKT_CURVE_BN254 ? sizeof(XyzzRaw<Bn254Fq>) : sizeof(XyzzRaw<Bls381Fq>);
}

int verify_leaves_enqueue(zkt_ctx* c, const void* d_proof_points, const void* d_other, const void* d_scalars, const void* d_rho,
                          size_t count, void* d_products, void* d_tree, size_t nodes) {
    if (count == 0 || count > ZKT_VERIFY_BATCH_DEV_MAX || nodes < count)
        return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "verify leaves: bad count");
    if (c->curve == ZKT_CURVE_BN254)
        return leaves_launch<Bn254Fq>(c, d_proof_points, d_other, d_scalars, d_rho, count, d_products, d_tree, nodes);
    return leaves_launch<Bls381Fq>(c, d_proof_points, d_other, d_scalars, d_rho, count, d_products, d_tree, nodes);
}

int verify_tree_enqueue(zkt_ctx* c, void* d_tree, size_t count, size_t nodes) {
    if (count == 0 || count > ZKT_VERIFY_BATCH_DEV_MAX) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "verify tree: bad count");
    if (c->curve == ZKT_CURVE_BN254) return tree_launch<Bn254Fq>(c, d_tree, count, nodes);
    return tree_launch<Bls381Fq>(c, d_tree, count, nodes);
}

}  // namespace zkt
