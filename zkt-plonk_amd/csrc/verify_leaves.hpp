// The per-proof point pairs of a verified batch and their binary tree (zkt_verify_batch_locate, verify.hip): the
// arithmetic of one term, one leaf and one inner node on the 29-bit limbs of fx.hpp and the XYZZ routines of ecx.hpp,
// written once for the kernels of verify_leaves.hip and for the host rehearsal (zkt_debug_verify_locate_host), and the
// enqueue entries.
//
// Proof i of a batch has the pair
//     P_i = sum_s acc_i[s] * base_i[s]   (s < VL_SOURCES: the proof's 13 commitments, ten verifier-key points, g;
//                                          acc_i[s] = the rho-weighted sum of both openings' scalars on that source),
//     Q_i = rho_2i W_2i + rho_2i+1 W_2i+1 (the two opening witnesses: commitments 11 and 12),
// and e(P_i, h) e(-Q_i, beta h) == 1 iff the proof verifies (up to 2^-128).  Level 0 of the tree holds the `count` pairs,
// every further level the sums of neighbours (2m, 2m + 1), an unpaired last node moving up unchanged; the root is the
// batch's (A, B).
#pragma once
#include "ctx.hpp"
#include "ec.hpp"
#include "ecx.hpp"

namespace zkt {

constexpr int VL_SOURCES = 24;            // Verifier::SRC_COUNT
constexpr int VL_PROOF_POINTS = 13;       // of which the proof's own commitments, in wire order
constexpr int VL_WITNESS0 = 11;           // the opening witnesses among them (aw, saw)
constexpr int VL_TERMS = VL_SOURCES + 2;  // products per proof: P's sources, then Q's two

constexpr int VL_MAX_LEVELS = 65;         // more than any size_t count has

// Levels of the tree over `count` leaves: sizes count, ceil(count / 2), ..., 1 and the offset of each level in a tree
// stored leaves first.  Returns the number of levels; *total = the number of nodes (< 2 count + 64).
inline int vl_levels(size_t count, size_t* sizes, size_t* offsets, size_t* total) {
    int n = 0;
    size_t at = 0;
    for (size_t w = count;; w = (w + 1) / 2) {
        sizes[n] = w;
        offsets[n] = at;
        at += w;
        ++n;
        if (w == 1) break;
    }
    *total = at;
    return n;
}

// [k] B for an affine base in arkworks' Montgomery form ((0, 0) = the identity) and a canonical scalar of eight 32-bit
// words: double-and-add from the top bit, the ladder of g1d_mul_x with a per-lane scalar.  The leading zero bits double
// the identity, which xx_double returns at once: a 128-bit coefficient costs half of a full-width scalar.
// In: x, y < q.  Out: the bounds of XyzzX (ecx.hpp): xx_double and xx_add_mixed keep them.
template <class Q>
ZKT_HD XyzzX<Q> vl_mul(const Affine<Q>& base, const uint32_t (&k)[8]) {
    XyzzX<Q> acc = xx_identity<Q>();
    if (aff_is_inf<Q>(base)) return acc;
    AffineX<Q> b;
    b.x = fx_cond_sub_p<Q>(fx_from_ark<Q>(base.x));   // < 2q -> canonical, R' form
    b.y = fx_cond_sub_p<Q>(fx_from_ark<Q>(base.y));
#pragma nounroll
    for (int w = 7; w >= 0; --w) {
        uint32_t e = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) e = j == w ? k[j] : e;   // no register array indexed by a loop counter
#pragma nounroll
        for (int bit = 31; bit >= 0; --bit) {
            acc = xx_double<Q>(acc);
            if ((e >> bit) & 1u) acc = xx_add_mixed<Q>(acc, b);
        }
    }
    return acc;
}

// sum of n products; load(t) yields product t
template <class Q, class Load>
ZKT_HD XyzzX<Q> vl_sum(int n, Load load) {
    XyzzX<Q> acc = xx_identity<Q>();
#pragma nounroll
    for (int t = 0; t < n; ++t) acc = xx_add<Q>(acc, load(t));
    return acc;
}

// A tree node in memory: canonical packed coordinates in arkworks' Montgomery form, zz = 0 for the identity -- what
// xyzz_to_affine_host normalises.  In: the bounds of XyzzX (every coordinate < 8q).
template <class Q>
ZKT_HD Xyzz<Q> vl_pack(const XyzzX<Q>& a) {
    if (a.inf) return xyzz_identity<Q>();
    Xyzz<Q> r;
    r.x = fx_to_ark<Q>(a.x);
    r.y = fx_to_ark<Q>(a.y);
    r.zz = fx_to_ark<Q>(a.zz);
    r.zzz = fx_to_ark<Q>(a.zzz);
    return r;
}
template <class Q>
ZKT_HD XyzzX<Q> vl_unpack(const Xyzz<Q>& p) {   // out: every coordinate < 2q
    XyzzX<Q> r;
    r.inf = fe_is_zero<Q>(p.zz);
    r.x = fx_from_ark<Q>(p.x);
    r.y = fx_from_ark<Q>(p.y);
    r.zz = fx_from_ark<Q>(p.zz);
    r.zzz = fx_from_ark<Q>(p.zzz);
    return r;
}
// the parent of two nodes
template <class Q>
ZKT_HD Xyzz<Q> vl_parent(const Xyzz<Q>& l, const Xyzz<Q>& r) {
    return vl_pack<Q>(xx_add<Q>(vl_unpack<Q>(l), vl_unpack<Q>(r)));
}

// Scratch of the two enqueue entries behind the stage-1 region of a batch (all offsets multiples of 256 bytes)
struct VlLayout {
    size_t other, scalars, rho, products, tree, end;   // byte offsets from the scratch base
    size_t nodes;                                       // per tree
};
inline VlLayout vl_layout(size_t start, size_t count, size_t fq_bytes, size_t raw_bytes) {
    auto up = [](size_t b) { return (b + 255) / 256 * 256; };
    size_t sizes[VL_MAX_LEVELS], offs[VL_MAX_LEVELS];
    VlLayout l;
    vl_levels(count, sizes, offs, &l.nodes);
    l.other = up(start);
    l.scalars = l.other + up(count * (VL_SOURCES - VL_PROOF_POINTS) * 2 * fq_bytes);
    l.rho = l.scalars + up(count * VL_SOURCES * 32);
    l.products = l.rho + up(count * 2 * 32);
    l.tree = l.products + up(count * VL_TERMS * raw_bytes);
    l.end = l.tree + up(2 * l.nodes * 4 * fq_bytes);
    return l;
}
size_t vl_raw_bytes(int curve);

// Enqueue on the context's stream, no synchronisation.  All pointers are device pointers, 16-byte aligned.
//   d_proof_points: count x 13 affine points (the output of g1_decompress_enqueue, proof-major)
//   d_other:        count x 11 affine points (ten verifier-key points and g)
//   d_scalars:      count x 24 canonical scalars, 32 bytes each
//   d_rho:          2 count canonical coefficients, 32 bytes each
//   d_products:     26 count raw XYZZ points (scratch)
//   d_tree:         2 x nodes XYZZ points: P's tree, then Q's, each level by level, leaves first
int verify_leaves_enqueue(zkt_ctx* c, const void* d_proof_points, const void* d_other, const void* d_scalars, const void* d_rho,
                          size_t count, void* d_products, void* d_tree, size_t nodes);
int verify_tree_enqueue(zkt_ctx* c, void* d_tree, size_t count, size_t nodes);

}  // namespace zkt
