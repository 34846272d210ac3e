// The note tree's handle, for the units that read its layers in place: poseidon.hip (create, append, paths) and
// storefile.hip (the MerkleTreeStore file).
#pragma once
#include "ctx.hpp"

#include <vector>

struct zkt_poseidon;

// the opaque handle of include/zkt_plonk.h: MerkleTree<F, G, H, HEIGHT> resident in HBM
struct zkt_merkle_tree {
    int curve = 0, height = 0;
    const zkt_poseidon* pos = nullptr;   // borrowed
    uint64_t count = 0, capacity = 0;
    std::vector<size_t> layer_len;       // elements of layer L: max(1, ceil(capacity / 2^L))
    void* d_nodes = nullptr;             // all the layers, one after the other
    void* d_layers = nullptr;            // height device pointers into d_nodes
    void* d_empties = nullptr;           // nodes[0 .. height)
    void* d_root = nullptr;
    // the index table of zkt_merkle_tree_paths*: k x (u64 index), k x (u32 sibling_var0), k x (u32 bit_var0), packed
    void* d_table = nullptr;
    void* h_table = nullptr;             // pinned: the upload is a stream copy, the caller's arrays are free on return
    hipEvent_t table_up = nullptr;       // the last upload out of h_table
    bool table_busy = false;
    int wide_min_parents = 0;            // zkt_debug_merkle_tree_split: 0 = the policy
};
