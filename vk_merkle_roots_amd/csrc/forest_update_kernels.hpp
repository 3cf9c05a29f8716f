// forest_update_kernels.hpp -- leaf updates of a stored forest (include/vkmr_hip.h: vkmr_hip_forest_update_async): the three
// kernels of tree_kernels.hpp's leaf update with a tree per entry.  Every lane is one update entry q < k, the pair
// (trees[q], indices[q]); the entries differ per lane, so their loads, and the two offsets a lane reads for its tree, are
// vector loads.  The check ORs the contract's violations into *status (zeroed by the host), and the two writers read *status
// first and write nothing when it is nonzero, so a rejected batch leaves the leaves, the forest and the roots as they were.
//
// Layout (vkmr_hip_reduce_forest_tree_async, forest_plan.hpp): level 0 is the caller's leaves, tree t at cell offsets[t]; node j
// of tree t's level l >= 1 is cell pos_l(t) + j = (offsets[t] >> l) + t + j of level l's buffer, for l < h_t; level h_t is
// roots[t].  The host passes the buffers of levels l - 1 and l, not the table of all of them.
#pragma once

#include "forest_plan.hpp"

// No hash: bit 0 when trees[q] >= ntrees or indices[q] >= c_t (the offsets are read only for a tree in range; every entry
// into an empty tree sets it), bit 1 when (trees[q-1], indices[q-1]) >= (trees[q], indices[q]) lexicographically (out of
// order or repeated).
__global__ __launch_bounds__(256) void forest_update_check_kernel(const uint64_t* __restrict__ offsets, uint32_t ntrees, const uint32_t* __restrict__ trees,
                                                                  const uint64_t* __restrict__ indices, uint32_t k, uint32_t* __restrict__ status)
{
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= k) return;
    const uint32_t t = trees[q];
    const uint64_t index = indices[q];
    uint32_t bits = 1u;
    if (t < ntrees && index < offsets[t + 1u] - offsets[t]) bits = 0u;
    if (q > 0) {
        const uint32_t t0 = trees[q - 1];
        if (t0 > t || (t0 == t && indices[q - 1] >= index)) bits |= 2u;
    }
    if (bits) atomicOr(status, bits);
}

// No hash: digests[offsets[t] + index_q] = leaves[q].  The check ran first: the cell is one of tree t's own.
__global__ __launch_bounds__(256) void forest_update_leaves_kernel(Node* __restrict__ digests, const uint64_t* __restrict__ offsets,
                                                                   const uint32_t* __restrict__ trees, const uint64_t* __restrict__ indices,
                                                                   const Node* __restrict__ leaves, uint32_t k, const uint32_t* __restrict__ status)
{
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= k || *status != 0u) return;
    vkmr_dev::store_node(digests + offsets[trees[q]] + indices[q], vkmr_dev::load_node(leaves + q));
}

// One level l >= 1 per launch: in = the buffer of level l - 1 (the leaves for l == 1), out = the buffer of level l.  Lane q
// hashes parent p = index_q >> l of its tree when the tree still takes part in level l and the lane is the first of its run
// (the entries are sorted by (tree, index), so lanes with the same parent are adjacent): each dirty node is hashed exactly
// once, distinct lanes write distinct cells and read only the level below.  A tree whose level l is one node gets it in
// roots[t].  The check ran first: index_q < c_t, so p is a node of level l and every cell read is one of tree t's own.
// forest_level_kernel's body with the tree and the node given, not searched for; its one hash_pair is the kernel's only
// hash block.
__global__ __launch_bounds__(256) void forest_update_level_kernel(const Node* __restrict__ in, Node* __restrict__ out, Node* __restrict__ roots,
                                                                  const uint64_t* __restrict__ offsets, const uint32_t* __restrict__ trees,
                                                                  const uint64_t* __restrict__ indices, uint32_t k, uint32_t l,
                                                                  const uint32_t* __restrict__ status)
{
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= k || *status != 0u) return;
    const uint32_t t = trees[q];
    const uint64_t index = indices[q];
    if (q > 0 && vkmr_forest::update_same_node(trees[q - 1], indices[q - 1], t, index, l)) return;   // not the head of p's run
    const uint64_t o = offsets[t], c = offsets[t + 1u] - o;
    const vkmr_forest::UpdateStep s = vkmr_forest::update_step(o, c, t, index, l);
    if (!s.active) return;                       // the tree's root was formed at a level below
    uint32_t x[8];
    vkmr_dev::hash_parent(in + s.in_first, s.n_in, s.p, x);
    vkmr_dev::store_node(s.root ? roots + t : out + s.out, x);
}
