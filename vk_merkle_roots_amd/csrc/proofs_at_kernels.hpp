// proofs_at_kernels.hpp -- inclusion proofs as of an earlier count (include/vkmr_hip.h: vkmr_hip_forest_proofs_at_async; the
// rules: proofs_at_plan.hpp).
//
// A stored forest answers k queries (epoch, leaf index), an epoch being (tree, old count c): the proof of the leaf under the root
// the tree had at c leaves.  The check first, a lane per epoch.  The edge launch behind it, a lane per epoch, hashes the nodes of
// the old tree that the grown tree no longer holds -- the last node of every level above the lowest set bit of c, the carry of
// the frontier's root walk -- into the epoch's edge row and its old root: H(c) - ctz(c) serial hashes through one hash_pair.
// The gather behind that, a lane per (query, level), hashes nothing: one load, from the stored forest or from the edge row, and
// one store.  Both read *status and do nothing when it is nonzero.
#pragma once

#include "proofs_at_plan.hpp"

// Node j of level l of tree t (offset o, c2 leaves now), where the build left it; j < level_count(c2, l).
__device__ __forceinline__ const Node* proofs_at_node(const Node* digests, const Node* forest, const ForestLevels& lv, const Node* roots, uint64_t o, uint32_t t,
                                                      uint64_t c2, uint32_t l, uint64_t j)
{
    const vkmr_frontier::GatherSource from = vkmr_frontier::node_source(c2, l);
    if (from == vkmr_frontier::GATHER_ROOT) return roots + t;
    return (from == vkmr_frontier::GATHER_LEAF ? digests : forest + lv.base[l]) + vkmr_frontier::node_cell(o, t, l, j);
}

// No hash, a lane per epoch: consistency_plan.hpp's refusal() ORed into *status, zeroed by the host.
__global__ __launch_bounds__(256) void proofs_at_check_kernel(const uint64_t* __restrict__ offsets, uint32_t ntrees, const uint32_t* __restrict__ epoch_trees,
                                                              const uint64_t* __restrict__ epoch_counts, uint32_t E, uint32_t stride,
                                                              uint32_t* __restrict__ status)
{
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const uint32_t bits = vkmr_proofs_at::refusal(epoch_trees[e], ntrees, offsets, epoch_counts[e], stride);
    if (bits) atomicOr(status, bits);
}

// The edge row and the old root of epoch e, a lane per epoch: proofs_at_plan.hpp's edge_step() in one loop over the levels.
// Level l forms E_(l+1), the node hash of (a, b): a is the peak P_l of a set bit, loaded from where the NEW tree keeps it, else the
// carry; b is the carry, or a again where there is no carry yet.  The operands are selected first, so there is one hash_pair,
// the kernel's only hash block.  The carry is stored as it is formed: to cell l + 1 of the edge row, or to the old root for
// l + 1 == H(c).  A level that forms nothing stores zero and cell H(c), which the root's level would form, is zeroed in front of
// the loop, so that every cell of the row is written; an epoch that never hashed takes its root behind the loop: zero for c == 0, node 0 of level H(c) of the new tree for a power of two of at least 2.
// Behind the check: the tree exists and c <= c2, so every node asked for lies inside its level; H(c) <= bits(c2) <= stride.
__global__ __launch_bounds__(256) void proofs_at_edge_kernel(const Node* __restrict__ digests, const Node* __restrict__ forest, ForestLevels lv,
                                                             const uint64_t* __restrict__ offsets, const Node* __restrict__ roots,
                                                             const uint32_t* __restrict__ epoch_trees, const uint64_t* __restrict__ epoch_counts, uint32_t E,
                                                             uint32_t stride, Node* __restrict__ edges_out, Node* __restrict__ old_roots_out,
                                                             const uint32_t* __restrict__ status)
{
    if (*status != 0u) return;                   // the same word in every lane
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const uint32_t t = epoch_trees[e];
    const uint64_t c = epoch_counts[e], o = offsets[t], c2 = offsets[t + 1u] - o;
    Node* row = edges_out + e * stride;
    Node* root = old_roots_out + e;
    const uint32_t H = vkmr_proofs_at::levels(c);
    const Node zero = {};
    Node carry = {};
    bool have = false;
    vkmr_dev::store_node(row, zero);             // no level has an E_0,
    if (H != 0u && H < stride) vkmr_dev::store_node(row + H, zero);   // and the row has no cell for the root: level H(c) forms that
#pragma unroll 1
    for (uint32_t l = 0; l < stride; ++l) {
        const vkmr_proofs_at::EdgeStep s = vkmr_proofs_at::edge_step(c, l, have);
        Node* dst = s.to_root ? root : row + (l + 1u);
        if (!s.hash) {
            if (!s.to_root && l + 1u < stride) vkmr_dev::store_node(dst, zero);
            continue;
        }
        Node a = carry;                          // a peak below H(c) lies in a level of two nodes at least: never in the roots
        if (s.peak) a = vkmr_dev::load_node((l == 0u ? digests : forest + lv.base[l]) + vkmr_frontier::node_cell(o, t, l, vkmr_proofs_at::peak_node(c, l)));
        const Node b = s.twice ? a : carry;
        vkmr_dev::hash_pair(a.w, b.w, carry.w);
        have = true;
        vkmr_dev::store_node(dst, carry);        // l + 1 <= H(c) <= stride: the root, or a cell of the row
    }
    // no hash: the tree not yet begun (zero), or a power of two of at least 2, whose root the new tree holds as node 0 of level H(c)
    if (!have) vkmr_dev::store_node(root, c == 0ull ? zero : vkmr_dev::load_node(proofs_at_node(digests, forest, lv, roots, o, t, c2, H, 0ull)));
}

// Cell l of the proof of query q = i / stride, l = i % stride: leaf indices[q] as of epoch epochs[q].  An epoch >= E or an index
// >= c gets height 0 and zero cells (vkmr_hip_forest_proofs_async's rule for a bad index).  Else, for l < H(c), the node
// sibling(c, l, index) of the old tree: from the stored forest when it is complete, from the epoch's edge row when not.  Behind
// the check and the edge launch.  Every cell is written, zeros included.
__global__ __launch_bounds__(256) void proofs_at_gather_kernel(const Node* __restrict__ digests, const Node* __restrict__ forest, ForestLevels lv,
                                                               const uint64_t* __restrict__ offsets, const Node* __restrict__ roots,
                                                               const uint32_t* __restrict__ epoch_trees, const uint64_t* __restrict__ epoch_counts, uint32_t E,
                                                               const uint32_t* __restrict__ epochs, const uint64_t* __restrict__ indices, uint32_t k,
                                                               uint32_t stride, const Node* __restrict__ edges, Node* __restrict__ siblings,
                                                               uint32_t* __restrict__ heights, const uint32_t* __restrict__ status)
{
    if (*status != 0u) return;                   // the same word in every lane
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint64_t)k * stride) return;
    const uint64_t q = i / stride;
    const uint32_t l = (uint32_t)(i - q * stride);
    const uint32_t e = epochs[q];
    const uint64_t index = indices[q];
    Node x = {};
    uint32_t h = 0u;
    if (e < E) {
        const uint64_t c = epoch_counts[e];
        if (index < c) {                           // never true for an epoch not yet begun
            h = vkmr_proofs_at::height(c);
            if (l < h) {
                const uint32_t t = epoch_trees[e];
                const uint64_t o = offsets[t], c2 = offsets[t + 1u] - o;
                const uint64_t s = vkmr_proofs_at::sibling(c, l, index);
                x = vkmr_dev::load_node(vkmr_proofs_at::complete(c, l, s) ? proofs_at_node(digests, forest, lv, roots, o, t, c2, l, s)
                                                                          : edges + (uint64_t)e * stride + l);
            }
        }
    }
    vkmr_dev::store_node(siblings + i, x);
    if (l == 0u) heights[q] = h;
}
