// forest_copy_kernels.hpp -- forests that slide (include/vkmr_hip.h: vkmr_hip_forest_drop_front_async,
// vkmr_hip_forest_copy_trees_async).  Dropping the oldest trees moves nothing: their offsets become the offset of the first tree
// kept.  Reclaiming the room in front is a copy of stored trees into another forest: the nodes are the same, only their cells
// differ (forest_plan.hpp: copy_step), so no kernel here holds a hash block.  The copy's launches are append's -- check, offsets
// (forest_append_offsets_kernel itself), then one launch per level over the new trees' cells alone -- with level 0, the leaves,
// as one more launch of the level kernel.
#pragma once

#include "forest_kernels.hpp"

// A lane per dropped tree t < k: it begins and ends where tree k begins, its root is zero and so is its mask, as a build over
// the new offsets leaves them.  offsets[k] is only read (k <= ntrees, and the offsets are ntrees + 1).
__global__ __launch_bounds__(256) void forest_drop_front_kernel(uint64_t* __restrict__ offsets, uint32_t k, Node* __restrict__ roots,
                                                                unsigned long long* __restrict__ mutated)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= k) return;
    offsets[t] = vkmr_forest::drop_front_offset(0ull, offsets[k], (uint32_t)t, k);
    const uint32_t zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    vkmr_dev::store_node(roots + t, zero);
    if (mutated != nullptr) mutated[t] = 0ull;
}

// forest_append_check_kernel's three bits over the destination, and bit 3 (value 8) for the selection: sel[i] names no tree of
// the source, or new count i is not that tree's count.  src_offsets is read only at an index the same lane has just checked.
__global__ __launch_bounds__(256) void forest_copy_check_kernel(const uint64_t* __restrict__ offsets, uint32_t ntrees, uint32_t first_tree, uint64_t used,
                                                                const uint64_t* __restrict__ new_offsets, uint32_t m, uint64_t n_leaves, uint64_t max_count,
                                                                const uint32_t* __restrict__ sel, const uint64_t* __restrict__ src_offsets,
                                                                uint32_t src_ntrees, uint32_t* __restrict__ status)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t bits = 0u;
    if (i < m) {
        const uint64_t lo = new_offsets[i], hi = new_offsets[i + 1];
        if (hi < lo || (i == 0 && lo != 0ull) || (i + 1 == m && hi != n_leaves)) bits |= 1u;
        if (hi >= lo && hi - lo > max_count) bits |= 2u;
        const uint32_t ts = sel[i];
        if (ts >= src_ntrees) bits |= 8u;
        else if (src_offsets[ts + 1u] - src_offsets[ts] != hi - lo) bits |= 8u;
    }
    if (i <= (uint64_t)(ntrees - first_tree) && offsets[first_tree + i] != used) bits |= 4u;
    if (bits) atomicOr(status, bits);
}

// One level l >= 0 of the copy, a lane per destination cell from `base` = append_first_cell(used, first_tree, l) to `end` =
// append_end_cell(used + n_leaves, first_tree + m, l), among the `end_tree` = first_tree + m trees in front of that end.  The
// check has passed and forest_append_offsets_kernel has written the destination offsets: every sel[] is a tree of the source
// and has the destination tree's count.  `src` and `dst` are level l's buffers (the leaves for l == 0).  For l >= 1 the tree of
// a lane is forest_find_tree's; at level 0 the trees' first cells are the offsets, which empty trees share, so the
// wavefront's first tree is searched the same way and every lane of a wavefront a tree begins in searches all trees behind it.
// Then copy_step: two 16-byte loads and two 16-byte stores a lane, the source cell a per-tree constant away.
__global__ __launch_bounds__(256) void forest_copy_level_kernel(const Node* __restrict__ src, const uint64_t* __restrict__ src_offsets,
                                                                const Node* __restrict__ src_roots, const unsigned long long* __restrict__ src_mutated,
                                                                const uint32_t* __restrict__ sel, const uint64_t* __restrict__ offsets, uint32_t first_tree,
                                                                uint32_t end_tree, uint32_t l, uint64_t base, uint64_t end, Node* __restrict__ dst,
                                                                Node* __restrict__ roots, unsigned long long* __restrict__ mutated,
                                                                const uint32_t* __restrict__ status)
{
    if (*status != 0u) return;                   // the same word in every lane
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t p0 = base + ((uint64_t)blockIdx.x * (256u / 64u) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6))) * 64ull;
    if (p0 >= end) return;                       // wave-uniform
    const uint64_t p = p0 + lane;
    uint32_t u;
    if (l != 0u) {
        u = forest_find_tree(offsets, end_tree, l, p0, lane).t;
    } else {
        u = vkmr_forest::copy_find_tree(offsets, end_tree, 0u, p0);
        if (u + 1u < end_tree && offsets[u + 1u] <= p0 + 63ull) u = vkmr_forest::copy_find_tree(offsets, end_tree, 0u, p, u);   // wave-uniform test
    }
    if (u < first_tree) return;                  // never: the first wavefront begins at the first new tree's first cell
    const uint64_t o_d = offsets[u], c = offsets[u + 1u] - o_d;
    const uint64_t first = vkmr_forest::pos(o_d, u, l);
    if (p < first) return;
    const uint32_t ts = sel[u - first_tree];
    const vkmr_forest::CopyStep step = vkmr_forest::copy_step(o_d, u, c, src_offsets[ts], ts, l, p - first);
    switch (step.kind) {
    case vkmr_forest::COPY_NOTHING: break;
    case vkmr_forest::COPY_ZERO_ROOT: {
        const uint32_t zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        vkmr_dev::store_node(roots + u, zero);
        break;
    }
    case vkmr_forest::COPY_ROOT: {
        const Node x = vkmr_dev::load_node(src_roots + ts);
        vkmr_dev::store_node(roots + u, x.w);
        if (mutated != nullptr && src_mutated != nullptr) mutated[u] = src_mutated[ts];   // zeroed by the offsets launch otherwise
        break;
    }
    case vkmr_forest::COPY_CELL:
    case vkmr_forest::COPY_LEAF: {
        const Node x = vkmr_dev::load_node(src + step.src);
        vkmr_dev::store_node(dst + step.dst, x.w);
        break;
    }
    }
}
