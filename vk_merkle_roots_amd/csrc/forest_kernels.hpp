// forest_kernels.hpp -- roots of many trees of unequal size in one call (include/vkmr_hip.h: vkmr_hip_reduce_forest_async).
//
// The leaves of all trees lie back to back; offsets[t] .. offsets[t+1] are tree t's.  One launch per level, one lane per
// cell of that level's buffer across the whole forest -- reduce_level_kernel's form, so every lane hashes wherever the work
// is -- with one addition: a lane must learn which tree its cell belongs to.  Level l of tree t starts at cell
// pos_l(t) = (offsets[t] >> l) + t (forest_plan.hpp: no prefix sum, no overlap, under one idle cell per tree and level), and
// pos_l grows strictly with t, so the tree is found by binary search over the offsets alone:
//   per wavefront  the tree t0 of its first cell, a wave-uniform search (about log2(ntrees) loads of one address each);
//                  when tree t0 + 1 starts behind the wavefront's 64 cells -- every wavefront inside a tree of more than
//                  64 << l leaves -- all lanes have t0 and nothing else is searched
//   per lane       otherwise lane i has one of t0 .. t0 + i (every tree takes at least one cell): at most 6 more steps
// A tree whose level h_t = max(1, ceil(log2 c_t)) has been formed writes that node to roots[t] instead of the level buffer
// and takes no part in later launches; an empty tree gets its all-zero root from the lane of its reserved cell at level 1.
#pragma once

#include "forest_plan.hpp"

// No hash: bit 0 when offsets[t+1] < offsets[t] or the last offset is past `total`, bit 1 when a tree holds more than
// max_count leaves.  ORed into *status (zeroed by the host); the level kernels read it first and do nothing when it is
// nonzero, so they never follow an offset that was not checked.
__global__ __launch_bounds__(256) void forest_check_kernel(const uint64_t* __restrict__ offsets, uint32_t ntrees, uint64_t total, uint64_t max_count,
                                                           uint32_t* __restrict__ status)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ntrees) return;
    const uint64_t lo = offsets[t], hi = offsets[t + 1];
    uint32_t bits = 0u;
    if (hi < lo || (t + 1 == ntrees && hi > total)) bits |= 1u;
    if (hi >= lo && hi - lo > max_count) bits |= 2u;
    if (bits) atomicOr(status, bits);
}

// Level l >= 1 from level l - 1 (`in`: the leaves for l == 1, else the buffer of level l - 1), `cells` lanes.  The check ran
// first: the offsets do not decrease and end inside the leaves, so every cell read below is one of tree t's own.  One
// hash_pair: the kernel's only hash block.
__global__ __launch_bounds__(256) void forest_level_kernel(const Node* __restrict__ in, const uint64_t* __restrict__ offsets, uint32_t ntrees, uint32_t l,
                                                           uint64_t cells, Node* __restrict__ out, Node* __restrict__ roots,
                                                           const uint32_t* __restrict__ status)
{
    if (*status != 0u) return;                   // the same word in every lane
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t p0 = ((uint64_t)blockIdx.x * (256u / 64u) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6))) * 64ull;
    if (p0 >= cells) return;                     // wave-uniform
    // the tree of the wavefront's first cell: the largest t0 with pos_l(t0) <= p0 (0 when there is none)
    uint32_t t0 = 0, top = ntrees - 1u;
    while (t0 < top) {
        const uint32_t mid = t0 + (top - t0 + 1u) / 2u;
        if (vkmr_forest::pos(offsets[mid], mid, l) <= p0) t0 = mid;
        else top = mid - 1u;
    }
    const uint64_t p = p0 + lane;
    uint32_t t = t0;
    if (t0 + 1u < ntrees && vkmr_forest::pos(offsets[t0 + 1u], t0 + 1u, l) <= p0 + 63ull) {   // wave-uniform: a tree begins inside the wavefront
        top = (ntrees - 1u - t0 < lane) ? ntrees - 1u : t0 + lane;
        while (t < top) {
            const uint32_t mid = t + (top - t + 1u) / 2u;
            if (vkmr_forest::pos(offsets[mid], mid, l) <= p) t = mid;
            else top = mid - 1u;
        }
    }
    const uint64_t o = offsets[t], c = offsets[t + 1u] - o;
    const uint64_t first = vkmr_forest::pos(o, t, l);
    if (p < first) return;                       // cells in front of tree 0 (offsets[0] > 0)
    const uint64_t j = p - first;                // this lane's node of tree t's level l
    if (c == 0ull) {                             // an empty tree: its reserved cell's lane writes the all-zero root, once
        if (l == 1u && j == 0ull) {
            const uint32_t zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            vkmr_dev::store_node(roots + t, zero);
        }
        return;
    }
    // without a count-leading-zeros: the tree takes part in level l when l == 1 or level l - 1 still had two nodes, and level l
    // is its last, h_t, when it has one node
    const uint64_t n_in = vkmr_forest::level_count(c, l - 1u), n_out = vkmr_forest::level_count(c, l);
    if ((l > 1u && n_in == 1ull) || j >= n_out) return;   // the tree is done, or the padding behind its nodes
    uint32_t x[8];
    vkmr_dev::hash_parent(in + vkmr_forest::pos(o, t, l - 1u), n_in, j, x);
    vkmr_dev::store_node(n_out == 1ull ? roots + t : out + p, x);
}
