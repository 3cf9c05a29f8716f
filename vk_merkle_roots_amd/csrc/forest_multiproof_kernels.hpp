// forest_multiproof_kernels.hpp -- one compact multiproof for leaves of many trees of a stored forest, and its verifier
// (include/vkmr_hip.h: vkmr_hip_forest_multiproof_async, vkmr_hip_verify_forest_multiproof_async): the multiproof kernels of
// tree_kernels.hpp with a tree and a height per entry.  Every lane is one entry q < k, the pair (trees[q], indices[q]); the
// pairs are strictly increasing, so the entries of one tree are adjacent and, inside a tree, lanes with the same node are.
//
// Order of the nodes: level-major over the WHOLE forest -- level l of every tree before level l + 1 of any, inside a level by
// tree, inside a tree by node.  With the entries sorted that is the order of the entries themselves at every level, so the
// ranking of tree_kernels.hpp (ballot words, block sums, block starts, word starts) serves unchanged with height := the
// forest's stride: only the flags differ.  Entry q owns the cell of (l, p = index_q >> l) when l < h_q and p is odd and q is
// the first lane of p's run with p - 1 not in front of it, or p is even and q is the last lane of the run with p + 1 not behind
// it; the lane in front or behind counts only when it names the same tree.
//
// Header (uint64 words) as in tree_kernels.hpp: [0] status, [1] M, [2 + l] m_l over the whole forest.  The checks OR into
// the low 32 bits of [0]; every kernel behind a check reads [0] first and does nothing when it is nonzero.
//
// Layout (vkmr_hip_reduce_forest_tree_async, forest_plan.hpp): level 0 is the caller's leaves, tree t at cell offsets[t]; node j
// of tree t's level l >= 1 is cell base[l] + pos_l(t) + j of the stored forest, for l < h_t.
#pragma once

#include "forest_plan.hpp"
#include "forest_tree_kernels.hpp"

// No hash: heights[q] = h_t = max(1, ceil(log2 c_t)) of entry q's tree (a count-leading-zeros, as forest_proofs_kernel).  The
// check ran first: the tree is one of the forest's and holds a leaf.
__global__ __launch_bounds__(256) void forest_multiproof_heights_kernel(const uint64_t* __restrict__ offsets, const uint32_t* __restrict__ trees,
                                                                        uint32_t k, const uint64_t* __restrict__ hdr, uint32_t* __restrict__ heights)
{
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= k || hdr[0] != 0ull) return;
    const uint32_t t = trees[q];
    heights[q] = vkmr_forest::height(offsets[t + 1u] - offsets[t]);
}

// The verifier's check (no hash; the heights are the caller's and nothing is trusted): bit 0 when trees[q] >= ntrees, the
// height is outside 1..stride or indices[q] >= 2^height; bit 1 when the pairs are not strictly increasing (the two bits of
// forest_update_check_kernel, with 2^height in the place of c_t); bit 3 when the entry in front names the same tree with
// another height.
__global__ __launch_bounds__(256) void verify_forest_multiproof_check_kernel(const uint32_t* __restrict__ trees, const uint64_t* __restrict__ indices,
                                                                             const uint32_t* __restrict__ heights, uint32_t k, uint32_t stride,
                                                                             uint32_t ntrees, uint32_t* __restrict__ status)
{
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= k) return;
    const uint32_t t = trees[q], h = heights[q];
    const uint64_t index = indices[q];
    uint32_t bits = 1u;
    if (t < ntrees && h >= 1u && h <= stride && (index >> h) == 0ull) bits = 0u;   // stride <= 63
    if (q > 0) {
        const uint32_t t0 = trees[q - 1];
        if (t0 > t || (t0 == t && indices[q - 1] >= index)) bits |= 2u;
        if (t0 == t && heights[q - 1] != h) bits |= 8u;
    }
    if (bits) atomicOr(status, bits);
}

// multiproof_masks_kernel with a tree and a height per entry: the flags of 64 entries as one ballot word,
// mask[l * words + (q >> 6)], for every l < stride.  The status is the same word in every lane and `stride` a kernel
// argument, so every lane of a wavefront reaches every ballot; lanes past k or past their height vote 0.
__global__ __launch_bounds__(256) void forest_multiproof_masks_kernel(const uint32_t* __restrict__ trees, const uint64_t* __restrict__ indices,
                                                                      const uint32_t* __restrict__ heights, uint32_t k, uint32_t stride, uint64_t words,
                                                                      const uint64_t* __restrict__ hdr, uint64_t* __restrict__ mask)
{
    if (hdr[0] != 0ull) return;
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = q < k;
    const uint32_t t = in ? trees[q] : 0u;
    const uint32_t h = in ? heights[q] : 0u;
    const uint64_t index = in ? indices[q] : 0ull;
    const bool has_prev = in && q > 0 && trees[q - 1] == t;          // a neighbour in another tree is no sibling
    const bool has_next = in && q + 1 < k && trees[q + 1] == t;
    const uint64_t prev = has_prev ? indices[q - 1] : 0ull;
    const uint64_t next = has_next ? indices[q + 1] : 0ull;
    const uint64_t w = q >> 6;
    for (uint32_t l = 0; l < stride; ++l) {      // wave-uniform trip count
        const uint64_t p = index >> l;
        const bool emit_odd = !has_prev || (prev >> l) + 1ull < p;    // first of the run, and p - 1 is not there
        const bool emit_even = !has_next || (next >> l) > p + 1ull;   // last of the run, and p + 1 is not there
        const uint64_t m = __ballot(l < h && ((p & 1ull) ? emit_odd : emit_even));
        if ((threadIdx.x & 63u) == 0u && w < words) mask[(uint64_t)l * words + w] = m;
    }
}

// Gather, one lane per (level, entry): blockIdx.y = l.  A lane whose flag is set (so l < h_q) loads the cell
// forest_proofs_kernel puts at (q, l) and stores it at its rank; a wavefront's ranks are consecutive, so its stores lie back
// to back.  The check ran first: the tree is in range and index < c_t, so p is a node of the tree's level l.  No hash.
__global__ __launch_bounds__(256) void forest_multiproof_gather_kernel(const Node* __restrict__ digests, const Node* __restrict__ forest, ForestLevels lv,
                                                                       const uint64_t* __restrict__ offsets, const uint32_t* __restrict__ trees,
                                                                       const uint64_t* __restrict__ indices, uint32_t k, uint64_t words,
                                                                       const uint64_t* __restrict__ mask, const uint64_t* __restrict__ word_start,
                                                                       const uint64_t* __restrict__ hdr, Node* __restrict__ nodes)
{
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= k || hdr[0] != 0ull) return;
    const uint32_t l = blockIdx.y;
    const uint64_t at = (uint64_t)l * words + (q >> 6);
    const uint64_t m = mask[at];
    const uint64_t bit = 1ull << (q & 63ull);
    if (!(m & bit)) return;
    const uint64_t rank = word_start[at] + (uint64_t)__popcll(m & (bit - 1ull));   // < M <= the buffer's capacity: the status is 0
    const uint32_t t = trees[q];
    const uint64_t off = offsets[t], c = offsets[t + 1u] - off;
    const uint64_t s = vkmr_math::sibling(indices[q] >> l, vkmr_forest::level_count(c, l));
    const Node v = vkmr_dev::load_node((l == 0) ? digests + off + s : forest + lv.base[l] + vkmr_forest::pos(off, t, l) + s);
    uint32_t o[8];
#pragma unroll
    for (int w = 0; w < 8; ++w) o[w] = v.w[w];
    vkmr_dev::store_node(nodes + rank, o);
}

// Verifier, one launch per level l = 0..stride-1, one lane per entry: verify_multiproof_level_kernel's in-place scheme with
// the tree compared wherever two entries are.  The value of node p of tree t's level l lives in cell[first lane of p's run]
// and end[that lane] is the first lane behind the run (level 0: the leaves, and q + 1).  The first lane of parent P's run
// hashes P; a lane whose tree has reached its root (l >= h_q) does nothing, and since the entries of a tree carry one height
// (the check), a tree stops as a whole and the cell of its first entry then holds its root.  The missing child is the
// proof's node at the rank of the entry that owns it.  One hash_pair: the only hash block.  For l > 0 `in` and `cell` are the
// same buffer, deliberately, as in the single-tree twin: a lane reads cells that no lane of this launch writes (its own
// before it writes it, and the cell at end[q], which is no run head), so __restrict__ on both holds for every lane.
__global__ __launch_bounds__(256) void verify_forest_multiproof_level_kernel(const Node* __restrict__ in, Node* __restrict__ cell, uint32_t* __restrict__ end,
                                                                             const uint32_t* __restrict__ trees, const uint64_t* __restrict__ indices,
                                                                             const uint32_t* __restrict__ heights, uint32_t k, uint32_t l, uint64_t words,
                                                                             const uint64_t* __restrict__ mask, const uint64_t* __restrict__ word_start,
                                                                             const Node* __restrict__ nodes, const uint64_t* __restrict__ hdr)
{
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= k || hdr[0] != 0ull) return;
    if (l >= heights[q]) return;                 // the tree's root was formed at a level below
    const uint32_t t = trees[q];
    const uint64_t p = indices[q] >> l;
    const uint64_t P = p >> 1;
    if (q > 0 && trees[q - 1] == t && (indices[q - 1] >> l) >> 1 == P) return;   // not the head of P's run
    const uint64_t e = (l == 0) ? q + 1 : (uint64_t)end[q];
    const bool right = p & 1ull;
    const Node* other;
    uint64_t e2 = e;
    if (right) {
        other = nodes + multiproof_rank(mask, word_start, words, l, q);
    } else if (e < k && trees[e] == t && (indices[e] >> l) >> 1 == P) {
        other = in + e;
        e2 = (l == 0) ? e + 1 : (uint64_t)end[e];
    } else {
        other = nodes + multiproof_rank(mask, word_start, words, l, e - 1);
    }
    // the operand order is chosen on the pointers: selecting between the loaded nodes word by word went through scratch
    const Node x = vkmr_dev::load_node(right ? other : in + q), y = vkmr_dev::load_node(right ? in + q : other);
    uint32_t o[8];
    vkmr_dev::hash_pair(x.w, y.w, o);
    vkmr_dev::store_node(cell + q, o);
    end[q] = (uint32_t)e2;
}

// One lane per entry; *ok was set to 1 before the launch.  A nonzero status (a check failed, or not exactly m nodes would be
// consumed) clears it; else the first entry of each tree's run compares its cell, the tree's root, with roots[trees[q]], and
// any mismatch clears it.  Roots of trees no entry names are not read.
__global__ __launch_bounds__(256) void verify_forest_multiproof_finish_kernel(const Node* __restrict__ cell, const uint32_t* __restrict__ trees, uint32_t k,
                                                                              const Node* __restrict__ roots, const uint64_t* __restrict__ hdr,
                                                                              uint32_t* __restrict__ ok)
{
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= k) return;
    if (hdr[0] != 0ull) {
        if (q == 0) ok[0] = 0u;                  // the cells are only written when the status is 0
        return;
    }
    const uint32_t t = trees[q];
    if (q > 0 && trees[q - 1] == t) return;      // not the first entry of its tree
    if (vkmr_dev::node_diff(vkmr_dev::load_node(cell + q), vkmr_dev::load_node(roots + t)) != 0u) ok[0] = 0u;
}
