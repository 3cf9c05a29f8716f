// forest_tree_kernels.hpp -- proofs from a stored forest and the batch verifier for proofs of unequal height
// (include/vkmr_hip.h: vkmr_hip_forest_proofs_async, vkmr_hip_verify_forest_proofs_async).  The stored forest itself is
// written by forest_level_kernel (forest_kernels.hpp), one launch per level: only the buffers the host passes differ.
//
// Layout (vkmr_hip_reduce_forest_tree_async, forest_plan.hpp): level 0 is the caller's leaves, tree t at cell offsets[t];
// level l >= 1 has its own buffer of level_cells(l) cells starting at cell base[l] = sum of level_cells(j) over 1 <= j < l,
// and tree t's n_l = ceil(c_t / 2^l) nodes start at cell pos_l(t) = (offsets[t] >> l) + t of it.  Level h_t of a tree is its
// root and lies in roots_dev, not here; a proof reads levels 0 .. h_t - 1 only.
#pragma once

#include "forest_plan.hpp"
#include "tree_kernels.hpp"

// First cell of every level's buffer inside the stored forest, passed by value as TreeLevels is.  base[0] is unused:
// level 0 is the leaves buffer.
struct ForestLevels { uint64_t base[VKMR_TREE_MAX_LEVELS]; };

// Gather, one lane per (query, level) pair, flattened as i = q * H + l: lane i stores siblings[i], so the 64 lanes of a
// wavefront write 2 KiB back to back.  Query q is leaf indices[q] of tree trees[q]; for l < h_t the cell is
// L_t[l][p ^ 1] with p = index >> l, or L_t[l][p] where p ^ 1 is past the level's end (tree_proofs_kernel's rule on tree t
// alone), for l >= h_t it is zero.  A tree >= ntrees or an index >= c_t gets height 0 and zero cells.  The lane of l == 0
// writes the height.  No hash: the count-leading-zeros of height() costs nothing that matters here.
__global__ __launch_bounds__(256) void forest_proofs_kernel(const Node* __restrict__ digests, const Node* __restrict__ forest, ForestLevels lv,
                                                            const uint64_t* __restrict__ offsets, uint32_t ntrees, uint32_t H,
                                                            const uint32_t* __restrict__ trees, const uint64_t* __restrict__ indices, uint64_t total,
                                                            Node* __restrict__ siblings, uint32_t* __restrict__ heights)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const uint64_t q = i / H;
    const uint32_t l = (uint32_t)(i - q * H);
    const uint32_t t = trees[q];
    const uint64_t index = indices[q];
    uint32_t o[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t h = 0;
    if (t < ntrees) {
        const uint64_t off = offsets[t], c = offsets[t + 1u] - off;
        if (index < c) {                               // never true for an empty tree
            h = vkmr_forest::height(c);                // <= H: the build checked c <= max_count
            if (l < h) {
                const uint64_t n = vkmr_forest::level_count(c, l);
                const uint64_t p = index >> l;
                const uint64_t s = vkmr_math::sibling(p, n);
                const Node* cell = (l == 0) ? digests + off + s : forest + lv.base[l] + vkmr_forest::pos(off, t, l) + s;
                const Node v = vkmr_dev::load_node(cell);
#pragma unroll
                for (int w = 0; w < 8; ++w) o[w] = v.w[w];
            }
        }
    }
    vkmr_dev::store_node(siblings + i, o);
    if (l == 0) heights[q] = h;
}

// Batch verifier, one lane per proof: verify_proofs_kernel's body with a height per lane.  Proof q is valid to fold when
// 1 <= heights[q] <= stride, indices[q] < 2^heights[q] and trees[q] < ntrees; it then folds leaves[q] with
// siblings[q * stride + 0 .. heights[q]) as vkmr_host_cpu_fold_proof does and is compared with roots[trees[q]].  The level
// loop runs while any lane of the wavefront still has a level to fold -- a ballot, so the trip count is wave-uniform and the
// loop's one hash_pair is the kernel's only hash block -- and a lane that has reached its own height keeps its value by a
// select.  Such a lane, and a lane whose proof is not valid, loads nothing behind its height: its sibling pointer stays on
// the last cell it may read (an invalid proof's on its own leaf).  The next level's sibling is loaded before the current
// level is hashed, as in verify_proofs_kernel.  Left alone the compiler keeps 105 scalar registers, one
// allocation block too many for 8 wavefronts per SIMD; held to 96 it still spills nothing.
__global__ __launch_bounds__(256) __attribute__((amdgpu_num_sgpr(96)))
void verify_forest_proofs_kernel(const Node* __restrict__ leaves, const uint32_t* __restrict__ trees, const uint64_t* __restrict__ indices,
                                 const Node* __restrict__ siblings, const uint32_t* __restrict__ heights, uint32_t k, uint32_t stride,
                                 const Node* __restrict__ roots, uint32_t ntrees, uint32_t* __restrict__ ok)
{
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= k) return;
    const uint64_t index = indices[q];
    const uint32_t t = trees[q];
    const uint32_t height = heights[q];
    const bool valid = height >= 1u && height <= stride && t < ntrees && (index >> (height & 63u)) == 0ull;   // stride <= 63
    const uint32_t h = valid ? height : 0u;            // the levels this lane folds
    const Node* sib = valid ? siblings + q * stride : leaves + q;
    const uint32_t last = valid ? h - 1u : 0u;
    Node cur = vkmr_dev::load_node(leaves + q);
    Node next = vkmr_dev::load_node(sib);
    for (uint32_t l = 0; __ballot(l < h) != 0ull; ++l) {
        const Node s = next;
        next = vkmr_dev::load_node(sib + (l + 1u < h ? l + 1u : last));   // behind the lane's height: its last cell again, no branch
        const bool right = (index >> l) & 1ull;
        uint32_t a[8], b[8], x[8];
#pragma unroll
        for (int w = 0; w < 8; ++w) {
            a[w] = right ? s.w[w] : cur.w[w];
            b[w] = right ? cur.w[w] : s.w[w];
        }
        vkmr_dev::hash_pair(a, b, x);
        const bool live = l < h;
#pragma unroll
        for (int w = 0; w < 8; ++w) cur.w[w] = live ? x[w] : cur.w[w];
    }
    uint32_t diff = 1u;
    if (valid) {
        const Node root = vkmr_dev::load_node(roots + t);
        diff = 0u;
#pragma unroll
        for (int w = 0; w < 8; ++w) diff |= cur.w[w] ^ root.w[w];
    }
    ok[q] = diff == 0u ? 1u : 0u;
}
