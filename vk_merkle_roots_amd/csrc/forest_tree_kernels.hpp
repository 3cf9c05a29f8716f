// forest_tree_kernels.hpp -- the stored forest's proof gather, the batch verifier for proofs of unequal height, the leaf update
// and the multiproofs (include/vkmr_hip.h: vkmr_hip_forest_proofs_async, vkmr_hip_verify_forest_proofs_async,
// vkmr_hip_forest_update_async, vkmr_hip_forest_multiproof_async, vkmr_hip_verify_forest_multiproof_async,
// vkmr_hip_apply_forest_multiproof_async).  The stored forest
// itself is written by forest_level_kernel (forest_kernels.hpp), one launch per level: only the buffers the host passes
// differ.  The layout, and the bodies of the kernels that have a counterpart in tree_kernels.hpp, are in entries.hpp: such a
// kernel here is its arguments as ForestEntries and ForestCells / ForestSpan, and the call.  Every lane is one entry q < k,
// the pair (trees[q], indices[q]); the updates and the multiproofs take the pairs strictly increasing, so the entries of one
// tree are adjacent and, inside a tree, lanes with the same node are.
#pragma once

#include "tree_kernels.hpp"

// Gather, one lane per (query, level) pair, flattened as i = q * H + l: lane i stores siblings[i], so the 64 lanes of a
// wavefront write 2 KiB back to back.  Query q is leaf indices[q] of tree trees[q]; for l < h_t the cell is the sibling cell
// of (l, index) in tree t alone, for l >= h_t it is zero.  A tree >= ntrees or an index >= c_t gets height 0 and zero
// cells.  The lane of l == 0 writes the height.  No hash: the count-leading-zeros of height() costs nothing that matters here.
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
        const uint64_t c = offsets[t + 1u] - offsets[t];
        if (index < c) {                               // never true for an empty tree
            h = vkmr_forest::height(c);                // <= H: the build checked c <= max_count
            if (l < h) {
                const Node v = vkmr_dev::load_node(ForestCells{digests, forest, lv, offsets}.sibling_cell(t, l, index));
#pragma unroll
                for (int w = 0; w < 8; ++w) o[w] = v.w[w];
            }
        }
    }
    vkmr_dev::store_node(siblings + i, o);
    if (l == 0) heights[q] = h;
}

// Batch verifier, one lane per proof: verify_proofs_kernel's scheme with a height per lane, in a body of its own (the loop
// here is ballot-driven, with per-lane selects and a cap on the scalar registers).  Proof q is valid to fold when 1 <= heights[q] <= stride, indices[q] < 2^heights[q] and trees[q] < ntrees; it then folds leaves[q] with
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

// ---- leaf updates (vkmr_hip_forest_update_async): the check, then entries.hpp's two writers -------------------------------

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

__global__ __launch_bounds__(256) void forest_update_leaves_kernel(Node* __restrict__ digests, const uint64_t* __restrict__ offsets,
                                                                   const uint32_t* __restrict__ trees, const uint64_t* __restrict__ indices,
                                                                   const Node* __restrict__ leaves, uint32_t k, const uint32_t* __restrict__ status)
{
    update_leaves(ForestEntries{trees, indices}, ForestSpan{offsets}, digests, leaves, k, status);
}

// in = the buffer of level l - 1 (the leaves for l == 1), out = the buffer of level l.  The check ran first: index_q < c_t, so
// p is a node of level l and every cell read is one of tree t's own.
__global__ __launch_bounds__(256) void forest_update_level_kernel(const Node* __restrict__ in, Node* __restrict__ out, Node* __restrict__ roots,
                                                                  const uint64_t* __restrict__ offsets, const uint32_t* __restrict__ trees,
                                                                  const uint64_t* __restrict__ indices, uint32_t k, uint32_t l,
                                                                  const uint32_t* __restrict__ status)
{
    update_level(ForestEntries{trees, indices}, ForestSpan{offsets}, in, out, roots, k, l, status);
}

// ---- multiproofs (vkmr_hip_forest_multiproof_async, vkmr_hip_verify_forest_multiproof_async): the scheme is in entries.hpp,
// the ranking kernels in tree_kernels.hpp, launched with height := the forest's stride --------------------------------------

// No hash: heights[q] = h_t = max(1, ceil(log2 c_t)) of entry q's tree (a count-leading-zeros, as forest_proofs_kernel).  The
// check ran first: the tree is one of the forest's and holds a leaf.  One tree's height is an argument: no counterpart.
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

__global__ __launch_bounds__(256) void forest_multiproof_masks_kernel(const uint32_t* __restrict__ trees, const uint64_t* __restrict__ indices,
                                                                      const uint32_t* __restrict__ heights, uint32_t k, uint32_t stride, uint64_t words,
                                                                      const uint64_t* __restrict__ hdr, uint64_t* __restrict__ mask)
{
    multiproof_masks(ForestEntries{trees, indices, heights}, k, stride, words, hdr, mask);
}

// The check ran first: the tree is in range and index < c_t, so p is a node of the tree's level l.
__global__ __launch_bounds__(256) void forest_multiproof_gather_kernel(const Node* __restrict__ digests, const Node* __restrict__ forest, ForestLevels lv,
                                                                       const uint64_t* __restrict__ offsets, const uint32_t* __restrict__ trees,
                                                                       const uint64_t* __restrict__ indices, uint32_t k, uint64_t words,
                                                                       const uint64_t* __restrict__ mask, const uint64_t* __restrict__ word_start,
                                                                       const uint64_t* __restrict__ hdr, Node* __restrict__ nodes)
{
    multiproof_gather(ForestEntries{trees, indices}, ForestCells{digests, forest, lv, offsets}, k, words, mask, word_start, hdr, nodes);
}

// One launch per level l = 0..stride-1.
__global__ __launch_bounds__(256) void verify_forest_multiproof_level_kernel(const Node* __restrict__ in, Node* __restrict__ cell, uint32_t* __restrict__ end,
                                                                             const uint32_t* __restrict__ trees, const uint64_t* __restrict__ indices,
                                                                             const uint32_t* __restrict__ heights, uint32_t k, uint32_t l, uint64_t words,
                                                                             const uint64_t* __restrict__ mask, const uint64_t* __restrict__ word_start,
                                                                             const Node* __restrict__ nodes, const uint64_t* __restrict__ hdr)
{
    multiproof_verify_level(ForestEntries{trees, indices, heights}, NeverOwn{}, in, cell, end, k, l, words, mask, word_start, nodes, hdr);
}

// One lane per entry; *ok was set to 1 before the launch.  A nonzero status (a check failed, or not exactly m nodes would be
// consumed) clears it; else the first entry of each tree's run compares its cell, the tree's root, with roots[trees[q]], and
// any mismatch clears it.  Roots of trees no entry names are not read.  One lane per tree run; the single tree's finish is
// one lane against one root, so the two stay apart.
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

// ---- applying a forest multiproof (vkmr_hip_apply_forest_multiproof_async): the verifier's launches on heights derived from
// the counts, the level kernel twice as wide, one commit behind the finish ---------------------------------------------------

// No hash, in front of the verifier's own check: heights[q] = max(1, ceil(log2 counts[q])), and what only the counts can
// violate ORed into the status -- bit 0 for a count of 0 (its height is written as 0, which the verifier's check refuses as
// well) or an index >= the count, bit 3 when the entry in front names the same tree with another count.
__global__ __launch_bounds__(256) void forest_apply_heights_kernel(const uint32_t* __restrict__ trees, const uint64_t* __restrict__ indices,
                                                                              const uint64_t* __restrict__ counts, uint32_t k,
                                                                              uint32_t* __restrict__ heights, uint32_t* __restrict__ status)
{
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= k) return;
    const uint64_t c = counts[q];
    heights[q] = c == 0ull ? 0u : vkmr_forest::height(c);
    uint32_t bits = (c == 0ull || indices[q] >= c) ? 1u : 0u;
    if (q > 0 && trees[q - 1] == trees[q] && counts[q - 1] != c) bits |= 8u;
    if (bits) atomicOr(status, bits);
}

// One launch per level l = 0..stride-1, grid.y = 2: tree_apply_level_kernel (tree_kernels.hpp) with a tree, a height
// and a count per entry.
__global__ __launch_bounds__(256) void forest_apply_level_kernel(const Node* __restrict__ in0, const Node* __restrict__ in1,
                                                                            Node* __restrict__ cell0, Node* __restrict__ cell1,
                                                                            uint32_t* __restrict__ end0, uint32_t* __restrict__ end1,
                                                                            const uint32_t* __restrict__ trees, const uint64_t* __restrict__ indices,
                                                                            const uint32_t* __restrict__ heights, const uint64_t* __restrict__ counts,
                                                                            uint32_t k, uint32_t l, uint64_t words, const uint64_t* __restrict__ mask,
                                                                            const uint64_t* __restrict__ word_start, const Node* __restrict__ nodes,
                                                                            const uint64_t* __restrict__ hdr)
{
    const uint32_t side = blockIdx.y;
    multiproof_verify_level(ForestEntries{trees, indices, heights}, ForestCountOwn{counts, side}, side ? in1 : in0, side ? cell1 : cell0,
                            side ? end1 : end0, k, l, words, mask, word_start, nodes, hdr);
}

// Behind the finish kernel, which compared side 0 with the old roots and left ok: when it is 1, the first entry of each
// tree's run stores its side-1 cell, the tree's new root, to new_roots[t], which may be the old roots themselves (the finish
// read them last).  Cells of trees no entry names are not written, and nothing is when ok is 0.
__global__ __launch_bounds__(256) void forest_apply_commit_kernel(const Node* __restrict__ cell1, const uint32_t* __restrict__ trees, uint32_t k,
                                                                             const uint32_t* __restrict__ ok, Node* __restrict__ new_roots)
{
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= k || ok[0] != 1u) return;
    const uint32_t t = trees[q];
    if (q > 0 && trees[q - 1] == t) return;      // not the first entry of its tree
    vkmr_dev::store_node(new_roots + t, vkmr_dev::load_node(cell1 + q));
}
