// tree_kernels.hpp -- the stored tree's proof gather, the batch verifier, the leaf update and the multiproofs (include/vkmr_hip.h:
// vkmr_hip_tree_proofs_async, vkmr_hip_verify_proofs_async, vkmr_hip_tree_update_async, vkmr_hip_tree_multiproof_async,
// vkmr_hip_verify_multiproof_async, vkmr_hip_apply_multiproof_async), and the ranking kernels that the forest's multiproofs
// launch as well.  The tree itself is built by reduce_level_kernel (reduce_kernels.hpp), one launch per level.  The layout,
// and the bodies of the kernels that have a counterpart in forest_tree_kernels.hpp, are in entries.hpp: such a kernel here
// is its arguments as TreeEntries and TreeCells / TreeSpan, and the call.
#pragma once

#include "entries.hpp"

// Gather, one lane per (proof, level) pair, flattened as i = q * height + l: lane i stores siblings[i], so the 64 lanes of
// a wavefront write 2 KiB back to back.  siblings[q * height + l] = the sibling cell of (l, index_q); an index >= count gets
// zero cells.  No hash: HBM-bound.  forest_proofs_kernel differs in what it writes behind a tree's height, and it writes the heights.
__global__ __launch_bounds__(256) void tree_proofs_kernel(const Node* __restrict__ digests, const Node* __restrict__ tree, TreeLevels lv, uint64_t count,
                                                          uint32_t height, const uint64_t* __restrict__ indices, uint64_t total, Node* __restrict__ siblings)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const uint64_t q = i / height;
    const uint32_t l = (uint32_t)(i - q * height);
    const uint64_t index = indices[q];
    uint32_t o[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (index < count) {
        const Node v = vkmr_dev::load_node(TreeCells{digests, tree, lv, count}.sibling_cell(0u, l, index));
#pragma unroll
        for (int w = 0; w < 8; ++w) o[w] = v.w[w];
    }
    vkmr_dev::store_node(siblings + i, o);
}

// Batch verifier, one lane per proof: folds leaves[q] with siblings[q * height + 0 .. height) as vkmr_host_cpu_fold_proof
// does (bit l of the index set: node = pair(sibling, cur), else pair(cur, sibling)) and compares with roots[q * root_stride];
// ok[q] = 1 when they agree and index_q < 2^height.  `height` is a kernel argument, the same in every lane, so the level
// loop is wave-uniform and its one hash_pair is the kernel's only hash block; the operand order is chosen with selects.
// The next level's sibling is loaded before the current level is hashed (its latency hides under the 3 x 64 rounds of the hash).
// Not one body with verify_forest_proofs_kernel: that one's loop is ballot-driven with per-lane selects, which would slow this one.
__global__ __launch_bounds__(256) void verify_proofs_kernel(const Node* __restrict__ leaves, const uint64_t* __restrict__ indices,
                                                            const Node* __restrict__ siblings, uint32_t k, uint32_t height,
                                                            const Node* __restrict__ roots, uint32_t root_stride, uint32_t* __restrict__ ok)
{
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= k) return;
    const uint64_t index = indices[q];
    const Node* sib = siblings + q * height;
    Node cur = vkmr_dev::load_node(leaves + q);
    Node next = vkmr_dev::load_node(sib);
    for (uint32_t l = 0; l < height; ++l) {
        const Node s = next;
        next = vkmr_dev::load_node(sib + (l + 1 < height ? l + 1 : l));   // the last trip reloads its own sibling: no branch
        const bool right = (index >> l) & 1ull;
        uint32_t a[8], b[8];
#pragma unroll
        for (int w = 0; w < 8; ++w) {
            a[w] = right ? s.w[w] : cur.w[w];
            b[w] = right ? cur.w[w] : s.w[w];
        }
        vkmr_dev::hash_pair(a, b, cur.w);
    }
    const Node root = vkmr_dev::load_node(roots + q * root_stride);
    uint32_t diff = (index >> height) != 0ull ? 1u : 0u;   // height <= 63: an index outside the tree fails
#pragma unroll
    for (int w = 0; w < 8; ++w) diff |= cur.w[w] ^ root.w[w];
    ok[q] = diff == 0u ? 1u : 0u;
}

// ---- leaf updates (vkmr_hip_tree_update_async): the check, then entries.hpp's two writers ----------------------------------

// No hash: bit 0 when index_q >= count, bit 1 when index_{q-1} >= index_q (out of order or repeated).  The checks of the
// entry points differ in their bounds and status bits and are a few lines each: one kernel per contract.
__global__ __launch_bounds__(256) void tree_update_check_kernel(const uint64_t* __restrict__ indices, uint32_t k, uint64_t count,
                                                                uint32_t* __restrict__ status)
{
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= k) return;
    const uint64_t index = indices[q];
    uint32_t bits = index >= count ? 1u : 0u;
    if (q > 0 && indices[q - 1] >= index) bits |= 2u;
    if (bits) atomicOr(status, bits);
}

__global__ __launch_bounds__(256) void tree_update_leaves_kernel(Node* __restrict__ digests, const uint64_t* __restrict__ indices,
                                                                 const Node* __restrict__ leaves, uint32_t k, const uint32_t* __restrict__ status)
{
    update_leaves(TreeEntries{indices}, TreeSpan{}, digests, leaves, k, status);
}

// in = level l - 1 (n_in cells), out = level l.  The check ran first: index_q < count, so p < n_l.
__global__ __launch_bounds__(256) void tree_update_level_kernel(const Node* __restrict__ in, uint64_t n_in, Node* __restrict__ out,
                                                                const uint64_t* __restrict__ indices, uint32_t k, uint32_t l,
                                                                const uint32_t* __restrict__ status)
{
    update_level(TreeEntries{indices}, TreeSpan{n_in}, in, out, (Node*)nullptr, k, l, status);
}

// ---- multiproofs (vkmr_hip_tree_multiproof_async, vkmr_hip_verify_multiproof_async): the scheme is in entries.hpp ----------

__global__ __launch_bounds__(256) void multiproof_masks_kernel(const uint64_t* __restrict__ indices, uint32_t k, uint32_t height, uint64_t words,
                                                               const uint64_t* __restrict__ hdr, uint64_t* __restrict__ mask)
{
    multiproof_masks(TreeEntries{indices, height}, k, height, words, hdr, mask);
}

// The three ranking kernels, the same for one tree and for a forest (height := the forest's stride).
__global__ __launch_bounds__(VKMR_MP_BLOCK_WORDS) void multiproof_block_sums_kernel(const uint64_t* __restrict__ mask, uint64_t words, uint64_t blocks,
                                                                                    uint64_t* __restrict__ block)
{
    __shared__ uint32_t s_wave[VKMR_MP_BLOCK_WORDS / 64];
    const uint64_t w = (uint64_t)blockIdx.x * VKMR_MP_BLOCK_WORDS + threadIdx.x;
    const uint32_t v = w < words ? (uint32_t)__popcll(mask[(uint64_t)blockIdx.y * words + w]) : 0u;
    uint32_t total;
    (void)vkmr_sizes::block_exclusive(v, s_wave, &total);
    if (threadIdx.x == 0) block[(uint64_t)blockIdx.y * blocks + blockIdx.x] = total;
}

// One workgroup.  block[] becomes its exclusive prefix; hdr[1] = M, hdr[2 + l] = m_l.  Status bit 2 when M > limit (the
// gather: the node buffer is too small) or, with `exact`, when M != limit (the verifier: not exactly m nodes would be
// consumed).  A status that the index check has set ends the call here: nothing else is written.
__global__ __launch_bounds__(256) void multiproof_block_starts_kernel(uint64_t* __restrict__ block, uint64_t blocks, uint32_t height, uint64_t limit,
                                                                      uint32_t exact, uint64_t* __restrict__ hdr)
{
    __shared__ uint32_t s_wave[256 / 64];
    __shared__ uint64_t s_level[VKMR_TREE_MAX_LEVELS + 1];
    if (hdr[0] != 0ull) return;                  // the same word in every lane
    const uint64_t n = blocks * height;
    uint64_t carry = 0;
    for (uint64_t base = 0; base < n; base += 256) {   // wave-uniform trip count
        const uint64_t i = base + threadIdx.x;
        const uint32_t v = i < n ? (uint32_t)block[i] : 0u;   // a block holds at most 16384 cells, a round 2^22
        uint32_t total;
        const uint64_t start = carry + vkmr_sizes::block_exclusive(v, s_wave, &total);
        if (i < n) {
            block[i] = start;
            if (i % blocks == 0) s_level[i / blocks] = start;
        }
        carry += total;
        __syncthreads();   // s_wave is reused by the next round
    }
    if (threadIdx.x == 0) {
        s_level[height] = carry;
        hdr[1] = carry;
        if (exact ? carry != limit : carry > limit) hdr[0] = 4ull;
    }
    __syncthreads();
    if (threadIdx.x < height) hdr[2 + threadIdx.x] = s_level[threadIdx.x + 1] - s_level[threadIdx.x];
}

__global__ __launch_bounds__(VKMR_MP_BLOCK_WORDS) void multiproof_word_starts_kernel(const uint64_t* __restrict__ mask, uint64_t words, uint64_t blocks,
                                                                                     const uint64_t* __restrict__ block, const uint64_t* __restrict__ hdr,
                                                                                     uint64_t* __restrict__ word_start)
{
    __shared__ uint32_t s_wave[VKMR_MP_BLOCK_WORDS / 64];
    if (hdr[0] != 0ull) return;                  // the same word in every lane
    const uint64_t w = (uint64_t)blockIdx.x * VKMR_MP_BLOCK_WORDS + threadIdx.x;
    const uint32_t v = w < words ? (uint32_t)__popcll(mask[(uint64_t)blockIdx.y * words + w]) : 0u;
    uint32_t total;
    const uint32_t ex = vkmr_sizes::block_exclusive(v, s_wave, &total);
    if (w < words) word_start[(uint64_t)blockIdx.y * words + w] = block[(uint64_t)blockIdx.y * blocks + blockIdx.x] + ex;
}

// The check ran: index < count.
__global__ __launch_bounds__(256) void tree_multiproof_gather_kernel(const Node* __restrict__ digests, const Node* __restrict__ tree, TreeLevels lv, uint64_t count,
                                                                     const uint64_t* __restrict__ indices, uint32_t k, uint64_t words,
                                                                     const uint64_t* __restrict__ mask, const uint64_t* __restrict__ word_start,
                                                                     const uint64_t* __restrict__ hdr, Node* __restrict__ nodes)
{
    multiproof_gather(TreeEntries{indices}, TreeCells{digests, tree, lv, count}, k, words, mask, word_start, hdr, nodes);
}

// One launch per level l = 0..height-1: the host stops at the height, which this kernel is not given.
__global__ __launch_bounds__(256) void verify_multiproof_level_kernel(const Node* __restrict__ in, Node* __restrict__ cell, uint32_t* __restrict__ end,
                                                                      const uint64_t* __restrict__ indices, uint32_t k, uint32_t l, uint64_t words,
                                                                      const uint64_t* __restrict__ mask, const uint64_t* __restrict__ word_start,
                                                                      const Node* __restrict__ nodes, const uint64_t* __restrict__ hdr)
{
    __builtin_assume(l < VKMR_TREE_MAX_LEVELS);
    multiproof_verify_level(TreeEntries{indices, VKMR_TREE_MAX_LEVELS}, NeverOwn{}, in, cell, end, k, l, words, mask, word_start, nodes, hdr);
}

// ok = 1 when the checks passed (status 0: indices strictly increasing and < 2^height, exactly m nodes consumed) and the
// value of node 0 of level `height` (cell 0) equals the root.  One lane against one root; the forest's finish is one lane
// per tree run, so the two stay apart.
__global__ void verify_multiproof_finish_kernel(const Node* __restrict__ cell, const Node* __restrict__ root, const uint64_t* __restrict__ hdr,
                                                uint32_t* __restrict__ ok)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    uint32_t diff = hdr[0] != 0ull ? 1u : 0u;
    if (!diff) diff = vkmr_dev::node_diff(vkmr_dev::load_node(cell), vkmr_dev::load_node(root));   // the cells are only written when the status is 0
    ok[0] = diff == 0u ? 1u : 0u;
}

// ---- applying a multiproof (vkmr_hip_apply_multiproof_async): the verifier's launches, the level kernel twice as wide ------

// One launch per level l = 0..height-1, grid.y = 2: blockIdx.y is the side, the same in every lane of a workgroup.  Side 0
// folds the old leaves in cell0 / end0, the verifier's fold to the letter; side 1 folds the new leaves in cell1 / end1 and
// takes its own cell where the tree of `count` leaves has no right sibling (entries.hpp: TreeCountOwn).  The sides share
// nothing they write: a lane reads end[q] and end[b] before it writes end[q], so one end array would let the other side's
// lane read a value already advanced.  in0 / in1 are the leaves at l == 0, the side's cells above.  One hash_pair.
__global__ __launch_bounds__(256) void tree_apply_level_kernel(const Node* __restrict__ in0, const Node* __restrict__ in1, Node* __restrict__ cell0,
                                                                     Node* __restrict__ cell1, uint32_t* __restrict__ end0, uint32_t* __restrict__ end1,
                                                                     const uint64_t* __restrict__ indices, uint64_t count, uint32_t k, uint32_t l,
                                                                     uint64_t words, const uint64_t* __restrict__ mask,
                                                                     const uint64_t* __restrict__ word_start, const Node* __restrict__ nodes,
                                                                     const uint64_t* __restrict__ hdr)
{
    __builtin_assume(l < VKMR_TREE_MAX_LEVELS);
    const uint32_t side = blockIdx.y;
    multiproof_verify_level(TreeEntries{indices, VKMR_TREE_MAX_LEVELS}, TreeCountOwn{count, side}, side ? in1 : in0, side ? cell1 : cell0,
                            side ? end1 : end0, k, l, words, mask, word_start, nodes, hdr);
}

// Behind the finish kernel, which compared side 0 with the old root and wrote ok: when it is 1, cell 0 of side 1 -- the new
// root -- goes to new_root, which may be the old root's own cell (it was last read by the finish).  Else nothing is written.
__global__ void tree_apply_commit_kernel(const Node* __restrict__ cell1, const uint32_t* __restrict__ ok, Node* __restrict__ new_root)
{
    if (threadIdx.x != 0 || blockIdx.x != 0 || ok[0] != 1u) return;
    vkmr_dev::store_node(new_root, vkmr_dev::load_node(cell1));
}
