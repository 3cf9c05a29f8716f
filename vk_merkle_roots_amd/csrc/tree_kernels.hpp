// tree_kernels.hpp -- the stored tree's proof gather, the batch verifier and the leaf update (include/vkmr_hip.h:
// vkmr_hip_tree_proofs_async, vkmr_hip_verify_proofs_async, vkmr_hip_tree_update_async).  The tree itself is built by
// reduce_level_kernel (reduce_kernels.hpp), one launch per level.
//
// Layout (vkmr_hip_reduce_tree_async): level 0 is the caller's digests; levels 1..height lie back to back in one buffer,
// level l (n_l = ceil(count / 2^l) cells) starting at cell off[l] = sum of n_j over 1 <= j < l.
#pragma once

#define VKMR_TREE_MAX_LEVELS 64

// Start cell of every level inside the tree buffer, passed by value (kernel arguments: 512 bytes).  off[0] is unused:
// level 0 is the digests buffer.
struct TreeLevels { uint64_t off[VKMR_TREE_MAX_LEVELS]; };

// Gather, one lane per (proof, level) pair, flattened as i = q * height + l: lane i stores siblings[i], so the 64 lanes of
// a wavefront write 2 KiB back to back.  siblings[q * height + l] = L[l][p ^ 1] with p = index_q >> l, or L[l][p] where
// p ^ 1 is past the level's end (duplicate-last rule); an index >= count gets zero cells.  No hash: HBM-bound.
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
        const uint64_t n = ((count - 1) >> l) + 1;     // cells of level l
        const uint64_t p = index >> l;
        const uint64_t s = ((p ^ 1ull) < n) ? (p ^ 1ull) : p;
        const Node* cell = (l == 0) ? digests + s : tree + lv.off[l] + s;
        const Node v = vkmr_dev::load_node(cell);
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

// ---- leaf updates (vkmr_hip_tree_update_async) --------------------------------------------------------------------------
// Three launches on one stream, every lane one update entry q < k: the check ORs the contract's violations into *status
// (zeroed by the host), and the two writers read *status first and write nothing when it is nonzero, so a rejected batch
// leaves the leaves and the tree as they were.

// No hash: bit 0 when index_q >= count, bit 1 when index_{q-1} >= index_q (out of order or repeated).
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

// No hash: digests[index_q] = leaves[q].
__global__ __launch_bounds__(256) void tree_update_leaves_kernel(Node* __restrict__ digests, const uint64_t* __restrict__ indices,
                                                                 const Node* __restrict__ leaves, uint32_t k, const uint32_t* __restrict__ status)
{
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= k || *status != 0u) return;
    const Node v = vkmr_dev::load_node(leaves + q);
    uint32_t o[8];
#pragma unroll
    for (int w = 0; w < 8; ++w) o[w] = v.w[w];
    vkmr_dev::store_node(digests + indices[q], o);
}

// One level l >= 1 per launch: in = level l - 1 (n_in cells), out = level l.  Lane q hashes parent p = index_q >> l when it
// is the first lane of its run (the indices are sorted, so lanes with the same parent are adjacent): each dirty node is
// hashed exactly once, distinct lanes write distinct cells and read only the level below.  reduce_level_kernel's body with
// a different index; its one hash_pair is the kernel's only hash block.  The check ran first: index_q < count, so p < n_l.
__global__ __launch_bounds__(256) void tree_update_level_kernel(const Node* __restrict__ in, uint64_t n_in, Node* __restrict__ out,
                                                                const uint64_t* __restrict__ indices, uint32_t k, uint32_t l,
                                                                const uint32_t* __restrict__ status)
{
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= k || *status != 0u) return;
    const uint64_t p = indices[q] >> l;
    if (q > 0 && (indices[q - 1] >> l) == p) return;
    const Node a = vkmr_dev::load_node(in + 2 * p);
    const Node b = vkmr_dev::load_node(in + ((2 * p + 1 < n_in) ? 2 * p + 1 : 2 * p));
    uint32_t o[8];
    vkmr_dev::hash_pair(a.w, b.w, o);
    vkmr_dev::store_node(out + p, o);
}
