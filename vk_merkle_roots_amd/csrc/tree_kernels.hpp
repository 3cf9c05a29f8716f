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
        const uint64_t s = vkmr_math::sibling(index >> l, n);
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
    vkmr_dev::store_node(digests + indices[q], vkmr_dev::load_node(leaves + q));
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
    uint32_t o[8];
    vkmr_dev::hash_parent(in, n_in, p, o);
    vkmr_dev::store_node(out + p, o);
}

// ---- multiproofs (vkmr_hip_tree_multiproof_async, vkmr_hip_verify_multiproof_async) -------------------------------------
// One proof for k leaves of one tree: per level l, for every node p of A_l = unique(indices >> l) whose sibling p ^ 1 is not
// in A_l, the sibling's cell (the node's own where it has none), in level-major, ascending-p order.  Who emits follows from
// the sorted indices alone: entry q "owns" the cell of (l, p = index_q >> l) when p is odd and q is the first lane of p's run
// (p - 1 is in A_l iff the lane before has it), or p is even and q is the last lane of the run (p + 1 iff the lane after).
// The gather and the verifier share the ranking of those flags:
//   masks        one lane per entry, a loop over the levels: the flags of 64 entries as one ballot word, mask[l * W + (q >> 6)]
//   block_sums   one lane per word: set bits per block of 256 words
//   block_starts one workgroup: exclusive prefix over the (level, block) sums in 64 bits; M, the per-level counts, the bound
//   word_starts  one lane per word: cells emitted before the word
// so that the cell of (l, q) has rank word_start + popcount(mask below q's bit): two loads, and no flag is computed twice.
// Header (uint64 words): [0] status (its low 32 bits are what tree_update_check_kernel ORs into), [1] M, [2 + l] m_l.  The
// gather's header is the caller's info_dev, the verifier's lies in its scratch.

#define VKMR_MP_HEADER_WORDS (2 + VKMR_TREE_MAX_LEVELS)   // status, M, up to 64 level counts
#define VKMR_MP_BLOCK_WORDS 256                           // ballot words per block of the prefix sum: 16384 entries

__global__ __launch_bounds__(256) void multiproof_masks_kernel(const uint64_t* __restrict__ indices, uint32_t k, uint32_t height, uint64_t words,
                                                               uint64_t* __restrict__ mask)
{
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = q < k;                       // the lanes past k vote 0: every lane of the wavefront reaches the ballots
    const uint64_t index = in ? indices[q] : 0ull;
    const bool has_prev = in && q > 0, has_next = in && q + 1 < k;
    const uint64_t prev = has_prev ? indices[q - 1] : 0ull;
    const uint64_t next = has_next ? indices[q + 1] : 0ull;
    const uint64_t w = q >> 6;
    for (uint32_t l = 0; l < height; ++l) {      // wave-uniform trip count
        const uint64_t p = index >> l;
        const bool emit_odd = !has_prev || (prev >> l) + 1ull < p;    // first of the run, and p - 1 is not there
        const bool emit_even = !has_next || (next >> l) > p + 1ull;   // last of the run, and p + 1 is not there
        const uint64_t m = __ballot(in && ((p & 1ull) ? emit_odd : emit_even));
        if ((threadIdx.x & 63u) == 0u && w < words) mask[(uint64_t)l * words + w] = m;
    }
}

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

// Rank of the cell that entry j owns at level l (its flag is set: the callers know).
__device__ __forceinline__ uint64_t multiproof_rank(const uint64_t* __restrict__ mask, const uint64_t* __restrict__ word_start, uint64_t words, uint32_t l,
                                                    uint64_t j)
{
    const uint64_t at = (uint64_t)l * words + (j >> 6);
    return word_start[at] + (uint64_t)__popcll(mask[at] & ((1ull << (j & 63ull)) - 1ull));
}

// Gather, one lane per (level, entry): blockIdx.y = l.  A lane whose flag is set loads the sibling cell as tree_proofs_kernel
// does and stores it at its rank; a wavefront's ranks are consecutive, so its stores lie back to back.  No hash.
__global__ __launch_bounds__(256) void tree_multiproof_gather_kernel(const Node* __restrict__ digests, const Node* __restrict__ tree, TreeLevels lv, uint64_t count,
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
    const uint64_t n = ((count - 1) >> l) + 1;     // cells of level l; the check ran: index < count, so p < n
    const uint64_t s = vkmr_math::sibling(indices[q] >> l, n);
    const Node v = vkmr_dev::load_node((l == 0) ? digests + s : tree + lv.off[l] + s);
    uint32_t o[8];
#pragma unroll
    for (int w = 0; w < 8; ++w) o[w] = v.w[w];
    vkmr_dev::store_node(nodes + rank, o);
}

// Verifier, one launch per level l = 0..height-1 (level l + 1 from level l), one lane per entry.  The value of node p of
// level l lives in cell[first lane of p's run], and end[that lane] is the first lane behind the run (level 0: the leaves,
// and q + 1).  The first lane of parent P's run hashes P: an even child p is its own cell, and the run that starts at end[q]
// is p + 1 when it has the same parent; an odd child at the head of P's run has no left sibling among the entries.  The
// missing child is the proof's node at the rank of the entry that owns it (the last lane of an even p's run, the first of an
// odd p's): the order the gather emits in.  A lane writes only its own cell and end, which no other lane of the launch reads
// (the lane at end[q] lies inside P's run, not at its head), so the levels run in place.  One hash_pair: the only hash block.
__global__ __launch_bounds__(256) void verify_multiproof_level_kernel(const Node* __restrict__ in, Node* __restrict__ cell, uint32_t* __restrict__ end,
                                                                      const uint64_t* __restrict__ indices, uint32_t k, uint32_t l, uint64_t words,
                                                                      const uint64_t* __restrict__ mask, const uint64_t* __restrict__ word_start,
                                                                      const Node* __restrict__ nodes, const uint64_t* __restrict__ hdr)
{
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= k || hdr[0] != 0ull) return;
    const uint64_t p = indices[q] >> l;
    const uint64_t P = p >> 1;
    if (q > 0 && (indices[q - 1] >> l) >> 1 == P) return;   // not the head of P's run
    const uint64_t e = (l == 0) ? q + 1 : (uint64_t)end[q];
    const bool right = p & 1ull;
    const Node* other;
    uint64_t e2 = e;
    if (right) {
        other = nodes + multiproof_rank(mask, word_start, words, l, q);
    } else if (e < k && (indices[e] >> l) >> 1 == P) {
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

// ok = 1 when the checks passed (status 0: indices strictly increasing and < 2^height, exactly m nodes consumed) and the
// value of node 0 of level `height` (cell 0) equals the root.
__global__ void verify_multiproof_finish_kernel(const Node* __restrict__ cell, const Node* __restrict__ root, const uint64_t* __restrict__ hdr,
                                                uint32_t* __restrict__ ok)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    uint32_t diff = hdr[0] != 0ull ? 1u : 0u;
    if (!diff) diff = vkmr_dev::node_diff(vkmr_dev::load_node(cell), vkmr_dev::load_node(root));   // the cells are only written when the status is 0
    ok[0] = diff == 0u ? 1u : 0u;
}
