// merkleblock_kernels.hpp -- partial Merkle trees in BIP37 order from a stored tree or forest (include/vkmr_hip.h:
// vkmr_hip_forest_merkleblocks_async, vkmr_hip_tree_merkleblock_async).  The rule and the closed form of every position are in
// merkleblock_plan.hpp; no kernel here hashes.  Every lane is one sorted entry q < k (or one named tree b < B), the entries
// checked by forest_update_check_kernel / tree_update_check_kernel into the low half of hdr[0] first; every kernel reads hdr[0]
// before anything else and does nothing when a check failed.  hdr is the caller's info_dev: [0] status, [1] B, [2] hashes,
// [3] flag bytes.
//   sums         per entry its group (flags, hashes, 1 when it is its tree's first), summed per workgroup of 256
//   starts       one workgroup: the exclusive prefix of the three sums in 64 bits; B and the hashes
//   places       per entry what lies in front of its group; the first entry of a tree writes its block's row
//   byte_sums    per block its flags, and the bytes they take, summed per workgroup
//   byte_starts  one workgroup: the prefix of those; the flag bytes; status bit 2 when either buffer is too small
//   byte_places  per block where its bytes begin (also under bit 2: the per-block arrays and the totals are valid then)
//   zero         the scratch words the flags are ORed into, as far as they are used
//   emit         one lane per (entry, level): at most three nodes copied, one atomicOr for the path flag
//   flags        the scratch words out to the caller's bytes, exactly info[3] of them
// One body per operation: a kernel is its arguments as TreeEntries / ForestEntries, TreeCounts / ForestCounts and TreeCells /
// ForestCells, and the call.
#pragma once

#include "merkleblock_plan.hpp"
#include "tree_kernels.hpp"

static_assert(VKMR_MB_THREADS == VKMR_SIZES_THREADS, "block_exclusive's workgroup");

// The leaves of the tree an entry names.
struct TreeCounts {
    uint64_t c;
    __device__ __forceinline__ uint64_t count(uint32_t) const { return c; }
};
struct ForestCounts {
    const uint64_t* offsets;
    __device__ __forceinline__ uint64_t count(uint32_t t) const { return offsets[t + 1u] - offsets[t]; }
};

// What lane q knows of entry q: its neighbours in the same tree, its group and the tail behind a tree's last entry.  A lane
// past k has an empty group.
struct MerkleblockEntry {
    bool in, has_prev, has_next;
    uint32_t t, h, tail;
    uint64_t a, i, c;
    vkmr_mb::Group g;
};

template <class Entries, class Counts>
__device__ __forceinline__ MerkleblockEntry merkleblock_entry(const Entries e, const Counts n, uint64_t q, uint32_t k)
{
    MerkleblockEntry m;
    m.in = q < k;
    m.t = m.in ? e.tree(q) : 0u;
    m.i = m.in ? e.indices[q] : 0ull;
    m.has_prev = m.in && q > 0 && e.tree(q - 1) == m.t;
    m.has_next = m.in && q + 1 < k && e.tree(q + 1) == m.t;
    m.a = m.has_prev ? e.indices[q - 1] : 0ull;
    m.c = m.in ? n.count(m.t) : 1ull;
    m.h = vkmr_mb::height(m.c);
    m.g = vkmr_mb::group(m.has_prev, m.a, m.i, m.h);
    m.tail = (m.in && !m.has_next) ? vkmr_mb::tail(m.i, m.c, m.h) : 0u;
    if (!m.in) m.g.flags = m.g.hashes = 0u;
    return m;
}

template <class Entries, class Counts>
__device__ __forceinline__ void merkleblock_sums(const Entries e, const Counts n, uint32_t k, uint64_t groups, const uint64_t* __restrict__ hdr,
                                                 uint64_t* __restrict__ sums)
{
    __shared__ uint32_t s_flags[VKMR_MB_THREADS / 64], s_hashes[VKMR_MB_THREADS / 64], s_heads[VKMR_MB_THREADS / 64];
    if (hdr[0] != 0ull) return;                  // the same word in every lane
    const uint64_t q = (uint64_t)blockIdx.x * VKMR_MB_THREADS + threadIdx.x;
    const MerkleblockEntry m = merkleblock_entry(e, n, q, k);
    uint32_t flags, hashes, heads;
    (void)vkmr_sizes::block_exclusive(m.g.flags + m.tail, s_flags, &flags);
    (void)vkmr_sizes::block_exclusive(m.g.hashes + m.tail, s_hashes, &hashes);
    (void)vkmr_sizes::block_exclusive((m.in && !m.has_prev) ? 1u : 0u, s_heads, &heads);
    if (threadIdx.x == 0) {
        sums[blockIdx.x] = flags;
        sums[groups + blockIdx.x] = hashes;
        sums[2 * groups + blockIdx.x] = heads;
    }
}

// One workgroup: v[0 .. n) becomes its exclusive prefix in 64 bits (every element is below 2^32); returns the sum.
__device__ __forceinline__ uint64_t merkleblock_prefix(uint64_t* __restrict__ v, uint64_t n, uint32_t* s_wave)
{
    uint64_t carry = 0;
    for (uint64_t base = 0; base < n; base += VKMR_MB_THREADS) {   // wave-uniform trip count
        const uint64_t i = base + threadIdx.x;
        const uint32_t x = i < n ? (uint32_t)v[i] : 0u;
        uint32_t total;
        const uint64_t start = carry + vkmr_sizes::block_exclusive(x, s_wave, &total);
        if (i < n) v[i] = start;
        carry += total;
        __syncthreads();                         // s_wave is reused by the next round
    }
    return carry;
}

__global__ __launch_bounds__(VKMR_MB_THREADS) void merkleblock_starts_kernel(uint64_t* __restrict__ sums, uint64_t groups, uint64_t* __restrict__ hdr,
                                                                             uint64_t* __restrict__ bit_start, uint64_t* __restrict__ hash_starts)
{
    __shared__ uint32_t s_wave[VKMR_MB_THREADS / 64];
    if (hdr[0] != 0ull) return;
    const uint64_t flags = merkleblock_prefix(sums, groups, s_wave);
    const uint64_t hashes = merkleblock_prefix(sums + groups, groups, s_wave);
    const uint64_t B = merkleblock_prefix(sums + 2 * groups, groups, s_wave);
    if (threadIdx.x == 0) {
        hdr[1] = B;
        hdr[2] = hashes;
        bit_start[B] = flags;                    // B <= k: the row behind the last block
        hash_starts[B] = hashes;
    }
}

template <class Entries, class Counts>
__device__ __forceinline__ void merkleblock_places(const Entries e, const Counts n, uint32_t k, uint64_t groups, const uint64_t* __restrict__ hdr,
                                                   const uint64_t* __restrict__ sums, uint64_t* __restrict__ flag_at, uint64_t* __restrict__ hash_at,
                                                   uint32_t* __restrict__ block_of, uint64_t* __restrict__ bit_start, uint32_t* __restrict__ block_trees,
                                                   uint64_t* __restrict__ block_counts, uint64_t* __restrict__ hash_starts)
{
    __shared__ uint32_t s_flags[VKMR_MB_THREADS / 64], s_hashes[VKMR_MB_THREADS / 64], s_heads[VKMR_MB_THREADS / 64];
    if (hdr[0] != 0ull) return;
    const uint64_t q = (uint64_t)blockIdx.x * VKMR_MB_THREADS + threadIdx.x;
    const MerkleblockEntry m = merkleblock_entry(e, n, q, k);
    const bool head = m.in && !m.has_prev;
    uint32_t total;
    const uint64_t f = sums[blockIdx.x] + vkmr_sizes::block_exclusive(m.g.flags + m.tail, s_flags, &total);
    const uint64_t x = sums[groups + blockIdx.x] + vkmr_sizes::block_exclusive(m.g.hashes + m.tail, s_hashes, &total);
    const uint64_t heads = sums[2 * groups + blockIdx.x] + vkmr_sizes::block_exclusive(head ? 1u : 0u, s_heads, &total);
    if (!m.in) return;
    const uint32_t b = (uint32_t)(head ? heads : heads - 1ull);   // an entry that is not its tree's first has one in front of it
    flag_at[q] = f;
    hash_at[q] = x;
    block_of[q] = b;
    if (head) {
        bit_start[b] = f;
        block_trees[b] = m.t;
        block_counts[b] = m.c;
        hash_starts[b] = x;
    }
}

// Lane b's block: its flags, 0 for a lane past B.
__device__ __forceinline__ uint64_t merkleblock_bits(const uint64_t* __restrict__ bit_start, uint64_t b, uint64_t B)
{
    return b < B ? bit_start[b + 1] - bit_start[b] : 0ull;
}

__global__ __launch_bounds__(VKMR_MB_THREADS) void merkleblock_byte_sums_kernel(const uint64_t* __restrict__ hdr, const uint64_t* __restrict__ bit_start,
                                                                                uint64_t* __restrict__ bit_counts, uint64_t* __restrict__ byte_sums)
{
    __shared__ uint32_t s_wave[VKMR_MB_THREADS / 64];
    if (hdr[0] != 0ull) return;
    const uint64_t b = (uint64_t)blockIdx.x * VKMR_MB_THREADS + threadIdx.x, B = hdr[1];
    // A block's flags are not bounded by its entries' number, but each flag is a visited node of a stored tree and each byte
    // holds eight: 2^32 flag bytes in one workgroup's 256 blocks would take 2^35 visited nodes, a terabyte of stored cells.  So
    // a block's bytes, and a workgroup's sum of them, fit 32 bits; the sums over workgroups are taken in 64.
    const uint64_t bits = merkleblock_bits(bit_start, b, B);
    if (b < B) bit_counts[b] = bits;
    uint32_t total;
    (void)vkmr_sizes::block_exclusive((uint32_t)((bits + 7ull) >> 3), s_wave, &total);
    if (threadIdx.x == 0) byte_sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(VKMR_MB_THREADS) void merkleblock_byte_starts_kernel(uint64_t* __restrict__ byte_sums, uint64_t groups, uint64_t hash_capacity,
                                                                                  uint64_t flag_capacity, uint64_t* __restrict__ hdr)
{
    __shared__ uint32_t s_wave[VKMR_MB_THREADS / 64];
    if (hdr[0] != 0ull) return;
    const uint64_t bytes = merkleblock_prefix(byte_sums, groups, s_wave);
    if (threadIdx.x == 0) {
        hdr[3] = bytes;
        if (hdr[2] > hash_capacity || bytes > flag_capacity) hdr[0] = 4ull;
    }
}

// Also when bit 2 is set, and only then besides 0: the caller reads the totals and the per-block arrays, allocates, calls again.
__global__ __launch_bounds__(VKMR_MB_THREADS) void merkleblock_byte_places_kernel(const uint64_t* __restrict__ hdr, const uint64_t* __restrict__ bit_start,
                                                                                  const uint64_t* __restrict__ byte_sums, uint64_t* __restrict__ byte_starts)
{
    __shared__ uint32_t s_wave[VKMR_MB_THREADS / 64];
    if ((hdr[0] & 3ull) != 0ull) return;
    const uint64_t b = (uint64_t)blockIdx.x * VKMR_MB_THREADS + threadIdx.x, B = hdr[1];
    const uint64_t bits = merkleblock_bits(bit_start, b, B);
    uint32_t total;
    const uint64_t ex = vkmr_sizes::block_exclusive((uint32_t)((bits + 7ull) >> 3), s_wave, &total);
    if (b < B) byte_starts[b] = byte_sums[blockIdx.x] + ex;      // b < B <= k: a workgroup the sums have
    else if (b == B) byte_starts[b] = hdr[3];                    // the row behind the last block; its workgroup may be one past the sums
}

__global__ __launch_bounds__(256) void merkleblock_zero_kernel(const uint64_t* __restrict__ hdr, uint32_t* __restrict__ flag_words)
{
    if (hdr[0] != 0ull) return;
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w < ((hdr[3] + 3ull) >> 2)) flag_words[w] = 0u;          // status 0: within the capacity, which the grid covers
}

// One lane per (entry, level): blockIdx.y = l < the stride.  The lane copies the right sibling the walk passes at level l on
// its climb from the entry in front, the left sibling it passes at level l on its way down to this entry, and -- behind a
// tree's last entry -- the right sibling at level l on the climb to the root; the lane of l == 0 copies the leaf.  Flags that
// are 0 stay as the zero kernel left them; the path node's 1 is ORed into its 32-bit word, which neighbouring lanes and, where
// trees are small, neighbouring blocks share.  A tree's first entry sets the root's flag, the first bit of its block.
template <class Entries, class Counts, class Cells>
__device__ __forceinline__ void merkleblock_emit(const Entries e, const Counts n, const Cells cells, uint32_t k, const uint64_t* __restrict__ hdr,
                                                 const uint64_t* __restrict__ flag_at, const uint64_t* __restrict__ hash_at,
                                                 const uint32_t* __restrict__ block_of, const uint64_t* __restrict__ bit_start,
                                                 const uint64_t* __restrict__ byte_starts, Node* __restrict__ hashes, uint32_t* __restrict__ flag_words)
{
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= k || hdr[0] != 0ull) return;
    const uint32_t l = blockIdx.y;
    const MerkleblockEntry m = merkleblock_entry(e, n, q, k);
    if (l >= m.h) return;
    const uint32_t b = block_of[q];
    const uint64_t bit0 = 8ull * byte_starts[b] + (flag_at[q] - bit_start[b]);   // the group's first flag among all flag bits
    const uint64_t hash0 = hash_at[q];
    if (m.has_prev && vkmr_mb::climbs(m.a, l, m.g.top))
        vkmr_dev::store_node(hashes + hash0 + vkmr_mb::climb_place(m.a, l), vkmr_dev::load_node(cells.node_cell(m.t, l, (m.a >> l) + 1ull)));
    if (vkmr_mb::descends(m.g, m.i, l))
        vkmr_dev::store_node(hashes + hash0 + vkmr_mb::left_hash(m.g, m.i, l), vkmr_dev::load_node(cells.node_cell(m.t, l, (m.i >> l) - 1ull)));
    if (l == 0u) vkmr_dev::store_node(hashes + hash0 + vkmr_mb::leaf_hash(m.g), vkmr_dev::load_node(cells.node_cell(m.t, 0u, m.i)));
    if (!m.has_next && vkmr_mb::climbs(m.i, l, vkmr_mb::edge_level(m.i, m.c, m.h)))
        vkmr_dev::store_node(hashes + hash0 + m.g.hashes + vkmr_mb::climb_place(m.i, l), vkmr_dev::load_node(cells.node_cell(m.t, l, (m.i >> l) + 1ull)));
    if (l <= m.g.top) {
        const uint64_t bit = bit0 + vkmr_mb::path_flag(m.g, m.i, l);
        atomicOr(flag_words + (bit >> 5), 1u << (bit & 31ull));
    }
    if (l == 0u && !m.has_prev) atomicOr(flag_words + (bit0 >> 5), 1u << (bit0 & 31ull));   // the root's flag, the block's first: level h has no lane
}

// The flag bytes out: whole words where all four bytes are used, the last word byte by byte.  flags_dev is 4-byte aligned.
__global__ __launch_bounds__(256) void merkleblock_flags_kernel(const uint64_t* __restrict__ hdr, const uint32_t* __restrict__ flag_words,
                                                                uint8_t* __restrict__ flags)
{
    if (hdr[0] != 0ull) return;
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, bytes = hdr[3];
    if (4ull * w >= bytes) return;
    const uint32_t v = flag_words[w];
    if (4ull * w + 4ull <= bytes) {
        reinterpret_cast<uint32_t*>(flags)[w] = v;
    } else {
        for (uint64_t j = 4ull * w; j < bytes; ++j) flags[j] = (uint8_t)(v >> (8u * (uint32_t)(j & 3ull)));
    }
}

// ---- the kernels of one tree and of a forest ----------------------------------------------------------------------------------

__global__ __launch_bounds__(VKMR_MB_THREADS) void merkleblock_tree_sums_kernel(const uint64_t* __restrict__ indices, uint64_t count, uint32_t k,
                                                                                uint64_t groups, const uint64_t* __restrict__ hdr, uint64_t* __restrict__ sums)
{
    merkleblock_sums(TreeEntries{indices, 0u}, TreeCounts{count}, k, groups, hdr, sums);
}

__global__ __launch_bounds__(VKMR_MB_THREADS) void merkleblock_forest_sums_kernel(const uint64_t* __restrict__ offsets, const uint32_t* __restrict__ trees,
                                                                                  const uint64_t* __restrict__ indices, uint32_t k, uint64_t groups,
                                                                                  const uint64_t* __restrict__ hdr, uint64_t* __restrict__ sums)
{
    merkleblock_sums(ForestEntries{trees, indices, nullptr}, ForestCounts{offsets}, k, groups, hdr, sums);
}

__global__ __launch_bounds__(VKMR_MB_THREADS) void merkleblock_tree_places_kernel(const uint64_t* __restrict__ indices, uint64_t count, uint32_t k,
                                                                                  uint64_t groups, const uint64_t* __restrict__ hdr,
                                                                                  const uint64_t* __restrict__ sums, uint64_t* __restrict__ flag_at,
                                                                                  uint64_t* __restrict__ hash_at, uint32_t* __restrict__ block_of,
                                                                                  uint64_t* __restrict__ bit_start, uint32_t* __restrict__ block_trees,
                                                                                  uint64_t* __restrict__ block_counts, uint64_t* __restrict__ hash_starts)
{
    merkleblock_places(TreeEntries{indices, 0u}, TreeCounts{count}, k, groups, hdr, sums, flag_at, hash_at, block_of, bit_start, block_trees, block_counts,
                       hash_starts);
}

__global__ __launch_bounds__(VKMR_MB_THREADS) void merkleblock_forest_places_kernel(const uint64_t* __restrict__ offsets, const uint32_t* __restrict__ trees,
                                                                                    const uint64_t* __restrict__ indices, uint32_t k, uint64_t groups,
                                                                                    const uint64_t* __restrict__ hdr, const uint64_t* __restrict__ sums,
                                                                                    uint64_t* __restrict__ flag_at, uint64_t* __restrict__ hash_at,
                                                                                    uint32_t* __restrict__ block_of, uint64_t* __restrict__ bit_start,
                                                                                    uint32_t* __restrict__ block_trees, uint64_t* __restrict__ block_counts,
                                                                                    uint64_t* __restrict__ hash_starts)
{
    merkleblock_places(ForestEntries{trees, indices, nullptr}, ForestCounts{offsets}, k, groups, hdr, sums, flag_at, hash_at, block_of, bit_start, block_trees,
                       block_counts, hash_starts);
}

__global__ __launch_bounds__(256) void merkleblock_tree_emit_kernel(const Node* __restrict__ digests, const Node* __restrict__ tree, TreeLevels lv,
                                                                    uint64_t count, const uint64_t* __restrict__ indices, uint32_t k,
                                                                    const uint64_t* __restrict__ hdr, const uint64_t* __restrict__ flag_at,
                                                                    const uint64_t* __restrict__ hash_at, const uint32_t* __restrict__ block_of,
                                                                    const uint64_t* __restrict__ bit_start, const uint64_t* __restrict__ byte_starts,
                                                                    Node* __restrict__ hashes, uint32_t* __restrict__ flag_words)
{
    merkleblock_emit(TreeEntries{indices, 0u}, TreeCounts{count}, TreeCells{digests, tree, lv, count}, k, hdr, flag_at, hash_at, block_of, bit_start,
                     byte_starts, hashes, flag_words);
}

__global__ __launch_bounds__(256) void merkleblock_forest_emit_kernel(const Node* __restrict__ digests, const Node* __restrict__ forest, ForestLevels lv,
                                                                      const uint64_t* __restrict__ offsets, const uint32_t* __restrict__ trees,
                                                                      const uint64_t* __restrict__ indices, uint32_t k, const uint64_t* __restrict__ hdr,
                                                                      const uint64_t* __restrict__ flag_at, const uint64_t* __restrict__ hash_at,
                                                                      const uint32_t* __restrict__ block_of, const uint64_t* __restrict__ bit_start,
                                                                      const uint64_t* __restrict__ byte_starts, Node* __restrict__ hashes,
                                                                      uint32_t* __restrict__ flag_words)
{
    merkleblock_emit(ForestEntries{trees, indices, nullptr}, ForestCounts{offsets}, ForestCells{digests, forest, lv, offsets}, k, hdr, flag_at, hash_at,
                     block_of, bit_start, byte_starts, hashes, flag_words);
}
