// find_kernels.hpp -- where in a tree or forest is this digest?  (include/vkmr_hip.h: vkmr_hip_forest_find_async,
// vkmr_hip_tree_find_async; sizes and scratch layout: find_plan.hpp.)  No hash is computed here.
//
// The answer to query q is the lowest flat position p of level 0 with digests[p] == queries[q].  The k queries go into an
// open-addressed table, and the leaves are streamed past it once:
//   find_insert_kernel   one lane per query: linear probing from word0 & (T - 1) with a 64-bit compare-and-swap.  Equal queries
//                        share one slot: the lane that meets its own digest in a slot records that query as its representative.
//   *_find_scan_kernel   the hot path, bound by memory: every leaf of [lo, hi) is read once (two 16-byte loads), looked up, and
//                        on a full match its position goes into best[q] by a 64-bit unsigned atomic min.
//   *_find_resolve_kernel one lane per query: best[rep[q]] as (tree, index), or the not-found pair.
// The table holds QUERIES only, so the length of a probe walk depends on the caller's own queries and never on the leaves: a
// forest cannot be built that slows a lookup down, short of leaves that equal a query (each costs its lane one compare).
//
// A forest and one tree differ in where level 0 begins and ends and in how a position is reported: the two structs below, in
// entries.hpp's manner -- one body per kernel, and a __global__ kernel is its arguments as the struct and the call.
#pragma once

#include "find_plan.hpp"

// A forest: the leaves are cells [offsets[0], offsets[ntrees]) of digests; cells outside belong to no tree.  The offsets are
// trusted as vkmr_hip_forest_proofs_async trusts them (non-decreasing, ending at or before `total`); the end is held to
// `total` all the same, so no leaf load leaves the buffer.  No tree: an empty range, and no offset is read.
struct FindForest {
    const uint64_t* offsets; uint32_t ntrees; uint64_t total; uint32_t* trees;
    __device__ __forceinline__ uint64_t lo() const { return ntrees ? offsets[0] : 0ull; }
    __device__ __forceinline__ uint64_t hi() const
    {
        if (!ntrees) return 0ull;
        const uint64_t end = offsets[ntrees];
        return end < total ? end : total;
    }
    // lo() <= p < hi(): the tree is the upper bound of p in offsets[0 .. ntrees], minus one; an empty tree has an empty range
    // and is never the answer.
    __device__ __forceinline__ void found(uint64_t q, uint64_t p, uint64_t* __restrict__ indices) const
    {
        uint32_t a = 1u, b = ntrees;                   // the first i in [1, ntrees] with offsets[i] > p: offsets[ntrees] > p
        while (a < b) {
            const uint32_t mid = a + (b - a) / 2u;
            if (offsets[mid] > p) b = mid;
            else a = mid + 1u;
        }
        trees[q] = a - 1u;
        indices[q] = p - offsets[a - 1u];
    }
    __device__ __forceinline__ void missing(uint64_t q, uint64_t* __restrict__ indices) const
    {
        trees[q] = vkmr_find::NO_TREE;
        indices[q] = vkmr_find::NONE;
    }
};

// One tree at cell 0.
struct FindTree {
    uint64_t count;
    __device__ __forceinline__ uint64_t lo() const { return 0ull; }
    __device__ __forceinline__ uint64_t hi() const { return count; }
    __device__ __forceinline__ void found(uint64_t q, uint64_t p, uint64_t* __restrict__ indices) const { indices[q] = p; }
    __device__ __forceinline__ void missing(uint64_t q, uint64_t* __restrict__ indices) const { indices[q] = vkmr_find::NONE; }
};

// (tag << 32) | q.
__device__ __forceinline__ unsigned long long find_slot(uint32_t tag, uint32_t q) { return ((unsigned long long)tag << 32) | q; }

// One lane per query; the scratch was set to 0xFF before.  No lane waits for another: a step either wins an empty slot, or
// finds the slot taken -- for good, a slot is written once -- and then stops on an equal digest or moves on.  The slots are
// read and written with agent-scope atomics: lanes of this launch on different XCDs must see each other's slots, and the L2s
// are not coherent.  queries[] is written by nobody, so its loads are plain.  At most half the slots are ever taken, so the
// walk meets an empty one; it is held to T probes all the same, and a lane that ran out would keep rep[q] = all ones, which
// the resolve reads as not found.
__global__ __launch_bounds__(256) void find_insert_kernel(const Node* __restrict__ queries, uint32_t k, unsigned long long* __restrict__ table,
                                                          uint64_t mask, uint32_t* __restrict__ rep)
{
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= k) return;
    const Node mine = vkmr_dev::load_node(queries + q);
    const unsigned long long want = find_slot(mine.w[1], (uint32_t)q);
    uint64_t slot = mine.w[0] & mask;
    for (uint64_t n = 0; n <= mask; ++n) {
        unsigned long long seen = __hip_atomic_load(table + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (seen == vkmr_find::NONE &&
            __hip_atomic_compare_exchange_strong(table + slot, &seen, want, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
            rep[q] = (uint32_t)q;                      // this query stands in the table
            return;
        }
        // taken, by `seen` (a failed exchange has put the winner there)
        const uint32_t other = (uint32_t)seen;
        if ((uint32_t)(seen >> 32) == mine.w[1] && other < k && vkmr_dev::node_diff(mine, vkmr_dev::load_node(queries + other)) == 0u) {
            rep[q] = other;                            // an equal query is in the table already
            return;
        }
        slot = (slot + 1ull) & mask;
    }
}

// The walk of one leaf at position p, from its first slot (already loaded: `seen`).  Until an empty slot: where the tag
// matches, all eight words are compared with the query; equal queries share one slot, so the first full match ends the walk.
// best[q] only ever falls, so a read that shows it at or below p -- however stale -- makes the atomic needless; the read is
// an agent-scope one (served by L2) so that a hot entry is not pinned at "none" in this CU's L1.  Table and queries were
// written before this launch: plain loads.
__device__ __forceinline__ void find_walk(const Node& leaf, uint64_t p, uint64_t slot, unsigned long long seen, const Node* __restrict__ queries,
                                          const unsigned long long* __restrict__ table, uint64_t mask, unsigned long long* __restrict__ best)
{
    for (uint64_t n = 0; seen != vkmr_find::NONE && n <= mask; ++n) {
        if ((uint32_t)(seen >> 32) == leaf.w[1]) {
            const uint32_t q = (uint32_t)seen;
            if (vkmr_dev::node_diff(leaf, vkmr_dev::load_node(queries + q)) == 0u) {
                if (__hip_atomic_load(best + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > p)
                    (void)__hip_atomic_fetch_min(best + q, (unsigned long long)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // no return value: fire and forget
                return;
            }
        }
        slot = (slot + 1ull) & mask;
        seen = table[slot];
    }
}

// The leaves a lane takes in one trip: cells first + u * 256, u < VKMR_FIND_LEAVES_PER_LANE, so that each load instruction of a
// wavefront reads 2 KiB back to back.  Cells at or past `hi` are not loaded.
struct FindLeaves { Node cell[VKMR_FIND_LEAVES_PER_LANE]; };

__device__ __forceinline__ FindLeaves find_load(const Node* __restrict__ digests, uint64_t first, uint64_t hi)
{
    FindLeaves x;
#pragma unroll
    for (uint32_t u = 0; u < VKMR_FIND_LEAVES_PER_LANE; ++u) {
        const uint64_t p = first + (uint64_t)u * VKMR_FIND_THREADS;
        if (p < hi) x.cell[u] = vkmr_dev::load_node(digests + p);
        else x.cell[u] = Node{{0, 0, 0, 0, 0, 0, 0, 0}};
    }
    return x;
}

// Workgroup b takes tiles b, b + gridDim.x, ... of vkmr_find::tile_leaves() leaves from lo on: at any time the workgroups read
// one contiguous stretch.  The next trip's leaves are requested before this trip's are looked up, so HBM's latency runs beside
// the table's; the first slots of a trip are loaded together before any walk goes on.
template <class Range>
__device__ __forceinline__ void find_scan(const Range r, const Node* __restrict__ digests, const Node* __restrict__ queries,
                                          const unsigned long long* __restrict__ table, uint64_t mask, unsigned long long* __restrict__ best)
{
    const uint64_t lo = r.lo(), hi = r.hi();           // the same two words in every lane
    const uint64_t tile = vkmr_find::tile_leaves();
    const uint64_t stride = (uint64_t)gridDim.x * tile;
    uint64_t start = lo + (uint64_t)blockIdx.x * tile; // the workgroup's tile; lo <= 2^58 and the grid is capped: no overflow
    if (start >= hi) return;                           // uniform: also an empty range
    FindLeaves cur = find_load(digests, start + threadIdx.x, hi);
    for (;;) {
        const uint64_t first = start + threadIdx.x;
        const bool more = hi - start > stride;         // uniform: start + stride < hi
        FindLeaves next;
        if (more) next = find_load(digests, first + stride, hi);
        uint64_t slot[VKMR_FIND_LEAVES_PER_LANE];
        unsigned long long seen[VKMR_FIND_LEAVES_PER_LANE];
#pragma unroll
        for (uint32_t u = 0; u < VKMR_FIND_LEAVES_PER_LANE; ++u) {
            slot[u] = cur.cell[u].w[0] & mask;
            seen[u] = (first + (uint64_t)u * VKMR_FIND_THREADS < hi) ? table[slot[u]] : vkmr_find::NONE;
        }
#pragma unroll
        for (uint32_t u = 0; u < VKMR_FIND_LEAVES_PER_LANE; ++u)
            find_walk(cur.cell[u], first + (uint64_t)u * VKMR_FIND_THREADS, slot[u], seen[u], queries, table, mask, best);
        if (!more) return;
        cur = next;
        start += stride;
    }
}

__global__ __launch_bounds__(VKMR_FIND_THREADS) void forest_find_scan_kernel(const Node* __restrict__ digests, const uint64_t* __restrict__ offsets,
                                                                             uint32_t ntrees, uint64_t total, const Node* __restrict__ queries,
                                                                             const unsigned long long* __restrict__ table, uint64_t mask,
                                                                             unsigned long long* __restrict__ best)
{
    find_scan(FindForest{offsets, ntrees, total, nullptr}, digests, queries, table, mask, best);
}

__global__ __launch_bounds__(VKMR_FIND_THREADS) void tree_find_scan_kernel(const Node* __restrict__ digests, uint64_t count,
                                                                           const Node* __restrict__ queries,
                                                                           const unsigned long long* __restrict__ table, uint64_t mask,
                                                                           unsigned long long* __restrict__ best)
{
    find_scan(FindTree{count}, digests, queries, table, mask, best);
}

// One lane per query: the position its representative collected, reported the range's way.
template <class Range>
__device__ __forceinline__ void find_resolve(const Range r, uint32_t k, const unsigned long long* __restrict__ best, const uint32_t* __restrict__ rep,
                                             uint64_t* __restrict__ indices)
{
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= k) return;
    const uint32_t of = rep[q];
    const uint64_t p = of < k ? best[of] : vkmr_find::NONE;
    if (p == vkmr_find::NONE) r.missing(q, indices);
    else r.found(q, p, indices);
}

__global__ __launch_bounds__(256) void forest_find_resolve_kernel(const uint64_t* __restrict__ offsets, uint32_t ntrees, uint64_t total, uint32_t k,
                                                                  const unsigned long long* __restrict__ best, const uint32_t* __restrict__ rep,
                                                                  uint32_t* __restrict__ trees, uint64_t* __restrict__ indices)
{
    find_resolve(FindForest{offsets, ntrees, total, trees}, k, best, rep, indices);
}

__global__ __launch_bounds__(256) void tree_find_resolve_kernel(uint64_t count, uint32_t k, const unsigned long long* __restrict__ best,
                                                                const uint32_t* __restrict__ rep, uint64_t* __restrict__ indices)
{
    find_resolve(FindTree{count}, k, best, rep, indices);
}
