// find_plan.hpp -- the sizes of a lookup by digest (include/vkmr_hip.h: vkmr_hip_forest_find_async, vkmr_hip_tree_find_async):
// the scratch layout and the launch constants of the scan.  Plain integer arithmetic, no HIP types: shared by the kernels
// (find_kernels.hpp), the C ABI (vkmr_hip.hip) and the tests, which read the constants below from this text.
//
// Scratch, in bytes from its start (8-byte aligned):
//   [0, 8 T)                 the table: T slots of 8 bytes, T the smallest power of two >= max(64, 2 k), so at most half are taken
//   [8 T, 8 T + 8 k)         best[q]: the lowest flat position at which query q's digest was seen
//   [8 T + 8 k, .. + 4 k)    rep[q]: the query that stands in the table for every query equal to q (q itself when it won a slot)
// A slot is (tag << 32) | q with tag = word 1 of query q's digest; word 0 picks the slot.  Empty is all ones, and so is "no
// position" in best[]: one memset of 0xFF over the whole scratch resets all three.  q < k <= 2^32 - 1, so no slot in use is
// all ones, whatever the tag.
#pragma once
#include <stdint.h>

#define VKMR_FIND_MIN_SLOTS 64u        // the smallest table
#define VKMR_FIND_THREADS 256u         // lanes of a scan workgroup
#define VKMR_FIND_LEAVES_PER_LANE 2u   // leaves a lane holds per trip (and as many more in flight for the next trip)
#define VKMR_FIND_GROUPS_PER_CU 8u     // the scan's grid is capped at this many workgroups per compute unit: 8 wavefronts per SIMD

namespace vkmr_find {

constexpr uint64_t NONE = ~0ull;       // an empty slot, and "no position"
constexpr uint32_t NO_TREE = ~0u;      // trees[q] of a query that was not found

// Leaves one workgroup takes per trip of its grid-stride loop.
constexpr uint64_t tile_leaves() { return (uint64_t)VKMR_FIND_THREADS * VKMR_FIND_LEAVES_PER_LANE; }

// T: the smallest power of two >= max(64, 2 k); at most 2^33.
inline uint64_t table_slots(uint32_t k)
{
    uint64_t t = VKMR_FIND_MIN_SLOTS;
    while (t < 2ull * k) t <<= 1;
    return t;
}

inline uint64_t best_offset(uint32_t k) { return 8ull * table_slots(k); }
inline uint64_t rep_offset(uint32_t k) { return best_offset(k) + 8ull * k; }
inline uint64_t scratch_bytes(uint32_t k) { return (rep_offset(k) + 4ull * k + 15ull) & ~15ull; }

// Workgroups of the scan over `leaves` cells on a device of `cus` compute units: one per tile, capped.
inline uint64_t scan_groups(uint64_t leaves, uint32_t cus)
{
    const uint64_t tiles = (leaves + tile_leaves() - 1) / tile_leaves();
    const uint64_t cap = (uint64_t)(cus ? cus : 1u) * VKMR_FIND_GROUPS_PER_CU;
    return tiles < cap ? tiles : cap;
}

}  // namespace vkmr_find
