// tree_plan.hpp -- where the levels of one stored tree lie (vkmr_hip_reduce_tree_async) and the sizes of its multiproofs:
// the node bound and the scratch layout, and the scratch layout of the calls that apply one.  Plain integer arithmetic, no HIP
// types: shared by the kernels (entries.hpp takes the constants), the C ABI (vkmr_hip.hip) and the CPU-side replays in
// tests/c/abi_plan_test.cpp and tests/c/apply_plan_test.cpp.
//
// Level 0 is the caller's digests; levels 1..height lie back to back in one buffer, level l (n_l = ceil(count / 2^l) cells)
// starting at cell off[l] = sum of n_j over 1 <= j < l.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "merkle_math.hpp"

#define VKMR_TREE_MAX_LEVELS 64
#define VKMR_MP_HEADER_WORDS (2 + VKMR_TREE_MAX_LEVELS)   // status, M, up to 64 level counts
#define VKMR_MP_BLOCK_WORDS 256                           // ballot words per block of the prefix sum: 16384 entries

namespace vkmr_tree {

constexpr size_t CELL_BYTES = 32;   // one node: sizeof(vkmr_digest)

// Start cell of every level 1..height (<= 63) inside the tree buffer (off[0] = 0, unused; off null: none wanted); returns
// the buffer's cell count.
inline uint64_t levels(uint64_t count, uint32_t height, uint64_t* off)
{
    uint64_t cells = 0;
    if (off) off[0] = 0;
    for (uint32_t l = 1; l <= height && l < VKMR_TREE_MAX_LEVELS; ++l) {
        if (off) off[l] = cells;
        cells += vkmr_math::ceil_shift(count, l);
    }
    return cells;
}

inline uint64_t cells(uint64_t count, uint32_t height) { return levels(count, height, nullptr); }

// The most nodes a multiproof of k leaves holds: at most one per pair of level l, and no more than k a level.
inline uint64_t multiproof_max_nodes(uint64_t count, uint32_t height, uint32_t k)
{
    uint64_t nodes = 0;
    for (uint32_t l = 0; l < height; ++l) {
        const uint64_t pairs = vkmr_math::ceil_shift(count, l + 1);
        nodes += pairs < k ? pairs : k;
    }
    return nodes;
}

// Where the parts of a multiproof's scratch lie, in bytes.  The cells come first (16-byte loads); the gather uses mask,
// word_start and block only.  `height` is one tree's height or a forest's stride.
struct MultiproofLayout {
    uint64_t words, blocks;   // ballot words per level, blocks of VKMR_MP_BLOCK_WORDS words per level
    size_t cell, mask, word_start, block, hdr, end, bytes;
};

inline MultiproofLayout multiproof_layout(uint32_t k, uint32_t height)
{
    MultiproofLayout L;
    L.words = ((uint64_t)k + 63) / 64;
    L.blocks = (L.words + VKMR_MP_BLOCK_WORDS - 1) / VKMR_MP_BLOCK_WORDS;
    size_t at = 0;
    L.cell = at;       at += (size_t)k * CELL_BYTES;
    L.mask = at;       at += (size_t)(L.words * height) * sizeof(uint64_t);
    L.word_start = at; at += (size_t)(L.words * height) * sizeof(uint64_t);
    L.block = at;      at += (size_t)(L.blocks * height) * sizeof(uint64_t);
    L.hdr = at;        at += VKMR_MP_HEADER_WORDS * sizeof(uint64_t);
    L.end = at;        at += (size_t)k * sizeof(uint32_t);
    L.bytes = at;
    return L;
}

// The scratch of an apply call (vkmr_hip_apply_multiproof_async and its forest twin): the verifier's layout whole -- side 0,
// the old leaves, folds in its cells and ends -- and behind it, each part starting on 16 bytes, the cells and ends of side 1
// (the new leaves) and the heights the check derives from the counts.  `levels` is one tree's height or a forest's stride.
struct ApplyLayout {
    MultiproofLayout mp;
    size_t cell1, end1, heights, bytes;
};

inline size_t round_up_16(size_t bytes) { return (bytes + 15u) & ~(size_t)15u; }

inline ApplyLayout apply_layout(uint32_t k, uint32_t levels)
{
    ApplyLayout A;
    A.mp = multiproof_layout(k, levels);
    size_t at = round_up_16(A.mp.bytes);
    A.cell1 = at;   at = round_up_16(at + (size_t)k * CELL_BYTES);
    A.end1 = at;    at = round_up_16(at + (size_t)k * sizeof(uint32_t));
    A.heights = at; at = round_up_16(at + (size_t)k * sizeof(uint32_t));
    A.bytes = at;
    return A;
}

}  // namespace vkmr_tree
