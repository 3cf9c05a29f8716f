// audit_plan.hpp -- the sizes of an audit of a stored forest or a stored tree (include/vkmr_hip.h: vkmr_hip_forest_audit_async,
// vkmr_hip_tree_audit_async): which nodes a structure holds, where the ballot word of a wavefront of cells lies, and the scratch
// layout.  Plain integer arithmetic, no HIP types: shared by the kernels (audit_kernels.hpp), the C ABI (vkmr_hip.hip), the CPU
// counterparts (host/host_api.cpp) and tests/c/audit_plan_test.cpp, which replays every launch's writes against the layout.
//
// The rule.  Node (t, l, j), 1 <= l <= h_t, is BAD when its stored cell differs from hash_pair of the two cells
// of level l - 1 beneath it as they are stored now; an empty tree's one checkable node (t, 1, 0) is bad when roots[t] is not all
// zero.  One lane per cell of a level's buffer, the build's grid; a wavefront of 64 cells leaves one 64-bit ballot word.
//
// The list.  The ballot words of levels 1 .. H lie back to back, level l's ceil(cells_l / 64) words behind those of the levels
// below it, so the rank of a bad node in (level, tree, node) order is the count of set bits in front of it: the multiproof's
// three ranking kernels (tree_kernels.hpp) over all the words as one level.
//
// Scratch (capacity > 0), in bytes from its start (16-byte aligned), every part rounded up to 16 bytes, W = words_bound():
//   mask        8 * W                 the ballot words
//   word_start  8 * W                 set bits before each word
//   block       8 * ceil(W / 256)     the sums / starts of blocks of 256 words
//   hdr         8 * VKMR_AUDIT_HEADER_WORDS   the ranking's header: [0] its status (stays 0), [1] the set bits, [2] the same
//                                     (the ranking's one level), [3] spare
// W is sized for every height the two calls accept (63 levels), from (total, ntrees) alone; a call uses the first words_used.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "forest_plan.hpp"
#include "tree_plan.hpp"

#define VKMR_AUDIT_THREADS 256u            // lanes of every workgroup of the audit
#define VKMR_AUDIT_RANK_BLOCK_WORDS 256u   // ballot words per block of the ranking (tree_plan.hpp: VKMR_MP_BLOCK_WORDS)
#define VKMR_AUDIT_HEADER_WORDS 4u         // uint64 words of the scratch's header
#define VKMR_AUDIT_MAX_LEVELS 63u          // the most levels a call walks: a tree's height is at most 63, a forest's stride 58

namespace vkmr_audit {

constexpr uint64_t MAX_LIST_CELLS = 0xFFFFFFFFull;   // a level of more cells is not ranked: the list form refuses it

// Ballot words of a level of `cells` lanes.
VKMR_FOREST_FN uint64_t words_of(uint64_t cells) { return (cells + 63u) / 64u; }

// Lanes of level l >= 1: the cells of the forest's level buffer, the nodes of the tree's level.
VKMR_FOREST_FN uint64_t forest_level_cells(uint64_t total, uint32_t ntrees, uint32_t l) { return vkmr_forest::level_cells(total, ntrees, l); }
VKMR_FOREST_FN uint64_t tree_level_cells(uint64_t count, uint32_t l) { return vkmr_math::ceil_shift(count, l); }

// First ballot word of level l >= 1: the words of levels 1 .. l - 1.  word_base(.., H + 1) is what a call of H levels uses.
inline uint64_t forest_word_base(uint64_t total, uint32_t ntrees, uint32_t l)
{
    uint64_t words = 0;
    for (uint32_t j = 1; j < l; ++j) words += words_of(forest_level_cells(total, ntrees, j));
    return words;
}

inline uint64_t tree_word_base(uint64_t count, uint32_t l)
{
    uint64_t words = 0;
    for (uint32_t j = 1; j < l; ++j) words += words_of(tree_level_cells(count, j));
    return words;
}

// What the scratch is sized for: a forest of `ntrees` trees (a tree: ntrees = 1, total = count) walked through 63 levels.  A
// tree's level holds at most (count >> l) + 1 nodes, the cells of a forest of one tree, so one bound serves both; monotone
// in both arguments.
inline uint64_t words_bound(uint64_t total, uint32_t ntrees) { return forest_word_base(total, ntrees, VKMR_AUDIT_MAX_LEVELS + 1u); }

// The nodes an audit checks, known on the host from the counts: every node of levels 1 .. h of a tree of c >= 1 leaves, the one
// root cell of an empty tree; a single tree walked to `height` also has its lone-node levels above ceil(log2 count).
inline uint64_t forest_tree_nodes(uint64_t c)
{
    if (c == 0) return 1;
    uint64_t nodes = 0;
    for (uint32_t l = 1, h = vkmr_math::height(c); l <= h; ++l) nodes += vkmr_forest::level_count(c, l);
    return nodes;
}

inline uint64_t tree_nodes(uint64_t count, uint32_t height) { return vkmr_tree::cells(count, height); }

struct Layout {
    uint64_t words, blocks;   // ballot words the scratch holds, blocks of VKMR_AUDIT_RANK_BLOCK_WORDS of them
    size_t mask, word_start, block, hdr, bytes;
};

inline size_t up16(size_t n) { return (n + 15u) & ~(size_t)15u; }
inline uint64_t rank_blocks(uint64_t words) { return (words + VKMR_AUDIT_RANK_BLOCK_WORDS - 1u) / VKMR_AUDIT_RANK_BLOCK_WORDS; }

inline Layout layout(uint64_t total, uint32_t ntrees, uint32_t capacity)
{
    Layout L;
    L.words = (capacity == 0 || ntrees == 0) ? 0 : words_bound(total, ntrees);
    L.blocks = rank_blocks(L.words);
    size_t at = 0;
    L.mask = at;        at += up16((size_t)L.words * 8u);
    L.word_start = at;  at += up16((size_t)L.words * 8u);
    L.block = at;       at += up16((size_t)L.blocks * 8u);
    L.hdr = at;         at += L.words ? up16((size_t)VKMR_AUDIT_HEADER_WORDS * 8u) : 0u;
    L.bytes = at;
    return L;
}

inline size_t scratch_bytes(uint64_t total, uint32_t ntrees, uint32_t capacity) { return layout(total, ntrees, capacity).bytes; }

}  // namespace vkmr_audit
