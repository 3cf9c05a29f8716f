// diff_plan.hpp -- the sizes and the steps of a diff of two stored forests or two stored trees of one shape (include/vkmr_hip.h:
// vkmr_hip_forest_diff_async, vkmr_hip_tree_diff_async): one step of one frontier entry, the host-known bound on every step's
// frontier, the grouping of step 0 and the scratch layout.  Plain integer arithmetic, no HIP types: shared by the kernels
// (diff_kernels.hpp), the C ABI (vkmr_hip.hip) and the tests, which read the constants below from this text;
// tests/c/diff_plan_test.cpp runs whole descents through these functions.
//
// The walk.  A and B have the same offsets and counts, so node (t, l, p) lies in the same cell of both.  The frontier is a
// list of (tree, node) entries sorted by (tree, node); all entries of one tree stand at one level, level_at(h_t, step).
//   step 0       the trees whose roots differ, each as node 0 of its level h_t = max(1, ceil(log2 c_t))
//   step s >= 1  an entry at level l >= 1 is replaced by those of its children 2p, 2p + 1 (nodes of level l - 1) that differ,
//                in child order; node 2p + 1 exists only below level_count(c_t, l - 1): the duplicated last node of an odd level
//                is no second child.  An entry at level 0 is a leaf of a tree shorter than the forest and is carried forward.
// Emission keeps order, so the frontier stays sorted and after step H (the forest's stride; the tree's height) it is the answer.
// Two facts the call relies on, both true of forests that their builds have written (status 0, same shape):
//   a differing node has a differing child, so the frontier never shrinks on the way down and is at most n, the number of
//     differing leaves, at every step: a frontier above `capacity` at any step proves n > capacity, and the call stops there;
//   equal nodes are taken to cover equal leaves (anything else is a SHA-256d collision); the counts being the same on both
//     sides, the duplicate-last ambiguity of two trees of different counts under one root does not arise.
//
// Two mask bits per entry (bit 2j: the left child, or the carried leaf; bit 2j + 1: the right child), so one 64-bit mask word
// covers VKMR_DIFF_WORD_ENTRIES entries and the rank of a child among the next frontier is a prefix count of set bits: the
// multiproof's three ranking kernels (tree_kernels.hpp) with one level.
//
// Scratch, in bytes from its start (16-byte aligned), every part rounded up to 16 bytes, W = ceil(capacity / 32):
//   node[0], node[1]   8 * capacity each   the ping-pong frontiers' nodes
//   tree[0], tree[1]   4 * capacity each   their trees (a single tree's diff leaves them unused)
//   mask               8 * W               the mask words of one step
//   word_start         8 * W               set bits before each word
//   block              8 * max(ceil(W / 256), VKMR_DIFF_ROOT_GROUPS)   the sums / starts of blocks of 256 words; in step 0 one
//                                          word per workgroup of the roots' compare
//   hdr                8 * VKMR_DIFF_HEADER_WORDS   [0] status, [1] the frontier's size, [2] the ranking's level count (unused),
//                                          [3] nodes whose children were compared, [4] trees whose roots differ, [5] spare
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "forest_plan.hpp"
#include "tree_plan.hpp"

#define VKMR_DIFF_THREADS 256u            // lanes of every workgroup of the diff
#define VKMR_DIFF_WORD_ENTRIES 32u        // frontier entries per 64-bit mask word: two bits each
#define VKMR_DIFF_RANK_BLOCK_WORDS 256u   // mask words per block of the ranking (tree_plan.hpp: VKMR_MP_BLOCK_WORDS)
#define VKMR_DIFF_ROOT_GROUPS 1024u       // the most workgroups of step 0: each takes a contiguous run of trees
#define VKMR_DIFF_HEADER_WORDS 6u         // uint64 words of the scratch's header

namespace vkmr_diff {

constexpr uint64_t MAX_TOTAL = 1ull << 58;

// The level at which the entries of a tree of height h stand when step `step` >= 1 begins: h, h - 1, .. 1, then 0 for good.
VKMR_FOREST_FN uint32_t level_at(uint32_t h, uint32_t step) { return h >= step ? h - (step - 1u) : 0u; }

// One step of one entry: the children of node p of a level l >= 1.  `left` is the cell of child 2p, counted from the start of
// the buffer that holds level l - 1; child 2p + 1 is the cell behind it and exists only when `has_right`.
struct Step {
    uint64_t left;
    bool has_right;
};

// A forest: tree t with offset o and count c >= 1.  Level l - 1 is the leaves buffer for l == 1, else the buffer of level
// l - 1, child_base() cells into the stored forest.
VKMR_FOREST_FN Step forest_step(uint64_t o, uint64_t c, uint32_t t, uint64_t p, uint32_t l)
{
    Step s;
    s.left = vkmr_forest::pos(o, t, l - 1u) + 2ull * p;
    s.has_right = 2ull * p + 1ull < vkmr_forest::level_count(c, l - 1u);
    return s;
}

inline uint64_t forest_child_base(uint64_t total, uint32_t ntrees, uint32_t l) { return l <= 1u ? 0ull : vkmr_forest::stored_level_base(total, ntrees, l - 1u); }

// One tree of `count` leaves, every entry at the same level l: level l - 1 is the digests buffer for l == 1, else it starts
// tree_child_base() cells into the tree buffer, off[] being vkmr_tree::levels()'s table.
inline uint64_t tree_child_base(const uint64_t* off, uint32_t l) { return l <= 1u ? 0ull : off[l - 1u]; }

VKMR_FOREST_FN Step tree_step(uint64_t count, uint64_t child_base, uint64_t p, uint32_t l)
{
    Step s;
    s.left = child_base + 2ull * p;
    s.has_right = 2ull * p + 1ull < vkmr_math::ceil_shift(count, l - 1u);
    return s;
}

// The most entries the frontier can hold when step `step` >= 1 begins, known on the host: a tree has at most 2^(step - 1)
// nodes that far below its root and never more than its leaves, and the call stops above `capacity`.  The grids are sized
// from it, so the top steps launch a handful of lanes.
inline uint64_t forest_frontier_bound(uint64_t total, uint32_t ntrees, uint32_t capacity, uint32_t step)
{
    uint64_t b = step - 1u >= 32u ? total : (uint64_t)ntrees << (step - 1u);   // ntrees < 2^32: no overflow
    if (b > total) b = total;
    return b < capacity ? b : capacity;
}

inline uint64_t tree_frontier_bound(uint64_t count, uint32_t height, uint32_t capacity, uint32_t step)
{
    const uint64_t b = vkmr_math::ceil_shift(count, height - (step - 1u));     // the nodes of the level the entries stand at
    return b < capacity ? b : capacity;
}

// Step 0: workgroup g compares the roots of trees [g * span, (g + 1) * span).
inline uint32_t root_groups(uint32_t ntrees)
{
    const uint64_t g = ((uint64_t)ntrees + VKMR_DIFF_THREADS - 1u) / VKMR_DIFF_THREADS;
    return (uint32_t)(g < VKMR_DIFF_ROOT_GROUPS ? g : VKMR_DIFF_ROOT_GROUPS);
}

inline uint64_t root_span(uint32_t ntrees)
{
    const uint32_t g = root_groups(ntrees);
    if (g == 0u) return 0ull;
    const uint64_t per = ((uint64_t)ntrees + g - 1u) / g;
    return (per + VKMR_DIFF_THREADS - 1u) / VKMR_DIFF_THREADS * VKMR_DIFF_THREADS;   // whole trips of one tree per lane
}

// Mask words and ranking blocks of a step whose frontier holds at most `entries`.
inline uint64_t mask_words(uint64_t entries) { return (entries + VKMR_DIFF_WORD_ENTRIES - 1u) / VKMR_DIFF_WORD_ENTRIES; }
inline uint64_t rank_blocks(uint64_t words) { return (words + VKMR_DIFF_RANK_BLOCK_WORDS - 1u) / VKMR_DIFF_RANK_BLOCK_WORDS; }

struct Layout {
    uint64_t words, blocks;   // of a full frontier of `capacity` entries
    size_t node[2], tree[2], mask, word_start, block, hdr, bytes;
};

inline size_t up16(size_t n) { return (n + 15u) & ~(size_t)15u; }

inline Layout layout(uint32_t capacity)
{
    Layout L;
    L.words = mask_words(capacity);
    L.blocks = rank_blocks(L.words);
    const uint64_t block_words = L.blocks > VKMR_DIFF_ROOT_GROUPS ? L.blocks : VKMR_DIFF_ROOT_GROUPS;
    size_t at = 0;
    L.node[0] = at;     at += up16((size_t)capacity * 8u);
    L.node[1] = at;     at += up16((size_t)capacity * 8u);
    L.tree[0] = at;     at += up16((size_t)capacity * 4u);
    L.tree[1] = at;     at += up16((size_t)capacity * 4u);
    L.mask = at;        at += up16((size_t)L.words * 8u);
    L.word_start = at;  at += up16((size_t)L.words * 8u);
    L.block = at;       at += up16((size_t)block_words * 8u);
    L.hdr = at;         at += up16((size_t)VKMR_DIFF_HEADER_WORDS * 8u);
    L.bytes = at;
    return L;
}

inline size_t scratch_bytes(uint32_t capacity) { return layout(capacity).bytes; }

}  // namespace vkmr_diff
