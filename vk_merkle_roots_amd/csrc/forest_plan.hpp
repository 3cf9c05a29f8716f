// forest_plan.hpp -- where the nodes of a forest lie, level by level, and the scratch budget of its reduction
// (vkmr_hip_reduce_forest_async).  Plain integer arithmetic, no HIP types: shared by the kernels (forest_kernels.hpp), the
// C ABI (vkmr_hip.hip) and the CPU-side sweep in tests/c/forest_plan_test.cpp, which checks that no two trees' cells
// overlap and that no launch writes past what vkmr_hip_forest_scratch_bytes() promises.
//
// A forest is `ntrees` trees whose leaves lie back to back: tree t is cells [offsets[t], offsets[t+1]) of the leaves,
// c_t of them.  Level 0 is the caller's buffer.  Level l >= 1 of tree t (ceil(c_t / 2^l) nodes) starts at cell
//     pos_l(t) = (offsets[t] >> l) + t
// of that level's buffer.  No prefix sum is needed to find it, and consecutive trees never overlap:
//     pos_l(t+1) - pos_l(t) = ((offsets[t] + c_t) >> l) - (offsets[t] >> l) + 1 >= (c_t >> l) + 1 >= ceil(c_t / 2^l).
// pos_l is strictly increasing in t, so the tree a cell belongs to is found by binary search over the offsets alone.
// The last tree ends at or before (offsets[ntrees] >> l) + 1 + (ntrees - 1) <= (total >> l) + ntrees: the cells of level l.
#pragma once
#include <stdint.h>

#include "merkle_math.hpp"
#define VKMR_FOREST_FN VKMR_MATH_FN

namespace vkmr_forest {

// Levels of the tree over c >= 1 leaves, and the nodes of its level l (0 for an empty tree): merkle_math.hpp.
using vkmr_math::height;
VKMR_FOREST_FN uint64_t level_count(uint64_t c, uint32_t l) { return c == 0 ? 0 : ((c - 1) >> l) + 1; }

// First cell of tree t's level l: in the caller's leaves for l == 0, in the level's own buffer otherwise.
VKMR_FOREST_FN uint64_t pos(uint64_t offset, uint32_t t, uint32_t l) { return l == 0 ? offset : (offset >> l) + t; }

// Cells of the buffer of level l >= 1 (one lane per cell in the launch that forms it).
VKMR_FOREST_FN uint64_t level_cells(uint64_t total, uint32_t ntrees, uint32_t l) { return (l >= 64 ? 0 : total >> l) + ntrees; }

// Launches: one per level up to the height of the largest tree the caller allows (max_count above total counts as total).
inline uint32_t launches(uint64_t total, uint64_t max_count)
{
    const uint64_t m = max_count < total ? max_count : total;
    return m <= 1 ? 1u : height(m);
}

// Two ping-pong buffers: odd levels in A = [0, level_cells(1)), even levels in B behind it (every later level is no
// larger than the one two below it).  A tree's last level goes to roots_dev, not to scratch, so the last launch writes none.
inline uint64_t level_base(uint64_t total, uint32_t ntrees, uint32_t l) { return (l & 1u) ? 0 : level_cells(total, ntrees, 1); }

// The scratch budget in cells: (total >> 1) + (total >> 2) + 2 * ntrees, and nothing for no tree.  Monotone in both.
inline uint64_t scratch_cells(uint64_t total, uint32_t ntrees)
{
    return ntrees == 0 ? 0 : level_cells(total, ntrees, 1) + level_cells(total, ntrees, 2);
}

// ---- stored forest (vkmr_hip_reduce_forest_tree_async): the same positions, one buffer per level instead of two that
// alternate.  Level l >= 1 keeps its level_cells(l) cells behind those of levels 1 .. l - 1; level 0 stays the caller's
// leaves.  `levels` = launches(total, max_count) is also the stride of a forest's proofs.

// First cell of level l's buffer inside the stored forest: the cells of levels 1 .. l - 1.
inline uint64_t stored_level_base(uint64_t total, uint32_t ntrees, uint32_t l)
{
    uint64_t cells = 0;
    for (uint32_t j = 1; j < l; ++j) cells += level_cells(total, ntrees, j);
    return cells;
}

// Cells of the stored forest: levels 1 .. `levels`.
inline uint64_t stored_cells(uint64_t total, uint32_t ntrees, uint32_t levels) { return stored_level_base(total, ntrees, levels + 1); }

// The most nodes a multiproof of k leaves of the forest holds (vkmr_hip_forest_multiproof_async): at most one per parent of
// a live tree -- the cells of level l + 1 -- and no more than k a level.
inline uint64_t multiproof_max_nodes(uint64_t total, uint32_t ntrees, uint64_t max_count, uint32_t k)
{
    const uint32_t levels = launches(total, max_count);
    uint64_t nodes = 0;
    for (uint32_t l = 0; l < levels; ++l) {
        const uint64_t parents = level_cells(total, ntrees, l + 1);
        nodes += parents < k ? parents : k;
    }
    return nodes;
}

// ---- leaf updates of a stored forest (vkmr_hip_forest_update_async): one step of one entry.  Entry (tree t with offset o
// and count c, leaf index i < c) at level l >= 1 rehashes parent p = i >> l of tree t's level l from the n_in cells of its
// level l - 1.  forest_update_level_kernel and the CPU replay in tests/c/forest_update_plan_test.cpp both run this text.
struct UpdateStep {
    bool active;        // tree t takes part in level l: l == 1, or its level l - 1 still had two nodes (forest_level_kernel's rule)
    bool root;          // level l of tree t is one node: it goes to roots[t], not to level l's buffer
    uint64_t p;         // the parent, a node of tree t's level l
    uint64_t in_first;  // first cell of tree t's level l - 1: in the leaves for l == 1, else in level l - 1's buffer
    uint64_t n_in;      // cells of tree t's level l - 1
    uint64_t out;       // the parent's cell in level l's buffer (unused when root)
};

VKMR_FOREST_FN UpdateStep update_step(uint64_t o, uint64_t c, uint32_t t, uint64_t i, uint32_t l)
{
    UpdateStep s;
    s.n_in = level_count(c, l - 1u);
    s.active = c != 0ull && (l == 1u || s.n_in >= 2ull);
    s.root = level_count(c, l) == 1ull;
    s.p = i >> l;
    s.in_first = pos(o, t, l - 1u);
    s.out = pos(o, t, l) + s.p;
    return s;
}

// Entries sorted by (tree, index) put equal parents side by side: entry q is the head of its run at level l, and alone
// hashes the parent, when the entry in front of it (t0, i0) names another node.
VKMR_FOREST_FN bool update_same_node(uint32_t t0, uint64_t i0, uint32_t t, uint64_t i, uint32_t l) { return t0 == t && (i0 >> l) == (i >> l); }

// ---- appending trees to a stored forest (vkmr_hip_forest_append_async): trees first_tree .. first_tree + m - 1, until now
// empty at offset `used`, take the n leaves behind `used`.  pos_l(t) depends on tree t's own offset and number alone, so
// nothing in front moves, and the cells of the new trees at level l are one range of that level's buffer:
//     [append_first_cell(used, first_tree, l), append_end_cell(used + n, first_tree + m, l))
// from the first cell of the first new tree to the first cell of the tree behind the last new one (which may not exist:
// the cell is inside level_cells all the same, see the head of this file).  Level 0's range is the new leaves themselves.
// The ABI sizes its launches by it, forest_append_level_kernel starts its wavefronts at the first cell and searches among
// trees 0 .. first_tree + m - 1 only, and tests/c/forest_append_plan_test.cpp replays both on the CPU.
VKMR_FOREST_FN uint64_t append_first_cell(uint64_t used, uint32_t first_tree, uint32_t l) { return pos(used, first_tree, l); }
VKMR_FOREST_FN uint64_t append_end_cell(uint64_t used_after, uint32_t end_tree, uint32_t l) { return pos(used_after, end_tree, l); }

// ---- growing or shrinking the open tree by leaves (vkmr_hip_forest_extend_async, vkmr_hip_forest_shrink_async): tree t, the
// last tree in use (every tree behind it empty), at offset o goes from c to c2 leaves at its right edge.  pos_l(o, t) does not
// move, so node j of its level l stays in its cell, and the nodes whose value changes are those from min(c, c2) >> l on: the
// launch of level l >= 1 covers nodes [extend_first_node(c, c2, l), extend_end_node(c2, l)) of tree t, the cells
//     [extend_first_cell(o, t, c, c2, l), extend_end_cell(o, t, c2, l))
// of level l's buffer.  THE LONE NODE.  The build writes a tree's last level to roots[t] only, never to its cell.  So where the
// old tree had one node at level l (c a power of two grows past it: 2 -> 3) that node's cell has never been stored and must be
// formed now; and where the new tree has one node at level l (c shrinks to a power of two: 3 -> 2) that node is an inner
// cell nothing touched, and must reach roots[t].  Both are node 0, so the range starts at 0 wherever either count leaves one
// node: the body needs no word of it, it takes the first cell.  The range is empty (first == end == 0) where the new tree
// takes no part in level l: l > 1 and its level l - 1 had one node, the body's own "tree is done" test.  A tree shrunk to no
// leaf gets one lane at level 1, its reserved cell's, which writes the zero root as in the build.  The ABI sizes its launches
// by these, forest_extend_level_kernel starts at the first cell and tests/c/forest_extend_plan_test.cpp replays both.
VKMR_FOREST_FN uint64_t extend_end_node(uint64_t c2, uint32_t l)
{
    if (c2 == 0) return l == 1u ? 1 : 0;
    return (l > 1u && level_count(c2, l - 1u) == 1) ? 0 : level_count(c2, l);
}
VKMR_FOREST_FN uint64_t extend_first_node(uint64_t c, uint64_t c2, uint32_t l)
{
    if (extend_end_node(c2, l) == 0) return 0;
    if (level_count(c, l) <= 1 || level_count(c2, l) <= 1) return 0;
    return (c < c2 ? c : c2) >> l;
}
VKMR_FOREST_FN uint64_t extend_first_cell(uint64_t o, uint32_t t, uint64_t c, uint64_t c2, uint32_t l) { return pos(o, t, l) + extend_first_node(c, c2, l); }
VKMR_FOREST_FN uint64_t extend_end_cell(uint64_t o, uint32_t t, uint64_t c2, uint32_t l) { return pos(o, t, l) + extend_end_node(c2, l); }

// ---- dropping the oldest trees (vkmr_hip_forest_drop_front_async): after dropping k trees, offsets[t] = offsets[k] for every
// t < k.  Trees 0 .. k - 1 are then empty trees at the offset where tree k begins, and nothing else changes:
//   - pos_l stays strictly increasing: for t + 1 < k, pos_l(t + 1) - pos_l(t) = (offsets[k] >> l) - (offsets[k] >> l) + 1 = 1; for
//     t + 1 == k it is 1 as well, tree k keeping its offset; from tree k on both terms are the old ones.
//   - no cell of a tree >= k moves: pos_l(t) is a function of offsets[t] and t alone, and neither changes for t >= k.
// The cells in front of offsets[k] belong to no tree afterwards and cannot be used again in place (offsets are monotone):
// copying the trees that remain into another forest (below) is what reclaims them.
VKMR_FOREST_FN uint64_t drop_front_offset(uint64_t offset_t, uint64_t offset_k, uint32_t t, uint32_t k) { return t < k ? offset_k : offset_t; }

// ---- copying stored trees into another forest (vkmr_hip_forest_copy_trees_async): one step of one lane.  Destination tree u
// (offset o_d, count c) is source tree ts (offset o_s, the same count); lane j of tree u's level l >= 0 moves one node, and hashes
// nothing: a stored tree at another offset, under another number or in another forest has the same nodes, only their cells
// differ, and differently per level, because (offset >> l) does not commute with a shift of the offset.  The source cell of a
// lane is its destination cell plus a constant of (tree, level), so both sides are contiguous inside a tree.
// THE PROPERTY: over l = 0 .. H_d and every lane of append's range of level l, the cells (leaves, level cells, roots) written are
// exactly those a fresh vkmr_hip_reduce_forest_tree_async over the destination offsets writes for trees first_tree ..
// first_tree + m - 1: the tests below are the build's own (forest_level), with "hash the two children" replaced by "copy".
// forest_copy_level_kernel and the CPU replay in tests/c/forest_copy_plan_test.cpp both run this text.
enum CopyKind : uint32_t {
    COPY_NOTHING = 0,   // padding behind the tree's nodes, or the tree was done a level below (the build's "tree is done" test)
    COPY_ZERO_ROOT,     // an empty tree: its reserved cell's lane at level 1 writes the all-zero root, once
    COPY_ROOT,          // level l is the tree's last: dst_roots[u] = src_roots[ts] (and the mask); no cell, as in the build
    COPY_CELL,          // cell src of the source's level l to cell dst of the destination's level l
    COPY_LEAF           // l == 0: cell src of the source's leaves to cell dst of the destination's
};
struct CopyStep {
    CopyKind kind;
    uint64_t src, dst;  // cells of level l's buffers (of the leaves for l == 0); unused for the roots
};

VKMR_FOREST_FN CopyStep copy_step(uint64_t o_d, uint32_t u, uint64_t c, uint64_t o_s, uint32_t ts, uint32_t l, uint64_t j)
{
    CopyStep s;
    s.kind = COPY_NOTHING;
    s.src = pos(o_s, ts, l) + j;
    s.dst = pos(o_d, u, l) + j;
    if (l == 0u) {
        if (j < c) s.kind = COPY_LEAF;
        return s;
    }
    if (c == 0ull) {
        if (l == 1u && j == 0ull) s.kind = COPY_ZERO_ROOT;
        return s;
    }
    const uint64_t n_out = level_count(c, l);
    if ((l > 1u && level_count(c, l - 1u) == 1ull) || j >= n_out) return s;
    s.kind = n_out == 1ull ? COPY_ROOT : COPY_CELL;
    return s;
}

// The tree of cell p of level l among trees 0 .. ntrees - 1 (ntrees >= 1): the last whose first cell is at or before p, 0 when
// there is none.  For l >= 1 pos_l is strictly increasing and this is forest_find_tree's answer.  At l == 0 the first cells are
// the offsets themselves, which only do not decrease -- empty trees share theirs with the tree behind them -- and the last tree
// at or before p is still the one that holds leaf p; forest_copy_level_kernel searches level 0 this way in every lane.
VKMR_FOREST_FN uint32_t copy_find_tree(const uint64_t* offsets, uint32_t ntrees, uint32_t l, uint64_t p, uint32_t t = 0)
{
    uint32_t top = ntrees - 1u;
    while (t < top) {
        const uint32_t mid = t + (top - t + 1u) / 2u;
        if (pos(offsets[mid], mid, l) <= p) t = mid;
        else top = mid - 1u;
    }
    return t;
}

}  // namespace vkmr_forest
