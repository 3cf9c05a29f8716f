// consistency_plan.hpp -- "the tree of c2 leaves extends the tree of c leaves", proved to a holder of the two roots alone
// (vkmr_hip_forest_consistency_async, vkmr_hip_verify_consistency_async): which cells a proof holds, where a stored forest
// keeps them, which of them the check reads and what each step of its walk hashes.  Plain integer arithmetic, no HIP types:
// shared by the kernels (consistency_kernels.hpp), the C ABI (vkmr_hip.hip), the CPU twins (host/host_api.cpp) and the replay
// in tests/c/consistency_plan_test.cpp.  Notation: frontier_plan.hpp's (H = height, level_count, P_l the peak of a set bit l).
//
// THE PROOF for c >= 1, l0 = ctz(c), is two rows of `stride` cells:
//   peaks    cell l = P_l of the OLD count c for every set bit l of c: node (c >> l) - 1 of level l, read from the NEW tree (a
//            complete node never changes).  Exactly a frontier of count c.
//   rights   for l0 <= l < H(c2) the new-root walk stands on node j = walk_node(c, l) of level l: (c >> l0) - 1 for l == l0,
//            c >> l above.  Where l == l0 or bit l of c is clear, j is a left child and cell l holds node j + 1 of the new
//            tree's level l when there is one (j + 1 < level_count(c2, l)); where bit l of c is set and l > l0, j is odd and its
//            left sibling is P_l, so no cell is needed.
// Every other cell of both rows is zero and is never read.
//
// THE CHECK, one lane a query, steps(c, c2) = H(c) + H(c2) - l0 steps through ONE node hash (step()):
//   steps 0 .. H(c) - 1        the root walk of the frontier (c, peaks), frontier_plan.hpp's rule; its root (P_H(c) where no step
//                              hashed: c a power of two, at least 2) must be the old root
//   steps H(c) .. the end      level l = l0 + (step - H(c)): acc starts as P_l0; a left child takes rights[l], or itself where
//                              the level ends with it; a right child goes behind P_l.  acc must be the new root
// c == c2 runs through the same rule.  c == 0: ok exactly when the old root is all zero, nothing else is read.  ok = 0 without
// reading a cell (checkable()): c > c2, c2 > 2^58, c2 of more bits than stride.
#pragma once
#include <stdint.h>

#include "frontier_plan.hpp"
#define VKMR_CONSISTENCY_FN VKMR_MATH_FN

// status_dev of vkmr_hip_forest_consistency_async
#define VKMR_CONSISTENCY_BAD_TREE 1u       // a tree index >= ntrees
#define VKMR_CONSISTENCY_OLD_ABOVE 2u      // an old count above the tree's count
#define VKMR_CONSISTENCY_OVER_STRIDE 4u    // a current count of more bits than a row has cells

namespace vkmr_consistency {

using vkmr_frontier::bit_length;
using vkmr_frontier::has_peak;
using vkmr_frontier::height;
using vkmr_frontier::level_count;
using vkmr_frontier::max_count;

// What the check kernel (and the CPU twin) refuses for one query (tree, c) of a forest of ntrees trees whose offsets are
// `offsets`; a tree's count is read only when the index is one.
VKMR_CONSISTENCY_FN uint32_t refusal(uint32_t tree, uint32_t ntrees, const uint64_t* offsets, uint64_t c, uint32_t stride)
{
    if (tree >= ntrees) return VKMR_CONSISTENCY_BAD_TREE;
    const uint64_t c2 = offsets[tree + 1u] - offsets[tree];
    return (c > c2 ? VKMR_CONSISTENCY_OLD_ABOVE : 0u) | (bit_length(c2) > stride ? VKMR_CONSISTENCY_OVER_STRIDE : 0u);
}

// What the verifier answers 0 for without reading a cell.
VKMR_CONSISTENCY_FN bool checkable(uint64_t c, uint64_t c2, uint32_t stride) { return c <= c2 && c2 <= max_count() && bit_length(c2) <= stride; }

VKMR_CONSISTENCY_FN uint32_t low_level(uint64_t c) { return (uint32_t)__builtin_ctzll(c); }                    // l0; c >= 1
// The node of level l >= l0 the new-root walk stands on.
VKMR_CONSISTENCY_FN uint64_t walk_node(uint64_t c, uint32_t l) { return l == low_level(c) ? (c >> l) - 1ull : c >> l; }
VKMR_CONSISTENCY_FN bool walk_is_left(uint64_t c, uint32_t l) { return l == low_level(c) || !has_peak(c, l); }

// The cells a proof holds (all others are zero): of the rights row, and -- has_peak(c, l) -- of the peaks row.  c >= 1.
VKMR_CONSISTENCY_FN bool has_right(uint64_t c, uint64_t c2, uint32_t l)
{
    return l < 64u && l >= low_level(c) && l < height(c2) && walk_is_left(c, l) && walk_node(c, l) + 1ull < level_count(c2, l);
}
// The node of the new tree's level l each holds; frontier_plan.hpp's node_source(c2, l) and node_cell say where it is stored.
VKMR_CONSISTENCY_FN uint64_t peak_node(uint64_t c, uint32_t l) { return (c >> l) - 1ull; }
VKMR_CONSISTENCY_FN uint64_t right_node(uint64_t c, uint32_t l) { return walk_node(c, l) + 1ull; }

// The walk.  H(c2) >= l0: c2 >= c >= 2^l0.
VKMR_CONSISTENCY_FN uint32_t steps(uint64_t c, uint64_t c2) { return height(c) + height(c2) - low_level(c); }

struct Step {
    uint32_t l;     // the level whose cell the step may read
    bool hash;      // the step hashes (an old-root step below the first set bit does not)
    bool peak;      // the left operand is peaks[l]; else acc
    bool right;     // the right operand is rights[l]; else acc, or the left operand again where the walk has no acc yet
};

// Step i < steps(c, c2) of a checkable query with c >= 1; `have`: an earlier old-root step has hashed (true in the new-root walk).
VKMR_CONSISTENCY_FN Step step(uint64_t c, uint64_t c2, uint32_t i, bool have)
{
    Step s = {};
    const uint32_t H1 = height(c);
    if (i < H1) {
        s.l = i;
        s.peak = has_peak(c, i);
        s.hash = s.peak || have;
        return s;
    }
    s.l = low_level(c) + (i - H1);
    s.hash = true;
    s.peak = !walk_is_left(c, s.l);
    s.right = !s.peak && walk_node(c, s.l) + 1ull < level_count(c2, s.l);
    return s;
}

}  // namespace vkmr_consistency
