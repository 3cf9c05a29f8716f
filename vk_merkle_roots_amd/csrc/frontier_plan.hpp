// frontier_plan.hpp -- a duplicate-last tree followed by its frontier alone (vkmr_hip_frontier_extend_async and its
// neighbours): which nodes an extension forms, where they lie in scratch, which old peak they read, which of them become
// the new peaks, and what is refused.  Plain integer arithmetic, no HIP types: shared by the kernels (frontier_kernels.hpp),
// the C ABI (vkmr_hip.hip), the CPU twins (host/host_api.cpp) and the replay in tests/c/frontier_plan_test.cpp.
//
// THE FRONTIER of a tree of c leaves is c and one PEAK per set bit l of c: P_l = node (c >> l) - 1 of level l, the root of a
// complete subtree of 2^l leaves that no later leaf changes.  A frontier is `stride` cells per tree, cell l for bit l; the
// cell of a clear bit is never read and is written as zero.  c == 0 is the tree not yet begun.
//
// ROOT FROM A FRONTIER.  c == 0: all zero.  Else with `carry` absent, for l = 0 .. H(c) - 1, H = merkle_math.hpp's height:
//     bit l of c set:            carry = hash_pair(P_l, carry if present else P_l)
//     else if carry is present:  carry = hash_pair(carry, carry)
// and the root is carry, or P_H(c) when there is none (c a power of two, at least 2).
//
// EXTENDING tree q from c to c2 = c + n leaves.  Level 0's nodes [c, c2) are the new leaves where they lie.  The launch of
// level l, 1 <= l <= H(c2), forms nodes [first_node(c, l), end_node(c2, l)) = [c >> l, ceil(c2 / 2^l)): at most (n >> l) + 2.
// Node j is hash_pair(child 2j, child right_child(j, ceil(c2 / 2^(l-1)))) of level l - 1.  A child at or above c >> (l - 1) is
// one the launch before formed (a new leaf for l == 1); the only other child that occurs is (c >> (l - 1)) - 1, as the left
// child of the first node and only when bit l - 1 of c is set: the old peak P_(l-1) (old_peak_child).  n == 0 runs through the
// same rule -- it forms the carry of the root walk, one node a level -- with one case apart: c a power of two, at least 2,
// forms no node at all and its root is P_H(c) (root_is_old_peak), which the commit copies.
// The new peak of a set bit l of c2 is the old P_l where c2 >> l == c >> l, else node (c2 >> l) - 1 of this call's level l
// (the last new leaf for l == 0), always inside the formed range (forms_peak).  The root is node 0 of level H(c2).
//
// SCRATCH.  Node j of tree q's level l >= 1 is cell
//     cell(o_q, q, c_q, l, j) = (o_q >> l) + 2 q + (j - (c_q >> l))
// of a level buffer of level_cells(total_new, T, l) = (total_new >> l) + 2 T cells, o_q the offset of tree q's new leaves:
// neighbouring trees lie ((o_q + n_q) >> l) - (o_q >> l) + 2 >= (n_q >> l) + 2 cells apart, and first_cell grows strictly
// with q, so a lane finds its tree by binary search over the offsets alone, as in a forest.  Two level buffers used in turn
// (level_base) and, behind them, 64 staging cells per tree for the new peaks: level l + 1 still reads the old P_l, and the new
// peaks may go where the old ones are, so they are committed behind the last level.
#pragma once
#include <stdint.h>

#include "merkle_math.hpp"
#define VKMR_FRONTIER_FN VKMR_MATH_FN

#define VKMR_FRONTIER_MAX_STRIDE 64u
// status_dev of vkmr_hip_frontier_extend_async
#define VKMR_FRONTIER_BAD_OFFSETS 1u     // offsets decrease, offsets[0] != 0 or offsets[T] != total_new
#define VKMR_FRONTIER_OVER_MAX_NEW 2u    // a tree takes more than max_new leaves
#define VKMR_FRONTIER_TOO_LARGE 4u       // a new count above 2^58
#define VKMR_FRONTIER_OVER_STRIDE 8u     // a new count of more bits than a frontier has cells

namespace vkmr_frontier {

using vkmr_math::height;
VKMR_FRONTIER_FN uint64_t level_count(uint64_t c, uint32_t l) { return c == 0 ? 0 : ((c - 1) >> l) + 1; }
VKMR_FRONTIER_FN uint32_t bit_length(uint64_t c) { return c == 0 ? 0u : 64u - (uint32_t)__builtin_clzll(c); }
VKMR_FRONTIER_FN bool has_peak(uint64_t c, uint32_t l) { return l < 64u && ((c >> l) & 1ull) != 0; }
VKMR_FRONTIER_FN uint64_t max_count() { return 1ull << 58; }

// What the check kernel (and the CPU twin) refuses for one tree: old count c, new leaves [lo, hi) of total_new, as tree q of T.
VKMR_FRONTIER_FN uint32_t refusal(uint64_t c, uint64_t lo, uint64_t hi, uint32_t q, uint32_t T, uint64_t total_new, uint64_t max_new, uint32_t stride)
{
    uint32_t bits = 0u;
    if (hi < lo || (q == 0u && lo != 0ull) || (q + 1u == T && hi != total_new)) bits |= VKMR_FRONTIER_BAD_OFFSETS;
    if (hi < lo) return bits;
    const uint64_t n = hi - lo;
    if (n > max_new) bits |= VKMR_FRONTIER_OVER_MAX_NEW;
    if (c > max_count() || n > max_count() - c) return bits | VKMR_FRONTIER_TOO_LARGE;
    if (bit_length(c + n) > stride) bits |= VKMR_FRONTIER_OVER_STRIDE;
    return bits;
}

// Tree q takes part in the launch of level l >= 1: it has a leaf, and level l - 1 of the new tree still had two nodes (or is
// the leaves: a lone leaf is hashed with itself once).
VKMR_FRONTIER_FN bool takes_part(uint64_t c2, uint32_t l) { return c2 != 0ull && (l == 1u || level_count(c2, l - 1u) > 1ull); }
VKMR_FRONTIER_FN uint64_t first_node(uint64_t c, uint32_t l) { return c >> l; }
VKMR_FRONTIER_FN uint64_t end_node(uint64_t c2, uint32_t l) { return takes_part(c2, l) ? level_count(c2, l) : 0ull; }

// Level buffers.  first_cell is where tree q's formed nodes begin at level l >= 1; for l == 0 the new leaves, at o.
VKMR_FRONTIER_FN uint64_t first_cell(uint64_t o, uint32_t q, uint32_t l) { return l == 0u ? o : (o >> l) + 2ull * q; }
VKMR_FRONTIER_FN uint64_t level_cells(uint64_t total_new, uint32_t T, uint32_t l) { return (l >= 64u ? 0ull : total_new >> l) + 2ull * T; }
inline uint64_t level_base(uint64_t total_new, uint32_t T, uint32_t l) { return (l & 1u) ? 0ull : level_cells(total_new, T, 1); }
inline uint64_t staging_base(uint64_t total_new, uint32_t T) { return 2ull * level_cells(total_new, T, 1); }
inline uint64_t scratch_cells(uint64_t total_new, uint32_t T) { return T == 0u ? 0ull : staging_base(total_new, T) + (uint64_t)VKMR_FRONTIER_MAX_STRIDE * T; }
// Launches of the extend: H(c2) <= bit_length(c2) <= stride for every tree the check lets through, and no count passes 2^58.
inline uint32_t launches(uint32_t stride) { return stride < 58u ? stride : 58u; }

// One node of one level: what frontier_level_kernel's lane does once it has its tree, and what the replay walks.
struct Step {
    bool active;        // the node exists: takes_part and j < end_node (j >= first_node by the cell rule)
    bool left_is_peak;  // the left child is the old peak P_(l-1), cell l - 1 of the tree's frontier; else in_left
    bool right_is_left; // the ragged edge: the left child again
    uint64_t in_left;   // cells of level l - 1's buffer (of the new leaves for l == 1)
    uint64_t in_right;
    bool root;          // the node is the root: node 0 of level H(c2)
    bool peak;          // the node is the new peak P_l
};

VKMR_FRONTIER_FN Step step(uint64_t o, uint32_t q, uint64_t c, uint64_t c2, uint32_t l, uint64_t j)
{
    Step s = {};
    const uint64_t n_out = end_node(c2, l);
    s.active = j < n_out;
    if (!s.active) return s;
    const uint64_t n_in = level_count(c2, l - 1u), lo_in = first_node(c, l - 1u), in0 = first_cell(o, q, l - 1u);
    const uint64_t r = vkmr_math::right_child(j, n_in);
    s.left_is_peak = 2ull * j < lo_in;              // then 2j == lo_in - 1 and bit l - 1 of c is set
    s.right_is_left = r == 2ull * j;
    s.in_left = in0 + (2ull * j - lo_in);           // unused (and wrapped) when left_is_peak
    s.in_right = in0 + (r - lo_in);                 // unused when right_is_left
    s.root = level_count(c2, l) == 1ull;
    s.peak = has_peak(c2, l) && j + 1ull == (c2 >> l);
    return s;
}

// Where the commit takes the new peak of a set bit l of c2 from.
enum PeakSource { PEAK_OLD = 0, PEAK_LAST_LEAF = 1, PEAK_STAGED = 2 };
VKMR_FRONTIER_FN PeakSource peak_source(uint64_t c, uint64_t c2, uint32_t l)
{
    if ((c2 >> l) == (c >> l)) return PEAK_OLD;
    return l == 0u ? PEAK_LAST_LEAF : PEAK_STAGED;
}
// The one tree no launch forms a root for: no new leaf and a power of two of at least 2 old ones; the root is P_H(c).
VKMR_FRONTIER_FN bool root_is_old_peak(uint64_t c, uint64_t c2) { return c2 == c && c >= 2ull && (c & (c - 1ull)) == 0ull; }

// ---- a node of a tree of a stored forest, read where the build left it: node j of level l of tree t with offset o and `count`
// leaves now (j < level_count(count, l)) is the leaf o + j for l == 0, roots[t] where level l has a single node (the build keeps
// a tree's last level in the roots alone), else cell (o >> l) + t + j of stored level l.  consistency_plan.hpp reads the peaks
// of an EARLIER count and their right neighbours by the same two functions.
enum GatherSource { GATHER_NONE = 0, GATHER_LEAF = 1, GATHER_ROOT = 2, GATHER_LEVEL = 3 };
VKMR_FRONTIER_FN GatherSource node_source(uint64_t count, uint32_t l)
{
    if (l == 0u) return GATHER_LEAF;
    return level_count(count, l) == 1ull ? GATHER_ROOT : GATHER_LEVEL;
}
VKMR_FRONTIER_FN uint64_t node_cell(uint64_t o, uint32_t t, uint32_t l, uint64_t j) { return l == 0u ? o + j : (o >> l) + t + j; }

// The frontier of such a tree (vkmr_hip_forest_frontier_async): peak l is node (c >> l) - 1 of level l, for c the count now:
// the last leaf for l == 0, roots[t] where c == 2^l, else a cell of stored level l.
VKMR_FRONTIER_FN GatherSource gather_source(uint64_t c, uint32_t l) { return has_peak(c, l) ? node_source(c, l) : GATHER_NONE; }
VKMR_FRONTIER_FN uint64_t gather_cell(uint64_t o, uint32_t t, uint64_t c, uint32_t l) { return node_cell(o, t, l, (c >> l) - 1ull); }

}  // namespace vkmr_frontier
