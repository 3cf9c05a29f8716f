// proofs_at_plan.hpp -- inclusion proofs as of an EARLIER count (vkmr_hip_forest_proofs_at_async): "leaf i was in the tree of c
// leaves", proved under the root the tree had then, out of the stored levels of the tree of c2 >= c leaves it has grown into.
// Which nodes of the old tree the grown tree still holds, the one other node a level of the old tree can have, when it is hashed
// and from what, and where every cell of a proof comes from.  Plain integer arithmetic, no HIP types: shared by the kernels
// (proofs_at_kernels.hpp), the C ABI (vkmr_hip.hip), the CPU twin (host/host_api.cpp) and the replay in
// tests/c/proofs_at_plan_test.cpp.  Notation: frontier_plan.hpp's and consistency_plan.hpp's (H = height, level_count, has_peak,
// P_l the peak of a set bit l, l0 = ctz(c)).
//
// AN EPOCH is (t, c): tree t as of c leaves, 1 <= c <= c2 (c == 0: the tree not yet begun; its root is zero and it proves nothing).
//
// THE OLD TREE'S NODES.  Node s of level l of the old tree is COMPLETE when (s + 1) << l <= c: all of its 2^l leaves exist, no
// later leaf changes it, so it is node s of level l of the new tree -- a leaf, a stored cell or roots[t] by frontier_plan.hpp's
// node_source(c2, l) / node_cell.  A level l <= l0 has complete nodes only.  A level l0 < l <= H(c) has exactly one more: its
// last node E_l, the carry of the frontier's root walk --
//     bit l - 1 of c set:     E_l = hash_pair(P_(l-1), E_(l-1)), E_(l-1) replaced by P_(l-1) itself where l - 1 == l0
//     bit l - 1 of c clear:   E_l = hash_pair(E_(l-1), E_(l-1))
// H(c) - l0 hashes an epoch, through one hash_pair (edge_step()).  The old root is E_H(c); for c a power of two of at least 2
// (l0 == H(c), no hash) it is node 0 of level H(c) of the new tree, which is P_H(c).
//
// THE EDGE ROW of an epoch, `stride` cells: cell l = E_l for l0 < l < H(c), every other cell zero.  The old root has a cell of
// its own.
//
// THE PROOF of leaf i < c, H(c) cells of a row of `stride`: cell l is node sibling(c, l, i) of the old tree's level l -- the
// existing proofs' rule for a missing sibling -- read from the new tree when complete, else from the edge row (cell_source()).
// No hash per query.  Refused, nothing written: consistency_plan.hpp's refusal() over the epochs.
#pragma once
#include <stdint.h>

#include "consistency_plan.hpp"
#define VKMR_PROOFS_AT_FN VKMR_MATH_FN

namespace vkmr_proofs_at {

using vkmr_consistency::low_level;
using vkmr_consistency::peak_node;
using vkmr_consistency::refusal;
using vkmr_frontier::bit_length;
using vkmr_frontier::has_peak;
using vkmr_frontier::height;
using vkmr_frontier::level_count;

// c is a power of two of at least 2: every node of the old tree is complete, the root included.
VKMR_PROOFS_AT_FN bool root_is_stored(uint64_t c) { return c >= 2ull && (c & (c - 1ull)) == 0ull; }
// Levels of the epoch's tree (the height every proof of the epoch gets); 0 for the tree not yet begun.
VKMR_PROOFS_AT_FN uint32_t levels(uint64_t c) { return c == 0ull ? 0u : height(c); }
// Node hashes of one epoch.
VKMR_PROOFS_AT_FN uint32_t hashes(uint64_t c) { return c == 0ull || root_is_stored(c) ? 0u : height(c) - low_level(c); }
// Cell l of the edge row holds E_l (else zero).
VKMR_PROOFS_AT_FN bool has_edge(uint64_t c, uint32_t l) { return c != 0ull && l < 64u && l > low_level(c) && l < height(c); }
// Node s of the old tree's level l (s < level_count(c, l), l < 64) is one of the new tree's.
VKMR_PROOFS_AT_FN bool complete(uint64_t c, uint32_t l, uint64_t s) { return s + 1ull <= (c >> l); }
// The node of level l a proof of leaf i < c takes.
VKMR_PROOFS_AT_FN uint64_t sibling(uint64_t c, uint32_t l, uint64_t i) { return vkmr_math::sibling(i >> l, level_count(c, l)); }

// Level l of the edge walk, l = 0 .. : what forms E_(l+1).  `have`: an earlier level has hashed.
struct EdgeStep {
    bool hash;       // E_(l+1) = hash_pair(a, b)
    bool peak;       // a is P_l, node peak_node(c, l) of the new tree's level l; else the carry
    bool twice;      // b is a again (no carry yet: l == l0); else the carry
    bool to_root;    // what this level gives is the old root, else cell l + 1 of the edge row (when the row has one)
    bool stored;     // no hash, and the old root is node 0 of level l + 1 of the new tree: c == 2^(l+1)
};
VKMR_PROOFS_AT_FN EdgeStep edge_step(uint64_t c, uint32_t l, bool have)
{
    EdgeStep s = {};
    const uint32_t H = levels(c);
    if (l >= H) return s;                       // c == 0 included: zero cells
    s.peak = has_peak(c, l);
    s.hash = s.peak || have;
    s.twice = !have;
    s.to_root = l + 1u == H;
    s.stored = s.to_root && !s.hash;
    return s;
}

// Where cell l of the proof of query (epoch of count c, leaf i) comes from.
enum CellSource { CELL_ZERO = 0, CELL_STORED = 1, CELL_EDGE = 2 };
VKMR_PROOFS_AT_FN CellSource cell_source(uint64_t c, uint32_t l, uint64_t i)
{
    if (i >= c || l >= height(c)) return CELL_ZERO;
    return complete(c, l, sibling(c, l, i)) ? CELL_STORED : CELL_EDGE;
}

}  // namespace vkmr_proofs_at
