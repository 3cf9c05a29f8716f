// merge_plan.hpp -- two sorted forests merged tree by tree on the device: union, difference, intersection (include/vkmr_hip.h:
// vkmr_hip_forest_merge_leaves_async, vkmr_hip_tree_merge_leaves_async): the slots, what a leaf of B does at its slot, where every
// leaf goes, the output counts and the scratch layout.  Plain integer arithmetic, no HIP types: shared by the kernels
// (merge_kernels.hpp), the C ABI (vkmr_hip.hip), the CPU twins (host/host_api.cpp) and the replay in tests/c/merge_plan_test.cpp.
//
// THE ORDER is absence_plan.hpp's: word 0 first, every word unsigned.  Every tree of A is strictly increasing, every tree of B
// non-decreasing; a leaf of B equal to its predecessor IN ITS TREE is a REPEAT and takes part in nothing.
//
// THE ELEMENTS.  Element i of A is cell a_offsets[0] + i for i < nA = a_offsets[ntrees] - a_offsets[0], element j of B likewise;
// base_A(t) = a_offsets[t] - a_offsets[0].  The grids and the scratch follow the bounds a_total >= nA and b_total >= nB, never
// where the forests lie in their buffers.
//
// THE SLOTS.  Slot x, 0 <= x <= a_total, stands for "in front of element x of A".  Leaf j of B_t has lb = the lower bound of b_j in
// A_t (absence_plan.hpp's loop) and the slot base_A(t) + lb.  A digest above a tree's last leaf has the slot of the next tree's
// first element, or slot nA behind the last tree: it shares that slot with the leaves of later trees of B that go in front of
// the same element.  That does no harm: B's leaves are placed by their own order (below), the slots only count, and a slot that
// is MARKED is always a real leaf of the tree of the leaf of B that marks it (a match has lb < count).  So there is no end slot
// per tree, and an element of A needs no search for its tree to find its slot.
//   match(j)   lb < count_A(t) and A_t[lb] == b_j
//   union         kept(j) = no repeat and no match;  slot += 1 for a kept j (an atomic add: several may share a slot);
//                 flag[j] = kept(j)
//   difference    a leaf j that is no repeat and matches stores 1 at its slot (distinct digests: distinct slots)
//   intersection  the same
// matches = the leaves that are no repeat and match, repeats = the repeats: both whatever the op.
//
// THE SCAN.  One array of WORDS(a_total, b_total) uint32 words, zeroed: the slots at [0, a_total], the flags at S + j with
// S = a_total + 1, one spare word.  Its exclusive prefix E is formed by sort_kernels.hpp's sort_scan_kernel as it is, launched
// twice: over the array as rows of VKMR_MERGE_SCAN_ROW words (in place; the row sums into `tot`), then over `tot` as one row.
// E(x) = row[x] + tot[x / ROW]: two loads.  The in-place scan consumes the counts and the marks; they come back as
// E(x + 1) - E(x).  Every sum is at most nA + nB < 2^32.
//
// PLACEMENT, with kB(j) = E(S + j) - E(S), the kept leaves of B in front of j in the whole forest (those of earlier trees are
// all in front of tree t's output, so the forest-wide count serves):
//   union         b_j kept   -> base_A(t) + lb + kB(j)              a_i -> i + E(i + 1)      n_out = nA + E(S)
//                 out_offsets[t] = base_A(t) + kB(base_B(t))
//   difference    a_i stays when E(i + 1) == E(i)  -> i - E(i)                               n_out = nA - E(S)
//                 out_offsets[t] = base_A(t) - E(base_A(t))
//   intersection  a_i stays when E(i + 1) != E(i)  -> E(i)                                   n_out = E(S)
//                 out_offsets[t] = E(base_A(t))
// E(S) is the sum of all the slots.  out_offsets[ntrees] = n_out follows from the same forms with base(ntrees) = n.
//
// Scratch, in bytes from its start (16-byte aligned), every part a multiple of 16 bytes:
//   scan     4 * ROWS * VKMR_MERGE_SCAN_ROW     the slots, the flags, the spare word, padded to whole rows
//   tot      4 * ROWS                           the row sums, then their prefix
//   grand    16                                 the sum of everything (not read)
//   pos0     4 * b_total                        base_A(t) + lb of a kept leaf of B (union), VKMR_MERGE_NONE for every other
//   hdr      8 * VKMR_MERGE_HEADER_WORDS        [0] status bits 2 and 3, [1] matches, [2] repeats, [3] A's offsets check, [4] B's
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "merkle_math.hpp"

#define VKMR_MERGE_UNION 0u
#define VKMR_MERGE_DIFFERENCE 1u
#define VKMR_MERGE_INTERSECTION 2u
// info_dev[0] of vkmr_hip_forest_merge_leaves_async
#define VKMR_MERGE_BAD_A_OFFSETS 1ull        // A's offsets decrease somewhere, or end behind a_total
#define VKMR_MERGE_BAD_B_OFFSETS 2ull        // the same for B
#define VKMR_MERGE_A_NOT_INCREASING 4ull     // some tree of A is not strictly increasing
#define VKMR_MERGE_B_DECREASES 8ull          // some tree of B decreases somewhere
#define VKMR_MERGE_SHORT_OUTPUT 16ull        // n_out > out_capacity; info[1] holds n_out
#define VKMR_MERGE_ORIGIN_B (1ull << 63)     // origin_out: a cell of B

#define VKMR_MERGE_SCAN_ROW 8192u            // words of one row of the scan: 32 trips of a sort_scan_kernel workgroup
#define VKMR_MERGE_HEADER_WORDS 8u
#define VKMR_MERGE_NONE 0xFFFFFFFFu

namespace vkmr_merge {

// a_total + b_total + 2 words must have 32-bit sums and positions.
constexpr uint64_t MAX_WORDS = 1ull << 32;

VKMR_MATH_FN uint64_t slots(uint64_t a_total) { return a_total + 1ull; }                     // S: where the flags begin
VKMR_MATH_FN uint64_t words(uint64_t a_total, uint64_t b_total) { return a_total + b_total + 2ull; }
VKMR_MATH_FN uint64_t rows(uint64_t w) { return (w + VKMR_MERGE_SCAN_ROW - 1u) / VKMR_MERGE_SCAN_ROW; }
VKMR_MATH_FN bool fits(uint64_t a_total, uint64_t b_total) { return a_total < MAX_WORDS && b_total < MAX_WORDS && words(a_total, b_total) < MAX_WORDS; }

// E(x) of the two-level scan.
VKMR_MATH_FN uint32_t prefix(const uint32_t* row, const uint32_t* tot, uint64_t x) { return row[x] + tot[x / VKMR_MERGE_SCAN_ROW]; }

// What a leaf of B does.
VKMR_MATH_FN bool kept(uint32_t op, bool repeat, bool match) { return op == VKMR_MERGE_UNION && !repeat && !match; }
VKMR_MATH_FN bool marks(uint32_t op, bool repeat, bool match) { return op != VKMR_MERGE_UNION && !repeat && match; }

// Where element i of A goes, given E(i) and E(i + 1); false: it does not stay.  Selects, no branch on op: every term is formed
// for every op and the op picks among them.
VKMR_MATH_FN bool a_dest(uint32_t op, uint64_t i, uint32_t e_i, uint32_t e_next, uint64_t* dest)
{
    const bool uni = op == VKMR_MERGE_UNION, dif = op == VKMR_MERGE_DIFFERENCE;
    const uint64_t own = (uni || dif) ? i : 0ull;                            // union and difference start from the leaf's own number
    const uint64_t up = uni ? (uint64_t)e_next : (dif ? 0ull : (uint64_t)e_i);
    const uint64_t down = dif ? (uint64_t)e_i : 0ull;
    *dest = own + up - down;
    return uni || ((e_next == e_i) == dif);
}
// Where a kept leaf of B goes (union): pos0 = base_A(t) + lb, k_b = E(S + j) - E(S).
VKMR_MATH_FN uint64_t b_dest(uint32_t pos0, uint32_t k_b) { return (uint64_t)pos0 + k_b; }
// out_offsets[t]: base_a = base_A(t), e_a = E(base_A(t)), k_b = E(S + base_B(t)) - E(S).  t == ntrees gives n_out.
VKMR_MATH_FN uint64_t tree_start(uint32_t op, uint64_t base_a, uint32_t e_a, uint32_t k_b)
{
    const bool uni = op == VKMR_MERGE_UNION, dif = op == VKMR_MERGE_DIFFERENCE;
    const uint64_t own = (uni || dif) ? base_a : 0ull;
    const uint64_t up = uni ? (uint64_t)k_b : (dif ? 0ull : (uint64_t)e_a);
    const uint64_t down = dif ? (uint64_t)e_a : 0ull;
    return own + up - down;
}
// n_out from nA and E(S), the sum of the slots.
VKMR_MATH_FN uint64_t n_out(uint32_t op, uint64_t nA, uint32_t e_S) { return tree_start(op, nA, e_S, e_S); }
// The identities info holds a call to.
VKMR_MATH_FN uint64_t n_out_of_counts(uint32_t op, uint64_t nA, uint64_t nB, uint64_t matches, uint64_t repeats)
{
    if (op == VKMR_MERGE_UNION) return nA + nB - matches - repeats;
    if (op == VKMR_MERGE_DIFFERENCE) return nA - matches;
    return matches;
}

inline size_t up16(size_t n) { return (n + 15u) & ~(size_t)15u; }

struct Layout {
    uint64_t S, words, rows;
    size_t scan, tot, grand, pos0, hdr, bytes;
};

inline Layout layout(uint64_t a_total, uint64_t b_total)   // fits(a_total, b_total)
{
    Layout L;
    L.S = slots(a_total);
    L.words = words(a_total, b_total);
    L.rows = rows(L.words);
    size_t at = 0;
    L.scan = at;    at += (size_t)L.rows * VKMR_MERGE_SCAN_ROW * 4u;
    L.tot = at;     at += up16((size_t)L.rows * 4u);
    L.grand = at;   at += 16u;
    L.pos0 = at;    at += up16((size_t)b_total * 4u);
    L.hdr = at;     at += up16((size_t)VKMR_MERGE_HEADER_WORDS * 8u);
    L.bytes = at;
    return L;
}

inline size_t scratch_bytes(uint64_t a_total, uint64_t b_total) { return fits(a_total, b_total) ? layout(a_total, b_total).bytes : 0u; }

}  // namespace vkmr_merge
