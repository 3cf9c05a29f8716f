// absence_plan.hpp -- "digest x is no leaf of this tree", proved to a holder of the root and the count of a tree whose leaves are
// strictly increasing (vkmr_hip_forest_sorted_async, vkmr_hip_forest_lower_bound_async, vkmr_hip_forest_absence_async,
// vkmr_hip_verify_forest_absence_async and their one-tree twins): the order on digests, the lower bound, which cells a proof holds,
// which of them the check reads and what it answers.  Plain integers and compares, no HIP types: shared by the kernels
// (absence_kernels.hpp), the C ABI (vkmr_hip.hip), the CPU twins (host/host_api.cpp) and the replay in
// tests/c/absence_plan_test.cpp.
//
// ORDER.  a < b compares data[0], then data[1], .. data[7] as UNSIGNED 32-bit values: the byte order of the canonical digest.  A
// tree of c leaves is SORTED when leaf[i-1] < leaf[i] for every 1 <= i < c; equal neighbours offend as well.
//
// LOWER BOUND of x in a tree of c leaves, fixed as a loop so that an unsorted tree still has one answer (lower_bound()): on a
// sorted tree the number of leaves below x.
//
// THE PROOF of (tree t of c leaves, x), i the lower bound, H = height(c):
//   index   i
//   pred    leaf i - 1, zero when i == 0;   succ   leaf i, zero when i == c
//   main    `stride` cells: the plain inclusion proof of the ANCHOR, leaf i when i < c, else leaf c - 1
//   low     `stride` cells, used only when 0 < i < c: with top = ctz(i), the siblings of leaf i - 1 at the levels below top (all
//           left siblings, all there: the bits of i - 1 below top are ones); zero from top up.  Above top the two paths are one,
//           and the node of leaf i - 1 at level top IS main[top].
// THE VERDICT (verdict()): 0 not proven, 1 absent, 2 present.  The fold is H + top node hashes where two plain proofs take 2 H.
// The proof binds under a root COMMITTED OVER A SORTED TREE; who holds the leaves checks that with the sortedness pass.
#pragma once
#include <stdint.h>

#include "merkle_math.hpp"
#define VKMR_ABSENCE_FN VKMR_MATH_FN

#define VKMR_ABSENCE_NOT_PROVEN 0u
#define VKMR_ABSENCE_ABSENT 1u
#define VKMR_ABSENCE_PRESENT 2u
// info_dev[0] of vkmr_hip_forest_sorted_async
#define VKMR_SORTED_BAD_OFFSETS 1ull     // offsets decrease somewhere, or end behind `total`

namespace vkmr_absence {

constexpr uint64_t NONE = ~0ull;         // "no offence", and the index of a query into no tree
constexpr uint64_t MAX_COUNT = 1ull << 58;

// a < b and a == b on eight words each.
VKMR_ABSENCE_FN bool less(const uint32_t* a, const uint32_t* b)
{
    bool lt = false, decided = false;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int w = 0; w < 8; ++w) {
        const bool ne = a[w] != b[w];
        lt = (!decided && ne) ? a[w] < b[w] : lt;
        decided = decided || ne;
    }
    return lt;
}
VKMR_ABSENCE_FN bool equal(const uint32_t* a, const uint32_t* b)
{
    uint32_t d = 0u;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int w = 0; w < 8; ++w) d |= a[w] ^ b[w];
    return d == 0u;
}

// H(c): the levels of a proof in a tree of c leaves; a tree without a leaf has none.
VKMR_ABSENCE_FN uint32_t height(uint64_t c) { return c == 0ull ? 0u : vkmr_math::height(c); }

// The rule's loop.  below(mid) says whether leaf[mid] < x; it is asked for mid < c only.
template <class Below>
VKMR_ABSENCE_FN uint64_t lower_bound(uint64_t c, Below below)
{
    uint64_t lo = 0ull, hi = c;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2ull;
        if (below(mid)) lo = mid + 1ull;
        else hi = mid;
    }
    return lo;
}

// The cells of a proof with index i in a tree of c >= 1 leaves, i <= c.
VKMR_ABSENCE_FN uint64_t anchor(uint64_t i, uint64_t c) { return i < c ? i : c - 1ull; }
VKMR_ABSENCE_FN bool has_pred(uint64_t i) { return i > 0ull; }
VKMR_ABSENCE_FN bool has_succ(uint64_t i, uint64_t c) { return i < c; }
VKMR_ABSENCE_FN bool two_sided(uint64_t i, uint64_t c) { return i > 0ull && i < c; }       // the low row matters
VKMR_ABSENCE_FN uint32_t top(uint64_t i) { return (uint32_t)__builtin_ctzll(i); }          // i >= 1
// Cell l of the low row holds a node (and the check reads it): the sibling of leaf i - 1 at level l, node ((i - 1) >> l) ^ 1.
VKMR_ABSENCE_FN bool low_cell(uint64_t i, uint64_t c, uint32_t l) { return two_sided(i, c) && l < top(i); }
VKMR_ABSENCE_FN uint32_t hashes(uint64_t i, uint64_t c) { return height(c) + (two_sided(i, c) ? top(i) : 0u); }

// What the check refuses before it reads a cell: checks 1 to 3, and a row too short for the proof.
VKMR_ABSENCE_FN bool checkable(uint32_t t, uint32_t ntrees, uint32_t h, uint64_t c, uint64_t i, uint32_t stride)
{
    return t < ntrees && c <= MAX_COUNT && h == height(c) && h <= stride && i <= c;
}

// The verdict, on digests as eight words each.  pair(a, b, out): out = the node hash of (a, b); out is neither a nor b.  The
// kernels run the same steps through one hash_pair (absence_kernels.hpp); this is the text the CPU twin and the replay run.
// `reads`, where given, is told every (row, level) the check reads: row 0 main, 1 low.
struct NoReads { void operator()(uint32_t, uint32_t) const {} };

template <class Pair, class Reads = NoReads>
inline uint32_t verdict(const uint32_t* x, uint32_t t, uint32_t ntrees, uint64_t i, const uint32_t* pred, const uint32_t* succ, const uint32_t* main_row,
                        const uint32_t* low_row, uint32_t h, uint32_t stride, const uint32_t* root, uint64_t c, Pair pair, Reads reads = Reads())
{
    if (!checkable(t, ntrees, h, c, i, stride)) return VKMR_ABSENCE_NOT_PROVEN;
    if (c == 0ull) {
        uint32_t any = 0u;
        for (int w = 0; w < 8; ++w) any |= root[w];
        return any == 0u ? VKMR_ABSENCE_ABSENT : VKMR_ABSENCE_NOT_PROVEN;
    }
    const bool present = has_succ(i, c) && equal(x, succ);
    if (!present) {
        if (has_pred(i) && !less(pred, x)) return VKMR_ABSENCE_NOT_PROVEN;
        if (has_succ(i, c) && !less(x, succ)) return VKMR_ABSENCE_NOT_PROVEN;
    }
    uint32_t cur[8], next[8];
    if (!present && two_sided(i, c)) {                   // pred up to level top: it must arrive at main[top]
        const uint32_t tp = top(i);
        for (int w = 0; w < 8; ++w) cur[w] = pred[w];
        for (uint32_t l = 0; l < tp; ++l) {
            reads(1u, l);
            pair(low_row + 8u * l, cur, next);
            for (int w = 0; w < 8; ++w) cur[w] = next[w];
        }
        if (!equal(cur, main_row + 8u * tp)) return VKMR_ABSENCE_NOT_PROVEN;    // read again by the main fold below
    }
    const uint64_t a = anchor(i, c);
    const uint32_t* leaf = has_succ(i, c) ? succ : pred;
    for (int w = 0; w < 8; ++w) cur[w] = leaf[w];
    for (uint32_t l = 0; l < h; ++l) {
        reads(0u, l);
        if ((a >> l) & 1ull) pair(main_row + 8u * l, cur, next);
        else pair(cur, main_row + 8u * l, next);
        for (int w = 0; w < 8; ++w) cur[w] = next[w];
    }
    if (!equal(cur, root)) return VKMR_ABSENCE_NOT_PROVEN;
    return present ? VKMR_ABSENCE_PRESENT : VKMR_ABSENCE_ABSENT;
}

}  // namespace vkmr_absence
