// range_plan.hpp -- "these are ALL the leaves of this tree between lo and hi", proved to a holder of the root and the count of a tree
// whose leaves are strictly increasing (vkmr_hip_forest_range_async, vkmr_hip_verify_forest_range_async and their one-tree twins):
// which leaves a proof carries, which cells its two rows hold, which of them the check reads, where the check keeps the nodes of a
// level, and what it answers.  Plain integers and compares, no HIP types: shared by the kernels (range_kernels.hpp), the C ABI
// (vkmr_hip.hip), the CPU twins (host/host_api.cpp) and the replay in tests/c/range_plan_test.cpp.  The order, the lower bound's loop
// and H(c) are absence_plan.hpp's.
//
// A QUERY is (t, lo, hi), a tree and a CLOSED interval of digests; the all-zero and the all-ones digest say "from the start" and "to
// the end".  For tree t of c leaves, H = height(c):
//   i0 = lower bound of lo;  i1 = upper bound of hi = lower bound of hi, + 1 when the leaf there is hi
//   the RUN is leaves [a, b], a = i0 > 0 ? i0 - 1 : 0, b = i1 < c ? i1 : c - 1, m = b - a + 1 >= 1: the leaves in [lo, hi] and the
//   neighbour on either side that fences them, where there is one.  An empty range carries its fence alone (one or two leaves).
//   c == 0: first 0, m 0.  t >= ntrees or hi < lo: REFUSED, first NONE, m 0, height 0; the check answers 0.
// THE ROWS, `stride` cells each:  left[l] = node (a >> l) - 1 of level l when (a >> l) is odd;  right[l] = node (b >> l) + 1 when
//   (b >> l) is even and that node exists (< ceil(c / 2^l));  zero cells otherwise and from H up.  The duplicate of a level's last
//   node is NOT carried: the check duplicates by the count, so that the count binds the right edge.
// THE CHECK (refused(), fences(), step()): verdict 1 when nothing is refused, the carried leaves are strictly increasing, the fences
//   and the canonical shape hold and the fold of levels 0 .. H - 1 arrives at the root; in_first / in_count = the leaves of the run
//   inside [lo, hi].  Every left / right decision of the fold is taken from a, m and c, so the position is bound, and no row cell is
//   read that the rule above does not name.  As with absence the verdict binds under a root COMMITTED OVER A SORTED TREE.
// THE CHECK'S LEVELS: node j of query q's level l >= 1 lies at cell (leaf_starts[q] >> l) + 2 q + j of the level's buffer
//   (level_cell()); level 0 is the leaves themselves.  nodes(l) = (b >> l) - (a >> l) + 1 <= (m >> l) + 2, so two queries never share
//   a cell and level l needs (N >> l) + 2 Q cells, N the leaves carried.  Odd levels in one buffer, even ones in another (layout()).
#pragma once
#include <stdint.h>

#include "absence_plan.hpp"
#define VKMR_RANGE_FN VKMR_MATH_FN

// info_dev[0] of the two gathers
#define VKMR_RANGE_LEAVES_CAPACITY 1ull    // the leaves carried exceed leaves_capacity: info[1] is the total, no leaf was written
#define VKMR_RANGE_THREADS 256             // lanes of a workgroup of the prefix over m

namespace vkmr_range {

constexpr uint64_t NONE = ~0ull;
constexpr uint64_t MAX_COUNT = vkmr_absence::MAX_COUNT;

struct Run { uint64_t first, m; uint32_t height; uint64_t inside; };   // inside: leaves in [lo, hi]

// The run of (lo, hi) in a tree of c leaves; leaf_less(i, x) says leaf[i] < x and leaf_equal(i, x) leaf[i] == x, both for i < c only.
// `known` false: the query names no tree.  On a tree that is not sorted the loops still end and first + m <= c.
template <class Less, class Equal>
VKMR_RANGE_FN Run run(bool known, uint64_t c, const uint32_t* lo, const uint32_t* hi, Less leaf_less, Equal leaf_equal)
{
    if (!known || vkmr_absence::less(hi, lo)) return Run{NONE, 0ull, 0u, 0ull};
    if (c == 0ull) return Run{0ull, 0ull, 0u, 0ull};
    const uint64_t i0 = vkmr_absence::lower_bound(c, [&](uint64_t mid) { return leaf_less(mid, lo); });
    uint64_t i1 = vkmr_absence::lower_bound(c, [&](uint64_t mid) { return leaf_less(mid, hi); });
    if (i1 < c && leaf_equal(i1, hi)) ++i1;
    const uint64_t a = i0 > 0ull ? i0 - 1ull : 0ull;
    uint64_t b = i1 < c ? i1 : c - 1ull;
    if (b < a) b = a;                            // an unsorted tree only
    return Run{a, b - a + 1ull, vkmr_absence::height(c), i1 > i0 ? i1 - i0 : 0ull};
}

// Cells of level l of a tree of c >= 1 leaves.
VKMR_RANGE_FN uint64_t level_count(uint64_t c, uint32_t l) { return ((c - 1ull) >> l) + 1ull; }

// Does cell l of a row hold a node (and does the check read it)?  The run is [a, b] in a tree of c leaves and height h.
VKMR_RANGE_FN bool left_cell(uint64_t a, uint32_t l, uint32_t h) { return l < h && ((a >> l) & 1ull) != 0ull; }
VKMR_RANGE_FN bool right_cell(uint64_t b, uint64_t c, uint32_t l, uint32_t h)
{
    return l < h && ((b >> l) & 1ull) == 0ull && (b >> l) + 1ull < level_count(c, l);
}

// What the check refuses before it reads a leaf or a cell.  m = leaf_starts[q + 1] - leaf_starts[q], formed by the caller without a wrap.
VKMR_RANGE_FN bool refused(uint32_t t, uint32_t ntrees, uint32_t h, uint32_t stride, uint64_t c, uint64_t a, uint64_t m, const uint32_t* lo,
                           const uint32_t* hi)
{
    if (t >= ntrees || c > MAX_COUNT || h != vkmr_absence::height(c) || h > stride) return true;
    if (a > c || m > c - a) return true;
    if (vkmr_absence::less(hi, lo)) return true;
    return c > 0ull && m == 0ull;
}

// The fences and the canonical shape of a run of m >= 1 leaves from index a in a tree of c: first, second, before_last, last are the
// run's leaves 0, 1, m - 2 and m - 1 (the middle two are read when m >= 2 only).  below / above: the first leaf is under lo, the last
// over hi -- the two leaves of the run that are NOT in the range.
struct Fences { bool ok, below, above; };
VKMR_RANGE_FN Fences fences(uint64_t a, uint64_t m, uint64_t c, const uint32_t* lo, const uint32_t* hi, const uint32_t* first, const uint32_t* second,
                            const uint32_t* before_last, const uint32_t* last)
{
    Fences f;
    f.below = vkmr_absence::less(first, lo);
    f.above = vkmr_absence::less(hi, last);
    f.ok = (f.below || a == 0ull) && (f.above || a + m == c);
    if (m >= 2ull) {
        if (f.below && vkmr_absence::less(second, lo)) f.ok = false;
        if (f.above && vkmr_absence::less(hi, before_last)) f.ok = false;
    }
    return f;
}

// Nodes of the run's level l, and of the level above: parents.
VKMR_RANGE_FN uint64_t nodes(uint64_t a, uint64_t m, uint32_t l) { return ((a + m - 1ull) >> l) - (a >> l) + 1ull; }

// Parent j of the fold from level l to l + 1 (l < H): where its two children come from.  FROM_LEVEL: node k of the run's level l;
// FROM_LEFT / FROM_RIGHT: cell l of that row.
enum Source : uint32_t { FROM_LEVEL = 0u, FROM_LEFT = 1u, FROM_RIGHT = 2u };
struct Step { bool active; uint32_t lsrc, rsrc; uint64_t lk, rk; };
VKMR_RANGE_FN Step step(uint64_t a, uint64_t m, uint64_t c, uint32_t l, uint64_t j)
{
    const uint64_t al = a >> l, bl = (a + m - 1ull) >> l;
    const uint64_t p = (al >> 1) + j;
    Step s;
    s.active = p <= (bl >> 1);
    const uint64_t x = 2ull * p, y = 2ull * p + 1ull;
    s.lsrc = x < al ? FROM_LEFT : FROM_LEVEL;
    s.lk = x < al ? 0ull : x - al;
    const bool beyond = y > bl;                   // then x <= bl: x is in the run, or p would not be a parent
    const bool exists = y < level_count(c, l);
    s.rsrc = !beyond ? FROM_LEVEL : (exists ? FROM_RIGHT : s.lsrc);
    s.rk = !beyond ? y - al : (exists ? 0ull : s.lk);
    return s;
}

// Where node j of query q's level l >= 1 lies in the level's buffer, and the cells of that buffer for N leaves carried by Q queries.
VKMR_RANGE_FN uint64_t level_cell(uint64_t leaf_start, uint64_t q, uint32_t l, uint64_t j) { return (leaf_start >> l) + 2ull * q + j; }
VKMR_RANGE_FN uint64_t level_cells(uint64_t N, uint64_t Q, uint32_t l) { return (l >= 64u ? 0ull : N >> l) + 2ull * Q; }

// The query of cell i of level l's buffer: the last q < Q with level_cell(leaf_starts[q], q, l, 0) <= i; starts(q) = leaf_starts[q],
// non-decreasing.  level_cell(.., q, ..) >= 2 q and <= (N >> l) + 2 q bound q from both sides before the first load.
template <class Starts>
VKMR_RANGE_FN uint64_t query_of_cell(uint64_t i, uint32_t l, uint64_t N, uint64_t Q, Starts starts)
{
    const uint64_t nl = N >> l;
    uint64_t lo = i > nl ? (i - nl) >> 1 : 0ull, hi = (i >> 1) + 1ull;      // the answer is in [lo, hi)
    if (hi > Q) hi = Q;
    if (lo >= hi) lo = hi - 1ull;
    while (hi - lo > 1ull) {
        const uint64_t mid = lo + (hi - lo) / 2ull;
        if (level_cell(starts(mid), mid, l, 0ull) <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

// The query of carried leaf j < leaf_starts[Q]: the last q < Q with leaf_starts[q] <= j (a query that carries nothing is skipped).
template <class Starts>
VKMR_RANGE_FN uint64_t query_of_leaf(uint64_t j, uint64_t Q, Starts starts)
{
    uint64_t lo = 0ull, hi = Q;
    while (hi - lo > 1ull) {
        const uint64_t mid = lo + (hi - lo) / 2ull;
        if (starts(mid) <= j) lo = mid;
        else hi = mid;
    }
    return lo;
}

// scratch_dev of the four calls, in bytes from its start: a header (word 0: leaf_starts is no prefix), the block sums of the prefix
// over m, a flag and a top cell per query, the buffer of the odd levels and that of the even ones.  The gathers use the first two.
struct Layout { uint64_t sums, ok, tops, odd, even, bytes, groups; };
VKMR_RANGE_FN uint64_t round32(uint64_t x) { return (x + 31ull) & ~31ull; }
VKMR_RANGE_FN Layout layout(uint64_t N, uint64_t Q)
{
    Layout L;
    L.groups = (Q + 1ull + VKMR_RANGE_THREADS - 1ull) / VKMR_RANGE_THREADS;
    L.sums = 32ull;
    L.ok = L.sums + round32(8ull * L.groups);
    L.tops = L.ok + round32(4ull * Q);
    L.odd = L.tops + 32ull * Q;
    L.even = L.odd + 32ull * level_cells(N, Q, 1u);
    L.bytes = L.even + 32ull * level_cells(N, Q, 2u);
    return L;
}

// The verdict of one query on digests as eight words each: the text the CPU twin runs.  pair(a, b, out): out = the node hash of
// (a, b).  leaves: the run's m cells; `work`: 8 * (nodes(a, m, 0) + 1) words of the caller's.  `reads`, where given, is told every
// (row, level) the check reads: row 1 left, 2 right.
struct NoReads { void operator()(uint32_t, uint32_t) const {} };
struct Verdict { uint32_t verdict; uint64_t in_first, in_count; };

template <class Pair, class Reads = NoReads>
inline Verdict verdict(uint32_t t, uint32_t ntrees, const uint32_t* lo, const uint32_t* hi, uint64_t a, uint64_t m, const uint32_t* leaves,
                       const uint32_t* left_row, const uint32_t* right_row, uint32_t h, uint32_t stride, const uint32_t* root, uint64_t c, uint32_t* work,
                       Pair pair, Reads reads = Reads())
{
    const Verdict no{0u, 0ull, 0ull};
    if (refused(t, ntrees, h, stride, c, a, m, lo, hi)) return no;
    if (c == 0ull) {
        uint32_t any = 0u;
        for (int w = 0; w < 8; ++w) any |= root[w];
        return any == 0u ? Verdict{1u, 0ull, 0ull} : no;
    }
    for (uint64_t j = 1; j < m; ++j)
        if (!vkmr_absence::less(leaves + 8ull * (j - 1ull), leaves + 8ull * j)) return no;
    const Fences f = fences(a, m, c, lo, hi, leaves, leaves + (m >= 2ull ? 8ull : 0ull), leaves + 8ull * (m >= 2ull ? m - 2ull : 0ull), leaves + 8ull * (m - 1ull));
    if (!f.ok) return no;
    for (uint64_t w = 0; w < 8ull * m; ++w) work[w] = leaves[w];
    for (uint32_t l = 0; l < h; ++l) {
        const uint64_t parents = nodes(a, m, l + 1u);
        for (uint64_t j = 0; j < parents; ++j) {        // in place: parent j is written behind the children of every parent >= j
            const Step s = step(a, m, c, l, j);
            if (s.lsrc != FROM_LEVEL) reads(s.lsrc, l);
            if (s.rsrc != FROM_LEVEL) reads(s.rsrc, l);
            uint32_t x[8], y[8], out[8];
            const uint32_t* xs = s.lsrc == FROM_LEVEL ? work + 8ull * s.lk : (s.lsrc == FROM_LEFT ? left_row : right_row) + 8u * l;
            const uint32_t* ys = s.rsrc == FROM_LEVEL ? work + 8ull * s.rk : (s.rsrc == FROM_LEFT ? left_row : right_row) + 8u * l;
            for (int w = 0; w < 8; ++w) { x[w] = xs[w]; y[w] = ys[w]; }
            pair(x, y, out);
            for (int w = 0; w < 8; ++w) work[8ull * j + w] = out[w];
        }
    }
    if (!vkmr_absence::equal(work, root)) return no;
    return Verdict{1u, a + (f.below ? 1ull : 0ull), m - (f.below ? 1ull : 0ull) - (f.above ? 1ull : 0ull)};
}

}  // namespace vkmr_range
