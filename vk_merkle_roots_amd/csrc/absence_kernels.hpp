// absence_kernels.hpp -- sorted trees: is a stored tree strictly increasing, where would a digest stand in it, and the proof that
// it is no leaf (include/vkmr_hip.h: vkmr_hip_forest_sorted_async, vkmr_hip_forest_lower_bound_async,
// vkmr_hip_forest_absence_async, vkmr_hip_verify_forest_absence_async and their one-tree twins; the rules: absence_plan.hpp).
//   *_sorted_scan_kernel     bound by memory: a lane per flat position of level 0 compares its cell with the one in front; only an
//                            offending lane looks for its tree and takes an atomic min on the tree's first offence
//   *_sorted_finish_kernel   a lane per tree: the counters, and whether a first offence is an equal pair
//   *_lower_bound_kernel     a lane per query: the plan's loop over the tree's leaves
//   *_absence_entries_kernel a lane per query: the lower bound, then the index, the two neighbours and the height
//   *_absence_rows_kernel    a lane per (query, level): the main and the low row out of the stored levels, entries.hpp's cells
//   *_absence_fold_kernel    a lane per proof, the one kernel that hashes: the low row's fold and the main row's through ONE
//                            hash_pair, operands selected
// A forest and one tree differ in where a query's tree lies and in what a proof is checked against: the structs below, in
// entries.hpp's manner -- one body per kernel, and a __global__ kernel is its arguments as the struct and the call.
#pragma once

#include "absence_plan.hpp"
#include "entries.hpp"

// ---- where the leaves lie ------------------------------------------------------------------------------------------------------------

// Level 0 of a forest: cells [offsets[0], min(offsets[ntrees], total)); the offsets are trusted to be non-decreasing, the end is
// held to `total` all the same, so that no leaf load leaves the buffer (find_kernels.hpp's rule).
struct SortedForest {
    const uint64_t* offsets; uint32_t ntrees; uint64_t total;
    __device__ __forceinline__ uint64_t lo() const { return ntrees ? offsets[0] : 0ull; }
    __device__ __forceinline__ uint64_t hi() const
    {
        if (!ntrees) return 0ull;
        const uint64_t end = offsets[ntrees];
        return end < total ? end : total;
    }
    __device__ __forceinline__ uint32_t trees() const { return ntrees; }
    // Tree t: its first cell, its count, and whether its offsets are none a forest has.
    __device__ __forceinline__ bool span(uint32_t t, uint64_t& o, uint64_t& c) const
    {
        o = offsets[t];
        const uint64_t e = offsets[t + 1u];
        c = e >= o ? e - o : 0ull;
        return e >= o && e <= total;
    }
    // lo() < p < hi() and !(cell[p-1] < cell[p]): the tree of p is the upper bound of p in offsets[0 .. ntrees], minus one.  The
    // pair straddles two trees when p is that tree's first leaf: no offence.  Else the offence is at index p - offsets[t] >= 1.
    __device__ __forceinline__ void offence(uint64_t p, unsigned long long* __restrict__ first_bad) const
    {
        uint32_t a = 1u, b = ntrees;
        while (a < b) {
            const uint32_t mid = a + (b - a) / 2u;
            if (offsets[mid] > p) b = mid;
            else a = mid + 1u;
        }
        const uint64_t o = offsets[a - 1u];
        if (p == o) return;
        const unsigned long long i = p - o;
        // first_bad only ever falls: a read that shows it at or below i, however stale, makes the atomic needless
        if (__hip_atomic_load(first_bad + (a - 1u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > i)
            (void)__hip_atomic_fetch_min(first_bad + (a - 1u), i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

// One tree at cell 0.
struct SortedTree {
    uint64_t count;
    __device__ __forceinline__ uint64_t lo() const { return 0ull; }
    __device__ __forceinline__ uint64_t hi() const { return count; }
    __device__ __forceinline__ uint32_t trees() const { return 1u; }
    __device__ __forceinline__ bool span(uint32_t, uint64_t& o, uint64_t& c) const
    {
        o = 0ull;
        c = count;
        return true;
    }
    __device__ __forceinline__ void offence(uint64_t p, unsigned long long* __restrict__ first_bad) const
    {
        if (__hip_atomic_load(first_bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > p)
            (void)__hip_atomic_fetch_min(first_bad, (unsigned long long)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

// The tree a query names: a forest's trees[q] (none when it is >= ntrees), its leaves held to `total`; one tree's is tree 0.
struct AbsenceForest {
    const uint64_t* offsets; uint32_t ntrees; uint64_t total; const uint32_t* trees;
    __device__ __forceinline__ bool tree(uint64_t q, uint32_t& t, uint64_t& o, uint64_t& c) const
    {
        t = trees[q];
        if (t >= ntrees) return false;
        o = offsets[t];
        const uint64_t e = offsets[t + 1u] < total ? offsets[t + 1u] : total;
        c = e > o ? e - o : 0ull;
        return true;
    }
};
struct AbsenceTree {
    uint64_t count;
    __device__ __forceinline__ bool tree(uint64_t, uint32_t& t, uint64_t& o, uint64_t& c) const
    {
        t = 0u;
        o = 0ull;
        c = count;
        return true;
    }
};

// What a proof is checked against: a forest's roots and counts by the proof's tree and its own height; one tree's by value.
struct AbsenceForestClaims {
    const uint32_t* trees; const uint32_t* heights; const Node* roots; const uint64_t* counts; uint32_t ntrees;
    __device__ __forceinline__ bool claim(uint64_t q, uint32_t& t, uint32_t& h, uint64_t& c) const
    {
        t = trees[q];
        h = heights[q];
        if (t >= ntrees) return false;
        c = counts[t];
        return true;
    }
    __device__ __forceinline__ const Node* root(uint32_t t) const { return roots + t; }
};
struct AbsenceTreeClaims {
    uint32_t height; const Node* root_cell; uint64_t count;
    __device__ __forceinline__ bool claim(uint64_t, uint32_t& t, uint32_t& h, uint64_t& c) const
    {
        t = 0u;
        h = height;
        c = count;
        return true;
    }
    __device__ __forceinline__ const Node* root(uint32_t) const { return root_cell; }
};

// ---- is it sorted? -----------------------------------------------------------------------------------------------------------------

// Lane j takes position p = lo + 1 + j < hi and loads cells p - 1 and p, both inside [lo, hi): a wavefront's two loads cover the
// same 2 KiB but for one cell, so the second is served by the cache.  No hash.
template <class Range>
__device__ __forceinline__ void sorted_scan(const Range r, const Node* __restrict__ digests, unsigned long long* __restrict__ first_bad)
{
    const uint64_t lo = r.lo(), hi = r.hi();           // the same two words in every lane
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (hi <= lo || j >= hi - lo - 1ull) return;
    const uint64_t p = lo + 1ull + j;
    const Node a = vkmr_dev::load_node(digests + (p - 1ull)), b = vkmr_dev::load_node(digests + p);
    if (!vkmr_absence::less(a.w, b.w)) r.offence(p, first_bad);
}

// Behind the scan, a lane per tree.  info[0] |= the status, info[1] += trees not sorted, info[2] += those whose first offence is an
// equal pair, info[3] += pairs compared; the host zeroed them.  Every lane of a wavefront reaches the ballots and the shuffles.
template <class Range>
__device__ __forceinline__ void sorted_finish(const Range r, const Node* __restrict__ digests, const unsigned long long* __restrict__ first_bad,
                                              unsigned long long* __restrict__ info)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = t < r.trees();
    uint64_t o = 0ull, c = 0ull;
    const bool good = in ? r.span((uint32_t)t, o, c) : true;
    const unsigned long long fb = in ? first_bad[t] : vkmr_absence::NONE;
    const bool unsorted = fb != vkmr_absence::NONE;      // then 1 <= fb < c and both cells were loaded by the scan
    bool same = false;
    if (unsorted) same = vkmr_dev::node_diff(vkmr_dev::load_node(digests + (o + fb - 1ull)), vkmr_dev::load_node(digests + (o + fb))) == 0u;
    unsigned long long pairs = (in && good && c >= 2ull) ? c - 1ull : 0ull;
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) pairs += __shfl_xor(pairs, m);
    const uint64_t n_bad = __popcll(__ballot(!good)), n_unsorted = __popcll(__ballot(unsorted)), n_same = __popcll(__ballot(same));
    if ((threadIdx.x & 63u) != 0u) return;
    if (n_bad) (void)__hip_atomic_fetch_or(info, (unsigned long long)VKMR_SORTED_BAD_OFFSETS, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (n_unsorted) (void)__hip_atomic_fetch_add(info + 1, (unsigned long long)n_unsorted, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (n_same) (void)__hip_atomic_fetch_add(info + 2, (unsigned long long)n_same, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (pairs) (void)__hip_atomic_fetch_add(info + 3, pairs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void forest_sorted_scan_kernel(const Node* __restrict__ digests, const uint64_t* __restrict__ offsets, uint32_t ntrees,
                                                                 uint64_t total, unsigned long long* __restrict__ first_bad)
{
    sorted_scan(SortedForest{offsets, ntrees, total}, digests, first_bad);
}

__global__ __launch_bounds__(256) void tree_sorted_scan_kernel(const Node* __restrict__ digests, uint64_t count, unsigned long long* __restrict__ first_bad)
{
    sorted_scan(SortedTree{count}, digests, first_bad);
}

__global__ __launch_bounds__(256) void forest_sorted_finish_kernel(const Node* __restrict__ digests, const uint64_t* __restrict__ offsets, uint32_t ntrees,
                                                                   uint64_t total, const unsigned long long* __restrict__ first_bad,
                                                                   unsigned long long* __restrict__ info)
{
    sorted_finish(SortedForest{offsets, ntrees, total}, digests, first_bad, info);
}

__global__ __launch_bounds__(64) void tree_sorted_finish_kernel(const Node* __restrict__ digests, uint64_t count,
                                                                const unsigned long long* __restrict__ first_bad, unsigned long long* __restrict__ info)
{
    sorted_finish(SortedTree{count}, digests, first_bad, info);
}

// ---- where would it stand? -----------------------------------------------------------------------------------------------------------

// The plan's loop for digest x over the c leaves from `leaves` on: H(c) + 1 dependent loads at the most.
__device__ __forceinline__ uint64_t absence_bound(const Node* __restrict__ leaves, uint64_t c, const Node& x)
{
    return vkmr_absence::lower_bound(c, [&](uint64_t mid) { return vkmr_absence::less(vkmr_dev::load_node(leaves + mid).w, x.w); });
}

// indices[q] = the lower bound of queries[q] in its tree and found[q] = 1 when the leaf there is the query; no tree: NONE and 0.
template <class Where>
__device__ __forceinline__ void absence_lower_bound(const Where w, const Node* __restrict__ digests, const Node* __restrict__ queries, uint32_t Q,
                                                    uint64_t* __restrict__ indices, uint32_t* __restrict__ found)
{
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= Q) return;
    uint32_t t;
    uint64_t o, c, i = vkmr_absence::NONE;
    uint32_t f = 0u;
    if (w.tree(q, t, o, c)) {
        const Node x = vkmr_dev::load_node(queries + q);
        i = absence_bound(digests + o, c, x);
        if (i < c) f = vkmr_dev::node_diff(vkmr_dev::load_node(digests + o + i), x) == 0u ? 1u : 0u;
    }
    indices[q] = i;
    found[q] = f;
}

__global__ __launch_bounds__(256) void forest_lower_bound_kernel(const Node* __restrict__ digests, const uint64_t* __restrict__ offsets, uint32_t ntrees,
                                                                 uint64_t total, const uint32_t* __restrict__ trees, const Node* __restrict__ queries,
                                                                 uint32_t Q, uint64_t* __restrict__ indices, uint32_t* __restrict__ found)
{
    absence_lower_bound(AbsenceForest{offsets, ntrees, total, trees}, digests, queries, Q, indices, found);
}

__global__ __launch_bounds__(256) void tree_lower_bound_kernel(const Node* __restrict__ digests, uint64_t count, const Node* __restrict__ queries, uint32_t Q,
                                                               uint64_t* __restrict__ indices, uint32_t* __restrict__ found)
{
    absence_lower_bound(AbsenceTree{count}, digests, queries, Q, indices, found);
}

// ---- the proof: a gather, no hash -------------------------------------------------------------------------------------------------------

// A lane per query: the index, leaf index - 1 and leaf index (zero cells where there is none) and, for a forest, the height.
template <class Where>
__device__ __forceinline__ void absence_entries(const Where w, const Node* __restrict__ digests, const Node* __restrict__ queries, uint32_t Q,
                                                uint64_t* __restrict__ indices, Node* __restrict__ neighbours, uint32_t* __restrict__ heights)
{
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= Q) return;
    uint32_t t;
    uint64_t o, c, i = vkmr_absence::NONE;
    uint32_t h = 0u;
    Node pred = {}, succ = {};
    if (w.tree(q, t, o, c)) {
        const Node* leaves = digests + o;
        i = absence_bound(leaves, c, vkmr_dev::load_node(queries + q));
        h = vkmr_absence::height(c);
        if (vkmr_absence::has_pred(i)) pred = vkmr_dev::load_node(leaves + (i - 1ull));
        if (vkmr_absence::has_succ(i, c)) succ = vkmr_dev::load_node(leaves + i);
    }
    indices[q] = i;
    vkmr_dev::store_node(neighbours + 2ull * q, pred);
    vkmr_dev::store_node(neighbours + 2ull * q + 1ull, succ);
    if (heights) heights[q] = h;
}

// Behind the entries, a lane per (query, level), i = q * stride + l: main[i] the sibling cell of the anchor at level l, low[i] that
// of leaf index - 1 where the plan's low_cell() says so; zero cells from the tree's height up, for a tree without a leaf and for
// no tree.  Every cell of both rows is written.  index <= c, so the anchor is a leaf; a low cell lies below ctz(index) < H(c) and
// is a left sibling, which exists.
template <class Where, class Cells>
__device__ __forceinline__ void absence_rows(const Where w, const Cells cells, const uint64_t* __restrict__ indices, uint32_t Q, uint32_t stride,
                                             Node* __restrict__ main_row, Node* __restrict__ low_row)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint64_t)Q * stride) return;
    const uint64_t q = i / stride;
    const uint32_t l = (uint32_t)(i - q * stride);
    uint32_t t;
    uint64_t o, c;
    Node m = {}, lw = {};
    if (w.tree(q, t, o, c) && c > 0ull) {
        const uint64_t index = indices[q];
        if (index <= c && l < vkmr_absence::height(c)) {
            m = vkmr_dev::load_node(cells.sibling_cell(t, l, vkmr_absence::anchor(index, c)));
            if (vkmr_absence::low_cell(index, c, l)) lw = vkmr_dev::load_node(cells.sibling_cell(t, l, index - 1ull));
        }
    }
    vkmr_dev::store_node(main_row + i, m);
    vkmr_dev::store_node(low_row + i, lw);
}

__global__ __launch_bounds__(256) void forest_absence_entries_kernel(const Node* __restrict__ digests, const uint64_t* __restrict__ offsets, uint32_t ntrees,
                                                                     uint64_t total, const uint32_t* __restrict__ trees, const Node* __restrict__ queries,
                                                                     uint32_t Q, uint64_t* __restrict__ indices, Node* __restrict__ neighbours,
                                                                     uint32_t* __restrict__ heights)
{
    absence_entries(AbsenceForest{offsets, ntrees, total, trees}, digests, queries, Q, indices, neighbours, heights);
}

__global__ __launch_bounds__(256) void tree_absence_entries_kernel(const Node* __restrict__ digests, uint64_t count, const Node* __restrict__ queries,
                                                                   uint32_t Q, uint64_t* __restrict__ indices, Node* __restrict__ neighbours)
{
    absence_entries(AbsenceTree{count}, digests, queries, Q, indices, neighbours, nullptr);
}

__global__ __launch_bounds__(256) void forest_absence_rows_kernel(const Node* __restrict__ digests, const Node* __restrict__ forest, ForestLevels lv,
                                                                  const uint64_t* __restrict__ offsets, uint32_t ntrees, uint64_t total,
                                                                  const uint32_t* __restrict__ trees, const uint64_t* __restrict__ indices, uint32_t Q,
                                                                  uint32_t stride, Node* __restrict__ main_row, Node* __restrict__ low_row)
{
    absence_rows(AbsenceForest{offsets, ntrees, total, trees}, ForestCells{digests, forest, lv, offsets}, indices, Q, stride, main_row, low_row);
}

__global__ __launch_bounds__(256) void tree_absence_rows_kernel(const Node* __restrict__ digests, const Node* __restrict__ tree, TreeLevels lv, uint64_t count,
                                                                const uint64_t* __restrict__ indices, uint32_t Q, uint32_t stride,
                                                                Node* __restrict__ main_row, Node* __restrict__ low_row)
{
    absence_rows(AbsenceTree{count}, TreeCells{digests, tree, lv, count}, indices, Q, stride, main_row, low_row);
}

// ---- the check -------------------------------------------------------------------------------------------------------------------------

// A lane per proof: absence_plan.hpp's verdict().  The compares come first and leave pointers behind, so that neither the query nor
// a neighbour stays in registers over the loop.  A lane then has n = H(c) + top steps (top = 0 unless the proof is two-sided):
// steps below top fold the predecessor with low[s] in front of it; at step top the value must be main[top], and the anchor takes
// its place; the steps from there fold the anchor with main[s - top] on the side the anchor's bit says.  The loop runs while any
// lane of the wavefront has a step left -- a ballot, so its trip count is wave-uniform and its one hash_pair is the kernel's only
// hash block -- and a lane that is through keeps its value by a select and loads its anchor's cell again, nothing behind its rows.
template <class Claims>
__device__ __forceinline__ void absence_fold(const Claims claims, const Node* __restrict__ queries, const uint64_t* __restrict__ indices,
                                             const Node* __restrict__ neighbours, const Node* __restrict__ main_row, const Node* __restrict__ low_row,
                                             uint32_t Q, uint32_t stride, uint32_t* __restrict__ verdict)
{
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= Q) return;
    const uint64_t index = indices[q];
    uint32_t t = 0u, h = 0u;
    uint64_t c = 0ull;
    bool ok = claims.claim(q, t, h, c) && vkmr_absence::checkable(0u, 1u, h, c, index, stride);
    const Node* pred_cell = neighbours + 2ull * q;
    const Node* succ_cell = pred_cell + 1;
    bool present = false;
    if (ok && c > 0ull) {
        const Node x = vkmr_dev::load_node(queries + q);
        if (vkmr_absence::has_succ(index, c)) {
            const Node succ = vkmr_dev::load_node(succ_cell);
            present = vkmr_absence::equal(x.w, succ.w);
            ok = present || vkmr_absence::less(x.w, succ.w);
        }
        if (!present && vkmr_absence::has_pred(index)) {
            const Node pred = vkmr_dev::load_node(pred_cell);
            ok = ok && vkmr_absence::less(pred.w, x.w);
        }
    }
    const bool fold = ok && c > 0ull;
    const bool two = fold && !present && vkmr_absence::two_sided(index, c);
    const uint32_t tp = two ? vkmr_absence::top(index) : 0u;         // < h: index < c <= 2^h
    const uint32_t n = fold ? h + tp : 0u;
    const uint64_t a = fold ? vkmr_absence::anchor(index, c) : 0ull;
    const Node* anchor_cell = (fold && !vkmr_absence::has_succ(index, c)) ? pred_cell : succ_cell;
    const Node* mrow = main_row + q * stride;
    const Node* lrow = low_row + q * stride;
    Node cur = vkmr_dev::load_node(two ? pred_cell : anchor_cell);
    for (uint32_t s = 0; __ballot(s < n) != 0ull; ++s) {
        const bool live = s < n;
        if (live && two && s == tp) {                                  // the predecessor has arrived at level top
            if (vkmr_dev::node_diff(cur, vkmr_dev::load_node(mrow + tp)) != 0u) ok = false;
            cur = vkmr_dev::load_node(anchor_cell);
        }
        const bool in_low = s < tp;
        const uint32_t l = in_low ? s : s - tp;
        const Node sib = vkmr_dev::load_node(live ? (in_low ? lrow : mrow) + l : anchor_cell);
        const bool right = in_low || ((a >> (l & 63u)) & 1ull);
        uint32_t u[8], v[8], x[8];
#pragma unroll
        for (int w = 0; w < 8; ++w) {
            u[w] = right ? sib.w[w] : cur.w[w];
            v[w] = right ? cur.w[w] : sib.w[w];
        }
        vkmr_dev::hash_pair(u, v, x);
#pragma unroll
        for (int w = 0; w < 8; ++w) cur.w[w] = live ? x[w] : cur.w[w];
    }
    uint32_t out = VKMR_ABSENCE_NOT_PROVEN;
    if (ok) {
        const Node root = vkmr_dev::load_node(claims.root(t));
        if (c == 0ull) {
            const Node zero = {};
            out = vkmr_dev::node_diff(root, zero) == 0u ? VKMR_ABSENCE_ABSENT : VKMR_ABSENCE_NOT_PROVEN;
        } else if (vkmr_dev::node_diff(cur, root) == 0u) {
            out = present ? VKMR_ABSENCE_PRESENT : VKMR_ABSENCE_ABSENT;
        }
    }
    verdict[q] = out;
}

__global__ __launch_bounds__(256) void forest_absence_fold_kernel(const Node* __restrict__ queries, const uint32_t* __restrict__ trees,
                                                                  const uint64_t* __restrict__ indices, const Node* __restrict__ neighbours,
                                                                  const Node* __restrict__ main_row, const Node* __restrict__ low_row,
                                                                  const uint32_t* __restrict__ heights, uint32_t Q, uint32_t stride,
                                                                  const Node* __restrict__ roots, const uint64_t* __restrict__ counts, uint32_t ntrees,
                                                                  uint32_t* __restrict__ verdict)
{
    absence_fold(AbsenceForestClaims{trees, heights, roots, counts, ntrees}, queries, indices, neighbours, main_row, low_row, Q, stride, verdict);
}

__global__ __launch_bounds__(256) void tree_absence_fold_kernel(const Node* __restrict__ queries, const uint64_t* __restrict__ indices,
                                                                const Node* __restrict__ neighbours, const Node* __restrict__ main_row,
                                                                const Node* __restrict__ low_row, uint32_t Q, uint32_t height, const Node* __restrict__ root,
                                                                uint64_t count, uint32_t* __restrict__ verdict)
{
    absence_fold(AbsenceTreeClaims{height, root, count}, queries, indices, neighbours, main_row, low_row, Q, height, verdict);
}
