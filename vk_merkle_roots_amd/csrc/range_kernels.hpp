// range_kernels.hpp -- sorted trees: every leaf between two digests, and the proof that none was left out (include/vkmr_hip.h:
// vkmr_hip_forest_range_async, vkmr_hip_verify_forest_range_async and their one-tree twins; the rules: range_plan.hpp).
//   *_range_runs_kernel     a lane per query: the two bound loops; first, m, the height, the workgroup's sum of m in 64 bits
//   range_starts_kernel     one workgroup: the exclusive prefix over the workgroups' sums in 64 bits, the total, the status
//   range_places_kernel     a lane per query: leaf_starts[q], m replaced in place
//   *_range_leaves_kernel   a lane per carried leaf: its query by a search of leaf_starts, one 32-byte load, one 32-byte store
//   *_range_rows_kernel     a lane per (query, level), blockIdx.y the level: the two row cells out of the stored levels
//   *_range_heads_kernel    the check, a lane per query: what is refused, the fences, the canonical shape, in_first / in_count
//   range_order_kernel      the check, a lane per carried leaf against the one in front of it
//   *_range_level_kernel    the fold, ONE LAUNCH PER LEVEL, a lane per cell of the level's buffer (a node of some range or nothing):
//                           the one kernel that hashes, through ONE hash_pair whose operands are selected as pointers
//   *_range_verdict_kernel  a lane per query: the top against the root
// None waits for another workgroup, none has a private segment.  A forest and one tree differ in where a query's tree lies and in
// what a proof is checked against: absence_kernels.hpp's structs, with the query's tree optional.
#pragma once

#include "absence_kernels.hpp"
#include "range_plan.hpp"

static_assert(VKMR_RANGE_THREADS == 256, "four wavefronts: range_block_exclusive's s_wave");

// Exclusive prefix of `v` over the workgroup's lanes in 64 bits; *total = the workgroup's sum.  vkmr_sizes::block_exclusive with
// wider words: a run may be a whole tree, and 256 of them do not fit 32 bits.
__device__ __forceinline__ uint64_t range_block_exclusive(uint64_t v, uint64_t* s_wave, uint64_t* total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned long long incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long o = __shfl_up(incl, d);
        if (lane >= (uint32_t)d) incl += o;
    }
    if (lane == 63u) s_wave[wave] = incl;
    __syncthreads();
    uint64_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < VKMR_RANGE_THREADS / 64; ++w) {
        const uint64_t t = s_wave[w];
        before += (uint32_t)w < wave ? t : 0ull;
        all += t;
    }
    *total = all;
    return before + incl - v;
}

// ---- the gather: no hash ---------------------------------------------------------------------------------------------------------------

// Lane q <= Q (lane Q carries nothing: it is leaf_starts[Q]'s).  info[2] += queries refused, info[3] += leaves in range; the host
// zeroed them.  Every lane of a workgroup reaches the prefix.
template <class Where>
__device__ __forceinline__ void range_runs(const Where w, const Node* __restrict__ digests, const Node* __restrict__ lo, const Node* __restrict__ hi,
                                           uint32_t Q, uint64_t* __restrict__ firsts, uint64_t* __restrict__ leaf_starts, uint32_t* __restrict__ heights,
                                           uint64_t* __restrict__ sums, unsigned long long* __restrict__ info)
{
    __shared__ uint64_t s_wave[VKMR_RANGE_THREADS / 64];
    const uint64_t q = (uint64_t)blockIdx.x * VKMR_RANGE_THREADS + threadIdx.x;
    vkmr_range::Run r{0ull, 0ull, 0u, 0ull};
    if (q < Q) {
        uint32_t t;
        uint64_t o = 0ull, c = 0ull;
        const bool known = w.tree(q, t, o, c);
        const Node x = vkmr_dev::load_node(lo + q), y = vkmr_dev::load_node(hi + q);
        const Node* leaves = digests + o;
        r = vkmr_range::run(
            known, c, x.w, y.w, [&](uint64_t i, const uint32_t* z) { return vkmr_absence::less(vkmr_dev::load_node(leaves + i).w, z); },
            [&](uint64_t i, const uint32_t* z) { return vkmr_absence::equal(vkmr_dev::load_node(leaves + i).w, z); });
        firsts[q] = r.first;
        if (heights) heights[q] = r.height;
    }
    if (q <= Q) leaf_starts[q] = r.m;
    uint64_t total;
    (void)range_block_exclusive(r.m, s_wave, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
    const uint64_t n_refused = __popcll(__ballot(q < Q && r.first == vkmr_range::NONE));
    unsigned long long inside = r.inside;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) inside += __shfl_xor(inside, d);
    if ((threadIdx.x & 63u) != 0u) return;
    if (n_refused) (void)__hip_atomic_fetch_add(info + 2, (unsigned long long)n_refused, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (inside) (void)__hip_atomic_fetch_add(info + 3, inside, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(VKMR_RANGE_THREADS) void forest_range_runs_kernel(const Node* __restrict__ digests, const uint64_t* __restrict__ offsets,
                                                                               uint32_t ntrees, uint64_t total, const uint32_t* __restrict__ trees,
                                                                               const Node* __restrict__ lo, const Node* __restrict__ hi, uint32_t Q,
                                                                               uint64_t* __restrict__ firsts, uint64_t* __restrict__ leaf_starts,
                                                                               uint32_t* __restrict__ heights, uint64_t* __restrict__ sums,
                                                                               unsigned long long* __restrict__ info)
{
    range_runs(AbsenceForest{offsets, ntrees, total, trees}, digests, lo, hi, Q, firsts, leaf_starts, heights, sums, info);
}

__global__ __launch_bounds__(VKMR_RANGE_THREADS) void tree_range_runs_kernel(const Node* __restrict__ digests, uint64_t count, const Node* __restrict__ lo,
                                                                             const Node* __restrict__ hi, uint32_t Q, uint64_t* __restrict__ firsts,
                                                                             uint64_t* __restrict__ leaf_starts, uint64_t* __restrict__ sums,
                                                                             unsigned long long* __restrict__ info)
{
    range_runs(AbsenceTree{count}, digests, lo, hi, Q, firsts, leaf_starts, nullptr, sums, info);
}

// One workgroup: sums[0 .. groups) becomes its exclusive prefix; info[1] = the leaves carried, info[0] bit 0 when they exceed capacity.
// Each sum is at most 256 * 2^58 and the total at most 2^32 * 2^58: the host holds Q * max_count below 2^63, so nothing wraps.
__global__ __launch_bounds__(VKMR_RANGE_THREADS) void range_starts_kernel(uint64_t* __restrict__ sums, uint64_t groups, uint64_t capacity,
                                                                          unsigned long long* __restrict__ info)
{
    __shared__ uint64_t s_wave[VKMR_RANGE_THREADS / 64];
    uint64_t carry = 0;
    for (uint64_t base = 0; base < groups; base += VKMR_RANGE_THREADS) {   // wave-uniform trip count
        const uint64_t i = base + threadIdx.x;
        const uint64_t x = i < groups ? sums[i] : 0ull;
        uint64_t total;
        const uint64_t start = carry + range_block_exclusive(x, s_wave, &total);
        if (i < groups) sums[i] = start;
        carry += total;
        __syncthreads();                         // s_wave is reused by the next round
    }
    if (threadIdx.x == 0) {
        info[1] = carry;
        info[0] = carry > capacity ? VKMR_RANGE_LEAVES_CAPACITY : 0ull;
    }
}

__global__ __launch_bounds__(VKMR_RANGE_THREADS) void range_places_kernel(const uint64_t* __restrict__ sums, uint32_t Q, uint64_t* __restrict__ leaf_starts)
{
    __shared__ uint64_t s_wave[VKMR_RANGE_THREADS / 64];
    const uint64_t q = (uint64_t)blockIdx.x * VKMR_RANGE_THREADS + threadIdx.x;
    const uint64_t m = q <= Q ? leaf_starts[q] : 0ull;
    uint64_t total;
    const uint64_t start = sums[blockIdx.x] + range_block_exclusive(m, s_wave, &total);
    if (q <= Q) leaf_starts[q] = start;
}

// Lane j < leaf_starts[Q] <= capacity (the status is 0): leaf j of the output is leaf first + (j - leaf_starts[q]) of its query's tree,
// inside the tree by the plan's first + m <= c.
template <class Where>
__device__ __forceinline__ void range_leaves(const Where w, const Node* __restrict__ digests, uint32_t Q, const uint64_t* __restrict__ firsts,
                                             const uint64_t* __restrict__ leaf_starts, const unsigned long long* __restrict__ info, Node* __restrict__ leaves)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (info[0] != 0ull || j >= info[1]) return;
    const uint64_t q = vkmr_range::query_of_leaf(j, Q, [&](uint64_t i) { return leaf_starts[i]; });
    uint32_t t;
    uint64_t o, c;
    if (!w.tree(q, t, o, c)) return;             // a refused query carries nothing: not reached
    vkmr_dev::store_node(leaves + j, vkmr_dev::load_node(digests + o + firsts[q] + (j - leaf_starts[q])));
}

__global__ __launch_bounds__(256) void forest_range_leaves_kernel(const Node* __restrict__ digests, const uint64_t* __restrict__ offsets, uint32_t ntrees,
                                                                  uint64_t total, const uint32_t* __restrict__ trees, uint32_t Q,
                                                                  const uint64_t* __restrict__ firsts, const uint64_t* __restrict__ leaf_starts,
                                                                  const unsigned long long* __restrict__ info, Node* __restrict__ leaves)
{
    range_leaves(AbsenceForest{offsets, ntrees, total, trees}, digests, Q, firsts, leaf_starts, info, leaves);
}

__global__ __launch_bounds__(256) void tree_range_leaves_kernel(const Node* __restrict__ digests, uint64_t count, uint32_t Q,
                                                                const uint64_t* __restrict__ firsts, const uint64_t* __restrict__ leaf_starts,
                                                                const unsigned long long* __restrict__ info, Node* __restrict__ leaves)
{
    range_leaves(AbsenceTree{count}, digests, Q, firsts, leaf_starts, info, leaves);
}

// Lane (q, l = blockIdx.y): cell q * stride + l of both rows, a node where the plan's left_cell() / right_cell() say so and zero
// otherwise.  m is leaf_starts[q + 1] - leaf_starts[q]; the nodes named exist: (a >> l) - 1 >= 0, (b >> l) + 1 < the level's cells.
template <class Where, class Cells>
__device__ __forceinline__ void range_rows(const Where w, const Cells cells, const uint64_t* __restrict__ firsts, const uint64_t* __restrict__ leaf_starts,
                                           uint32_t Q, uint32_t stride, Node* __restrict__ left_row, Node* __restrict__ right_row)
{
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= Q) return;
    const uint32_t l = blockIdx.y;
    uint32_t t;
    uint64_t o, c;
    Node lf = {}, rt = {};
    const uint64_t m = leaf_starts[q + 1ull] - leaf_starts[q];
    if (w.tree(q, t, o, c) && m > 0ull) {
        const uint64_t a = firsts[q], b = a + m - 1ull;
        const uint32_t h = vkmr_absence::height(c);
        if (vkmr_range::left_cell(a, l, h)) lf = vkmr_dev::load_node(cells.node_cell(t, l, (a >> l) - 1ull));
        if (vkmr_range::right_cell(b, c, l, h)) rt = vkmr_dev::load_node(cells.node_cell(t, l, (b >> l) + 1ull));
    }
    vkmr_dev::store_node(left_row + q * stride + l, lf);
    vkmr_dev::store_node(right_row + q * stride + l, rt);
}

__global__ __launch_bounds__(256) void forest_range_rows_kernel(const Node* __restrict__ digests, const Node* __restrict__ forest, ForestLevels lv,
                                                                const uint64_t* __restrict__ offsets, uint32_t ntrees, uint64_t total,
                                                                const uint32_t* __restrict__ trees, const uint64_t* __restrict__ firsts,
                                                                const uint64_t* __restrict__ leaf_starts, uint32_t Q, uint32_t stride,
                                                                Node* __restrict__ left_row, Node* __restrict__ right_row)
{
    range_rows(AbsenceForest{offsets, ntrees, total, trees}, ForestCells{digests, forest, lv, offsets}, firsts, leaf_starts, Q, stride, left_row, right_row);
}

__global__ __launch_bounds__(256) void tree_range_rows_kernel(const Node* __restrict__ digests, const Node* __restrict__ tree, TreeLevels lv, uint64_t count,
                                                              const uint64_t* __restrict__ firsts, const uint64_t* __restrict__ leaf_starts, uint32_t Q,
                                                              uint32_t stride, Node* __restrict__ left_row, Node* __restrict__ right_row)
{
    range_rows(AbsenceTree{count}, TreeCells{digests, tree, lv, count}, firsts, leaf_starts, Q, stride, left_row, right_row);
}

// ---- the check -------------------------------------------------------------------------------------------------------------------------

// What a query is checked against: absence_kernels.hpp's claims; one tree's queries name no tree.
struct RangeForestClaims {
    const uint32_t* trees; const uint32_t* heights; const Node* roots; const uint64_t* counts; uint32_t ntrees;
    __device__ __forceinline__ bool claim(uint64_t q, uint32_t& h, uint64_t& c) const
    {
        const uint32_t t = trees[q];
        h = heights[q];
        if (t >= ntrees) return false;
        c = counts[t];
        return true;
    }
    __device__ __forceinline__ const Node* root(uint64_t q) const { return roots + trees[q]; }      // after claim() said yes
};
struct RangeTreeClaims {
    uint32_t height; const Node* root_cell; uint64_t count;
    __device__ __forceinline__ bool claim(uint64_t, uint32_t& h, uint64_t& c) const
    {
        h = height;
        c = count;
        return true;
    }
    __device__ __forceinline__ const Node* root(uint64_t) const { return root_cell; }
};

// A lane per query: ok[q] = 1 when nothing is refused and the fences and the shape hold; in_first / in_count on that footing.  *bad
// (zeroed by the host) is set when leaf_starts is no prefix over [0, nleaves]: the searches of the other kernels rest on that, and
// every verdict is then 0.  A lane loads leaves only behind the refusals: cells leaf_starts[q] .. leaf_starts[q + 1] - 1 < nleaves.
template <class Claims>
__device__ __forceinline__ void range_heads(const Claims claims, const Node* __restrict__ lo, const Node* __restrict__ hi, const uint64_t* __restrict__ firsts,
                                            const uint64_t* __restrict__ leaf_starts, const Node* __restrict__ leaves, uint64_t nleaves, uint32_t Q,
                                            uint32_t stride, uint32_t* __restrict__ bad, uint32_t* __restrict__ ok, uint64_t* __restrict__ in_first,
                                            uint64_t* __restrict__ in_count)
{
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= Q) return;
    const uint64_t s0 = leaf_starts[q], s1 = leaf_starts[q + 1ull];
    const bool prefix = s0 <= s1 && s1 <= nleaves;
    if (!prefix) *bad = 1u;
    uint32_t h = 0u;
    uint64_t c = 0ull;
    const bool known = claims.claim(q, h, c);
    const uint64_t a = firsts[q], m = prefix ? s1 - s0 : 0ull;
    const Node x = vkmr_dev::load_node(lo + q), y = vkmr_dev::load_node(hi + q);
    bool good = prefix && !vkmr_range::refused(known ? 0u : 1u, 1u, h, stride, c, a, m, x.w, y.w);
    uint64_t first = 0ull, count = 0ull;
    if (good && c > 0ull) {
        const Node* run = leaves + s0;
        const Node f0 = vkmr_dev::load_node(run), f1 = vkmr_dev::load_node(run + (m >= 2ull ? 1ull : 0ull));
        const Node l1 = vkmr_dev::load_node(run + (m >= 2ull ? m - 2ull : 0ull)), l0 = vkmr_dev::load_node(run + (m - 1ull));
        const vkmr_range::Fences f = vkmr_range::fences(a, m, c, x.w, y.w, f0.w, f1.w, l1.w, l0.w);
        good = f.ok;
        first = a + (f.below ? 1ull : 0ull);
        count = m - (f.below ? 1ull : 0ull) - (f.above ? 1ull : 0ull);
    }
    ok[q] = good ? 1u : 0u;
    in_first[q] = good ? first : 0ull;
    in_count[q] = good ? count : 0ull;
}

__global__ __launch_bounds__(256) void forest_range_heads_kernel(const uint32_t* __restrict__ trees, const uint32_t* __restrict__ heights,
                                                                 const Node* __restrict__ roots, const uint64_t* __restrict__ counts, uint32_t ntrees,
                                                                 const Node* __restrict__ lo, const Node* __restrict__ hi,
                                                                 const uint64_t* __restrict__ firsts, const uint64_t* __restrict__ leaf_starts,
                                                                 const Node* __restrict__ leaves, uint64_t nleaves, uint32_t Q, uint32_t stride,
                                                                 uint32_t* __restrict__ bad, uint32_t* __restrict__ ok, uint64_t* __restrict__ in_first,
                                                                 uint64_t* __restrict__ in_count)
{
    range_heads(RangeForestClaims{trees, heights, roots, counts, ntrees}, lo, hi, firsts, leaf_starts, leaves, nleaves, Q, stride, bad, ok, in_first, in_count);
}

__global__ __launch_bounds__(256) void tree_range_heads_kernel(uint32_t height, const Node* __restrict__ root, uint64_t count, const Node* __restrict__ lo,
                                                               const Node* __restrict__ hi, const uint64_t* __restrict__ firsts,
                                                               const uint64_t* __restrict__ leaf_starts, const Node* __restrict__ leaves, uint64_t nleaves,
                                                               uint32_t Q, uint32_t* __restrict__ bad, uint32_t* __restrict__ ok,
                                                               uint64_t* __restrict__ in_first, uint64_t* __restrict__ in_count)
{
    range_heads(RangeTreeClaims{height, root, count}, lo, hi, firsts, leaf_starts, leaves, nleaves, Q, height, bad, ok, in_first, in_count);
}

// Behind the heads, a lane per carried leaf 1 <= j < nleaves: where leaf j is not its run's first and is not above leaf j - 1, the
// run's query is not proven.  Lanes only ever store 0 over the heads' 1.  With *bad set the search may name any query: all are 0 then.
__global__ __launch_bounds__(256) void range_order_kernel(const uint64_t* __restrict__ leaf_starts, const Node* __restrict__ leaves, uint64_t nleaves,
                                                          uint32_t Q, uint32_t* __restrict__ ok)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x + 1ull;
    if (j >= nleaves || j >= leaf_starts[Q]) return;
    const Node before = vkmr_dev::load_node(leaves + (j - 1ull)), mine = vkmr_dev::load_node(leaves + j);
    if (vkmr_absence::less(before.w, mine.w)) return;
    const uint64_t q = vkmr_range::query_of_leaf(j, Q, [&](uint64_t i) { return leaf_starts[i]; });
    if (leaf_starts[q] != j) ok[q] = 0u;
}

// The fold from level l to l + 1: lane i is cell i of level l + 1's buffer, the parent j of some query or nothing.  Level 0 is the
// carried leaves; a query's last parent, at level H, goes to tops[q].  The plan's step() says where the two children come from; the
// choice is made on the pointers, then two loads and the kernel's one hash_pair.  Every address lies in the query's own cells of the
// two buffers (range_plan.hpp), in its own row cells l < H <= stride, or in its own run of the leaves.
template <class Claims>
__device__ __forceinline__ void range_level(const Claims claims, const uint64_t* __restrict__ firsts, const uint64_t* __restrict__ leaf_starts,
                                            const Node* __restrict__ leaves, uint64_t nleaves, const Node* __restrict__ left_row,
                                            const Node* __restrict__ right_row, uint32_t Q, uint32_t stride, uint32_t l, const uint32_t* __restrict__ bad,
                                            const uint32_t* __restrict__ ok, const Node* __restrict__ in, Node* __restrict__ out, Node* __restrict__ tops)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (*bad != 0u || i >= vkmr_range::level_cells(nleaves, Q, l + 1u)) return;
    const uint64_t q = vkmr_range::query_of_cell(i, l + 1u, nleaves, Q, [&](uint64_t k) { return leaf_starts[k]; });
    if (ok[q] == 0u) return;
    uint32_t h = 0u;
    uint64_t c = 0ull;
    (void)claims.claim(q, h, c);                  // ok[q]: it has a tree, h == H(c) <= stride, first + m <= c
    if (l >= h) return;
    const uint64_t s0 = leaf_starts[q], a = firsts[q], m = leaf_starts[q + 1ull] - s0;
    const uint64_t j = i - vkmr_range::level_cell(s0, q, l + 1u, 0ull);
    if (j >= vkmr_range::nodes(a, m, l + 1u)) return;
    const vkmr_range::Step s = vkmr_range::step(a, m, c, l, j);
    const Node* level = l == 0u ? leaves + s0 : in + vkmr_range::level_cell(s0, q, l, 0ull);
    const Node* lrow = left_row + q * stride + l;
    const Node* rrow = right_row + q * stride + l;
    const Node* xs = s.lsrc == vkmr_range::FROM_LEVEL ? level + s.lk : lrow;
    const Node* ys = s.rsrc == vkmr_range::FROM_LEVEL ? level + s.rk : (s.rsrc == vkmr_range::FROM_RIGHT ? rrow : lrow);
    const Node x = vkmr_dev::load_node(xs), y = vkmr_dev::load_node(ys);
    uint32_t o[8];
    vkmr_dev::hash_pair(x.w, y.w, o);
    vkmr_dev::store_node(l + 1u == h ? tops + q : out + i, o);
}

__global__ __launch_bounds__(256) void forest_range_level_kernel(const uint32_t* __restrict__ trees, const uint32_t* __restrict__ heights,
                                                                 const uint64_t* __restrict__ counts, uint32_t ntrees,
                                                                 const uint64_t* __restrict__ firsts, const uint64_t* __restrict__ leaf_starts,
                                                                 const Node* __restrict__ leaves, uint64_t nleaves, const Node* __restrict__ left_row,
                                                                 const Node* __restrict__ right_row, uint32_t Q, uint32_t stride, uint32_t l,
                                                                 const uint32_t* __restrict__ bad, const uint32_t* __restrict__ ok,
                                                                 const Node* __restrict__ in, Node* __restrict__ out, Node* __restrict__ tops)
{
    range_level(RangeForestClaims{trees, heights, nullptr, counts, ntrees}, firsts, leaf_starts, leaves, nleaves, left_row, right_row, Q, stride, l, bad, ok,
                in, out, tops);
}

__global__ __launch_bounds__(256) void tree_range_level_kernel(uint32_t height, uint64_t count, const uint64_t* __restrict__ firsts,
                                                               const uint64_t* __restrict__ leaf_starts, const Node* __restrict__ leaves, uint64_t nleaves,
                                                               const Node* __restrict__ left_row, const Node* __restrict__ right_row, uint32_t Q, uint32_t l,
                                                               const uint32_t* __restrict__ bad, const uint32_t* __restrict__ ok,
                                                               const Node* __restrict__ in, Node* __restrict__ out, Node* __restrict__ tops)
{
    range_level(RangeTreeClaims{height, nullptr, count}, firsts, leaf_starts, leaves, nleaves, left_row, right_row, Q, height, l, bad, ok, in, out, tops);
}

// Behind the last level, a lane per query: 1 when ok[q] and the top is the root (a tree without a leaf: the root is all zero).
template <class Claims>
__device__ __forceinline__ void range_verdict(const Claims claims, uint32_t Q, const uint32_t* __restrict__ bad, const uint32_t* __restrict__ ok,
                                              const Node* __restrict__ tops, uint32_t* __restrict__ verdict, uint64_t* __restrict__ in_first,
                                              uint64_t* __restrict__ in_count)
{
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= Q) return;
    bool good = *bad == 0u && ok[q] != 0u;
    if (good) {
        uint32_t h = 0u;
        uint64_t c = 0ull;
        (void)claims.claim(q, h, c);
        const Node zero = {};
        const Node root = vkmr_dev::load_node(claims.root(q));
        const Node top = c == 0ull ? zero : vkmr_dev::load_node(tops + q);
        good = vkmr_dev::node_diff(top, root) == 0u;
    }
    verdict[q] = good ? 1u : 0u;
    if (!good) {
        in_first[q] = 0ull;
        in_count[q] = 0ull;
    }
}

__global__ __launch_bounds__(256) void forest_range_verdict_kernel(const uint32_t* __restrict__ trees, const uint32_t* __restrict__ heights,
                                                                   const Node* __restrict__ roots, const uint64_t* __restrict__ counts, uint32_t ntrees,
                                                                   uint32_t Q, const uint32_t* __restrict__ bad, const uint32_t* __restrict__ ok,
                                                                   const Node* __restrict__ tops, uint32_t* __restrict__ verdict,
                                                                   uint64_t* __restrict__ in_first, uint64_t* __restrict__ in_count)
{
    range_verdict(RangeForestClaims{trees, heights, roots, counts, ntrees}, Q, bad, ok, tops, verdict, in_first, in_count);
}

__global__ __launch_bounds__(256) void tree_range_verdict_kernel(uint32_t height, const Node* __restrict__ root, uint64_t count, uint32_t Q,
                                                                 const uint32_t* __restrict__ bad, const uint32_t* __restrict__ ok,
                                                                 const Node* __restrict__ tops, uint32_t* __restrict__ verdict,
                                                                 uint64_t* __restrict__ in_first, uint64_t* __restrict__ in_count)
{
    range_verdict(RangeTreeClaims{height, root, count}, Q, bad, ok, tops, verdict, in_first, in_count);
}
