// forest_kernels.hpp -- roots of many trees of unequal size in one call (include/vkmr_hip.h: vkmr_hip_reduce_forest_async).
//
// The leaves of all trees lie back to back; offsets[t] .. offsets[t+1] are tree t's.  One launch per level, one lane per
// cell of that level's buffer across the whole forest -- reduce_level_kernel's form, so every lane hashes wherever the work
// is -- with one addition: a lane must learn which tree its cell belongs to.  Level l of tree t starts at cell
// pos_l(t) = (offsets[t] >> l) + t (forest_plan.hpp: no prefix sum, no overlap, under one idle cell per tree and level), and
// pos_l grows strictly with t, so the tree is found by binary search over the offsets alone:
//   per wavefront  the tree t0 of its first cell, a wave-uniform search (about log2(ntrees) loads of one address each);
//                  when tree t0 + 1 starts behind the wavefront's 64 cells -- every wavefront inside a tree of more than
//                  64 << l leaves -- all lanes have t0 and nothing else is searched
//   per lane       otherwise lane i has one of t0 .. t0 + i (every tree takes at least one cell): at most 6 more steps
// A tree whose level h_t = max(1, ceil(log2 c_t)) has been formed writes that node to roots[t] instead of the level buffer
// and takes no part in later launches; an empty tree gets its all-zero root from the lane of its reserved cell at level 1.
#pragma once

#include "forest_plan.hpp"

// No hash: bit 0 when offsets[t+1] < offsets[t] or the last offset is past `total`, bit 1 when a tree holds more than
// max_count leaves.  ORed into *status (zeroed by the host); the level kernels read it first and do nothing when it is
// nonzero, so they never follow an offset that was not checked.
__global__ __launch_bounds__(256) void forest_check_kernel(const uint64_t* __restrict__ offsets, uint32_t ntrees, uint64_t total, uint64_t max_count,
                                                           uint32_t* __restrict__ status)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ntrees) return;
    const uint64_t lo = offsets[t], hi = offsets[t + 1];
    uint32_t bits = 0u;
    if (hi < lo || (t + 1 == ntrees && hi > total)) bits |= 1u;
    if (hi >= lo && hi - lo > max_count) bits |= 2u;
    if (bits) atomicOr(status, bits);
}

// ---- the search every level kernel of a forest begins with (forest_level below, audit_kernels.hpp) -----------------------------
// The tree of lane `lane`'s cell p0 + lane of level l, p0 the wavefront's first cell; `mixed` (wave-uniform) says that a tree
// begins inside the wavefront, so that its lanes may hold different trees.
struct ForestLane {
    uint32_t t;
    bool mixed;
};

__device__ __forceinline__ ForestLane forest_find_tree(const uint64_t* __restrict__ offsets, uint32_t ntrees, uint32_t l, uint64_t p0, uint32_t lane)
{
    // the tree of the wavefront's first cell: the largest t0 with pos_l(t0) <= p0 (0 when there is none)
    uint32_t t0 = 0, top = ntrees - 1u;
    while (t0 < top) {
        const uint32_t mid = t0 + (top - t0 + 1u) / 2u;
        if (vkmr_forest::pos(offsets[mid], mid, l) <= p0) t0 = mid;
        else top = mid - 1u;
    }
    const uint64_t p = p0 + lane;
    uint32_t t = t0;
    const bool mixed = t0 + 1u < ntrees && vkmr_forest::pos(offsets[t0 + 1u], t0 + 1u, l) <= p0 + 63ull;   // wave-uniform: a tree begins inside the wavefront
    if (mixed) {
        top = (ntrees - 1u - t0 < lane) ? ntrees - 1u : t0 + lane;
        while (t < top) {
            const uint32_t mid = t + (top - t + 1u) / 2u;
            if (vkmr_forest::pos(offsets[mid], mid, l) <= p) t = mid;
            else top = mid - 1u;
        }
    }
    return {t, mixed};
}

// ---- one level of a forest: the body of the three level kernels below ------------------------------------------------------
// Level l >= 1 from level l - 1 (`in`: the leaves for l == 1, else the buffer of level l - 1), `cells` lanes, in entries.hpp's
// manner: one body, and a __global__ kernel is its arguments and the call.  Two compile-time switches say what a lane does with
// the two children of its node once it has found them:
//   HASH     parent = hash_pair(children), stored to the level buffer, or to roots[t] when it is the tree's last (the builds).
//            The check ran first and the body reads *status: the offsets do not decrease and end inside the leaves, so every
//            cell read is one of tree t's own.  Without HASH nothing is stored and there is no status to read: the caller
//            vouches for the offsets (vkmr_hip_forest_proofs_async's rule).
//   COMPARE  the mutation flag (CVE-2012-2459; Bitcoin Core's ComputeMerkleRoot(hashes, &mutated) with the level kept): when
//            both children exist (2j + 1 < n_in -- right_child() reads the last node twice at a ragged edge, and that is no
//            pair) and are equal, bit l - 1 is ORed into mutated[t], zeroed by the host.
// With HASH: one hash_pair, the kernel's only hash block.
//
// The atomics.  A forest of all-equal leaves hits in every lane.  A lane reads mutated[t] first and skips the atomic when its
// bit is there already (a stale read only costs an atomic).  Where every lane of the wavefront has tree t0 -- the search's
// existing wave-uniform case -- the hits are one ballot and the first hit lane alone issues the atomic; where a tree begins
// inside the wavefront each hit lane issues its own, at most 64 to at least 2 addresses.
//
// `base` is the cell the first wavefront begins at: 0 in the kernels that cover a level's whole buffer, the first cell of the
// first new tree in the append's (below), whose `cells` is the end of its range and whose `ntrees` ends with the last new tree.
template <bool HASH, bool COMPARE>
__device__ __forceinline__ void forest_level(const Node* __restrict__ in, const uint64_t* __restrict__ offsets, uint32_t ntrees, uint32_t l, uint64_t base,
                                             uint64_t cells, Node* __restrict__ out, Node* __restrict__ roots, unsigned long long* __restrict__ mutated,
                                             const uint32_t* __restrict__ status)
{
    if constexpr (HASH) {
        if (*status != 0u) return;               // the same word in every lane
    }
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t p0 = base + ((uint64_t)blockIdx.x * (256u / 64u) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6))) * 64ull;
    if (p0 >= cells) return;                     // wave-uniform
    const uint64_t p = p0 + lane;
    const ForestLane at = forest_find_tree(offsets, ntrees, l, p0, lane);
    const uint32_t t = at.t;
    const bool mixed = at.mixed;
    const uint64_t o = offsets[t], c = offsets[t + 1u] - o;
    const uint64_t first = vkmr_forest::pos(o, t, l);
    if (p < first) return;                       // cells in front of tree 0 (offsets[0] > 0)
    const uint64_t j = p - first;                // this lane's node of tree t's level l
    if (c == 0ull) {                             // an empty tree: its reserved cell's lane writes the all-zero root, once
        if constexpr (HASH) {
            if (l == 1u && j == 0ull) {
                const uint32_t zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                vkmr_dev::store_node(roots + t, zero);
            }
        }
        return;
    }
    // without a count-leading-zeros: the tree takes part in level l when l == 1 or level l - 1 still had two nodes, and level l
    // is its last, h_t, when it has one node
    const uint64_t n_in = vkmr_forest::level_count(c, l - 1u), n_out = vkmr_forest::level_count(c, l);
    if ((l > 1u && n_in == 1ull) || j >= n_out) return;   // the tree is done, or the padding behind its nodes
    const Node* level = in + vkmr_forest::pos(o, t, l - 1u);
    const Node a = vkmr_dev::load_node(level + 2 * j), b = vkmr_dev::load_node(level + vkmr_math::right_child(j, n_in));   // hash_parent's loads
    if constexpr (COMPARE) {
        const bool hit = (vkmr_dev::node_diff(a, b) | (uint32_t)(2ull * j + 1ull >= n_in)) == 0u;   // one OR chain, no second branch
        const unsigned long long bit = 1ull << (l - 1u);
        if (mixed) {
            if (hit && !(mutated[t] & bit)) atomicOr(mutated + t, bit);
        } else {                                 // t == t0 in every lane that is still here
            const uint64_t hits = __ballot(hit);
            if (hits != 0ull && lane == (uint32_t)__builtin_ctzll(hits) && !(mutated[t] & bit)) atomicOr(mutated + t, bit);
        }
    }
    if constexpr (HASH) {
        uint32_t x[8];
        vkmr_dev::hash_pair(a.w, b.w, x);
        vkmr_dev::store_node(n_out == 1ull ? roots + t : out + p, x);
    }
}

// The build's level: hash, no compare.
__global__ __launch_bounds__(256) void forest_level_kernel(const Node* __restrict__ in, const uint64_t* __restrict__ offsets, uint32_t ntrees, uint32_t l,
                                                           uint64_t cells, Node* __restrict__ out, Node* __restrict__ roots,
                                                           const uint32_t* __restrict__ status)
{
    forest_level<true, false>(in, offsets, ntrees, l, 0ull, cells, out, roots, nullptr, status);
}

// The flagged build's level (vkmr_hip_reduce_forest_mutated_async, vkmr_hip_reduce_forest_tree_mutated_async): forest_level_kernel
// plus the compare of the two children it holds anyway.
__global__ __launch_bounds__(256) void forest_level_mutated_kernel(const Node* __restrict__ in, const uint64_t* __restrict__ offsets, uint32_t ntrees,
                                                                   uint32_t l, uint64_t cells, Node* __restrict__ out, Node* __restrict__ roots,
                                                                   unsigned long long* __restrict__ mutated, const uint32_t* __restrict__ status)
{
    forest_level<true, true>(in, offsets, ntrees, l, 0ull, cells, out, roots, mutated, status);
}

// The scan of a stored forest (vkmr_hip_forest_tree_mutated_async): the same search, the compare, no hash.  `in` is level l - 1
// as the build or an update left it; a tree is read below its root only, so every cell read is one the build wrote.
__global__ __launch_bounds__(256) void forest_scan_mutated_kernel(const Node* __restrict__ in, const uint64_t* __restrict__ offsets, uint32_t ntrees,
                                                                  uint32_t l, uint64_t cells, unsigned long long* __restrict__ mutated)
{
    forest_level<false, true>(in, offsets, ntrees, l, 0ull, cells, nullptr, nullptr, mutated, nullptr);
}

// ---- appending trees to a stored forest (vkmr_hip_forest_append_async; forest_plan.hpp: append_first_cell, append_end_cell) ----
// Trees first_tree .. first_tree + m - 1, empty at offset `used` until now, take the n_leaves cells behind `used`.  The check,
// the leaves, the offsets, then the build's own level body over the new trees' range of every level.  Every kernel behind the
// check reads *status first and does nothing when it is nonzero.

// No hash, a lane per item i: the new offsets (new_offsets[0] == 0, none decreasing, new_offsets[m] == n_leaves: bit 0; a
// count above max_count: bit 1) for i < m, and the placement (offsets[first_tree + i] == used for every i up to
// ntrees - first_tree, the forest's last offset included: bit 2, value 4).  ORed into *status, zeroed by the host.
__global__ __launch_bounds__(256) void forest_append_check_kernel(const uint64_t* __restrict__ offsets, uint32_t ntrees, uint32_t first_tree, uint64_t used,
                                                                  const uint64_t* __restrict__ new_offsets, uint32_t m, uint64_t n_leaves,
                                                                  uint64_t max_count, uint32_t* __restrict__ status)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t bits = 0u;
    if (i < m) {
        const uint64_t lo = new_offsets[i], hi = new_offsets[i + 1];
        if (hi < lo || (i == 0 && lo != 0ull) || (i + 1 == m && hi != n_leaves)) bits |= 1u;
        if (hi >= lo && hi - lo > max_count) bits |= 2u;
    }
    if (i <= (uint64_t)(ntrees - first_tree) && offsets[first_tree + i] != used) bits |= 4u;
    if (bits) atomicOr(status, bits);
}

// The new leaves into level 0, a lane per leaf (not launched when the caller has put them there).  The check has passed: the
// new offsets end at n_leaves and the host has seen used + n_leaves <= total.
__global__ __launch_bounds__(256) void forest_append_leaves_kernel(Node* __restrict__ digests, uint64_t used, const Node* __restrict__ leaves,
                                                                   uint64_t n_leaves, const uint32_t* __restrict__ status)
{
    if (*status != 0u) return;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_leaves) return;
    const Node x = vkmr_dev::load_node(leaves + i);
    vkmr_dev::store_node(digests + used + i, x.w);
}

// A lane per tree first_tree + i, i < ntrees - first_tree: offsets[first_tree + i + 1], the end of that tree -- of a new one
// used + new_offsets[i + 1], of every tree still empty behind them used + n_leaves.  offsets[first_tree] stays `used`.  With
// `mutated` the mask of a new tree is zeroed here, so that a refused append leaves the masks alone as well.
__global__ __launch_bounds__(256) void forest_append_offsets_kernel(uint64_t* __restrict__ offsets, uint32_t ntrees, uint32_t first_tree, uint64_t used,
                                                                    const uint64_t* __restrict__ new_offsets, uint32_t m,
                                                                    unsigned long long* __restrict__ mutated, const uint32_t* __restrict__ status)
{
    if (*status != 0u) return;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint64_t)(ntrees - first_tree)) return;
    offsets[first_tree + i + 1] = used + new_offsets[i < m ? i + 1 : m];
    if (mutated != nullptr && i < m) mutated[first_tree + i] = 0ull;
}

// The build's level over the new trees alone: forest_level from cell `base` = append_first_cell(used, first_tree, l) to `end` =
// append_end_cell(used + n_leaves, first_tree + m, l), searching among the `end_tree` = first_tree + m trees in front of that
// end.  The first wavefront begins at the first new tree's first cell, so no lane holds a cell of an earlier tree; a lane
// behind `end` finds the last new tree and is padding behind its nodes; a new tree without a leaf gets its zero root from the
// lane of its reserved cell at level 1, as in the build.
__global__ __launch_bounds__(256) void forest_append_level_kernel(const Node* __restrict__ in, const uint64_t* __restrict__ offsets, uint32_t end_tree,
                                                                  uint32_t l, uint64_t base, uint64_t end, Node* __restrict__ out, Node* __restrict__ roots,
                                                                  const uint32_t* __restrict__ status)
{
    forest_level<true, false>(in, offsets, end_tree, l, base, end, out, roots, nullptr, status);
}

// The same with the compare of the flagged build: the masks of the new trees, zeroed by forest_append_offsets_kernel.
__global__ __launch_bounds__(256) void forest_append_level_flagged_kernel(const Node* __restrict__ in, const uint64_t* __restrict__ offsets,
                                                                          uint32_t end_tree, uint32_t l, uint64_t base, uint64_t end, Node* __restrict__ out,
                                                                          Node* __restrict__ roots, unsigned long long* __restrict__ mutated,
                                                                          const uint32_t* __restrict__ status)
{
    forest_level<true, true>(in, offsets, end_tree, l, base, end, out, roots, mutated, status);
}

// Dropping the last trees (vkmr_hip_forest_truncate_async): a lane per tree t = keep_trees + i < ntrees ends it where tree
// keep_trees begins and zeroes its root, as a build over the shortened offsets would.  offsets[keep_trees] is only read.
__global__ __launch_bounds__(256) void forest_truncate_kernel(uint64_t* __restrict__ offsets, uint32_t ntrees, uint32_t keep_trees, Node* __restrict__ roots)
{
    const uint64_t t = (uint64_t)keep_trees + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ntrees) return;
    offsets[t + 1] = offsets[keep_trees];
    const uint32_t zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    vkmr_dev::store_node(roots + t, zero);
}

// ---- the open tree grown or shrunk by leaves (vkmr_hip_forest_extend_async, vkmr_hip_forest_shrink_async; forest_plan.hpp:
// extend_first_cell, extend_end_cell) ----
// Tree `tree`, the last in use, at offset used - count goes from `count` to `new_end - (used - count)` leaves; every tree
// behind it is empty at `used`.  The check, the leaves (forest_append_leaves_kernel, when growing and not in place), the
// offsets, then the build's own level body over the dirty nodes of the tree's right edge.  Every kernel behind the check
// reads *status first and does nothing when it is nonzero.

// No hash, a lane per offset tree + i, i <= ntrees - tree: the open tree begins where the caller says (offsets[tree] + count ==
// used) and every later offset, the forest's last included, is `used`: the trees behind are empty.  Bit 2 (value 4), the
// append's numbering, ORed into *status, zeroed by the host.  count <= used is the host's.
__global__ __launch_bounds__(256) void forest_extend_check_kernel(const uint64_t* __restrict__ offsets, uint32_t ntrees, uint32_t tree, uint64_t count,
                                                                  uint64_t used, uint32_t* __restrict__ status)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > (uint64_t)(ntrees - tree)) return;
    if (offsets[tree + i] != (i == 0ull ? used - count : used)) atomicOr(status, 4u);
}

// A lane per tree tree + i, i < ntrees - tree: offsets[tree + i + 1] = new_end, the end of the open tree and of every empty tree
// behind it.  offsets[tree] stays.  With `mutated` the open tree's mask is zeroed here, not by a memset, so that a refused
// call leaves it alone; forest_extend_scan_kernel forms it again.
__global__ __launch_bounds__(256) void forest_extend_offsets_kernel(uint64_t* __restrict__ offsets, uint32_t ntrees, uint32_t tree, uint64_t new_end,
                                                                    unsigned long long* __restrict__ mutated, const uint32_t* __restrict__ status)
{
    if (*status != 0u) return;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint64_t)(ntrees - tree)) return;
    offsets[tree + i + 1] = new_end;
    if (mutated != nullptr && i == 0ull) mutated[tree] = 0ull;
}

// The build's level over the open tree's dirty nodes alone: forest_level from cell `base` = extend_first_cell to `end` =
// extend_end_cell, searching among the `end_tree` = tree + 1 trees up to the open one.  What the body does at the edges:
//   the first wavefront begins at pos_l(tree) + first_l, inside the open tree, and pos_l grows with t: the search ends at the
//     last of its end_tree trees, `tree`, in every wavefront, t0 + 1 == end_tree makes `mixed` false, and no lane holds an
//     earlier tree's cell (p >= pos_l(tree) always);
//   the offsets kernel ran first, so c is the NEW count; a lane behind `end` finds the open tree as well and has
//     j >= n_out: padding, it returns in front of every load and store.  The reserved cells and the roots of the empty trees
//     behind are therefore not written -- the search does not know those trees;
//   a tree shrunk to no leaf: the range is its reserved cell at level 1, whose lane writes the zero root (the c == 0 branch).
// Forcing the first node to 0 at a lone-node level (forest_plan.hpp) is the host's: it arrives here as `base`, the body's
// existing argument, and the body is the text the build and the append compile.
__global__ __launch_bounds__(256) void forest_extend_level_kernel(const Node* __restrict__ in, const uint64_t* __restrict__ offsets, uint32_t end_tree,
                                                                  uint32_t l, uint64_t base, uint64_t end, Node* __restrict__ out, Node* __restrict__ roots,
                                                                  const uint32_t* __restrict__ status)
{
    forest_level<true, false>(in, offsets, end_tree, l, base, end, out, roots, nullptr, status);
}

// The open tree's mask formed again: the scan's body (compare, no hash) over ALL nodes of the tree at level l, from `base` =
// pos_l(tree) to `end` = extend_end_cell -- an old right-edge pair may have set a bit that no pair of the new tree sets, so
// the edge alone cannot say.  `in` is level l - 1 as the hash launches of this call have left it.  The scan's body reads no
// status word, so this kernel does.
__global__ __launch_bounds__(256) void forest_extend_scan_kernel(const Node* __restrict__ in, const uint64_t* __restrict__ offsets, uint32_t end_tree,
                                                                 uint32_t l, uint64_t base, uint64_t end, unsigned long long* __restrict__ mutated,
                                                                 const uint32_t* __restrict__ status)
{
    if (*status != 0u) return;
    forest_level<false, true>(in, offsets, end_tree, l, base, end, nullptr, nullptr, mutated, nullptr);
}
