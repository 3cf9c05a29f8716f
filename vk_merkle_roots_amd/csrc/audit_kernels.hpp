// audit_kernels.hpp -- which nodes of a stored forest, or a stored tree, are not the hash of their children?  (include/vkmr_hip.h:
// vkmr_hip_forest_audit_async, vkmr_hip_tree_audit_async; the rule, the ballot words and the scratch layout: audit_plan.hpp.)
//
// The build's launches again, reading where the build wrote: level l from level l - 1, one lane per cell of level l's buffer.
// A lane finds its node as the build does (forest_kernels.hpp: forest_find_tree), loads the two stored children AND the stored
// cell of the node itself, hashes the children once -- the kernel's only hash block -- and compares.  Nothing of the
// structure is written.  What a level's launch leaves:
//   masks[t]    bit l - 1 when level l of tree t holds a bad node -- mutated[t]'s shape and discipline: read first, and where
//               every lane of the wavefront has one tree the first bad lane alone issues the atomic.  The atomic that finds the
//               mask still zero counts the tree (info[2]).  A single tree keeps its one mask in info[2] itself.
//   info[1]     the bad nodes, one atomic add per wavefront that holds one; info[3] the nodes checked, one per workgroup
//   ballots     (the list form) one word per wavefront of cells, bit i = lane i's node is bad
// The list form ranks all the levels' ballot words at once with the multiproof's three ranking kernels (tree_kernels.hpp, one
// level), and one emit launch per level finds the bad nodes again -- the search only in wavefronts whose word is not zero -- and
// writes (tree, level, node) at rank = set bits in front, when that is below `capacity`: strictly increasing (level, tree,
// node), nothing appended through a counter in memory, and no kernel waits for another workgroup.
//
// A forest and one tree differ in how a lane finds its node: the two structs below, in entries.hpp's manner -- one body per
// kernel, and a __global__ kernel is its arguments as the struct and the call.
#pragma once

#include "audit_plan.hpp"
#include "forest_kernels.hpp"

// What a lane knows once it has found its cell, as numbers alone: `live` when the cell is a node that is checked (`empty`: the
// root cell of a tree without leaves, checked against zero), the node's name (t, j), its own cell p of level l's buffer (`root`:
// the node is the tree's last and lies in roots[t] instead) and the cells of its two children in level l - 1's buffer.  `mixed`
// is wave-uniform: the lanes of this wavefront may hold different trees.  The emit launches need no more than this.
struct AuditPlace {
    bool live, empty, mixed, root;
    uint32_t t;
    uint64_t j, p, left, right;
};

// The three cells a live lane loads.  An empty tree's all name its root cell.
struct AuditNode {
    const Node *left, *right, *stored;
};

// A forest: forest_level's search and its rules for which trees take part in level l.
struct AuditForest {
    static constexpr bool forest = true;
    const uint64_t* offsets; uint32_t ntrees, l;
    __device__ __forceinline__ AuditPlace place(uint64_t p0, uint32_t lane) const
    {
        AuditPlace at = {false, false, false, false, 0u, 0ull, p0 + lane, 0ull, 0ull};
        const ForestLane found = forest_find_tree(offsets, ntrees, l, p0, lane);
        at.t = found.t;
        at.mixed = found.mixed;
        const uint64_t o = offsets[at.t], c = offsets[at.t + 1u] - o;
        const uint64_t first = vkmr_forest::pos(o, at.t, l);
        if (at.p < first) return at;             // cells in front of tree 0 (offsets[0] > 0)
        at.j = at.p - first;
        if (c == 0ull) {                         // an empty tree: the lane of its reserved cell at level 1 checks the root
            at.live = at.empty = at.root = l == 1u && at.j == 0ull;
            return at;
        }
        const uint64_t n_in = vkmr_forest::level_count(c, l - 1u), n_out = vkmr_forest::level_count(c, l);
        if ((l > 1u && n_in == 1ull) || at.j >= n_out) return at;   // the tree is done, or the padding behind its nodes
        const uint64_t level = vkmr_forest::pos(o, at.t, l - 1u);
        at.live = true;
        at.root = n_out == 1ull;
        at.left = level + 2 * at.j;
        at.right = level + vkmr_math::right_child(at.j, n_in);
        return at;
    }
};

// The forest's cells: `in` is level l - 1 (the leaves for l == 1), `out` level l's buffer; the stored cell of a tree's last
// level is roots[t].
struct AuditForestCells : AuditForest {
    const Node *in, *out, *roots;
    __device__ __forceinline__ AuditNode node(const AuditPlace& at) const
    {
        if (at.empty) return {roots + at.t, roots + at.t, roots + at.t};
        return {in + at.left, in + at.right, at.root ? roots + at.t : out + at.p};
    }
};

// One tree: cell p of level l is node p; a lone-node level above ceil(log2 count) is hash(a, a) of the node below, which is
// right_child()'s answer for n_in == 1.  Level l - 1 has n_in cells, level l n_out.
struct AuditTree {
    static constexpr bool forest = false;
    uint64_t n_in, n_out;
    __device__ __forceinline__ AuditPlace place(uint64_t p0, uint32_t lane) const
    {
        const uint64_t p = p0 + lane;
        return {p < n_out, false, false, false, 0u, p, p, 2 * p, vkmr_math::right_child(p, n_in)};
    }
};

struct AuditTreeCells : AuditTree {
    const Node *in, *out;
    __device__ __forceinline__ AuditNode node(const AuditPlace& at) const { return {in + at.left, in + at.right, out + at.p}; }
};

// ---- one level: hash the stored children, compare with the stored node --------------------------------------------------------
// `cells` lanes of level l.  info[0] is the check's status (a forest's; the same word in every lane): nonzero, and nothing is
// read; the list form's ballot words are then zero.  Every lane reaches the ballots and the barrier.
template <class Shape>
__device__ __forceinline__ void audit_level(const Shape sh, uint32_t l, uint64_t cells, uint64_t* __restrict__ masks, uint64_t* __restrict__ ballots,
                                            uint64_t* info)
{
    __shared__ uint32_t s_checked[VKMR_AUDIT_THREADS / 64];
    const uint32_t lane = threadIdx.x & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t p0 = ((uint64_t)blockIdx.x * (VKMR_AUDIT_THREADS / 64u) + wave) * 64ull;
    const bool inside = p0 < cells;              // wave-uniform
    bool bad = false, live = false, mixed = false;
    uint32_t t = 0u;
    if (inside && info[0] == 0ull) {
        const AuditPlace at = sh.place(p0, lane);
        live = at.live;
        mixed = at.mixed;
        t = at.t;
        if (at.live) {
            const AuditNode nd = sh.node(at);
            const Node a = vkmr_dev::load_node(nd.left), b = vkmr_dev::load_node(nd.right), stored = vkmr_dev::load_node(nd.stored);
            Node parent;
            vkmr_dev::hash_pair(a.w, b.w, parent.w);
            const Node zero = {{0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u}};
            uint32_t diff = vkmr_dev::node_diff(at.empty ? zero : parent, stored);
            // opaque here: the compiler otherwise splits the OR chain into eight compares packed with 16-bit shifts, which the
            // build's issue model (isa_prio_pass) has no measured price for
            asm volatile("" : "+v"(diff));
            bad = diff != 0u;
        }
    }
    const uint64_t bads = __ballot(bad), lives = __ballot(live);
    if (ballots && inside && lane == 0u) ballots[p0 >> 6] = bads;
    if (bads != 0ull) {
        const uint64_t bit = 1ull << (l - 1u);
        const bool first = lane == (uint32_t)__builtin_ctzll(bads);
        if constexpr (Shape::forest) {
            if ((mixed ? bad : first) && !(masks[t] & bit)) {   // not mixed: t is the same in every lane
                const uint64_t before = __hip_atomic_fetch_or(masks + t, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (before == 0ull) (void)__hip_atomic_fetch_add(info + 2, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        } else {
            if (first && !(info[2] & bit)) (void)__hip_atomic_fetch_or(info + 2, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (first) (void)__hip_atomic_fetch_add(info + 1, (uint64_t)__popcll(bads), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (lane == 0u) s_checked[wave] = (uint32_t)__popcll(lives);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t sum = 0u;
#pragma unroll
        for (uint32_t w = 0; w < VKMR_AUDIT_THREADS / 64; ++w) sum += s_checked[w];
        if (sum) (void)__hip_atomic_fetch_add(info + 3, (uint64_t)sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // no return value
    }
}

// ---- the list: a level's bad nodes at their ranks -----------------------------------------------------------------------------
// The same lanes as audit_level.  A wavefront whose ballot word is zero, or whose first rank is at or behind `capacity`, ends
// at once; the others find their nodes again and each bad lane writes its entry at word_start + the set bits below its own, when
// that is below `capacity`.  A refused forest left every word zero.  With `finish` this is the call's last launch, and one lane
// sets status bit 2 when there were more bad nodes than `capacity`: nothing else reads or writes info[] in this launch.
template <class Shape>
__device__ __forceinline__ void audit_emit(const Shape sh, uint32_t l, uint64_t cells, const uint64_t* __restrict__ ballots,
                                           const uint64_t* __restrict__ word_start, uint32_t* __restrict__ bad_trees, uint32_t* __restrict__ bad_levels,
                                           uint64_t* __restrict__ bad_nodes, uint32_t capacity, uint64_t* __restrict__ info, uint32_t finish)
{
    if (finish && blockIdx.x == 0 && threadIdx.x == 0 && info[1] > (uint64_t)capacity) info[0] |= 4ull;
    const uint32_t lane = threadIdx.x & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t p0 = ((uint64_t)blockIdx.x * (VKMR_AUDIT_THREADS / 64u) + wave) * 64ull;
    if (p0 >= cells) return;                     // wave-uniform, as the two below
    const uint64_t bads = ballots[p0 >> 6];
    if (bads == 0ull) return;
    const uint64_t start = word_start[p0 >> 6];
    if (start >= (uint64_t)capacity) return;
    const AuditPlace at = sh.place(p0, lane);
    const uint64_t rank = start + (uint64_t)__popcll(bads & ((1ull << lane) - 1ull));
    if (!((bads >> lane) & 1ull) || rank >= (uint64_t)capacity) return;
    if constexpr (Shape::forest) bad_trees[rank] = at.t;
    bad_levels[rank] = l;
    bad_nodes[rank] = at.j;
}

// ---- the kernels: their arguments as the struct, and the call ------------------------------------------------------------------

__global__ __launch_bounds__(VKMR_AUDIT_THREADS) void forest_audit_level_kernel(const Node* __restrict__ in, const Node* __restrict__ out,
                                                                               const Node* __restrict__ roots, const uint64_t* __restrict__ offsets,
                                                                               uint32_t ntrees, uint32_t l, uint64_t cells, uint64_t* __restrict__ masks,
                                                                               uint64_t* __restrict__ ballots, uint64_t* info)
{
    audit_level(AuditForestCells{{offsets, ntrees, l}, in, out, roots}, l, cells, masks, ballots, info);
}

__global__ __launch_bounds__(VKMR_AUDIT_THREADS) void tree_audit_level_kernel(const Node* __restrict__ in, const Node* __restrict__ out, uint64_t n_in,
                                                                             uint64_t n_out, uint32_t l, uint64_t* __restrict__ ballots, uint64_t* info)
{
    audit_level(AuditTreeCells{{n_in, n_out}, in, out}, l, n_out, (uint64_t*)nullptr, ballots, info);
}

__global__ __launch_bounds__(VKMR_AUDIT_THREADS) void forest_audit_emit_kernel(const uint64_t* __restrict__ offsets, uint32_t ntrees, uint32_t l, uint64_t cells,
                                                                              const uint64_t* __restrict__ ballots, const uint64_t* __restrict__ word_start,
                                                                              uint32_t* __restrict__ bad_trees, uint32_t* __restrict__ bad_levels,
                                                                              uint64_t* __restrict__ bad_nodes, uint32_t capacity, uint64_t* __restrict__ info,
                                                                              uint32_t finish)
{
    audit_emit(AuditForest{offsets, ntrees, l}, l, cells, ballots, word_start, bad_trees, bad_levels, bad_nodes, capacity, info,
               finish);
}

__global__ __launch_bounds__(VKMR_AUDIT_THREADS) void tree_audit_emit_kernel(uint64_t n_out, uint32_t l, const uint64_t* __restrict__ ballots,
                                                                            const uint64_t* __restrict__ word_start, uint32_t* __restrict__ bad_levels,
                                                                            uint64_t* __restrict__ bad_nodes, uint32_t capacity, uint64_t* __restrict__ info,
                                                                            uint32_t finish)
{
    audit_emit(AuditTree{0ull, n_out}, l, n_out, ballots, word_start, (uint32_t*)nullptr, bad_levels, bad_nodes, capacity, info, finish);
}
