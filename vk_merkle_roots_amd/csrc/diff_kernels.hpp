// diff_kernels.hpp -- which leaves differ between two stored forests, or two stored trees, of one shape?  (include/vkmr_hip.h:
// vkmr_hip_forest_diff_async, vkmr_hip_tree_diff_async; the rule, the steps and the scratch layout: diff_plan.hpp.)  No hash
// is computed here: nodes are loaded and compared.
//
// A descent from the roots, never a scan of level 0: equal roots end a tree, equal inner nodes prune their subtrees, and the
// work is that of the changed paths.  It relies on two facts (diff_plan.hpp has them in full): a differing node of consistent
// forests has a differing child, so the frontier never shrinks and a frontier above `capacity` proves that more than
// `capacity` leaves differ; and equal nodes are taken to cover equal leaves, which with equal counts on both sides leaves no
// room for the duplicate-last ambiguity.
//   step 0   *_diff_roots_count_kernel   workgroup g counts the differing roots among its run of trees (diff_plan.hpp: root_span)
//            multiproof_block_starts_kernel over the workgroups' counts: their starts, the total, status bit 2 above `capacity`
//            *_diff_roots_emit_kernel    the same compare again; a differing tree goes to its rank, in tree order
//   step s   *_diff_mask_kernel          one lane per frontier entry: the two children from both sides (four load_node, two
//            of 1..H                     node_diff), two mask bits per entry, one 64-bit word per 32 entries; the entries that
//                                        compared children are counted, one atomic add per workgroup
//            multiproof_block_sums_kernel, multiproof_block_starts_kernel, multiproof_word_starts_kernel   (tree_kernels.hpp,
//                                        unchanged, one level): set bits before every word; status bit 2 above `capacity`
//            *_diff_emit_kernel          every set bit's child at its rank in the other frontier buffer; in step H, in the
//                                        caller's outputs, with B's leaf beside it when asked for
// Emission by rank keeps the frontier sorted by (tree, node) at every step, so after step H it is the answer: no sort, and
// nothing depends on scheduling.  Step 0 ranks per workgroup and not per tree because the scratch is sized from `capacity`
// alone and cannot hold a word per 64 trees; it reads every root twice.  No entry is appended through a counter in memory
// (DESIGN 3.18 measured that), and no kernel waits for another workgroup.  A nonzero status ends the call: every kernel
// behind it reads hdr[0] first and does nothing, as the ranking kernels do.
//
// A forest and one tree differ in where a node's cell lies and in whether an entry carries a tree: the two structs below, in
// entries.hpp's manner -- one body per kernel, and a __global__ kernel is its arguments as the struct and the call.
#pragma once

#include "diff_plan.hpp"
#include "entries.hpp"

static_assert(VKMR_DIFF_THREADS == VKMR_SIZES_THREADS, "block_exclusive's workgroup");

// The two children of an entry's node in A and in B (the right ones lie in the cells behind), or `carried`: the entry is a
// leaf of a tree shorter than the forest and has none.
struct DiffKids {
    const Node *a, *b;
    bool has_right, carried;
};

// A forest: tree t's nodes through its offset and count, as forest_plan.hpp places them; the offsets are trusted as
// vkmr_hip_forest_proofs_async trusts them.  An empty tree never enters, whatever its two root cells hold.
struct DiffForest {
    static constexpr bool forest = true;
    const Node *digests_a, *forest_a, *roots_a, *digests_b, *forest_b, *roots_b;
    const uint64_t* offsets; uint32_t ntrees; const uint64_t* level_base;   // ForestLevels::base, null where no child is looked up
    __device__ __forceinline__ uint64_t trees() const { return ntrees; }
    __device__ __forceinline__ bool enters(uint64_t t) const { return offsets[t + 1u] > offsets[t]; }
    __device__ __forceinline__ const Node* root_a(uint64_t t) const { return roots_a + t; }
    __device__ __forceinline__ const Node* root_b(uint64_t t) const { return roots_b + t; }
    __device__ __forceinline__ bool carried(uint32_t t, uint32_t step) const
    {
        return vkmr_math::height(offsets[t + 1u] - offsets[t]) < step;
    }
    __device__ __forceinline__ DiffKids kids(uint32_t t, uint64_t p, uint32_t step) const
    {
        const uint64_t o = offsets[t], c = offsets[t + 1u] - o;
        const uint32_t l = vkmr_diff::level_at(vkmr_math::height(c), step);
        if (l == 0u) return {nullptr, nullptr, false, true};
        const vkmr_diff::Step s = vkmr_diff::forest_step(o, c, t, p, l);
        if (l == 1u) return {digests_a + s.left, digests_b + s.left, s.has_right, false};
        const uint64_t at = level_base[l - 1u] + s.left;
        return {forest_a + at, forest_b + at, s.has_right, false};
    }
    __device__ __forceinline__ const Node* leaf_b(uint32_t t, uint64_t i) const { return digests_b + offsets[t] + i; }
};

// One tree: every entry stands at the launch's level, so the host passes where its children's level begins (step 0: where
// the root lies; height 0: the root is the leaf).
struct DiffTree {
    static constexpr bool forest = false;
    const Node *digests_a, *tree_a, *digests_b, *tree_b;
    uint64_t count; uint32_t height; uint64_t base;   // step 0: the root's cell of the tree buffer; step s: tree_child_base()
    __device__ __forceinline__ uint64_t trees() const { return 1ull; }
    __device__ __forceinline__ bool enters(uint64_t) const { return true; }
    __device__ __forceinline__ const Node* root_a(uint64_t) const { return height ? tree_a + base : digests_a; }
    __device__ __forceinline__ const Node* root_b(uint64_t) const { return height ? tree_b + base : digests_b; }
    __device__ __forceinline__ bool carried(uint32_t, uint32_t) const { return false; }
    __device__ __forceinline__ DiffKids kids(uint32_t, uint64_t p, uint32_t step) const
    {
        const uint32_t l = vkmr_diff::level_at(height, step);          // >= 1: the host stops at step `height`
        const vkmr_diff::Step s = vkmr_diff::tree_step(count, base, p, l);
        if (l == 1u) return {digests_a + s.left, digests_b + s.left, s.has_right, false};
        return {tree_a + s.left, tree_b + s.left, s.has_right, false};
    }
    __device__ __forceinline__ const Node* leaf_b(uint32_t, uint64_t i) const { return digests_b + i; }
};

// Where emitted entries go: a frontier buffer of the scratch, or the caller's outputs (then with B's leaf when leaves_b is
// given).  A single tree's entries carry no tree.
struct DiffOut {
    uint32_t* trees; uint64_t* nodes; Node* leaves_b;
    template <class Shape>
    __device__ __forceinline__ void put(const Shape& sh, uint64_t rank, uint32_t t, uint64_t p) const
    {
        if constexpr (Shape::forest) trees[rank] = t;
        nodes[rank] = p;
        if (leaves_b) vkmr_dev::store_node(leaves_b + rank, vkmr_dev::load_node(sh.leaf_b(t, p)));
    }
};

// The call's four counters, written by one lane of its last launch: status, n (or the frontier that overflowed), trees whose
// roots differ, nodes whose children were compared.
__device__ __forceinline__ void diff_finish(const uint64_t* hdr, uint64_t trees_differing, uint64_t* __restrict__ info)
{
    info[0] = hdr[0];
    info[1] = hdr[1];
    info[2] = trees_differing;
    info[3] = hdr[3];
}

// Bit i of x to bit 2i: the two ballots of a wavefront half interleave into one mask word.  The same value in every lane.
__device__ __forceinline__ uint64_t diff_spread(uint32_t x)
{
    uint64_t v = x;
    v = (v | (v << 16)) & 0x0000FFFF0000FFFFull;
    v = (v | (v << 8)) & 0x00FF00FF00FF00FFull;
    v = (v | (v << 4)) & 0x0F0F0F0F0F0F0F0Full;
    v = (v | (v << 2)) & 0x3333333333333333ull;
    v = (v | (v << 1)) & 0x5555555555555555ull;
    return v;
}

template <class Shape>
__device__ __forceinline__ bool diff_root_differs(const Shape& sh, uint64_t t)
{
    return sh.enters(t) && vkmr_dev::node_diff(vkmr_dev::load_node(sh.root_a(t)), vkmr_dev::load_node(sh.root_b(t))) != 0u;
}

// ---- step 0 ------------------------------------------------------------------------------------------------------------------
// Workgroup g takes trees [g * span, (g + 1) * span), one per lane and trip; block[g] = the differing roots among them.
template <class Shape>
__device__ __forceinline__ void diff_roots_count(const Shape sh, uint64_t span, uint64_t* __restrict__ block)
{
    __shared__ uint32_t s_wave[VKMR_DIFF_THREADS / 64];
    const uint64_t first = (uint64_t)blockIdx.x * span;
    const uint64_t end = first + span < sh.trees() ? first + span : sh.trees();
    uint32_t mine = 0u;
    for (uint64_t t = first + threadIdx.x; t < end; t += VKMR_DIFF_THREADS) mine += diff_root_differs(sh, t) ? 1u : 0u;
    uint32_t total;
    (void)vkmr_sizes::block_exclusive(mine, s_wave, &total);
    if (threadIdx.x == 0) block[blockIdx.x] = total;
}

// block[g] is now the rank of workgroup g's first differing tree, hdr[1] their number.  The same trees again, a trip at a
// time in tree order: a differing tree goes to the rank of its workgroup plus the differing trees before it.  With `finish`
// no step follows (capacity 0, no leaf at all, or a tree of one leaf): the counters are written here.
template <class Shape>
__device__ __forceinline__ void diff_roots_emit(const Shape sh, const DiffOut out, uint64_t span, const uint64_t* __restrict__ block, uint64_t* hdr,
                                                uint64_t* __restrict__ info, uint32_t finish)
{
    __shared__ uint32_t s_wave[VKMR_DIFF_THREADS / 64];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        hdr[4] = hdr[1];                          // written by the ranking, also when it set the status
        if (finish) diff_finish(hdr, hdr[1], info);
    }
    if (hdr[0] != 0ull) return;                   // the same word in every lane
    const uint64_t first = (uint64_t)blockIdx.x * span;
    const uint64_t end = first + span < sh.trees() ? first + span : sh.trees();
    uint64_t rank = block[blockIdx.x];
    for (uint64_t t0 = first; t0 < end; t0 += VKMR_DIFF_THREADS) {   // the same trips in every lane
        const uint64_t t = t0 + threadIdx.x;
        const bool differs = t < end && diff_root_differs(sh, t);
        uint32_t total;
        const uint32_t before = vkmr_sizes::block_exclusive(differs ? 1u : 0u, s_wave, &total);
        if (differs) out.put(sh, rank + before, (uint32_t)t, 0ull);   // < hdr[1] <= capacity: the status is 0
        rank += total;
        __syncthreads();                          // s_wave is reused by the next trip
    }
}

// ---- steps 1 .. H ------------------------------------------------------------------------------------------------------------
// One lane per entry j < hdr[1] of the frontier (trees[], nodes[]).  The status and the frontier's size are the same words in
// every lane and the grid covers every mask word of the step, so every lane of a wavefront reaches the ballots; lanes past
// the frontier load nothing and vote 0.  A right child that does not exist is not loaded.
template <class Shape>
__device__ __forceinline__ void diff_mask(const Shape sh, const uint32_t* __restrict__ trees, const uint64_t* __restrict__ nodes, uint32_t step,
                                          uint64_t words, uint64_t* hdr, uint64_t* __restrict__ mask)
{
    __shared__ uint32_t s_compared[VKMR_DIFF_THREADS / 64];
    if (hdr[0] != 0ull) return;
    const uint64_t n = hdr[1];
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool left = false, right = false, compared = false;
    if (j < n) {
        uint32_t t = 0u;
        if constexpr (Shape::forest) t = trees[j];
        const DiffKids k = sh.kids(t, nodes[j], step);
        if (k.carried) {
            left = true;
        } else {
            compared = true;
            const Node la = vkmr_dev::load_node(k.a), lb = vkmr_dev::load_node(k.b);
            left = vkmr_dev::node_diff(la, lb) != 0u;
            if (k.has_right) {
                const Node ra = vkmr_dev::load_node(k.a + 1), rb = vkmr_dev::load_node(k.b + 1);
                right = vkmr_dev::node_diff(ra, rb) != 0u;
            }
        }
    }
    const uint64_t lefts = __ballot(left), rights = __ballot(right), visited = __ballot(compared);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0u) {
        const uint64_t w = j >> 5;                // this wavefront's 64 entries: words w and w + 1
        if (w < words) mask[w] = diff_spread((uint32_t)lefts) | (diff_spread((uint32_t)rights) << 1);
        if (w + 1ull < words) mask[w + 1ull] = diff_spread((uint32_t)(lefts >> 32)) | (diff_spread((uint32_t)(rights >> 32)) << 1);
        s_compared[wave] = (uint32_t)__popcll(visited);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t sum = 0u;
#pragma unroll
        for (uint32_t w = 0; w < VKMR_DIFF_THREADS / 64; ++w) sum += s_compared[w];
        if (sum) (void)__hip_atomic_fetch_add(hdr + 3, (uint64_t)sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // no return value
    }
}

// One lane per entry j < bound of the frontier that was masked: each set bit's child at its rank.  An entry's two children
// are neighbours in the next frontier, and a wavefront's ranks are consecutive.  With `finish` this is step H: `out` is the
// caller's outputs and lane 0 writes the counters, whatever the status.
template <class Shape>
__device__ __forceinline__ void diff_emit(const Shape sh, const DiffOut out, const uint32_t* __restrict__ trees, const uint64_t* __restrict__ nodes,
                                          uint32_t step, uint64_t bound, const uint64_t* __restrict__ mask, const uint64_t* __restrict__ word_start,
                                          const uint64_t* __restrict__ hdr, uint64_t* __restrict__ info, uint32_t finish)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (finish && j == 0) diff_finish(hdr, hdr[4], info);
    if (hdr[0] != 0ull || j >= bound) return;
    const uint64_t m = mask[j >> 5];
    const uint32_t shift = 2u * ((uint32_t)j & 31u);
    const uint32_t bits = (uint32_t)(m >> shift) & 3u;
    if (!bits) return;                            // also every lane past the frontier: its bits are 0
    const uint64_t rank = word_start[j >> 5] + (uint64_t)__popcll(m & ((1ull << shift) - 1ull));   // < hdr[1] <= capacity: the status is 0
    uint32_t t = 0u;
    if constexpr (Shape::forest) t = trees[j];
    const uint64_t p = nodes[j];
    if (sh.carried(t, step)) {
        out.put(sh, rank, t, p);
        return;
    }
    if (bits & 1u) out.put(sh, rank, t, 2ull * p);
    if (bits & 2u) out.put(sh, rank + (bits & 1u), t, 2ull * p + 1ull);
}

// ---- the kernels: their arguments as the struct, and the call ------------------------------------------------------------------

__global__ __launch_bounds__(VKMR_DIFF_THREADS) void forest_diff_roots_count_kernel(const Node* __restrict__ roots_a, const Node* __restrict__ roots_b,
                                                                                   const uint64_t* __restrict__ offsets, uint32_t ntrees, uint64_t span,
                                                                                   uint64_t* __restrict__ block)
{
    diff_roots_count(DiffForest{nullptr, nullptr, roots_a, nullptr, nullptr, roots_b, offsets, ntrees, nullptr}, span, block);
}

__global__ __launch_bounds__(VKMR_DIFF_THREADS) void forest_diff_roots_emit_kernel(const Node* __restrict__ roots_a, const Node* __restrict__ roots_b,
                                                                                  const uint64_t* __restrict__ offsets, uint32_t ntrees, uint64_t span,
                                                                                  const uint64_t* __restrict__ block, uint64_t* hdr,
                                                                                  uint32_t* __restrict__ trees_out, uint64_t* __restrict__ nodes_out,
                                                                                  uint64_t* __restrict__ info, uint32_t finish)
{
    diff_roots_emit(DiffForest{nullptr, nullptr, roots_a, nullptr, nullptr, roots_b, offsets, ntrees, nullptr}, DiffOut{trees_out, nodes_out, nullptr}, span,
                    block, hdr, info, finish);
}

__global__ __launch_bounds__(VKMR_DIFF_THREADS) void forest_diff_mask_kernel(const Node* __restrict__ digests_a, const Node* __restrict__ forest_a,
                                                                            const Node* __restrict__ digests_b, const Node* __restrict__ forest_b,
                                                                            ForestLevels lv, const uint64_t* __restrict__ offsets, uint32_t ntrees,
                                                                            const uint32_t* __restrict__ trees, const uint64_t* __restrict__ nodes,
                                                                            uint32_t step, uint64_t words, uint64_t* hdr, uint64_t* __restrict__ mask)
{
    diff_mask(DiffForest{digests_a, forest_a, nullptr, digests_b, forest_b, nullptr, offsets, ntrees, lv.base}, trees, nodes, step, words, hdr, mask);
}

__global__ __launch_bounds__(VKMR_DIFF_THREADS) void forest_diff_emit_kernel(const Node* __restrict__ digests_b, const uint64_t* __restrict__ offsets,
                                                                            uint32_t ntrees, const uint32_t* __restrict__ trees,
                                                                            const uint64_t* __restrict__ nodes, uint32_t step, uint64_t bound,
                                                                            const uint64_t* __restrict__ mask, const uint64_t* __restrict__ word_start,
                                                                            const uint64_t* __restrict__ hdr, uint32_t* __restrict__ trees_out,
                                                                            uint64_t* __restrict__ nodes_out, Node* __restrict__ leaves_b_out,
                                                                            uint64_t* __restrict__ info, uint32_t finish)
{
    diff_emit(DiffForest{nullptr, nullptr, nullptr, digests_b, nullptr, nullptr, offsets, ntrees, nullptr}, DiffOut{trees_out, nodes_out, leaves_b_out}, trees,
              nodes, step, bound, mask, word_start, hdr, info, finish);
}

__global__ __launch_bounds__(VKMR_DIFF_THREADS) void tree_diff_roots_count_kernel(const Node* __restrict__ digests_a, const Node* __restrict__ tree_a,
                                                                                 const Node* __restrict__ digests_b, const Node* __restrict__ tree_b,
                                                                                 uint64_t count, uint32_t height, uint64_t root_cell,
                                                                                 uint64_t* __restrict__ block)
{
    diff_roots_count(DiffTree{digests_a, tree_a, digests_b, tree_b, count, height, root_cell}, 1ull, block);
}

__global__ __launch_bounds__(VKMR_DIFF_THREADS) void tree_diff_roots_emit_kernel(const Node* __restrict__ digests_a, const Node* __restrict__ tree_a,
                                                                                const Node* __restrict__ digests_b, const Node* __restrict__ tree_b,
                                                                                uint64_t count, uint32_t height, uint64_t root_cell,
                                                                                const uint64_t* __restrict__ block, uint64_t* hdr,
                                                                                uint64_t* __restrict__ nodes_out, Node* __restrict__ leaves_b_out,
                                                                                uint64_t* __restrict__ info, uint32_t finish)
{
    diff_roots_emit(DiffTree{digests_a, tree_a, digests_b, tree_b, count, height, root_cell}, DiffOut{nullptr, nodes_out, leaves_b_out}, 1ull, block, hdr,
                    info, finish);
}

__global__ __launch_bounds__(VKMR_DIFF_THREADS) void tree_diff_mask_kernel(const Node* __restrict__ digests_a, const Node* __restrict__ tree_a,
                                                                          const Node* __restrict__ digests_b, const Node* __restrict__ tree_b,
                                                                          uint64_t count, uint32_t height, uint64_t child_base,
                                                                          const uint64_t* __restrict__ nodes, uint32_t step, uint64_t words, uint64_t* hdr,
                                                                          uint64_t* __restrict__ mask)
{
    diff_mask(DiffTree{digests_a, tree_a, digests_b, tree_b, count, height, child_base}, (const uint32_t*)nullptr, nodes, step, words, hdr, mask);
}

__global__ __launch_bounds__(VKMR_DIFF_THREADS) void tree_diff_emit_kernel(const Node* __restrict__ digests_b, const uint64_t* __restrict__ nodes,
                                                                          uint32_t step, uint64_t bound, const uint64_t* __restrict__ mask,
                                                                          const uint64_t* __restrict__ word_start, const uint64_t* __restrict__ hdr,
                                                                          uint64_t* __restrict__ nodes_out, Node* __restrict__ leaves_b_out,
                                                                          uint64_t* __restrict__ info, uint32_t finish)
{
    diff_emit(DiffTree{nullptr, nullptr, digests_b, nullptr, 0ull, 0u, 0ull}, DiffOut{nullptr, nodes_out, leaves_b_out}, (const uint32_t*)nullptr, nodes, step,
              bound, mask, word_start, hdr, info, finish);
}
