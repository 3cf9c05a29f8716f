// entries.hpp -- what the kernels of one stored tree (tree_kernels.hpp) and of a stored forest (forest_tree_kernels.hpp) share:
// plain structs that say where the two differ, and one body per operation written on them.  A __global__ kernel builds the
// structs from its own arguments and calls the body; they are passed by value and every member is inlined, so nothing is
// decided at run time.
//   Entries  what lane q knows of entry q and its neighbours: the tree it names (none but tree 0 in a single tree) and its height
//   Cells    where a tree's nodes lie in the stored levels: the sibling cell a proof takes beside a node
//   Span     the same for the two level buffers one launch of a leaf update is given: a leaf's cell, an entry's step
//
// Layouts.  One tree (vkmr_hip_reduce_tree_async): level 0 is the caller's digests; levels 1..height lie back to back in one
// buffer, level l (n_l = ceil(count / 2^l) cells) starting at cell off[l] = sum of n_j over 1 <= j < l.  A forest
// (vkmr_hip_reduce_forest_tree_async, forest_plan.hpp): level 0 is the caller's leaves, tree t at cell offsets[t]; level l >= 1
// has a buffer of level_cells(l) cells at cell base[l] = sum of level_cells(j) over 1 <= j < l, in which tree t's
// n_l = ceil(c_t / 2^l) nodes start at cell pos_l(t) = (offsets[t] >> l) + t.  Level h_t of a tree is its root: roots[t].
#pragma once

#include "forest_plan.hpp"
#include "tree_plan.hpp"   // VKMR_TREE_MAX_LEVELS, VKMR_MP_HEADER_WORDS, VKMR_MP_BLOCK_WORDS

// off[l] / base[l] for every level, passed by value (kernel arguments: 512 bytes).  Entry 0 is unused: level 0 is the digests.
struct TreeLevels { uint64_t off[VKMR_TREE_MAX_LEVELS]; };
struct ForestLevels { uint64_t base[VKMR_TREE_MAX_LEVELS]; };

// One tree: every entry is in tree 0, and its height is the launch's.
struct TreeEntries {
    const uint64_t* indices; uint32_t h;
    __device__ __forceinline__ uint32_t tree(uint64_t) const { return 0u; }
    __device__ __forceinline__ uint32_t height(uint64_t) const { return h; }
};

// A forest: entry q is the pair (trees[q], indices[q]); the entries differ per lane, so these are vector loads.  `heights`
// is null in the kernels that never ask for one.
struct ForestEntries {
    const uint32_t* trees; const uint64_t* indices; const uint32_t* heights;
    __device__ __forceinline__ uint32_t tree(uint64_t q) const { return trees[q]; }
    __device__ __forceinline__ uint32_t height(uint64_t q) const { return heights[q]; }
};

// sibling_cell(t, l, index): the cell a proof of leaf `index` of tree t takes at level l -- L[l][p ^ 1] with p = index >> l,
// or L[l][p] where p ^ 1 is past the level's end (vkmr_math::sibling).  The caller knows: t is a tree, index < its count, l < its height.
struct TreeCells {
    const Node *digests, *tree; const TreeLevels& lv; uint64_t count;
    __device__ __forceinline__ const Node* sibling_cell(uint32_t, uint32_t l, uint64_t index) const
    {
        const uint64_t n = ((count - 1) >> l) + 1;     // cells of level l
        const uint64_t s = vkmr_math::sibling(index >> l, n);
        return (l == 0) ? digests + s : tree + lv.off[l] + s;
    }
    // node_cell(t, l, p): the cell of node p of level l itself; the caller knows that l is below the height and p < n_l.
    __device__ __forceinline__ const Node* node_cell(uint32_t, uint32_t l, uint64_t p) const { return (l == 0) ? digests + p : tree + lv.off[l] + p; }
};

struct ForestCells {
    const Node *digests, *forest; const ForestLevels& lv; const uint64_t* offsets;
    __device__ __forceinline__ const Node* sibling_cell(uint32_t t, uint32_t l, uint64_t index) const
    {
        const uint64_t off = offsets[t], c = offsets[t + 1u] - off;
        const uint64_t s = vkmr_math::sibling(index >> l, vkmr_forest::level_count(c, l));
        return (l == 0) ? digests + off + s : forest + lv.base[l] + vkmr_forest::pos(off, t, l) + s;
    }
    __device__ __forceinline__ const Node* node_cell(uint32_t t, uint32_t l, uint64_t p) const
    {
        const uint64_t off = offsets[t];
        return (l == 0) ? digests + off + p : forest + lv.base[l] + vkmr_forest::pos(off, t, l) + p;
    }
};

// An update launch is given the buffers of levels l - 1 and l, not the table of all.  leaf(): a leaf's cell in the level-0 buffer.
struct TreeSpan {
    static constexpr bool forest = false;
    uint64_t n_in;   // cells of level l - 1
    __device__ __forceinline__ uint64_t leaf(uint32_t, uint64_t index) const { return index; }
};

struct ForestSpan {
    static constexpr bool forest = true;
    const uint64_t* offsets;
    __device__ __forceinline__ uint64_t leaf(uint32_t t, uint64_t index) const { return offsets[t] + index; }
};

// ---- leaf updates ---------------------------------------------------------------------------------------------------------
// Every lane is one update entry q < k.  The entry point's check ORs the contract's violations into *status (zeroed by the
// host) first; the two writers read *status and write nothing when it is nonzero, so a rejected batch leaves everything as it
// was.  After the check an entry's tree is there and its index is one of the tree's leaves.

// No hash: the leaf's cell = leaves[q].
template <class Entries, class Span>
__device__ __forceinline__ void update_leaves(const Entries e, const Span span, Node* __restrict__ digests, const Node* __restrict__ leaves, uint32_t k,
                                              const uint32_t* __restrict__ status)
{
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= k || *status != 0u) return;
    vkmr_dev::store_node(digests + span.leaf(e.tree(q), e.indices[q]), vkmr_dev::load_node(leaves + q));
}

// One level l >= 1 per launch.  Lane q hashes parent p = index_q >> l of its tree when the tree still takes part in level l
// and the lane is the first of its run (the entries are sorted by (tree, index), so lanes with the same parent are adjacent):
// each dirty node is hashed exactly once, distinct lanes write distinct cells and read only the level below.  A tree of the
// forest whose level l is one node gets it in roots[t].  reduce_level_kernel's / forest_level_kernel's body with the node
// given, not searched for; its one hash_parent is the kernel's only hash block.
template <class Entries, class Span>
__device__ __forceinline__ void update_level(const Entries e, const Span span, const Node* __restrict__ in, Node* __restrict__ out, Node* __restrict__ roots,
                                             uint32_t k, uint32_t l, const uint32_t* __restrict__ status)
{
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= k || *status != 0u) return;
    const uint32_t t = e.tree(q);
    const uint64_t index = e.indices[q];
    const uint64_t p = index >> l;
    if (q > 0 && vkmr_forest::update_same_node(e.tree(q - 1), e.indices[q - 1], t, index, l)) return;   // not the head of p's run
    vkmr_forest::UpdateStep s;
    if constexpr (Span::forest) {                // the text tests/c/forest_update_plan_test.cpp replays, called from here: behind a
        const uint64_t o = span.offsets[t], c = span.offsets[t + 1u] - o;   // member of Span it cost the hash block four instructions
        s = vkmr_forest::update_step(o, c, t, index, l);
    } else {
        s = {true, false, p, 0ull, span.n_in, p};   // the same fields for one tree: `in` and `out` are its levels l - 1 and l whole
    }
    if (!s.active) return;                       // the tree's root was formed at a level below
    uint32_t x[8];
    vkmr_dev::hash_parent(in + s.in_first, s.n_in, s.p, x);
    vkmr_dev::store_node(s.root ? roots + t : out + s.out, x);
}

// ---- multiproofs ----------------------------------------------------------------------------------------------------------
// One proof for k leaves: per level l and tree, for every node p of A_l = unique(indices >> l) whose sibling p ^ 1 is not in
// A_l, the sibling's cell (the node's own where it has none), level-major over the WHOLE forest -- level l of every tree
// before level l + 1 of any, inside a level by tree, inside a tree by node.  With the entries sorted by (tree, index) that is
// the order of the entries themselves at every level, and who emits follows from the sorted entries alone: entry q "owns"
// the cell of (l, p = index_q >> l) when l is below its tree's height and p is odd and q is the first lane of p's run (p - 1
// is in A_l iff the lane before has it), or p is even and q is the last lane of the run (p + 1 iff the lane after); the lane
// before or after counts only when it names the same tree.  The gather and the verifier share the ranking of those flags:
//   masks        one lane per entry, a loop over the levels: the flags of 64 entries as one ballot word, mask[l * W + (q >> 6)]
//   block_sums   one lane per word: set bits per block of 256 words
//   block_starts one workgroup: exclusive prefix over the (level, block) sums in 64 bits; M, the per-level counts, the bound
//   word_starts  one lane per word: cells emitted before the word
// so that the cell of (l, q) has rank word_start + popcount(mask below q's bit): two loads, and no flag is computed twice.
// Header (uint64 words): [0] status (the checks OR into its low 32 bits), [1] M, [2 + l] m_l over all trees.  Every kernel
// behind a check reads [0] first and does nothing when it is nonzero.  The gather's header is the caller's info_dev, the
// verifier's lies in its scratch.

// The flags of every level l < levels (the height of one tree, the stride of a forest).  The status is the same word in
// every lane and `levels` a kernel argument, so every lane of a wavefront reaches every ballot: the predicate goes inside it,
// and the lanes past k, which load nothing, or past their height vote 0.
template <class Entries>
__device__ __forceinline__ void multiproof_masks(const Entries e, uint32_t k, uint32_t levels, uint64_t words, const uint64_t* __restrict__ hdr,
                                                 uint64_t* __restrict__ mask)
{
    if (hdr[0] != 0ull) return;
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = q < k;
    const uint32_t t = in ? e.tree(q) : 0u;
    const uint32_t h = in ? e.height(q) : 0u;
    const uint64_t index = in ? e.indices[q] : 0ull;
    const bool has_prev = in && q > 0 && e.tree(q - 1) == t;          // a neighbour in another tree is no sibling
    const bool has_next = in && q + 1 < k && e.tree(q + 1) == t;
    const uint64_t prev = has_prev ? e.indices[q - 1] : 0ull;
    const uint64_t next = has_next ? e.indices[q + 1] : 0ull;
    const uint64_t w = q >> 6;
    for (uint32_t l = 0; l < levels; ++l) {      // wave-uniform trip count
        const uint64_t p = index >> l;
        const bool emit_odd = !has_prev || (prev >> l) + 1ull < p;    // first of the run, and p - 1 is not there
        const bool emit_even = !has_next || (next >> l) > p + 1ull;   // last of the run, and p + 1 is not there
        const uint64_t m = __ballot(l < h && ((p & 1ull) ? emit_odd : emit_even));
        if ((threadIdx.x & 63u) == 0u && w < words) mask[(uint64_t)l * words + w] = m;
    }
}

// Rank of the cell that entry j owns at level l (its flag is set: the callers know).
__device__ __forceinline__ uint64_t multiproof_rank(const uint64_t* __restrict__ mask, const uint64_t* __restrict__ word_start, uint64_t words, uint32_t l,
                                                    uint64_t j)
{
    const uint64_t at = (uint64_t)l * words + (j >> 6);
    return word_start[at] + (uint64_t)__popcll(mask[at] & ((1ull << (j & 63ull)) - 1ull));
}

// Gather, one lane per (level, entry): blockIdx.y = l.  A lane whose flag is set (so l is below its tree's height) loads the
// sibling cell and stores it at its rank; a wavefront's ranks are consecutive, so its stores lie back to back.  No hash.
template <class Entries, class Cells>
__device__ __forceinline__ void multiproof_gather(const Entries e, const Cells cells, uint32_t k, uint64_t words, const uint64_t* __restrict__ mask,
                                                  const uint64_t* __restrict__ word_start, const uint64_t* __restrict__ hdr, Node* __restrict__ nodes)
{
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= k || hdr[0] != 0ull) return;
    const uint32_t l = blockIdx.y;
    const uint64_t at = (uint64_t)l * words + (q >> 6);
    const uint64_t m = mask[at];
    const uint64_t bit = 1ull << (q & 63ull);
    if (!(m & bit)) return;
    const uint64_t rank = word_start[at] + (uint64_t)__popcll(m & (bit - 1ull));   // < M <= the buffer's capacity: the status is 0
    vkmr_dev::store_node(nodes + rank, vkmr_dev::load_node(cells.sibling_cell(e.tree(q), l, e.indices[q])));
}

// Verifier, one launch per level l (level l + 1 from level l), one lane per entry.  The value of node p of a tree's level l
// lives in cell[first lane of p's run], and end[that lane] is the first lane behind the run (level 0: the leaves, and q + 1).
// The first lane of parent P's run hashes P: an even child p is its own cell, and the run that starts at end[q] is p + 1 when
// it has the same tree and parent; an odd child at the head of P's run has no left sibling among the entries.  The missing
// child is the proof's node at the rank of the entry that owns it (the last lane of an even p's run, the first of an odd
// p's): the order the gather emits in.  A lane whose tree has reached its root (l >= its height) does nothing, and since the
// entries of a tree carry one height (the check), a tree stops as a whole and the cell of its first entry then holds its root.
// For l > 0 `in` and `cell` are the same buffer, deliberately: a lane writes only its own cell and end, and reads cells that
// no lane of this launch writes (its own before it writes it, and the cell at end[q], which lies inside P's run, not at its
// head), so __restrict__ on both holds for every lane and the levels run in place.  One hash_pair: the only hash block.
//
// `Own` is where applying a proof parts from checking it (vkmr_hip_apply_multiproof_async).  The verifier never learns a
// count: a duplicated last node arrives as an ordinary node of the proof, the node's own OLD value.  A fold over NEW leaves
// must take the node's own new value there, which is its own cell: own(q, p, l) says that the even node p of entry q's tree
// has no right sibling at level l (p + 1 >= n_l).  The proof's node is consumed all the same -- the ranks do not move.
struct NeverOwn {                                // the verifiers: every missing child is the proof's node
    static constexpr bool substitutes = false;
    __device__ __forceinline__ bool own(uint64_t, uint64_t, uint32_t) const { return false; }
};
struct TreeCountOwn {                            // one tree of `count` leaves; `side` 1 folds the new leaves
    static constexpr bool substitutes = true;
    uint64_t count; uint32_t side;
    __device__ __forceinline__ bool own(uint64_t, uint64_t p, uint32_t l) const { return side != 0u && p + 1ull >= vkmr_forest::level_count(count, l); }
};
struct ForestCountOwn {                          // counts[q] = c_t of entry q's tree (the check: >= 1, one per tree)
    static constexpr bool substitutes = true;
    const uint64_t* counts; uint32_t side;
    __device__ __forceinline__ bool own(uint64_t q, uint64_t p, uint32_t l) const { return side != 0u && p + 1ull >= vkmr_forest::level_count(counts[q], l); }
};

template <class Entries, class Own>
__device__ __forceinline__ void multiproof_verify_level(const Entries e, const Own own, const Node* __restrict__ in, Node* __restrict__ cell,
                                                        uint32_t* __restrict__ end,
                                                        uint32_t k, uint32_t l, uint64_t words, const uint64_t* __restrict__ mask,
                                                        const uint64_t* __restrict__ word_start, const Node* __restrict__ nodes,
                                                        const uint64_t* __restrict__ hdr)
{
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= k || hdr[0] != 0ull) return;
    if (l >= e.height(q)) return;                // the tree's root was formed at a level below
    const uint32_t t = e.tree(q);
    const uint64_t p = e.indices[q] >> l;
    const uint64_t P = p >> 1;
    if (q > 0 && e.tree(q - 1) == t && (e.indices[q - 1] >> l) >> 1 == P) return;   // not the head of P's run
    const uint64_t b = (l == 0) ? q + 1 : (uint64_t)end[q];
    const bool right = p & 1ull;
    const Node* other;
    uint64_t b2 = b;
    if (right) {
        other = nodes + multiproof_rank(mask, word_start, words, l, q);
    } else if (b < k && e.tree(b) == t && (e.indices[b] >> l) >> 1 == P) {
        other = in + b;
        b2 = (l == 0) ? b + 1 : (uint64_t)end[b];
    } else {
        other = nodes + multiproof_rank(mask, word_start, words, l, b - 1);
        if constexpr (Own::substitutes)          // a select on the pointer, like the operand order below
            if (own.own(q, p, l)) other = in + q;
    }
    // the operand order is chosen on the pointers: selecting between the loaded nodes word by word went through scratch
    const Node x = vkmr_dev::load_node(right ? other : in + q), y = vkmr_dev::load_node(right ? in + q : other);
    uint32_t o[8];
    vkmr_dev::hash_pair(x.w, y.w, o);
    vkmr_dev::store_node(cell + q, o);
    end[q] = (uint32_t)b2;
}
