// frontier_kernels.hpp -- trees followed by their frontiers alone (include/vkmr_hip.h: vkmr_hip_frontier_extend_async,
// vkmr_hip_frontier_roots_async, vkmr_hip_verify_frontier_async, vkmr_hip_forest_frontier_async).
//
// A holder of T frontiers (frontier_plan.hpp: a count and one peak per set bit of it, `stride` cells a tree) takes the new
// leaves of all its trees back to back, offsets[q] .. offsets[q+1] tree q's, and forms every tree's new root and new frontier
// from them: one launch per level for all trees, one lane per cell of that level's buffer, in forest_level's form.  No stored
// level is read -- there is none -- and the only old value a level reads is one peak per tree.  The check first; every kernel
// behind it reads *status and does nothing when it is nonzero.
#pragma once

#include "frontier_plan.hpp"

// No hash, a lane per tree: frontier_plan.hpp's refusal() ORed into *status, zeroed by the host.
__global__ __launch_bounds__(256) void frontier_check_kernel(const uint64_t* __restrict__ counts, const uint64_t* __restrict__ offsets, uint32_t T,
                                                             uint64_t total_new, uint64_t max_new, uint32_t stride, uint32_t* __restrict__ status)
{
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= T) return;
    const uint32_t bits = vkmr_frontier::refusal(counts[q], offsets[q], offsets[q + 1], (uint32_t)q, T, total_new, max_new, stride);
    if (bits) atomicOr(status, bits);
}

// The tree of lane `lane`'s cell p0 + lane of level l, p0 the wavefront's first cell: forest_find_tree's search with
// frontier_plan.hpp's first_cell (two spare cells a tree, not one).  first_cell(offsets[0] == 0, 0, l) == 0, so every cell has a
// tree; every tree takes at least two cells, so lane i has one of t0 .. t0 + i.
__device__ __forceinline__ uint32_t frontier_find_tree(const uint64_t* __restrict__ offsets, uint32_t T, uint32_t l, uint64_t p0, uint32_t lane)
{
    uint32_t t0 = 0, top = T - 1u;
    while (t0 < top) {                           // wave-uniform
        const uint32_t mid = t0 + (top - t0 + 1u) / 2u;
        if (vkmr_frontier::first_cell(offsets[mid], mid, l) <= p0) t0 = mid;
        else top = mid - 1u;
    }
    uint32_t t = t0;
    if (t0 + 1u < T && vkmr_frontier::first_cell(offsets[t0 + 1u], t0 + 1u, l) <= p0 + 63ull) {   // a tree begins inside the wavefront
        const uint64_t p = p0 + lane;
        top = (T - 1u - t0 < lane) ? T - 1u : t0 + lane;
        while (t < top) {
            const uint32_t mid = t + (top - t + 1u) / 2u;
            if (vkmr_frontier::first_cell(offsets[mid], mid, l) <= p) t = mid;
            else top = mid - 1u;
        }
    }
    return t;
}

// Level l >= 1 of every tree's extension from level l - 1 (`in`: the new leaves for l == 1, else the buffer of level l - 1),
// `cells` = level_cells lanes.  A lane finds its tree, its node j = (c >> l) + (p - first_cell) and frontier_plan.hpp's step():
// padding returns before any load of a node; the two operands are pointers -- the left one the buffer's cell or the old peak
// P_(l-1), the right one its own cell or the left one again at a ragged edge -- so there is one hash_pair, the kernel's only
// hash block.  The node goes to its cell, to roots[q] when it is the root, to the staging cell (q, l) when it is a new peak.
__global__ __launch_bounds__(256) void frontier_level_kernel(const Node* __restrict__ in, const uint64_t* __restrict__ counts,
                                                             const Node* __restrict__ peaks, uint32_t stride, const uint64_t* __restrict__ offsets,
                                                             uint32_t T, uint32_t l, uint64_t cells, Node* __restrict__ out, Node* __restrict__ staging,
                                                             Node* __restrict__ roots, const uint32_t* __restrict__ status)
{
    if (*status != 0u) return;                   // the same word in every lane
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t p0 = ((uint64_t)blockIdx.x * (256u / 64u) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6))) * 64ull;
    if (p0 >= cells) return;                     // wave-uniform
    const uint64_t p = p0 + lane;
    const uint32_t q = frontier_find_tree(offsets, T, l, p0, lane);
    const uint64_t o = offsets[q], c = counts[q], c2 = c + (offsets[q + 1u] - o);
    const uint64_t j = vkmr_frontier::first_node(c, l) + (p - vkmr_frontier::first_cell(o, q, l));
    const vkmr_frontier::Step s = vkmr_frontier::step(o, q, c, c2, l, j);
    if (!s.active) return;                       // the tree is done, or the padding behind its nodes
    const Node* left = s.left_is_peak ? peaks + (uint64_t)q * stride + (l - 1u) : in + s.in_left;
    const Node* right = s.right_is_left ? left : in + s.in_right;
    const Node a = vkmr_dev::load_node(left), b = vkmr_dev::load_node(right);
    uint32_t x[8];
    vkmr_dev::hash_pair(a.w, b.w, x);
    vkmr_dev::store_node(s.root ? roots + q : out + p, x);
    if (s.peak) vkmr_dev::store_node(staging + (uint64_t)q * VKMR_FRONTIER_MAX_STRIDE + l, x);
}

// Behind the last level, a wavefront per tree (four trees a workgroup), lane l < stride for cell l of the new frontier: the old
// peak where the bit's node did not move, the last new leaf for bit 0, the staged node otherwise, zero for a clear bit, so that
// frontiers compare byte for byte.  Every lane has read its tree's old count and its old peak in front of the barrier, so the
// new arrays may be the old ones.  Lane 0 writes the count, and the two roots no launch forms: zero for a tree still without a
// leaf, P_H(c) for a power of two that took no leaf.
__global__ __launch_bounds__(256) void frontier_commit_kernel(const uint64_t* __restrict__ counts, const Node* __restrict__ peaks, uint32_t stride,
                                                              const uint64_t* __restrict__ offsets, uint32_t T, const Node* __restrict__ leaves,
                                                              const Node* __restrict__ staging, uint64_t* __restrict__ new_counts,
                                                              Node* __restrict__ new_peaks, Node* __restrict__ roots, const uint32_t* __restrict__ status)
{
    if (*status != 0u) return;                   // the same word in every lane: no lane is left at the barrier
    const uint32_t l = threadIdx.x & 63u;
    const uint64_t q = (uint64_t)blockIdx.x * (256u / 64u) + (threadIdx.x >> 6);
    const bool mine = q < T && l < stride;
    uint64_t c = 0, c2 = 0, hi = 0;
    Node x = {};
    if (mine) {
        c = counts[q];
        hi = offsets[q + 1];
        c2 = c + (hi - offsets[q]);
        if (vkmr_frontier::has_peak(c2, l)) {
            const vkmr_frontier::PeakSource from = vkmr_frontier::peak_source(c, c2, l);
            x = vkmr_dev::load_node(from == vkmr_frontier::PEAK_OLD         ? peaks + q * stride + l
                                    : from == vkmr_frontier::PEAK_LAST_LEAF ? leaves + (hi - 1ull)
                                                                            : staging + q * VKMR_FRONTIER_MAX_STRIDE + l);
        }
    }
    __syncthreads();
    if (!mine) return;
    vkmr_dev::store_node(new_peaks + q * stride + l, x);
    if (l == 0u) new_counts[q] = c2;
    if (c2 == 0ull ? l == 0u : (vkmr_frontier::root_is_old_peak(c, c2) && l == vkmr_frontier::height(c)))
        vkmr_dev::store_node(roots + q, x);      // zero, or the peak this lane holds
}

// The root of every tree from its frontier, a lane per tree: frontier_plan.hpp's walk, at most 63 serial hashes through one
// hash_pair.  A count of more bits than the frontier has cells, or above 2^58, reads nothing and gives the zero root.  With
// `want` the lane compares instead of storing: ok[q] = 1 when the root is want[q] (a refused count: 0).
__global__ __launch_bounds__(256) void frontier_roots_kernel(const uint64_t* __restrict__ counts, const Node* __restrict__ peaks, uint32_t stride, uint32_t T,
                                                             Node* __restrict__ roots, const Node* __restrict__ want, uint32_t* __restrict__ ok)
{
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= T) return;
    const uint64_t c = counts[q];
    const bool good = c <= vkmr_frontier::max_count() && vkmr_frontier::bit_length(c) <= stride;
    const Node* mine = peaks + q * stride;
    Node carry = {};
    bool have = false;
    if (good && c != 0ull) {
        const uint32_t H = vkmr_frontier::height(c);
#pragma unroll 1
        for (uint32_t l = 0; l < H; ++l) {
            const bool bit = vkmr_frontier::has_peak(c, l);
            if (!bit && !have) continue;
            Node a = carry;
            if (bit) a = vkmr_dev::load_node(mine + l);
            const Node b = have ? carry : a;
            vkmr_dev::hash_pair(a.w, b.w, carry.w);
            have = true;
        }
        if (!have) carry = vkmr_dev::load_node(mine + H);
    }
    if (want == nullptr) {
        vkmr_dev::store_node(roots + q, carry);
        return;
    }
    const Node w = vkmr_dev::load_node(want + q);
    ok[q] = (good && vkmr_dev::node_diff(carry, w) == 0u) ? 1u : 0u;
}

// The frontier of every tree of a stored forest, a lane per (tree, cell): frontier_plan.hpp's gather_source.  The offsets are
// the build's, trusted as vkmr_hip_forest_proofs_async trusts them; a count of more bits than `stride` loses its upper peaks
// (the host refuses a max_count that allows one).
__global__ __launch_bounds__(256) void frontier_gather_kernel(const Node* __restrict__ digests, const Node* __restrict__ forest, ForestLevels lv,
                                                              const uint64_t* __restrict__ offsets, uint32_t ntrees, const Node* __restrict__ roots,
                                                              uint32_t stride, uint64_t* __restrict__ counts_out, Node* __restrict__ peaks_out)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint64_t)ntrees * stride) return;
    const uint32_t t = (uint32_t)(i / stride), l = (uint32_t)(i % stride);
    const uint64_t o = offsets[t], c = offsets[t + 1u] - o;
    Node x = {};
    const vkmr_frontier::GatherSource from = vkmr_frontier::gather_source(c, l);
    if (from != vkmr_frontier::GATHER_NONE)
        x = vkmr_dev::load_node(from == vkmr_frontier::GATHER_LEAF   ? digests + vkmr_frontier::gather_cell(o, t, c, 0u)
                                : from == vkmr_frontier::GATHER_ROOT ? roots + t
                                                                     : forest + lv.base[l] + vkmr_frontier::gather_cell(o, t, c, l));
    vkmr_dev::store_node(peaks_out + i, x);
    if (l == 0u) counts_out[t] = c;
}
