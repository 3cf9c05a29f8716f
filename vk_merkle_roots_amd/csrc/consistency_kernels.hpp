// consistency_kernels.hpp -- consistency proofs (include/vkmr_hip.h: vkmr_hip_forest_consistency_async,
// vkmr_hip_verify_consistency_async; the rules: consistency_plan.hpp).
//
// A stored forest answers Q queries (tree, old count c): the tree's count now, c2, and the two rows of `stride` cells that prove
// "the tree of c2 leaves extends the one of c leaves" to a holder of the two roots.  The check first, a lane per query; the
// gather behind it reads *status and does nothing when it is nonzero: a lane per (query, cell), two loads at most, no hash.
// The verifier is the other party's: a lane per query, nothing but the proof and the two roots, both root walks through one
// hash_pair.
#pragma once

#include "consistency_plan.hpp"

// No hash, a lane per query: consistency_plan.hpp's refusal() ORed into *status, zeroed by the host.
__global__ __launch_bounds__(256) void consistency_check_kernel(const uint64_t* __restrict__ offsets, uint32_t ntrees, const uint32_t* __restrict__ trees,
                                                                const uint64_t* __restrict__ old_counts, uint32_t Q, uint32_t stride,
                                                                uint32_t* __restrict__ status)
{
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= Q) return;
    const uint32_t bits = vkmr_consistency::refusal(trees[q], ntrees, offsets, old_counts[q], stride);
    if (bits) atomicOr(status, bits);
}

// Cell l of both rows of query q = i / stride, l = i % stride.  Behind the check: the tree exists, c <= c2 and c2 has at most
// `stride` bits, so every node asked for lies inside its level (node < level_count(c2, l)); the offsets are the build's, trusted
// as vkmr_hip_forest_proofs_async trusts them.  Every cell is written, zeros included.
__global__ __launch_bounds__(256) void consistency_gather_kernel(const Node* __restrict__ digests, const Node* __restrict__ forest, ForestLevels lv,
                                                                 const uint64_t* __restrict__ offsets, const Node* __restrict__ roots,
                                                                 const uint32_t* __restrict__ trees, const uint64_t* __restrict__ old_counts, uint32_t Q,
                                                                 uint32_t stride, uint64_t* __restrict__ new_counts_out, Node* __restrict__ peaks_out,
                                                                 Node* __restrict__ rights_out, const uint32_t* __restrict__ status)
{
    if (*status != 0u) return;                   // the same word in every lane
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint64_t)Q * stride) return;
    const uint32_t q = (uint32_t)(i / stride), l = (uint32_t)(i % stride);
    const uint32_t t = trees[q];
    const uint64_t o = offsets[t], c2 = offsets[t + 1u] - o, c = old_counts[q];
    Node peak = {}, right = {};
    if (c != 0ull) {
        const vkmr_frontier::GatherSource from = vkmr_frontier::node_source(c2, l);
        const Node* level = from == vkmr_frontier::GATHER_LEAF ? digests : forest + lv.base[l];
        if (vkmr_consistency::has_peak(c, l))
            peak = vkmr_dev::load_node(from == vkmr_frontier::GATHER_ROOT ? roots + t
                                                                          : level + vkmr_frontier::node_cell(o, t, l, vkmr_consistency::peak_node(c, l)));
        if (vkmr_consistency::has_right(c, c2, l))   // a level of two nodes at least: never the roots
            right = vkmr_dev::load_node(level + vkmr_frontier::node_cell(o, t, l, vkmr_consistency::right_node(c, l)));
    }
    vkmr_dev::store_node(peaks_out + i, peak);
    vkmr_dev::store_node(rights_out + i, right);
    if (l == 0u) new_counts_out[q] = c2;
}

// ok[q] = 1 when proof q shows that the tree of new_counts[q] leaves under new_roots[q] extends the one of old_counts[q] leaves
// under old_roots[q].  A lane per query and consistency_plan.hpp's step() in one loop: steps 0 .. H(c) - 1 are the root walk of
// the frontier (c, peaks), the rest the walk from P_l0 to the new root.  Each step loads at most one cell -- peaks[l] as the left
// operand or rights[l] as the right one -- and the other operand is the accumulator, so there is one hash_pair, the kernel's
// only hash block; the lanes of a wavefront run walks of different lengths side by side.  Where the first walk ends the
// accumulator is compared with the old root and starts again as P_l0; behind the last step it is compared with the new root.
__global__ __launch_bounds__(256) void consistency_fold_kernel(const uint64_t* __restrict__ old_counts, const uint64_t* __restrict__ new_counts,
                                                               const Node* __restrict__ peaks, const Node* __restrict__ rights, uint32_t stride, uint32_t Q,
                                                               const Node* __restrict__ old_roots, const Node* __restrict__ new_roots, uint32_t* __restrict__ ok)
{
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= Q) return;
    const uint64_t c = old_counts[q], c2 = new_counts[q];
    if (!vkmr_consistency::checkable(c, c2, stride)) {
        ok[q] = 0u;
        return;
    }
    Node acc = {};
    if (c == 0ull) {                             // any tree extends one not yet begun
        ok[q] = vkmr_dev::node_diff(vkmr_dev::load_node(old_roots + q), acc) == 0u ? 1u : 0u;
        return;
    }
    const Node* my_peaks = peaks + q * stride;
    const Node* my_rights = rights + q * stride;
    const uint32_t H1 = vkmr_consistency::height(c), n = vkmr_consistency::steps(c, c2);
    bool have = false;
    uint32_t diff = 0u;
#pragma unroll 1
    for (uint32_t i = 0;; ++i) {
        if (i == H1) {                           // the old root is formed: compare, and begin the new root's walk at P_l0
            if (!have) acc = vkmr_dev::load_node(my_peaks + H1);            // a power of two, at least 2: l0 == H(c)
            diff |= vkmr_dev::node_diff(acc, vkmr_dev::load_node(old_roots + q));
            if (have) acc = vkmr_dev::load_node(my_peaks + vkmr_consistency::low_level(c));
            have = true;
        }
        if (i == n) break;
        const vkmr_consistency::Step s = vkmr_consistency::step(c, c2, i, have);
        if (!s.hash) continue;
        Node a = acc;
        if (s.peak) a = vkmr_dev::load_node(my_peaks + s.l);
        Node b = have ? acc : a;
        if (s.right) b = vkmr_dev::load_node(my_rights + s.l);
        vkmr_dev::hash_pair(a.w, b.w, acc.w);
        have = true;
    }
    diff |= vkmr_dev::node_diff(acc, vkmr_dev::load_node(new_roots + q));
    ok[q] = diff == 0u ? 1u : 0u;
}
