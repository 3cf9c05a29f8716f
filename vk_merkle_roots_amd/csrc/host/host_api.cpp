// host_api.cpp -- the vkmr_host_cpu_* entry points of libvkmr_host.so: the "CPU" backend on packed batches and slice roots and
// the CPU twins of the stored-structure operations.  include/vkmr_host.h declares every one and holds its contract; linkage
// and visibility come from there, and the definitions below stand in the header's order.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "../absence_plan.hpp"
#include "../range_plan.hpp"
#include "../audit_plan.hpp"   // forest_plan.hpp, tree_plan.hpp: where the stored levels lie
#include "../consistency_plan.hpp"
#include "../frontier_plan.hpp"
#include "../leafsort_plan.hpp"
#include "../merge_plan.hpp"
#include "../merkle_math.hpp"
#include "../proofs_at_plan.hpp"
#include "cpu_sha256d.hpp"
#include "vkmr_host.h"

namespace {

// The node over `cur` and the node beside it: `other` is the left operand when cur is a right child.
void pair_beside(const vkmr_digest& cur, const vkmr_digest& other, bool right, vkmr_digest* out)
{
    if (right)
        vkmr::cpu_sha256d_pair(other.data, cur.data, out->data);
    else
        vkmr::cpu_sha256d_pair(cur.data, other.data, out->data);
}

// One level of a multiproof over the sorted, unique nodes pos[] of one tree: pairs p with p + 1 when both are there, else
// takes p alone.  node(i, out, both) is called for each -- pos[i] is the node, both says that pos[i + 1] is its right sibling,
// out is where the parent goes (out <= i: written behind what is still to be read) -- and may end the walk by returning
// false, which level_walk then returns too.  pos[] becomes the parents.
template <class Each>
bool level_walk(std::vector<uint64_t>& pos, Each node)
{
    size_t out = 0;
    for (size_t i = 0; i < pos.size();) {   // the children of one parent are adjacent
        const uint64_t p = pos[i];
        const bool both = !(p & 1ull) && i + 1 < pos.size() && pos[i + 1] == p + 1;
        if (!node(i, out, both)) return false;
        i += both ? 2 : 1;
        pos[out++] = p >> 1;
    }
    pos.resize(out);
    return true;
}

// The entries [a, b) of one tree (sorted, unique): adds to per_level[l], l < h, the nodes its multiproof emits at level l.
// Index arithmetic only: a node is emitted for every p of A_l whose sibling p ^ 1 is not in A_l.
void forest_multiproof_counts(const uint64_t* indices, uint32_t a, uint32_t b, uint32_t h, uint64_t* per_level)
{
    std::vector<uint64_t> cur(indices + a, indices + b);
    for (uint32_t l = 0; l < h; ++l)
        level_walk(cur, [&](size_t, size_t, bool both) {
            if (!both) ++per_level[l];
            return true;
        });
}

// First entry behind the run of entries that name trees[a].
uint32_t forest_run_end(const uint32_t* trees, uint32_t a, uint32_t k)
{
    uint32_t b = a + 1;
    while (b < k && trees[b] == trees[a]) ++b;
    return b;
}

// levels[l], l < h, of the tree over the leaves [first, last): level 0 the leaves themselves.
void tree_levels(const vkmr_digest* first, const vkmr_digest* last, uint32_t h, std::vector<std::vector<vkmr_digest>>& levels)
{
    levels.assign(h, {});
    levels[0].assign(first, last);
    for (uint32_t l = 1; l < h; ++l) {
        const std::vector<vkmr_digest>& in = levels[l - 1];
        levels[l].resize((in.size() + 1) / 2);
        for (size_t j = 0; j < levels[l].size(); ++j)
            vkmr::cpu_sha256d_pair(in[2 * j].data, in[vkmr_math::right_child(j, in.size())].data, levels[l][j].data);
    }
}

}  // namespace

void vkmr_host_cpu_leaves(const uint32_t* data, const vkmr_metadata* meta, uint64_t count, vkmr_digest* out)
{
    for (uint64_t i = 0; i < count; ++i)
        vkmr::cpu_sha256d_words(reinterpret_cast<const unsigned char*>(data + meta[i].start), meta[i].size, out[i].data);
}

int vkmr_host_cpu_reduce(const vkmr_digest* digests, uint64_t count, uint32_t height, vkmr_digest* root)
{
    if (!digests || !root || count == 0) return -1;
    std::vector<uint32_t> nodes(8 * count);
    std::memcpy(nodes.data(), digests, 32 * count);
    uint64_t n = count;
    for (uint32_t lv = 0; lv < height; ++lv) {
        const uint64_t pairs = (n + 1) / 2;
        for (uint64_t p = 0; p < pairs; ++p) {
            uint32_t h[8];
            vkmr::cpu_sha256d_pair(nodes.data() + 16 * p, nodes.data() + 8 * vkmr_math::right_child(p, n), h);
            std::memcpy(nodes.data() + 8 * p, h, 32);
        }
        n = pairs;
    }
    if (n != 1) return -1;
    std::memcpy(root->data, nodes.data(), 32);
    return 0;
}

int vkmr_host_cpu_combine(const vkmr_digest* roots, uint32_t n, vkmr_digest* out)
{
    if (!roots || !out || n == 0) return -1;
    std::vector<uint32_t> nodes(8 * (size_t)n);
    std::memcpy(nodes.data(), roots, 32 * (size_t)n);
    vkmr::cpu_merkle_root_inplace(nodes.data(), n);
    std::memcpy(out->data, nodes.data(), 32);
    return 0;
}

void vkmr_host_cpu_fold_proof(const vkmr_digest* leaf, uint64_t index, const vkmr_digest* siblings, uint32_t height, vkmr_digest* root)
{
    vkmr_digest cur = *leaf;
    for (uint32_t l = 0; l < height; ++l) {
        vkmr_digest next;
        pair_beside(cur, siblings[l], (l < 64) && ((index >> l) & 1ull), &next);
        cur = next;
    }
    *root = cur;
}

int vkmr_host_cpu_verify_multiproof(const vkmr_digest* leaves, const uint64_t* indices, uint32_t k, uint32_t height, const vkmr_digest* nodes,
                                    uint64_t m, const vkmr_digest* root)
{
    if (!leaves || !indices || !root || k == 0 || height > 63 || (!nodes && m > 0)) return 0;
    for (uint32_t q = 0; q < k; ++q)
        if ((indices[q] >> height) != 0 || (q > 0 && indices[q - 1] >= indices[q])) return 0;
    std::vector<uint64_t> pos(indices, indices + k);
    std::vector<vkmr_digest> cur(leaves, leaves + k);
    uint64_t used = 0;
    for (uint32_t l = 0; l < height; ++l) {
        const bool enough = level_walk(pos, [&](size_t i, size_t out, bool both) {
            if (!both && used >= m) return false;
            vkmr_digest h;
            pair_beside(cur[i], both ? cur[i + 1] : nodes[used++], pos[i] & 1ull, &h);
            cur[out] = h;
            return true;
        });
        if (!enough) return 0;
        cur.resize(pos.size());
    }
    return used == m && pos.size() == 1 && pos[0] == 0 && std::memcmp(cur[0].data, root->data, 32) == 0 ? 1 : 0;
}

int vkmr_host_cpu_forest_roots(const vkmr_digest* digests, const uint64_t* offsets, uint32_t ntrees, vkmr_digest* roots)
{
    if (ntrees == 0) return 0;
    if (!offsets || !roots) return -1;
    for (uint32_t t = 0; t < ntrees; ++t)
        if (offsets[t + 1] < offsets[t]) return 1;
    if (!digests && offsets[ntrees] > offsets[0]) return -1;
    for (uint32_t t = 0; t < ntrees; ++t) {
        const uint64_t c = offsets[t + 1] - offsets[t];
        if (c == 0) {
            std::memset(roots[t].data, 0, 32);
            continue;
        }
        if (vkmr_host_cpu_reduce(digests + offsets[t], c, vkmr_math::height(c), &roots[t]) != 0) return -1;
    }
    return 0;
}

int vkmr_host_cpu_forest_mutated(const vkmr_digest* digests, const uint64_t* offsets, uint32_t ntrees, vkmr_digest* roots, uint64_t* mutated)
{
    if (ntrees == 0) return 0;
    if (!offsets || !mutated) return -1;
    for (uint32_t t = 0; t < ntrees; ++t)
        if (offsets[t + 1] < offsets[t]) return 1;
    if (!digests && offsets[ntrees] > offsets[0]) return -1;
    std::vector<vkmr_digest> cur;
    for (uint32_t t = 0; t < ntrees; ++t) {
        const uint64_t c = offsets[t + 1] - offsets[t];
        mutated[t] = 0;
        if (c == 0) {
            if (roots) std::memset(roots[t].data, 0, 32);
            continue;
        }
        cur.assign(digests + offsets[t], digests + offsets[t + 1]);
        const uint32_t h = vkmr_math::height(c);
        for (uint32_t l = 0; l < h; ++l) {
            const size_t n = cur.size();
            for (size_t j = 0; 2 * j + 1 < n; ++j)
                if (std::memcmp(cur[2 * j].data, cur[2 * j + 1].data, 32) == 0) {
                    mutated[t] |= 1ull << l;
                    break;
                }
            for (size_t j = 0; 2 * j < n; ++j) {   // in place: parent j is written behind what is still to be read
                vkmr_digest p;
                vkmr::cpu_sha256d_pair(cur[2 * j].data, cur[vkmr_math::right_child(j, n)].data, p.data);
                cur[j] = p;
            }
            cur.resize((n + 1) / 2);
        }
        if (roots) roots[t] = cur[0];
    }
    return 0;
}

int vkmr_host_cpu_forest_proofs(const vkmr_digest* digests, const uint64_t* offsets, uint32_t ntrees, const uint32_t* trees, const uint64_t* indices,
                                uint32_t k, uint32_t stride, vkmr_digest* siblings, uint32_t* heights)
{
    if (k == 0) return 0;
    if (!trees || !indices || !heights || (!siblings && stride > 0) || (!offsets && ntrees > 0)) return -1;
    for (uint32_t t = 0; t < ntrees; ++t)
        if (offsets[t + 1] < offsets[t]) return 1;
    if (ntrees > 0 && !digests && offsets[ntrees] > offsets[0]) return -1;
    auto count_of = [&](uint32_t q) -> uint64_t {      // c_t of a query that names a leaf, else 0
        if (trees[q] >= ntrees) return 0;
        const uint64_t c = offsets[trees[q] + 1] - offsets[trees[q]];
        return indices[q] < c ? c : 0;
    };
    std::vector<uint32_t> order;                       // the queries that name a leaf, by tree
    for (uint32_t q = 0; q < k; ++q) {
        const uint64_t c = count_of(q);
        if (c == 0) continue;
        if (vkmr_math::height(c) > stride) return 2;
        order.push_back(q);
    }
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return trees[x] < trees[y]; });
    std::memset(heights, 0, sizeof(uint32_t) * (size_t)k);
    if (stride > 0) std::memset(siblings, 0, sizeof(vkmr_digest) * (size_t)k * stride);
    std::vector<std::vector<vkmr_digest>> levels;      // levels[l] of the tree the queries at hand ask for, l < h_t
    for (size_t i = 0; i < order.size(); ++i) {
        const uint32_t q = order[i], t = trees[q];
        const uint64_t c = offsets[t + 1] - offsets[t];
        const uint32_t h = vkmr_math::height(c);
        if (i == 0 || trees[order[i - 1]] != t) tree_levels(digests + offsets[t], digests + offsets[t + 1], h, levels);
        heights[q] = h;
        for (uint32_t l = 0; l < h; ++l) {
            siblings[(size_t)q * stride + l] = levels[l][vkmr_math::sibling(indices[q] >> l, levels[l].size())];
        }
    }
    return 0;
}

int vkmr_host_cpu_forest_multiproof(const vkmr_digest* digests, const uint64_t* offsets, uint32_t ntrees, const uint32_t* trees,
                                    const uint64_t* indices, uint32_t k, uint32_t stride, vkmr_digest* nodes, uint64_t nodes_capacity,
                                    uint32_t* heights, uint64_t* info)
{
    if (k == 0 || !digests || !offsets || !trees || !indices || !heights || !info || (!nodes && nodes_capacity > 0)) return -1;
    if (stride > 63) return -3;
    for (uint32_t t = 0; t < ntrees; ++t)
        if (offsets[t + 1] < offsets[t]) return -2;
    int status = 0;
    for (uint32_t q = 0; q < k; ++q) {
        if (trees[q] >= ntrees || indices[q] >= offsets[trees[q] + 1] - offsets[trees[q]]) status |= 1;
        if (q > 0 && (trees[q - 1] > trees[q] || (trees[q - 1] == trees[q] && indices[q - 1] >= indices[q]))) status |= 2;
    }
    if (status == 0)
        for (uint32_t q = 0; q < k; ++q)
            if (vkmr_math::height(offsets[trees[q] + 1] - offsets[trees[q]]) > stride) return -3;
    info[0] = (uint64_t)status;
    if (status) return status;
    std::vector<uint64_t> per_level(stride + 1u, 0);
    for (uint32_t a = 0; a < k;) {
        const uint32_t b = forest_run_end(trees, a, k), t = trees[a];
        const uint32_t h = vkmr_math::height(offsets[t + 1] - offsets[t]);
        for (uint32_t q = a; q < b; ++q) heights[q] = h;
        forest_multiproof_counts(indices, a, b, h, per_level.data());
        a = b;
    }
    std::vector<uint64_t> at(stride + 1u, 0);             // where the next node of level l goes
    uint64_t M = 0;
    for (uint32_t l = 0; l < stride; ++l) {
        at[l] = M;
        M += per_level[l];
        info[2 + l] = per_level[l];
    }
    info[1] = M;
    if (M > nodes_capacity) {
        info[0] = 4;
        return 4;
    }
    std::vector<std::vector<vkmr_digest>> levels;
    for (uint32_t a = 0; a < k;) {
        const uint32_t b = forest_run_end(trees, a, k), t = trees[a];
        const uint32_t h = heights[a];
        tree_levels(digests + offsets[t], digests + offsets[t + 1], h, levels);
        std::vector<uint64_t> cur(indices + a, indices + b);
        for (uint32_t l = 0; l < h; ++l)
            level_walk(cur, [&](size_t i, size_t, bool both) {
                if (!both) nodes[at[l]++] = levels[l][vkmr_math::sibling(cur[i], levels[l].size())];
                return true;
            });
        a = b;
    }
    return 0;
}

int vkmr_host_cpu_verify_forest_multiproof(const vkmr_digest* leaves, const uint32_t* trees, const uint64_t* indices, const uint32_t* heights,
                                           uint32_t k, uint32_t stride, const vkmr_digest* nodes, uint64_t m, const vkmr_digest* roots,
                                           uint32_t ntrees)
{
    if (!leaves || !trees || !indices || !heights || !roots || k == 0 || stride == 0 || stride > 63 || (!nodes && m > 0)) return 0;
    for (uint32_t q = 0; q < k; ++q) {
        const uint32_t h = heights[q];
        if (trees[q] >= ntrees || h < 1 || h > stride || (indices[q] >> h) != 0) return 0;
        if (q == 0) continue;
        if (trees[q - 1] > trees[q] || (trees[q - 1] == trees[q] && (indices[q - 1] >= indices[q] || heights[q - 1] != h))) return 0;
    }
    std::vector<uint64_t> per_level(stride + 1u, 0);
    for (uint32_t a = 0; a < k;) {
        const uint32_t b = forest_run_end(trees, a, k);
        forest_multiproof_counts(indices, a, b, heights[a], per_level.data());
        a = b;
    }
    std::vector<uint64_t> at(stride + 1u, 0);             // the next unread node of level l
    uint64_t M = 0;
    for (uint32_t l = 0; l < stride; ++l) {
        at[l] = M;
        M += per_level[l];
    }
    if (M != m) return 0;
    for (uint32_t a = 0; a < k;) {
        const uint32_t b = forest_run_end(trees, a, k), h = heights[a];
        std::vector<uint64_t> pos(indices + a, indices + b);
        std::vector<vkmr_digest> cur(leaves + a, leaves + b);
        for (uint32_t l = 0; l < h; ++l) {
            level_walk(pos, [&](size_t i, size_t out, bool both) {
                vkmr_digest x;
                pair_beside(cur[i], both ? cur[i + 1] : nodes[at[l]++], pos[i] & 1ull, &x);   // at[l] < the level's end: the counts above
                cur[out] = x;
                return true;
            });
            cur.resize(pos.size());
        }
        if (pos.size() != 1 || pos[0] != 0 || std::memcmp(cur[0].data, roots[trees[a]].data, 32) != 0) return 0;
        a = b;
    }
    return 1;
}

namespace {

// One tree's fold on both sides at once, by the rule of vkmr_hip_apply_multiproof_async: the entries [a, b) of a tree of
// `count` leaves through h levels, `old_cur` and `new_cur` their old and new leaves, a missing child being nodes[at[l]++] --
// consumed on both sides -- except that the new side takes its own node where p is even and p + 1 >= ceil(count / 2^l).
// False when the proof runs out (at[l] reaches end[l]); the two roots are left in old_cur[0] and new_cur[0].
bool apply_fold(const uint64_t* indices, uint32_t a, uint32_t b, uint64_t count, uint32_t h, std::vector<vkmr_digest>& old_cur,
                std::vector<vkmr_digest>& new_cur, const vkmr_digest* nodes, uint64_t* at, const uint64_t* end)
{
    std::vector<uint64_t> pos(indices + a, indices + b);
    for (uint32_t l = 0; l < h; ++l) {
        const uint64_t n = vkmr_forest::level_count(count, l);
        const bool enough = level_walk(pos, [&](size_t i, size_t out, bool both) {
            if (!both && at[l] >= end[l]) return false;
            const vkmr_digest* node = both ? nullptr : &nodes[at[l]++];
            const bool right = pos[i] & 1ull, own = !both && !right && pos[i] + 1 >= n;
            vkmr_digest x, y;
            pair_beside(old_cur[i], both ? old_cur[i + 1] : *node, right, &x);
            pair_beside(new_cur[i], both ? new_cur[i + 1] : own ? new_cur[i] : *node, right, &y);
            old_cur[out] = x;
            new_cur[out] = y;
            return true;
        });
        if (!enough) return false;
        old_cur.resize(pos.size());
        new_cur.resize(pos.size());
    }
    return pos.size() == 1 && pos[0] == 0;
}

}  // namespace

int vkmr_host_cpu_apply_multiproof(const vkmr_digest* old_leaves, const vkmr_digest* new_leaves, const uint64_t* indices, uint32_t k, uint64_t count,
                                   uint32_t height, const vkmr_digest* nodes, uint64_t m, const vkmr_digest* root, vkmr_digest* new_root)
{
    if (!old_leaves || !new_leaves || !indices || !root || !new_root || k == 0 || height == 0 || height > 63 || (!nodes && m > 0)) return 0;
    if (count == 0 || count > (1ull << height)) return 0;
    for (uint32_t q = 0; q < k; ++q)
        if (indices[q] >= count || (q > 0 && indices[q - 1] >= indices[q])) return 0;
    std::vector<uint64_t> at(height, 0), end(height, 0);   // the next unread node of level l, and the level's end
    std::vector<vkmr_digest> old_cur(old_leaves, old_leaves + k), new_cur(new_leaves, new_leaves + k);
    std::vector<uint64_t> per_level(height + 1u, 0);
    forest_multiproof_counts(indices, 0, k, height, per_level.data());
    uint64_t M = 0;
    for (uint32_t l = 0; l < height; ++l) {
        at[l] = M;
        M += per_level[l];
        end[l] = M;
    }
    if (M != m) return 0;
    if (!apply_fold(indices, 0, k, count, height, old_cur, new_cur, nodes, at.data(), end.data())) return 0;
    if (std::memcmp(old_cur[0].data, root->data, 32) != 0) return 0;
    *new_root = new_cur[0];
    return 1;
}

int vkmr_host_cpu_apply_forest_multiproof(const vkmr_digest* old_leaves, const vkmr_digest* new_leaves, const uint32_t* trees,
                                          const uint64_t* indices, const uint64_t* counts, uint32_t k, uint32_t stride, const vkmr_digest* nodes,
                                          uint64_t m, const vkmr_digest* roots, uint32_t ntrees, vkmr_digest* new_roots)
{
    if (!old_leaves || !new_leaves || !trees || !indices || !counts || !roots || !new_roots || k == 0 || stride == 0 || stride > 63 ||
        (!nodes && m > 0))
        return 0;
    std::vector<uint32_t> heights(k);
    for (uint32_t q = 0; q < k; ++q) {
        if (counts[q] == 0 || indices[q] >= counts[q] || trees[q] >= ntrees) return 0;
        heights[q] = vkmr_math::height(counts[q]);
        if (heights[q] > stride) return 0;
        if (q == 0) continue;
        if (trees[q - 1] > trees[q] || (trees[q - 1] == trees[q] && (indices[q - 1] >= indices[q] || counts[q - 1] != counts[q]))) return 0;
    }
    std::vector<uint64_t> per_level(stride + 1u, 0);
    for (uint32_t a = 0; a < k;) {
        const uint32_t b = forest_run_end(trees, a, k);
        forest_multiproof_counts(indices, a, b, heights[a], per_level.data());
        a = b;
    }
    std::vector<uint64_t> at(stride, 0), end(stride, 0);   // the next unread node of level l, and the level's end
    uint64_t M = 0;
    for (uint32_t l = 0; l < stride; ++l) {
        at[l] = M;
        M += per_level[l];
        end[l] = M;
    }
    if (M != m) return 0;
    std::vector<std::pair<uint32_t, vkmr_digest>> fresh;    // written only when every tree's old fold has met its root
    for (uint32_t a = 0; a < k;) {
        const uint32_t b = forest_run_end(trees, a, k);
        std::vector<vkmr_digest> old_cur(old_leaves + a, old_leaves + b), new_cur(new_leaves + a, new_leaves + b);
        if (!apply_fold(indices, a, b, counts[a], heights[a], old_cur, new_cur, nodes, at.data(), end.data())) return 0;
        if (std::memcmp(old_cur[0].data, roots[trees[a]].data, 32) != 0) return 0;
        fresh.emplace_back(trees[a], new_cur[0]);
        a = b;
    }
    for (const auto& f : fresh) new_roots[f.first] = f.second;
    return 1;
}

int vkmr_host_cpu_forest_find(const vkmr_digest* digests, uint64_t total, const uint64_t* offsets, uint32_t ntrees, const vkmr_digest* queries,
                              uint32_t k, uint32_t* trees, uint64_t* indices)
{
    if (k == 0) return 0;
    if (!queries || !trees || !indices || (ntrees > 0 && !offsets)) return -1;
    for (uint32_t t = 0; t < ntrees; ++t)
        if (offsets[t + 1] < offsets[t]) return 1;
    const uint64_t lo = ntrees ? offsets[0] : 0, hi = ntrees ? offsets[ntrees] : 0;
    if (hi > total) return 1;
    if (!digests && hi > lo) return -1;
    const auto less = [&](uint32_t a, uint32_t b) { return std::memcmp(queries[a].data, queries[b].data, 32) < 0; };
    std::vector<uint32_t> order(k);
    for (uint32_t q = 0; q < k; ++q) order[q] = q;
    std::sort(order.begin(), order.end(), less);
    std::vector<uint64_t> best(k, UINT64_MAX);             // per place in `order`; kept at the first of a run of equal queries
    for (uint64_t p = lo; p < hi; ++p) {
        const auto at = std::lower_bound(order.begin(), order.end(), digests[p],
                                         [&](uint32_t a, const vkmr_digest& d) { return std::memcmp(queries[a].data, d.data, 32) < 0; });
        if (at == order.end() || std::memcmp(queries[*at].data, digests[p].data, 32) != 0) continue;
        uint64_t& b = best[at - order.begin()];
        if (b == UINT64_MAX) b = p;                        // p rises: the first one seen is the lowest
    }
    for (uint32_t i = 0; i < k; ++i) {
        if (i > 0 && std::memcmp(queries[order[i]].data, queries[order[i - 1]].data, 32) == 0) best[i] = best[i - 1];
        const uint32_t q = order[i];
        if (best[i] == UINT64_MAX) {
            trees[q] = UINT32_MAX;
            indices[q] = UINT64_MAX;
            continue;
        }
        const uint64_t* next = std::upper_bound(offsets, offsets + ntrees + 1, best[i]);   // the first offset above p: behind p's tree
        trees[q] = (uint32_t)(next - offsets) - 1u;
        indices[q] = best[i] - next[-1];
    }
    return 0;
}

int vkmr_host_cpu_tree_find(const vkmr_digest* digests, uint64_t count, const vkmr_digest* queries, uint32_t k, uint64_t* indices)
{
    if (k == 0) return 0;
    if (!indices) return -1;
    const uint64_t offsets[2] = {0, count};
    std::vector<uint32_t> trees(k);
    return vkmr_host_cpu_forest_find(digests, count, offsets, 1, queries, k, trees.data(), indices);
}

// Both sort entry points (vkmr_host.h has the contract).  trees == NULL: one tree (offsets {0, total}), the marker being
// indices[q] == UINT64_MAX, and trees_out is not written.  k == 0 is the callers' to see to.
static int sort_entries_cpu(uint64_t total, const uint64_t* offsets, uint32_t ntrees, const uint32_t* trees, const uint64_t* indices, uint32_t k,
                           uint32_t* trees_out, uint64_t* indices_out, uint32_t* order_out, uint64_t* info)
{
    if (!indices || !indices_out || !order_out || !info || (ntrees > 0 && !offsets)) return -1;
    for (uint32_t t = 0; t < ntrees; ++t)
        if (offsets[t + 1] < offsets[t]) return 1;
    if (ntrees && offsets[ntrees] > total) return 1;
    uint64_t markers = 0, outside = 0, repeats = 0, n = 0;
    std::vector<uint64_t> key(k);
    std::vector<uint32_t> order;
    order.reserve(k);
    for (uint32_t q = 0; q < k; ++q) {
        const uint32_t t = trees ? trees[q] : 0u;
        if (trees ? t == UINT32_MAX : indices[q] == UINT64_MAX) {
            ++markers;
        } else if (t >= ntrees || indices[q] >= offsets[t + 1] - offsets[t]) {
            ++outside;
        } else {
            key[q] = offsets[t] + indices[q];
            order.push_back(q);
        }
    }
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
    for (size_t j = 0; j < order.size(); ++j) {
        const uint32_t q = order[j];
        if (j + 1 < order.size() && key[order[j + 1]] == key[q]) {   // repeats stay in call order: the last of a run is the last occurrence
            ++repeats;
            continue;
        }
        if (trees) trees_out[n] = trees[q];
        indices_out[n] = indices[q];
        order_out[n] = q;
        ++n;
    }
    info[0] = n;
    info[1] = markers;
    info[2] = outside;
    info[3] = repeats;
    return 0;
}

int vkmr_host_cpu_forest_sort_entries(uint64_t total, const uint64_t* offsets, uint32_t ntrees, const uint32_t* trees, const uint64_t* indices,
                                      uint32_t k, uint32_t* trees_out, uint64_t* indices_out, uint32_t* order_out, uint64_t* info)
{
    if (k == 0) return 0;
    if (!trees || !trees_out) return -1;
    return sort_entries_cpu(total, offsets, ntrees, trees, indices, k, trees_out, indices_out, order_out, info);
}

int vkmr_host_cpu_tree_sort_entries(uint64_t count, const uint64_t* indices, uint32_t k, uint64_t* indices_out, uint32_t* order_out, uint64_t* info)
{
    if (k == 0) return 0;
    const uint64_t offsets[2] = {0, count};
    return sort_entries_cpu(count, offsets, 1, nullptr, indices, k, nullptr, indices_out, order_out, info);
}

int vkmr_host_cpu_forest_audit(const vkmr_digest* digests, const vkmr_digest* forest, const vkmr_digest* roots, uint64_t total,
                               const uint64_t* offsets, uint32_t ntrees, uint64_t max_count, uint64_t* masks, uint32_t* bad_trees,
                               uint32_t* bad_levels, uint64_t* bad_nodes, uint32_t capacity, uint64_t* info)
{
    if (ntrees == 0) return 0;
    if ((!digests && total > 0) || !forest || !roots || !offsets || !masks || !info || (capacity > 0 && (!bad_trees || !bad_levels || !bad_nodes)))
        return -1;
    if (max_count == 0 || total > (1ull << 58)) return -1;
    if (max_count > total) max_count = total;
    info[0] = info[1] = info[2] = info[3] = 0;
    std::memset(masks, 0, sizeof(uint64_t) * ntrees);
    for (uint32_t t = 0; t < ntrees; ++t) {
        if (offsets[t + 1] < offsets[t] || (t + 1 == ntrees && offsets[t + 1] > total)) info[0] |= 1u;
        if (offsets[t + 1] >= offsets[t] && offsets[t + 1] - offsets[t] > max_count) info[0] |= 2u;
    }
    if (info[0]) return 0;
    const uint32_t H = vkmr_forest::launches(total, max_count);
    static const vkmr_digest zero = {{0, 0, 0, 0, 0, 0, 0, 0}};
    for (uint32_t l = 1; l <= H; ++l) {
        const vkmr_digest* in = l == 1 ? digests : forest + vkmr_forest::stored_level_base(total, ntrees, l - 1);
        const vkmr_digest* out = forest + vkmr_forest::stored_level_base(total, ntrees, l);
        for (uint32_t t = 0; t < ntrees; ++t) {
            const uint64_t o = offsets[t], c = offsets[t + 1] - o;
            const uint64_t n_in = vkmr_forest::level_count(c, l - 1), n_out = vkmr_forest::level_count(c, l);
            const bool empty = c == 0 && l == 1;
            if (!empty && (c == 0 || (l > 1 && n_in == 1))) continue;   // no such level in this tree
            for (uint64_t j = 0; j < (empty ? 1 : n_out); ++j) {
                const vkmr_digest* stored = (empty || n_out == 1) ? roots + t : out + vkmr_forest::pos(o, t, l) + j;
                vkmr_digest want = zero;
                if (!empty) {
                    const vkmr_digest* level = in + vkmr_forest::pos(o, t, l - 1);
                    vkmr::cpu_sha256d_pair(level[2 * j].data, level[vkmr_math::right_child(j, n_in)].data, want.data);
                }
                ++info[3];
                if (std::memcmp(want.data, stored->data, 32) == 0) continue;
                if (masks[t] == 0) ++info[2];
                masks[t] |= 1ull << (l - 1);
                if (info[1] < capacity) {
                    bad_trees[info[1]] = t;
                    bad_levels[info[1]] = l;
                    bad_nodes[info[1]] = j;
                }
                ++info[1];
            }
        }
    }
    if (capacity > 0 && info[1] > capacity) info[0] |= 4u;
    return 0;
}

int vkmr_host_cpu_tree_audit(const vkmr_digest* digests, const vkmr_digest* tree, uint64_t count, uint32_t height, uint32_t* bad_levels,
                             uint64_t* bad_nodes, uint32_t capacity, uint64_t* info)
{
    if (count == 0) return 0;
    if (!digests || (height > 0 && !tree) || !info || (capacity > 0 && (!bad_levels || !bad_nodes))) return -1;
    if (height > 63 || count > (1ull << 58) || vkmr_math::ceil_shift(count, height) != 1) return -1;
    info[0] = info[1] = info[2] = info[3] = 0;
    uint64_t off[VKMR_TREE_MAX_LEVELS];
    vkmr_tree::levels(count, height, off);
    for (uint32_t l = 1; l <= height; ++l) {
        const vkmr_digest* in = l == 1 ? digests : tree + off[l - 1];
        const uint64_t n_in = vkmr_math::ceil_shift(count, l - 1), n_out = vkmr_math::ceil_shift(count, l);
        for (uint64_t j = 0; j < n_out; ++j) {
            vkmr_digest want;
            vkmr::cpu_sha256d_pair(in[2 * j].data, in[vkmr_math::right_child(j, n_in)].data, want.data);
            ++info[3];
            if (std::memcmp(want.data, tree[off[l] + j].data, 32) == 0) continue;
            info[2] |= 1ull << (l - 1);
            if (info[1] < capacity) {
                bad_levels[info[1]] = l;
                bad_nodes[info[1]] = j;
            }
            ++info[1];
        }
    }
    if (capacity > 0 && info[1] > capacity) info[0] |= 4u;
    return 0;
}

// ---- frontiers (frontier_plan.hpp).  The extension here is NOT the device's level rule: a leaf at a time, the carry chain of a
// binary counter (the node climbs while the count's bit is set, merging with the peak it meets), so the two check each other.

// The root of one frontier by the rule of vkmr_hip_frontier_roots_async; `peaks` are its stride cells, c fits them.
static void frontier_root(uint64_t c, const vkmr_digest* peaks, vkmr_digest* root)
{
    std::memset(root->data, 0, 32);
    if (c == 0) return;
    const uint32_t H = vkmr_math::height(c);
    bool have = false;
    vkmr_digest carry;
    for (uint32_t l = 0; l < H; ++l) {
        if (vkmr_frontier::has_peak(c, l)) {
            vkmr_digest next;
            vkmr::cpu_sha256d_pair(peaks[l].data, have ? carry.data : peaks[l].data, next.data);
            carry = next;
            have = true;
        } else if (have) {
            vkmr_digest next;
            vkmr::cpu_sha256d_pair(carry.data, carry.data, next.data);
            carry = next;
        }
    }
    *root = have ? carry : peaks[H];
}

// One more leaf for the frontier (c, peaks[0 .. 64)): c + 1 and its peaks; cells of bits that clear are zeroed.
static void frontier_push(uint64_t& c, vkmr_digest* peaks, const vkmr_digest& leaf)
{
    vkmr_digest node = leaf;
    uint32_t l = 0;
    for (; vkmr_frontier::has_peak(c, l); ++l) {
        vkmr_digest next;
        vkmr::cpu_sha256d_pair(peaks[l].data, node.data, next.data);
        node = next;
        std::memset(peaks[l].data, 0, 32);
    }
    peaks[l] = node;
    ++c;
}

int vkmr_host_cpu_frontier_roots(const uint64_t* counts, const vkmr_digest* peaks, uint32_t stride, uint32_t T, vkmr_digest* roots)
{
    if (T == 0) return 0;
    if (!counts || !peaks || !roots || stride == 0 || stride > VKMR_FRONTIER_MAX_STRIDE) return -1;
    int rc = 0;
    for (uint32_t q = 0; q < T; ++q) {
        if (counts[q] > vkmr_frontier::max_count() || vkmr_frontier::bit_length(counts[q]) > stride) {
            std::memset(roots[q].data, 0, 32);
            rc = 1;
            continue;
        }
        frontier_root(counts[q], peaks + (size_t)q * stride, &roots[q]);
    }
    return rc;
}

int vkmr_host_cpu_frontier_extend(const uint64_t* counts, const vkmr_digest* peaks, uint32_t stride, uint32_t T, const vkmr_digest* leaves,
                                  uint64_t total_new, const uint64_t* offsets, uint64_t max_new, uint64_t* new_counts, vkmr_digest* new_peaks,
                                  vkmr_digest* roots)
{
    if (T == 0) return 0;
    if (!counts || !peaks || (!leaves && total_new > 0) || !offsets || !new_counts || !new_peaks || !roots) return -1;
    if (stride == 0 || stride > VKMR_FRONTIER_MAX_STRIDE) return -1;
    uint32_t status = 0;
    for (uint32_t q = 0; q < T; ++q) status |= vkmr_frontier::refusal(counts[q], offsets[q], offsets[q + 1], q, T, total_new, max_new, stride);
    if (status) return (int)status;
    for (uint32_t q = 0; q < T; ++q) {
        vkmr_digest mine[VKMR_FRONTIER_MAX_STRIDE + 1];
        std::memset(mine, 0, sizeof mine);
        uint64_t c = counts[q];
        for (uint32_t l = 0; l < stride; ++l)
            if (vkmr_frontier::has_peak(c, l)) mine[l] = peaks[(size_t)q * stride + l];
        for (uint64_t i = offsets[q]; i < offsets[q + 1]; ++i) frontier_push(c, mine, leaves[i]);
        new_counts[q] = c;
        std::memcpy(new_peaks + (size_t)q * stride, mine, sizeof(vkmr_digest) * stride);
        frontier_root(c, mine, &roots[q]);
    }
    return 0;
}

int vkmr_host_cpu_forest_frontier(const vkmr_digest* digests, const uint64_t* offsets, uint32_t ntrees, uint32_t stride, uint64_t* counts_out,
                                  vkmr_digest* peaks_out)
{
    if (ntrees == 0) return 0;
    if (!offsets || !counts_out || !peaks_out || stride == 0 || stride > VKMR_FRONTIER_MAX_STRIDE) return -1;
    for (uint32_t t = 0; t < ntrees; ++t) {
        if (offsets[t + 1] < offsets[t]) return 1;
        const uint64_t c = offsets[t + 1] - offsets[t];
        if (c > vkmr_frontier::max_count() || vkmr_frontier::bit_length(c) > stride) return 1;
    }
    if (!digests && offsets[ntrees] > offsets[0]) return -1;
    for (uint32_t t = 0; t < ntrees; ++t) {
        vkmr_digest mine[VKMR_FRONTIER_MAX_STRIDE + 1];
        std::memset(mine, 0, sizeof mine);
        uint64_t c = 0;
        for (uint64_t i = offsets[t]; i < offsets[t + 1]; ++i) frontier_push(c, mine, digests[i]);
        counts_out[t] = c;
        std::memcpy(peaks_out + (size_t)t * stride, mine, sizeof(vkmr_digest) * stride);
    }
    return 0;
}

// ---- consistency proofs (consistency_plan.hpp).  The gather here has no stored forest: it builds every level of a queried tree
// from its leaves and takes the nodes the plan names out of them.

int vkmr_host_cpu_forest_consistency(const vkmr_digest* digests, const uint64_t* offsets, uint32_t ntrees, const uint32_t* trees,
                                     const uint64_t* old_counts, uint32_t Q, uint32_t stride, uint64_t* new_counts_out, vkmr_digest* peaks_out,
                                     vkmr_digest* rights_out)
{
    if (Q == 0) return 0;
    if (!offsets || !trees || !old_counts || !new_counts_out || !peaks_out || !rights_out || stride == 0 || stride > VKMR_FRONTIER_MAX_STRIDE) return -1;
    for (uint32_t t = 0; t < ntrees; ++t)
        if (offsets[t + 1] < offsets[t]) return -1;
    if (!digests && ntrees > 0 && offsets[ntrees] > offsets[0]) return -1;
    uint32_t status = 0;
    for (uint32_t q = 0; q < Q; ++q) status |= vkmr_consistency::refusal(trees[q], ntrees, offsets, old_counts[q], stride);
    if (status) return (int)status;
    std::vector<uint32_t> order(Q);
    for (uint32_t q = 0; q < Q; ++q) order[q] = q;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return trees[a] < trees[b]; });   // a tree's levels are built once
    std::vector<std::vector<vkmr_digest>> levels;
    uint32_t built = UINT32_MAX;
    for (uint32_t q : order) {
        const uint32_t t = trees[q];
        const uint64_t c = old_counts[q], c2 = offsets[t + 1] - offsets[t];
        new_counts_out[q] = c2;
        vkmr_digest* peaks = peaks_out + (size_t)q * stride;
        vkmr_digest* rights = rights_out + (size_t)q * stride;
        std::memset(peaks, 0, sizeof(vkmr_digest) * stride);
        std::memset(rights, 0, sizeof(vkmr_digest) * stride);
        if (c == 0) continue;
        if (built != t) {
            levels.assign(1, std::vector<vkmr_digest>(digests + offsets[t], digests + offsets[t + 1]));
            for (uint32_t l = 0; l < vkmr_math::height(c2); ++l) {
                const std::vector<vkmr_digest>& in = levels[l];
                std::vector<vkmr_digest> out((in.size() + 1) / 2);
                for (uint64_t j = 0; j < out.size(); ++j) vkmr::cpu_sha256d_pair(in[2 * j].data, in[vkmr_math::right_child(j, in.size())].data, out[j].data);
                levels.push_back(std::move(out));
            }
            built = t;
        }
        for (uint32_t l = 0; l < stride; ++l) {
            if (vkmr_consistency::has_peak(c, l)) peaks[l] = levels[l][vkmr_consistency::peak_node(c, l)];
            if (vkmr_consistency::has_right(c, c2, l)) rights[l] = levels[l][vkmr_consistency::right_node(c, l)];
        }
    }
    return 0;
}

int vkmr_host_cpu_verify_consistency(const uint64_t* old_counts, const uint64_t* new_counts, const vkmr_digest* peaks, const vkmr_digest* rights,
                                     uint32_t stride, uint32_t Q, const vkmr_digest* old_roots, const vkmr_digest* new_roots, uint32_t* ok)
{
    if (Q == 0) return 0;
    if (!old_counts || !new_counts || !peaks || !rights || !old_roots || !new_roots || !ok || stride == 0 || stride > VKMR_FRONTIER_MAX_STRIDE) return -1;
    for (uint32_t q = 0; q < Q; ++q) {
        const uint64_t c = old_counts[q], c2 = new_counts[q];
        const vkmr_digest* P = peaks + (size_t)q * stride;
        const vkmr_digest* R = rights + (size_t)q * stride;
        ok[q] = 0u;
        if (!vkmr_consistency::checkable(c, c2, stride)) continue;
        vkmr_digest acc;
        if (c == 0) {
            std::memset(acc.data, 0, 32);
            ok[q] = std::memcmp(acc.data, old_roots[q].data, 32) == 0 ? 1u : 0u;
            continue;
        }
        frontier_root(c, P, &acc);
        if (std::memcmp(acc.data, old_roots[q].data, 32) != 0) continue;
        const uint32_t l0 = vkmr_consistency::low_level(c);
        acc = P[l0];
        for (uint32_t l = l0; l < vkmr_math::height(c2); ++l) {
            vkmr_digest next;
            if (!vkmr_consistency::walk_is_left(c, l))
                vkmr::cpu_sha256d_pair(P[l].data, acc.data, next.data);
            else
                vkmr::cpu_sha256d_pair(acc.data, vkmr_consistency::has_right(c, c2, l) ? R[l].data : acc.data, next.data);
            acc = next;
        }
        ok[q] = std::memcmp(acc.data, new_roots[q].data, 32) == 0 ? 1u : 0u;
    }
    return 0;
}

// ---- inclusion proofs as of an earlier count (proofs_at_plan.hpp).  As the consistency gather above, there is no stored forest:
// every level of a tree that has an epoch is built from its leaves as they are NOW, the complete nodes are taken out of them and
// the old tree's right edge is hashed by the plan's edge_step().

int vkmr_host_cpu_forest_proofs_at(const vkmr_digest* digests, const uint64_t* offsets, uint32_t ntrees, const uint32_t* epoch_trees,
                                   const uint64_t* epoch_counts, uint32_t E, const uint32_t* epochs, const uint64_t* indices, uint32_t k,
                                   uint32_t stride, vkmr_digest* edges_out, vkmr_digest* old_roots_out, vkmr_digest* siblings, uint32_t* heights)
{
    if (E == 0) return 0;
    if (!offsets || !epoch_trees || !epoch_counts || !edges_out || !old_roots_out || stride == 0 || stride > 63) return -1;
    if (k > 0 && (!epochs || !indices || !siblings || !heights)) return -1;
    for (uint32_t t = 0; t < ntrees; ++t)
        if (offsets[t + 1] < offsets[t]) return -1;
    if (!digests && ntrees > 0 && offsets[ntrees] > offsets[0]) return -1;
    uint32_t status = 0;
    for (uint32_t e = 0; e < E; ++e) status |= vkmr_proofs_at::refusal(epoch_trees[e], ntrees, offsets, epoch_counts[e], stride);
    if (status) return (int)status;
    // the levels of every tree that has an epoch, built once
    std::vector<std::vector<std::vector<vkmr_digest>>> levels(ntrees);
    for (uint32_t e = 0; e < E; ++e) {
        const uint32_t t = epoch_trees[e];
        const uint64_t c2 = offsets[t + 1] - offsets[t];
        if (epoch_counts[e] == 0 || !levels[t].empty()) continue;
        levels[t].assign(1, std::vector<vkmr_digest>(digests + offsets[t], digests + offsets[t + 1]));
        for (uint32_t l = 0; l < vkmr_math::height(c2); ++l) {
            const std::vector<vkmr_digest>& in = levels[t][l];
            std::vector<vkmr_digest> out((in.size() + 1) / 2);
            for (uint64_t j = 0; j < out.size(); ++j) vkmr::cpu_sha256d_pair(in[2 * j].data, in[vkmr_math::right_child(j, in.size())].data, out[j].data);
            levels[t].push_back(std::move(out));
        }
    }
    std::memset(edges_out, 0, sizeof(vkmr_digest) * (size_t)E * stride);
    std::memset(old_roots_out, 0, sizeof(vkmr_digest) * (size_t)E);
    for (uint32_t e = 0; e < E; ++e) {
        const uint32_t t = epoch_trees[e];
        const uint64_t c = epoch_counts[e];
        vkmr_digest carry = {};
        bool have = false;
        for (uint32_t l = 0; l < vkmr_proofs_at::levels(c); ++l) {
            const vkmr_proofs_at::EdgeStep s = vkmr_proofs_at::edge_step(c, l, have);
            vkmr_digest* dst = s.to_root ? old_roots_out + e : edges_out + (size_t)e * stride + (l + 1);
            if (s.stored) *dst = levels[t][l + 1][0];
            if (!s.hash) continue;
            const vkmr_digest a = s.peak ? levels[t][l][vkmr_proofs_at::peak_node(c, l)] : carry;
            const vkmr_digest b = s.twice ? a : carry;
            vkmr::cpu_sha256d_pair(a.data, b.data, carry.data);
            have = true;
            *dst = carry;
        }
    }
    for (uint32_t q = 0; q < k; ++q) {
        vkmr_digest* mine = siblings + (size_t)q * stride;
        std::memset(mine, 0, sizeof(vkmr_digest) * stride);
        heights[q] = 0;
        const uint32_t e = epochs[q];
        if (e >= E || indices[q] >= epoch_counts[e]) continue;
        const uint64_t c = epoch_counts[e], i = indices[q];
        heights[q] = vkmr_proofs_at::height(c);
        for (uint32_t l = 0; l < heights[q]; ++l)
            mine[l] = vkmr_proofs_at::cell_source(c, l, i) == vkmr_proofs_at::CELL_STORED ? levels[epoch_trees[e]][l][vkmr_proofs_at::sibling(c, l, i)]
                                                                                          : edges_out[(size_t)e * stride + l];
    }
    return 0;
}

int vkmr_host_cpu_forest_merkleblocks(const vkmr_digest* digests, const uint64_t* offsets, uint32_t ntrees, const uint32_t* trees,
                                      const uint64_t* indices, uint32_t k, uint32_t* block_trees, uint64_t* block_counts, uint64_t* bit_counts,
                                      uint64_t* hash_starts, uint64_t* byte_starts, vkmr_digest* hashes, uint64_t hash_capacity, uint8_t* flags,
                                      uint64_t flag_capacity, uint64_t* info)
{
    if (k == 0 || !digests || !offsets || !trees || !indices || !block_trees || !block_counts || !bit_counts || !hash_starts || !byte_starts || !info ||
        (!hashes && hash_capacity > 0) || (!flags && flag_capacity > 0))
        return -1;
    for (uint32_t t = 0; t < ntrees; ++t)
        if (offsets[t + 1] < offsets[t]) return -2;
    int status = 0;
    for (uint32_t q = 0; q < k; ++q) {
        if (trees[q] >= ntrees || indices[q] >= offsets[trees[q] + 1] - offsets[trees[q]]) status |= 1;
        if (q > 0 && (trees[q - 1] > trees[q] || (trees[q - 1] == trees[q] && indices[q - 1] >= indices[q]))) status |= 2;
    }
    info[0] = (uint64_t)status;
    if (status) return status;
    // the walk of one tree over the sorted indices [a, b): in(l, p) says whether node p of level l has a matched leaf below it
    struct Walk {
        const uint64_t* idx; uint32_t a, b; uint64_t c;
        std::vector<uint8_t> bits;
        std::vector<std::pair<uint32_t, uint64_t>> cells;
        bool in(uint32_t l, uint64_t p) const
        {
            const uint64_t* lo = std::lower_bound(idx + a, idx + b, p << l);
            return lo != idx + b && (*lo >> l) == p;
        }
        void visit(uint32_t l, uint64_t p)
        {
            const bool f = in(l, p);
            bits.push_back(f ? 1 : 0);
            if (l == 0 || !f) {
                cells.push_back({l, p});
                return;
            }
            visit(l - 1, 2 * p);
            if (2 * p + 1 < vkmr_forest::level_count(c, l - 1)) visit(l - 1, 2 * p + 1);
        }
    };
    std::vector<Walk> walks;
    uint64_t nhashes = 0, nbytes = 0;
    for (uint32_t a = 0; a < k;) {
        const uint32_t b = forest_run_end(trees, a, k), t = trees[a];
        Walk w{indices, a, b, offsets[t + 1] - offsets[t], {}, {}};
        w.visit(vkmr_math::height(w.c), 0);
        const size_t n = walks.size();
        block_trees[n] = t;
        block_counts[n] = w.c;
        bit_counts[n] = w.bits.size();
        hash_starts[n] = nhashes;
        byte_starts[n] = nbytes;
        nhashes += w.cells.size();
        nbytes += (w.bits.size() + 7) / 8;
        walks.push_back(std::move(w));
        a = b;
    }
    hash_starts[walks.size()] = nhashes;
    byte_starts[walks.size()] = nbytes;
    info[1] = walks.size();
    info[2] = nhashes;
    info[3] = nbytes;
    if (nhashes > hash_capacity || nbytes > flag_capacity) {
        info[0] = 4;
        return 4;
    }
    std::vector<std::vector<vkmr_digest>> levels;
    for (size_t n = 0; n < walks.size(); ++n) {
        const Walk& w = walks[n];
        const uint32_t t = block_trees[n];
        tree_levels(digests + offsets[t], digests + offsets[t + 1], vkmr_math::height(w.c), levels);
        for (size_t j = 0; j < w.cells.size(); ++j) hashes[hash_starts[n] + j] = levels[w.cells[j].first][w.cells[j].second];
        uint8_t* out = flags + byte_starts[n];
        std::memset(out, 0, (w.bits.size() + 7) / 8);
        for (size_t i = 0; i < w.bits.size(); ++i) out[i >> 3] |= (uint8_t)(w.bits[i] << (i & 7));
    }
    return 0;
}

int vkmr_host_cpu_merkleblock_extract(uint64_t count, const vkmr_digest* hashes, uint64_t nhashes, const uint8_t* flag_bytes, uint64_t nbytes,
                                      vkmr_digest* root_out, uint64_t* matched_idx_out, vkmr_digest* matched_hash_out, uint64_t* nmatched_out)
{
    if (!root_out || !matched_idx_out || !matched_hash_out || !nmatched_out || (!hashes && nhashes > 0) || (!flag_bytes && nbytes > 0)) return -1;
    if (count == 0) return -2;
    if (nhashes > count) return -3;
    if (nbytes < (nhashes + 7) / 8) return -4;       // fewer flag bits than hashes
    struct Extract {
        uint64_t count; const vkmr_digest* hashes; uint64_t nhashes; const uint8_t* bytes; uint64_t nbits;
        uint64_t bit = 0, hash = 0;
        int bad = 0;
        std::vector<uint64_t> idx;
        std::vector<vkmr_digest> leaves;
        vkmr_digest visit(uint32_t l, uint64_t p)
        {
            vkmr_digest x{};
            if (bad) return x;
            if (bit >= nbits) { bad = -5; return x; }
            const bool f = (bytes[bit >> 3] >> (bit & 7)) & 1;
            ++bit;
            if (l == 0 || !f) {
                if (hash >= nhashes) { bad = -5; return x; }
                x = hashes[hash++];
                if (l == 0 && f) { idx.push_back(p); leaves.push_back(x); }
                return x;
            }
            const vkmr_digest left = visit(l - 1, 2 * p);
            vkmr_digest right = left;
            if (2 * p + 1 < vkmr_forest::level_count(count, l - 1)) {
                right = visit(l - 1, 2 * p + 1);
                if (!bad && std::memcmp(left.data, right.data, sizeof(left.data)) == 0) bad = -8;
            }
            if (bad) return x;
            vkmr::cpu_sha256d_pair(left.data, right.data, x.data);
            return x;
        }
    };
    Extract e{count, hashes, nhashes, flag_bytes, nbytes * 8};
    const vkmr_digest root = e.visit(vkmr_math::height(count), 0);
    if (e.bad) return e.bad;
    if (e.hash != nhashes) return -6;
    if ((e.bit + 7) / 8 != nbytes) return -7;
    *root_out = root;
    for (size_t j = 0; j < e.idx.size(); ++j) {
        matched_idx_out[j] = e.idx[j];
        matched_hash_out[j] = e.leaves[j];
    }
    *nmatched_out = e.idx.size();
    return 0;
}

// ---- sorted trees: order, lower bound, absence proofs (absence_plan.hpp)

static int absence_offsets_bad(const uint64_t* offsets, uint32_t ntrees, uint64_t total)
{
    for (uint32_t t = 0; t < ntrees; ++t)
        if (offsets[t + 1] < offsets[t]) return 1;
    return ntrees > 0 && offsets[ntrees] > total ? 1 : 0;
}

int vkmr_host_cpu_forest_sorted(const vkmr_digest* digests, uint64_t total, const uint64_t* offsets, uint32_t ntrees, uint64_t* first_bad,
                                uint64_t* info)
{
    if (ntrees == 0) return 0;
    if (!offsets || !first_bad || !info) return -1;
    if (absence_offsets_bad(offsets, ntrees, total)) return 1;
    if (!digests && offsets[ntrees] > offsets[0]) return -1;
    info[0] = info[1] = info[2] = info[3] = 0;
    for (uint32_t t = 0; t < ntrees; ++t) {
        const vkmr_digest* leaf = digests + offsets[t];
        const uint64_t c = offsets[t + 1] - offsets[t];
        first_bad[t] = vkmr_absence::NONE;
        if (c >= 2) info[3] += c - 1;
        for (uint64_t i = 1; i < c; ++i) {
            if (vkmr_absence::less(leaf[i - 1].data, leaf[i].data)) continue;
            first_bad[t] = i;
            ++info[1];
            if (vkmr_absence::equal(leaf[i - 1].data, leaf[i].data)) ++info[2];
            break;
        }
    }
    return 0;
}

int vkmr_host_cpu_forest_lower_bound(const vkmr_digest* digests, uint64_t total, const uint64_t* offsets, uint32_t ntrees, const uint32_t* trees,
                                     const vkmr_digest* queries, uint32_t Q, uint64_t* indices, uint32_t* found)
{
    if (Q == 0) return 0;
    if (!trees || !queries || !indices || !found || (ntrees > 0 && !offsets)) return -1;
    if (absence_offsets_bad(offsets, ntrees, total)) return 1;
    if (ntrees > 0 && !digests && offsets[ntrees] > offsets[0]) return -1;
    for (uint32_t q = 0; q < Q; ++q) {
        indices[q] = vkmr_absence::NONE;
        found[q] = 0;
        if (trees[q] >= ntrees) continue;
        const vkmr_digest* leaf = digests + offsets[trees[q]];
        const uint64_t c = offsets[trees[q] + 1] - offsets[trees[q]];
        const uint64_t i = vkmr_absence::lower_bound(c, [&](uint64_t mid) { return vkmr_absence::less(leaf[mid].data, queries[q].data); });
        indices[q] = i;
        found[q] = i < c && vkmr_absence::equal(leaf[i].data, queries[q].data) ? 1u : 0u;
    }
    return 0;
}

int vkmr_host_cpu_forest_absence(const vkmr_digest* digests, uint64_t total, const uint64_t* offsets, uint32_t ntrees, const uint32_t* trees,
                                 const vkmr_digest* queries, uint32_t Q, uint32_t stride, uint64_t* indices, vkmr_digest* neighbours,
                                 vkmr_digest* main_row, vkmr_digest* low_row, uint32_t* heights)
{
    if (Q == 0) return 0;
    if (!trees || !queries || !indices || !neighbours || !heights || (stride > 0 && (!main_row || !low_row)) || (ntrees > 0 && !offsets)) return -1;
    if (absence_offsets_bad(offsets, ntrees, total)) return 1;
    if (ntrees > 0 && !digests && offsets[ntrees] > offsets[0]) return -1;
    std::vector<uint32_t> order;
    for (uint32_t q = 0; q < Q; ++q) {
        if (trees[q] >= ntrees) continue;
        if (vkmr_absence::height(offsets[trees[q] + 1] - offsets[trees[q]]) > stride) return 2;
        order.push_back(q);
    }
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return trees[x] < trees[y]; });
    for (uint32_t q = 0; q < Q; ++q) indices[q] = vkmr_absence::NONE;
    std::memset(heights, 0, sizeof(uint32_t) * (size_t)Q);
    std::memset(neighbours, 0, sizeof(vkmr_digest) * 2 * (size_t)Q);
    if (stride > 0) {
        std::memset(main_row, 0, sizeof(vkmr_digest) * (size_t)Q * stride);
        std::memset(low_row, 0, sizeof(vkmr_digest) * (size_t)Q * stride);
    }
    std::vector<std::vector<vkmr_digest>> levels;
    for (size_t n = 0; n < order.size(); ++n) {
        const uint32_t q = order[n], t = trees[q];
        const vkmr_digest* leaf = digests + offsets[t];
        const uint64_t c = offsets[t + 1] - offsets[t];
        const uint32_t h = vkmr_absence::height(c);
        const uint64_t i = vkmr_absence::lower_bound(c, [&](uint64_t mid) { return vkmr_absence::less(leaf[mid].data, queries[q].data); });
        indices[q] = i;
        heights[q] = h;
        if (c == 0) continue;
        if (n == 0 || trees[order[n - 1]] != t) tree_levels(leaf, leaf + c, h, levels);
        if (vkmr_absence::has_pred(i)) neighbours[2 * (size_t)q] = leaf[i - 1];
        if (vkmr_absence::has_succ(i, c)) neighbours[2 * (size_t)q + 1] = leaf[i];
        const uint64_t a = vkmr_absence::anchor(i, c);
        for (uint32_t l = 0; l < h; ++l) {
            main_row[(size_t)q * stride + l] = levels[l][vkmr_math::sibling(a >> l, levels[l].size())];
            if (vkmr_absence::low_cell(i, c, l)) low_row[(size_t)q * stride + l] = levels[l][vkmr_math::sibling((i - 1) >> l, levels[l].size())];
        }
    }
    return 0;
}

int vkmr_host_cpu_verify_absence(const vkmr_digest* queries, const uint32_t* trees, const uint64_t* indices, const vkmr_digest* neighbours,
                                 const vkmr_digest* main_row, const vkmr_digest* low_row, const uint32_t* heights, uint32_t Q, uint32_t stride,
                                 const vkmr_digest* roots, const uint64_t* counts, uint32_t ntrees, uint32_t* verdict)
{
    if (Q == 0) return 0;
    if (!queries || !trees || !indices || !neighbours || !heights || !verdict || (stride > 0 && (!main_row || !low_row)) ||
        (ntrees > 0 && (!roots || !counts)) || stride > 63)
        return -1;
    for (uint32_t q = 0; q < Q; ++q) {
        const uint32_t t = trees[q];
        const bool known = t < ntrees;
        verdict[q] = vkmr_absence::verdict(queries[q].data, t, ntrees, indices[q], neighbours[2 * (size_t)q].data, neighbours[2 * (size_t)q + 1].data,
                                           stride ? main_row[(size_t)q * stride].data : nullptr, stride ? low_row[(size_t)q * stride].data : nullptr,
                                           heights[q], stride, known ? roots[t].data : nullptr, known ? counts[t] : 0ull,
                                           [](const uint32_t* a, const uint32_t* b, uint32_t* out) { vkmr::cpu_sha256d_pair(a, b, out); });
    }
    return 0;
}

// ---- sorted trees: every leaf between two digests, proved complete (range_plan.hpp)

int vkmr_host_cpu_forest_range(const vkmr_digest* digests, uint64_t total, const uint64_t* offsets, uint32_t ntrees, const uint32_t* trees,
                               const vkmr_digest* lo, const vkmr_digest* hi, uint32_t Q, uint32_t stride, uint64_t* firsts, uint64_t* leaf_starts,
                               vkmr_digest* leaves, uint64_t leaves_capacity, vkmr_digest* left_row, vkmr_digest* right_row, uint32_t* heights,
                               uint64_t* info)
{
    if (Q == 0) return 0;
    if (!trees || !lo || !hi || !firsts || !leaf_starts || !heights || !info || (leaves_capacity > 0 && !leaves) ||
        (stride > 0 && (!left_row || !right_row)) || (ntrees > 0 && !offsets))
        return -1;
    if (absence_offsets_bad(offsets, ntrees, total)) return 1;
    if (ntrees > 0 && !digests && offsets[ntrees] > offsets[0]) return -1;
    for (uint32_t q = 0; q < Q; ++q)
        if (trees[q] < ntrees && vkmr_absence::height(offsets[trees[q] + 1] - offsets[trees[q]]) > stride) return 2;
    info[0] = info[1] = info[2] = info[3] = 0;
    for (uint32_t q = 0; q < Q; ++q) {
        const bool known = trees[q] < ntrees;
        const vkmr_digest* leaf = known ? digests + offsets[trees[q]] : nullptr;
        const uint64_t c = known ? offsets[trees[q] + 1] - offsets[trees[q]] : 0;
        const vkmr_range::Run r = vkmr_range::run(
            known, c, lo[q].data, hi[q].data, [&](uint64_t i, const uint32_t* x) { return vkmr_absence::less(leaf[i].data, x); },
            [&](uint64_t i, const uint32_t* x) { return vkmr_absence::equal(leaf[i].data, x); });
        firsts[q] = r.first;
        heights[q] = r.height;
        leaf_starts[q] = info[1];
        info[1] += r.m;
        info[2] += r.first == vkmr_range::NONE ? 1 : 0;
        info[3] += r.inside;
    }
    leaf_starts[Q] = info[1];
    if (stride > 0) {
        std::memset(left_row, 0, sizeof(vkmr_digest) * (size_t)Q * stride);
        std::memset(right_row, 0, sizeof(vkmr_digest) * (size_t)Q * stride);
    }
    if (info[1] > leaves_capacity) info[0] = VKMR_RANGE_LEAVES_CAPACITY;
    std::vector<uint32_t> order;
    for (uint32_t q = 0; q < Q; ++q)
        if (leaf_starts[q + 1] > leaf_starts[q]) order.push_back(q);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return trees[x] < trees[y]; });
    std::vector<std::vector<vkmr_digest>> levels;
    for (size_t n = 0; n < order.size(); ++n) {
        const uint32_t q = order[n], t = trees[q];
        const vkmr_digest* leaf = digests + offsets[t];
        const uint64_t c = offsets[t + 1] - offsets[t], a = firsts[q], m = leaf_starts[q + 1] - leaf_starts[q], b = a + m - 1;
        const uint32_t h = heights[q];
        if (n == 0 || trees[order[n - 1]] != t) tree_levels(leaf, leaf + c, h, levels);
        if (info[0] == 0)
            for (uint64_t j = 0; j < m; ++j) leaves[leaf_starts[q] + j] = leaf[a + j];
        for (uint32_t l = 0; l < h; ++l) {
            if (vkmr_range::left_cell(a, l, h)) left_row[(size_t)q * stride + l] = levels[l][(a >> l) - 1];
            if (vkmr_range::right_cell(b, c, l, h)) right_row[(size_t)q * stride + l] = levels[l][(b >> l) + 1];
        }
    }
    return 0;
}

int vkmr_host_cpu_tree_range(const vkmr_digest* digests, uint64_t count, const vkmr_digest* lo, const vkmr_digest* hi, uint32_t Q, uint32_t stride,
                             uint64_t* firsts, uint64_t* leaf_starts, vkmr_digest* leaves, uint64_t leaves_capacity, vkmr_digest* left_row,
                             vkmr_digest* right_row, uint64_t* info)
{
    if (Q == 0) return 0;
    const uint64_t offsets[2] = {0, count};
    std::vector<uint32_t> trees(Q, 0u), heights(Q);
    return vkmr_host_cpu_forest_range(digests, count, offsets, 1, trees.data(), lo, hi, Q, stride, firsts, leaf_starts, leaves, leaves_capacity, left_row,
                                      right_row, heights.data(), info);
}

int vkmr_host_cpu_verify_range(const uint32_t* trees, const vkmr_digest* lo, const vkmr_digest* hi, const uint64_t* firsts, const uint64_t* leaf_starts,
                               const vkmr_digest* leaves, uint64_t nleaves, const vkmr_digest* left_row, const vkmr_digest* right_row,
                               const uint32_t* heights, uint32_t Q, uint32_t stride, const vkmr_digest* roots, const uint64_t* counts, uint32_t ntrees,
                               uint32_t* verdict, uint64_t* in_first, uint64_t* in_count)
{
    if (Q == 0) return 0;
    if (!trees || !lo || !hi || !firsts || !leaf_starts || !heights || !verdict || !in_first || !in_count || (nleaves > 0 && !leaves) ||
        (stride > 0 && (!left_row || !right_row)) || (ntrees > 0 && (!roots || !counts)) || stride > 63)
        return -1;
    bool prefix = true;                          // leaf_starts is no prefix over [0, nleaves]: nothing is proven
    for (uint32_t q = 0; q < Q; ++q) prefix = prefix && leaf_starts[q] <= leaf_starts[q + 1] && leaf_starts[q + 1] <= nleaves;
    std::vector<uint32_t> work;
    for (uint32_t q = 0; q < Q; ++q) {
        const uint32_t t = trees[q];
        const bool known = t < ntrees;
        vkmr_range::Verdict v{0u, 0ull, 0ull};
        if (prefix) {
            const uint64_t m = leaf_starts[q + 1] - leaf_starts[q];
            work.resize(8 * (size_t)m + 8);
            v = vkmr_range::verdict(t, ntrees, lo[q].data, hi[q].data, firsts[q], m, m ? leaves[leaf_starts[q]].data : nullptr,
                                    stride ? left_row[(size_t)q * stride].data : nullptr, stride ? right_row[(size_t)q * stride].data : nullptr, heights[q],
                                    stride, known ? roots[t].data : nullptr, known ? counts[t] : 0ull, work.data(),
                                    [](const uint32_t* a, const uint32_t* b, uint32_t* out) { vkmr::cpu_sha256d_pair(a, b, out); });
        }
        verdict[q] = v.verdict;
        in_first[q] = v.in_first;
        in_count[q] = v.in_count;
    }
    return 0;
}

// ---- the leaves of a forest sorted tree by tree (leafsort_plan.hpp)

int vkmr_host_cpu_forest_sort_leaves(const vkmr_digest* digests_in, uint64_t total, const uint64_t* offsets, uint32_t ntrees, uint64_t max_count,
                                     vkmr_digest* digests_out, uint32_t* order_out, uint64_t* info)
{
    if (ntrees == 0) return 0;
    if (!offsets || !info || total >= vkmr_leafsort::MAX_TOTAL) return -1;
    uint64_t status = absence_offsets_bad(offsets, ntrees, total) ? VKMR_LEAFSORT_BAD_OFFSETS : 0ull;
    for (uint32_t t = 0; t < ntrees; ++t)
        if (offsets[t + 1] >= offsets[t] && offsets[t + 1] - offsets[t] > max_count) status |= VKMR_LEAFSORT_ABOVE_MAX_COUNT;
    const uint64_t lo = offsets[0], n = (status & VKMR_LEAFSORT_BAD_OFFSETS) ? 0ull : offsets[ntrees] - lo;
    if (!status && n > 0 && (!digests_in || !digests_out)) return -1;
    info[0] = status;
    info[1] = n;
    info[2] = info[3] = 0;
    if (status) return 0;
    const vkmr_leafsort::Shape shape = vkmr_leafsort::shape(ntrees, max_count);
    std::vector<uint32_t> order((size_t)n);
    for (uint64_t i = 0; i < n; ++i) order[(size_t)i] = (uint32_t)(lo + i);
    std::vector<uint64_t> keys((size_t)n);
    for (uint32_t t = 0; t < ntrees; ++t) {
        const auto first = order.begin() + (ptrdiff_t)(offsets[t] - lo), last = order.begin() + (ptrdiff_t)(offsets[t + 1] - lo);
        std::stable_sort(first, last, [&](uint32_t x, uint32_t y) { return vkmr_absence::less(digests_in[x].data, digests_in[y].data); });
        for (auto it = first; it != last; ++it) {
            const uint32_t* w = digests_in[*it].data;
            keys[(size_t)(it - order.begin())] = vkmr_leafsort::key(t, w[0], w[1], shape.P);
            if (it != first && vkmr_absence::equal(w, digests_in[*(it - 1)].data)) ++info[3];
        }
    }
    for (uint64_t j = 0; j < n; ++j) {
        if ((j > 0 && keys[(size_t)j - 1] == keys[(size_t)j]) || (j + 1 < n && keys[(size_t)j + 1] == keys[(size_t)j])) ++info[2];
        digests_out[lo + j] = digests_in[order[(size_t)j]];
        if (order_out) order_out[lo + j] = order[(size_t)j];
    }
    return 0;
}

int vkmr_host_cpu_tree_sort_leaves(const vkmr_digest* digests_in, uint64_t count, vkmr_digest* digests_out, uint32_t* order_out, uint64_t* info)
{
    const uint64_t offsets[2] = {0, count};
    return vkmr_host_cpu_forest_sort_leaves(digests_in, count, offsets, 1, count, digests_out, order_out, info);
}

// ---- two sorted forests merged tree by tree (merge_plan.hpp)

// offsets == nullptr: one tree a side at cell 0.
static int merge_leaves_cpu(const vkmr_digest* a, uint64_t a_total, const uint64_t* a_offsets, const vkmr_digest* b, uint64_t b_total,
                            const uint64_t* b_offsets, uint32_t ntrees, uint32_t op, vkmr_digest* out, uint64_t out_capacity, uint64_t* out_offsets,
                            uint64_t* origin_out, uint64_t* info)
{
    if (!info || op > VKMR_MERGE_INTERSECTION || (a_total && !a) || (b_total && !b) || (out_capacity && !out)) return -1;
    const uint64_t one_a[2] = {0, a_total}, one_b[2] = {0, b_total};
    const uint64_t *ao = a_offsets ? a_offsets : one_a, *bo = b_offsets ? b_offsets : one_b;
    uint64_t status = 0;
    if (a_offsets && absence_offsets_bad(ao, ntrees, a_total)) status |= VKMR_MERGE_BAD_A_OFFSETS;
    if (b_offsets && absence_offsets_bad(bo, ntrees, b_total)) status |= VKMR_MERGE_BAD_B_OFFSETS;
    info[0] = status;
    info[1] = info[2] = info[3] = 0;
    if (status) return 0;
    for (uint32_t t = 0; t < ntrees; ++t) {
        for (uint64_t i = ao[t] + 1; i < ao[t + 1]; ++i)
            if (!vkmr_absence::less(a[i - 1].data, a[i].data)) status |= VKMR_MERGE_A_NOT_INCREASING;
        for (uint64_t j = bo[t] + 1; j < bo[t + 1]; ++j)
            if (vkmr_absence::less(b[j].data, b[j - 1].data)) status |= VKMR_MERGE_B_DECREASES;
    }
    info[0] = status;
    if (status) return 0;
    // every output cell as the input cell it comes from; the counts
    std::vector<uint64_t> from, starts(ntrees + 1u, 0);
    uint64_t matches = 0, repeats = 0;
    for (uint32_t t = 0; t < ntrees; ++t) {
        starts[t] = from.size();
        uint64_t i = ao[t], j = bo[t];
        const uint64_t ie = ao[t + 1], je = bo[t + 1];
        while (i < ie || j < je) {
            if (j < je && j > bo[t] && vkmr_absence::equal(b[j].data, b[j - 1].data)) { ++repeats; ++j; continue; }
            if (j == je || (i < ie && vkmr_absence::less(a[i].data, b[j].data))) {          // A's leaf alone
                if (op != VKMR_MERGE_INTERSECTION) from.push_back(i);
                ++i;
            } else if (i == ie || vkmr_absence::less(b[j].data, a[i].data)) {               // B's leaf alone
                if (op == VKMR_MERGE_UNION) from.push_back(j | VKMR_MERGE_ORIGIN_B);
                ++j;
            } else {                                                                        // in both: A's cell
                ++matches;
                if (op != VKMR_MERGE_DIFFERENCE) from.push_back(i);
                ++i; ++j;
            }
        }
    }
    starts[ntrees] = from.size();
    info[1] = from.size();
    info[2] = matches;
    info[3] = repeats;
    if (from.size() > out_capacity) { info[0] = VKMR_MERGE_SHORT_OUTPUT; return 0; }
    if (out_offsets) std::copy(starts.begin(), starts.end(), out_offsets);
    for (size_t k = 0; k < from.size(); ++k) {
        out[k] = (from[k] & VKMR_MERGE_ORIGIN_B) ? b[from[k] & ~VKMR_MERGE_ORIGIN_B] : a[from[k]];
        if (origin_out) origin_out[k] = from[k];
    }
    return 0;
}

int vkmr_host_cpu_forest_merge_leaves(const vkmr_digest* a_digests, uint64_t a_total, const uint64_t* a_offsets, const vkmr_digest* b_digests,
                                      uint64_t b_total, const uint64_t* b_offsets, uint32_t ntrees, uint32_t op, vkmr_digest* out_digests,
                                      uint64_t out_capacity, uint64_t* out_offsets, uint64_t* origin_out, uint64_t* info)
{
    if (ntrees == 0) return 0;
    if (!a_offsets || !b_offsets || !out_offsets) return -1;
    return merge_leaves_cpu(a_digests, a_total, a_offsets, b_digests, b_total, b_offsets, ntrees, op, out_digests, out_capacity, out_offsets, origin_out, info);
}

int vkmr_host_cpu_tree_merge_leaves(const vkmr_digest* a_digests, uint64_t a_count, const vkmr_digest* b_digests, uint64_t b_count, uint32_t op,
                                    vkmr_digest* out_digests, uint64_t out_capacity, uint64_t* origin_out, uint64_t* info)
{
    return merge_leaves_cpu(a_digests, a_count, nullptr, b_digests, b_count, nullptr, 1u, op, out_digests, out_capacity, nullptr, origin_out, info);
}
