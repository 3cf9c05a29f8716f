/*
 * vkmr_host.h -- C ABI of the host libraries: every vkmr_host_* function that libvkmr_host.so and libvkmr_pipeline.so
 * export, with its contract.  Plain C entry points over the host-side C++ (csrc/host), for bindings and tests; none of
 * them but the pipeline's two needs a GPU.
 *
 * The vkmr_host_cpu_* functions are the "CPU" backend on packed batches and slice roots and the CPU twins of the
 * stored-structure operations of vkmr_hip.h: the same rules over host memory, for a party without a GPU and as the
 * second opinion of the device's tests.  Every pointer is host memory; a digest is a vkmr_digest as vkmr_hip.h lays it
 * out.  A function that returns int says in its comment what each value means; none sets vkmr_hip_last_error().
 *
 * The definitions (csrc/host/host_api.cpp, stream_pack.cpp, rndm_stream.cpp, packed_pipeline.cpp) include this header
 * and take linkage and visibility from it.  A definition whose parameters differ from its declaration would be another,
 * undeclared function: the build compiles them with -Werror=missing-declarations, which stops there.
 */
#ifndef VKMR_HOST_H
#define VKMR_HOST_H

#include "vkmr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- packed batches and slice roots ---- */

/* Leaf digests of a packed batch with the CPU backend (CpuSha256D::Add per string). */
VKMR_API void vkmr_host_cpu_leaves(const uint32_t* data, const vkmr_metadata* meta, uint64_t count, vkmr_digest* out);

/* Sub-tree root of `count` digests through exactly `height` levels (the per-slice
 * contract of vkmr_hip_reduce_async), on the CPU backend's node function. */
VKMR_API int vkmr_host_cpu_reduce(const vkmr_digest* digests, uint64_t count, uint32_t height, vkmr_digest* root);

/* Combine of slice roots in slice order: duplicate-last tree, at least one level
 * (CpuSha256D::Root over already-hashed nodes; reference CpuSha256DforReductions,
 * src/vkmr/Reductions.cpp:56-69, :703-712). */
VKMR_API int vkmr_host_cpu_combine(const vkmr_digest* roots, uint32_t n, vkmr_digest* out);

/* ---- proofs and multiproofs: one tree, then forests (their roots first) ---- */

/* Folds a leaf digest with the siblings of its authentication path (vkmr_hip_proof_async):
 * bit l of `index` tells whether the path node is the right (1) or left (0) operand at level l. */
VKMR_API void vkmr_host_cpu_fold_proof(const vkmr_digest* leaf, uint64_t index, const vkmr_digest* siblings, uint32_t height, vkmr_digest* root);

/* Multiproof verification on the CPU, by the rule of vkmr_hip_verify_multiproof_async: 1 when the indices are strictly
 * increasing and < 2^height, the fold of leaves and nodes consumes exactly m nodes and ends in `root`; else 0. */
VKMR_API int vkmr_host_cpu_verify_multiproof(const vkmr_digest* leaves, const uint64_t* indices, uint32_t k, uint32_t height,
                                             const vkmr_digest* nodes, uint64_t m, const vkmr_digest* root);

/* Roots of a forest on the CPU, by the rule of vkmr_hip_reduce_forest_async: tree t is digests[offsets[t] .. offsets[t+1]),
 * reduced through max(1, ceil(log2 c_t)) levels (vkmr_host_cpu_reduce); an empty tree gets an all-zero root.  Nonzero when
 * the offsets decrease somewhere (nothing is written then) or a pointer is missing. */
VKMR_API int vkmr_host_cpu_forest_roots(const vkmr_digest* digests, const uint64_t* offsets, uint32_t ntrees, vkmr_digest* roots);

/* Roots and mutation masks of a forest on the CPU, by the rule of vkmr_hip_reduce_forest_mutated_async: bit l of mutated[t] is
 * set iff level l of tree t (n_l nodes) holds a j with 2j + 1 < n_l and node 2j equal to node 2j + 1 -- Bitcoin Core's
 * ComputeMerkleRoot(hashes, &mutated) with the level kept; the last node of an odd level, hashed with itself, is no pair.  An
 * empty tree gets an all-zero root and mask 0.  `roots` may be null (the masks alone).  Nonzero, and nothing written, when the
 * offsets decrease somewhere (1) or a pointer is missing (-1). */
VKMR_API int vkmr_host_cpu_forest_mutated(const vkmr_digest* digests, const uint64_t* offsets, uint32_t ntrees, vkmr_digest* roots,
                                          uint64_t* mutated);

/* Proofs from a forest on the CPU, by the rule of vkmr_hip_forest_proofs_async: query q is leaf indices[q] of tree trees[q]
 * (tree t: digests[offsets[t] .. offsets[t+1])); heights[q] = h_t = max(1, ceil(log2 c_t)) and siblings[q * stride + l] is
 * L_t[l][p ^ 1] with p = index >> l, or L_t[l][p] where p ^ 1 is past the level's end, for l < h_t and all-zero behind.  A
 * tree >= ntrees or an index >= c_t gets height 0 and `stride` zero cells.  Nonzero, and nothing written, when the offsets
 * decrease somewhere (1), when `stride` is below the largest h_t a query needs (2) or a pointer is missing (-1).  A tree's
 * levels are formed once, however many queries ask for it.  The proofs verify through vkmr_host_cpu_fold_proof. */
VKMR_API int vkmr_host_cpu_forest_proofs(const vkmr_digest* digests, const uint64_t* offsets, uint32_t ntrees, const uint32_t* trees,
                                         const uint64_t* indices, uint32_t k, uint32_t stride, vkmr_digest* siblings, uint32_t* heights);

/* Multiproof for leaves of many trees on the CPU, by the rule of vkmr_hip_forest_multiproof_async: entry q is leaf indices[q]
 * of tree trees[q] (tree t: digests[offsets[t] .. offsets[t+1])), the pairs strictly increasing; nodes[] receives the M nodes
 * in level-major order over the whole forest, heights[q] = h of entry q's tree, info[0] = status, info[1] = M,
 * info[2 + l] = m_l for l < stride.  Returns the status: 0 done; bit 0 a tree >= ntrees or an index >= c_t, bit 1 pairs not
 * strictly increasing (then only info[0] is written); bit 2 M > nodes_capacity (the heights, M and the counts are written, no
 * node is).  -1 for a missing pointer or k == 0, -2 when the offsets decrease somewhere, -3 when `stride` is above 63 or below
 * the height of a tree some entry names (nothing written).  A touched tree's levels are formed once, tree by tree. */
VKMR_API int vkmr_host_cpu_forest_multiproof(const vkmr_digest* digests, const uint64_t* offsets, uint32_t ntrees, const uint32_t* trees,
                                             const uint64_t* indices, uint32_t k, uint32_t stride, vkmr_digest* nodes, uint64_t nodes_capacity,
                                             uint32_t* heights, uint64_t* info);

/* Forest multiproof verification on the CPU, by the rule of vkmr_hip_verify_forest_multiproof_async: 1 when the (tree, index)
 * pairs are strictly increasing, every tree < ntrees, 1 <= heights[q] <= stride <= 63, indices[q] < 2^heights[q], the entries
 * of one tree carry one height, the indices and heights imply exactly m nodes, and every named tree's fold -- a missing child
 * being the next unread node of its level in forest order -- ends in roots[t]; else 0. */
VKMR_API int vkmr_host_cpu_verify_forest_multiproof(const vkmr_digest* leaves, const uint32_t* trees, const uint64_t* indices,
                                                    const uint32_t* heights, uint32_t k, uint32_t stride, const vkmr_digest* nodes, uint64_t m,
                                                    const vkmr_digest* roots, uint32_t ntrees);

/* ---- apply ---- */

/* Applying a multiproof on the CPU, by the rule of vkmr_hip_apply_multiproof_async: 1, and *new_root written, when
 * 1 <= count <= 2^height, height is 1..63, the indices are strictly increasing and < count, the fold of the old leaves
 * consumes exactly m nodes and ends in `root`; else 0 and nothing written.  new_root may be root. */
VKMR_API int vkmr_host_cpu_apply_multiproof(const vkmr_digest* old_leaves, const vkmr_digest* new_leaves, const uint64_t* indices, uint32_t k,
                                            uint64_t count, uint32_t height, const vkmr_digest* nodes, uint64_t m, const vkmr_digest* root,
                                            vkmr_digest* new_root);

/* Applying a forest multiproof on the CPU, by the rule of vkmr_hip_apply_forest_multiproof_async: 1 when every count is
 * >= 1, indices[q] < counts[q], the entries of one tree carry one count and vkmr_host_cpu_verify_forest_multiproof answers 1
 * for the old leaves with the heights max(1, ceil(log2 count)); then new_roots[t] of every named tree is written (new_roots
 * may be roots; the cells of other trees are not touched).  Else 0 and nothing written. */
VKMR_API int vkmr_host_cpu_apply_forest_multiproof(const vkmr_digest* old_leaves, const vkmr_digest* new_leaves, const uint32_t* trees,
                                                   const uint64_t* indices, const uint64_t* counts, uint32_t k, uint32_t stride,
                                                   const vkmr_digest* nodes, uint64_t m, const vkmr_digest* roots, uint32_t ntrees,
                                                   vkmr_digest* new_roots);

/* ---- find and sort ---- */

/* Leaves by digest on the CPU, by the rule of vkmr_hip_forest_find_async: query q's answer is the lowest flat position p in
 * [offsets[0], offsets[ntrees]) with digests[p] == queries[q] on all 32 bytes, as trees[q] = the tree that holds p and
 * indices[q] = p - offsets[trees[q]]; no such p: 0xFFFFFFFF and UINT64_MAX.  The queries are sorted once and every leaf is
 * looked up among them: O((total + k) log k).  Nonzero, and nothing written, when the offsets decrease somewhere or end past
 * `total` (1) or a needed pointer is missing (-1).  k == 0 does nothing. */
VKMR_API int vkmr_host_cpu_forest_find(const vkmr_digest* digests, uint64_t total, const uint64_t* offsets, uint32_t ntrees,
                                       const vkmr_digest* queries, uint32_t k, uint32_t* trees, uint64_t* indices);

/* The same for one tree over digests[0 .. count): indices[q] = the lowest index whose leaf equals queries[q], or UINT64_MAX. */
VKMR_API int vkmr_host_cpu_tree_find(const vkmr_digest* digests, uint64_t count, const vkmr_digest* queries, uint32_t k, uint64_t* indices);

/* Leaf entries sorted and deduplicated on the CPU, by the rule of vkmr_hip_forest_sort_entries_async: cells [0, n) of the
 * outputs are the distinct valid (tree, index) pairs, strictly increasing, order_out[j] the largest q whose pair is output
 * pair j; info[0..4) = survivors n, "not found" markers (trees[q] == 0xFFFFFFFF), entries out of range, earlier repeats.
 * A stable sort of q by flat position.  Nonzero, and nothing written, when the offsets decrease somewhere or end past
 * `total` (1) or a needed pointer is missing (-1).  k == 0 does nothing. */
VKMR_API int vkmr_host_cpu_forest_sort_entries(uint64_t total, const uint64_t* offsets, uint32_t ntrees, const uint32_t* trees,
                                               const uint64_t* indices, uint32_t k, uint32_t* trees_out, uint64_t* indices_out, uint32_t* order_out,
                                               uint64_t* info);

/* The same for one tree of `count` leaves: every entry in tree 0, the "not found" marker being indices[q] == UINT64_MAX. */
VKMR_API int vkmr_host_cpu_tree_sort_entries(uint64_t count, const uint64_t* indices, uint32_t k, uint64_t* indices_out, uint32_t* order_out,
                                             uint64_t* info);

/* ---- audit ---- */

/* A stored forest audited on the CPU, by the rule of vkmr_hip_forest_audit_async and with its outputs: node (t, l, j) is bad when
 * its stored cell -- roots[t] for the tree's last level, else cell stored_level_base(l) + pos_l(t) + j of `forest` -- is not
 * hash_pair of the two stored cells beneath it; an empty tree's root must be all zero.  masks[t] bit l - 1, the first
 * `capacity` bad nodes in (level, tree, node) order, info[0..4) = status (bits 0, 1: the offsets and max_count check, and then
 * nothing is audited; bit 2: more than `capacity` > 0 bad nodes), bad nodes, trees with a nonzero mask, nodes checked.  Reads
 * only.  -1, and nothing written, when a needed pointer is missing, max_count is 0 or total is above 2^58. */
VKMR_API int vkmr_host_cpu_forest_audit(const vkmr_digest* digests, const vkmr_digest* forest, const vkmr_digest* roots, uint64_t total,
                                        const uint64_t* offsets, uint32_t ntrees, uint64_t max_count, uint64_t* masks, uint32_t* bad_trees,
                                        uint32_t* bad_levels, uint64_t* bad_nodes, uint32_t capacity, uint64_t* info);

/* The same for one stored tree (vkmr_hip_tree_audit_async): levels 1 .. height in `tree` as tree_plan.hpp lays them out, a
 * lone-node level above ceil(log2 count) being hash(a, a) of the node below; info[2] is the tree's own level mask.  -1 when a
 * needed pointer is missing or `height` does not reduce `count` to one node. */
VKMR_API int vkmr_host_cpu_tree_audit(const vkmr_digest* digests, const vkmr_digest* tree, uint64_t count, uint32_t height, uint32_t* bad_levels,
                                      uint64_t* bad_nodes, uint32_t capacity, uint64_t* info);

/* ---- frontiers (vkmr_hip_frontier_roots_async, vkmr_hip_frontier_extend_async, vkmr_hip_forest_frontier_async), for a
 * follower without a GPU ---- */

/* roots[q] = the root of frontier q (counts[q], the stride cells behind peaks + q * stride), T of them.  A count above 2^58 or
 * of more bits than stride gives the zero root and makes the call return 1; -1 for a missing pointer or a stride outside 1..64. */
VKMR_API int vkmr_host_cpu_frontier_roots(const uint64_t* counts, const vkmr_digest* peaks, uint32_t stride, uint32_t T, vkmr_digest* roots);

/* T frontiers each take leaves[offsets[q] .. offsets[q+1]): the new counts, the new peaks (cells of clear bits zero) and the
 * roots, by the contract of vkmr_hip_frontier_extend_async; new_counts / new_peaks may be counts / peaks.  Returns the status
 * word of that call (0: done; nonzero: nothing written), or -1 for a missing pointer or a stride outside 1..64. */
VKMR_API int vkmr_host_cpu_frontier_extend(const uint64_t* counts, const vkmr_digest* peaks, uint32_t stride, uint32_t T, const vkmr_digest* leaves,
                                           uint64_t total_new, const uint64_t* offsets, uint64_t max_new, uint64_t* new_counts,
                                           vkmr_digest* new_peaks, vkmr_digest* roots);

/* The frontiers of the trees of a forest from its leaves: tree t is digests[offsets[t] .. offsets[t+1]).  What
 * vkmr_hip_forest_frontier_async reads out of a stored forest.  1, and nothing written, when the offsets decrease or a tree has
 * more leaves than 2^58 or than stride bits hold; -1 for a missing pointer or a stride outside 1..64. */
VKMR_API int vkmr_host_cpu_forest_frontier(const vkmr_digest* digests, const uint64_t* offsets, uint32_t ntrees, uint32_t stride,
                                           uint64_t* counts_out, vkmr_digest* peaks_out);

/* ---- consistency (vkmr_hip_forest_consistency_async, vkmr_hip_verify_consistency_async), for a primary or a monitor
 * without a GPU ---- */

/* The proofs of Q queries (trees[q], old_counts[q]) over the trees of a forest given by its leaves, tree t is
 * digests[offsets[t] .. offsets[t+1]): new_counts_out[q], and the stride cells of peaks_out and rights_out behind q * stride,
 * every cell written.  Returns the status word of vkmr_hip_forest_consistency_async (0: done; nonzero: nothing written), or -1
 * for a missing pointer, a stride outside 1..64 or offsets that decrease. */
VKMR_API int vkmr_host_cpu_forest_consistency(const vkmr_digest* digests, const uint64_t* offsets, uint32_t ntrees, const uint32_t* trees,
                                              const uint64_t* old_counts, uint32_t Q, uint32_t stride, uint64_t* new_counts_out,
                                              vkmr_digest* peaks_out, vkmr_digest* rights_out);

/* ok[q] = 1 when proof q holds under old_roots[q] and new_roots[q], else 0: vkmr_hip_verify_consistency_async's check, the two
 * walks written out one behind the other.  -1 for a missing pointer or a stride outside 1..64. */
VKMR_API int vkmr_host_cpu_verify_consistency(const uint64_t* old_counts, const uint64_t* new_counts, const vkmr_digest* peaks,
                                              const vkmr_digest* rights, uint32_t stride, uint32_t Q, const vkmr_digest* old_roots,
                                              const vkmr_digest* new_roots, uint32_t* ok);

/* ---- proofs as of a count (vkmr_hip_forest_proofs_at_async), for a log without a GPU ---- */

/* E epochs (epoch_trees[e], epoch_counts[e]) over the trees of a forest given by its leaves, and k queries (epochs[q],
 * indices[q]): edges_out (E x stride), old_roots_out (E), siblings (k x stride) and heights (k), every cell written.  Returns
 * the status word of vkmr_hip_forest_proofs_at_async (0: done; nonzero: nothing written), or -1 for a missing pointer, a stride
 * outside 1..63 or offsets that decrease. */
VKMR_API int vkmr_host_cpu_forest_proofs_at(const vkmr_digest* digests, const uint64_t* offsets, uint32_t ntrees, const uint32_t* epoch_trees,
                                            const uint64_t* epoch_counts, uint32_t E, const uint32_t* epochs, const uint64_t* indices, uint32_t k,
                                            uint32_t stride, vkmr_digest* edges_out, vkmr_digest* old_roots_out, vkmr_digest* siblings,
                                            uint32_t* heights);

/* ---- merkleblocks ---- */

/* Partial Merkle trees in BIP37 order on the CPU, by the rule of vkmr_hip_forest_merkleblocks_async, walked as the rule is
 * written (the device places everything by csrc/merkleblock_plan.hpp's closed form instead): the same entries, the same eight
 * outputs, info[0..4) = status, B, hashes, flag bytes.  Returns the status: 0 done; bit 0 a tree >= ntrees or an index >= c_t,
 * bit 1 pairs not strictly increasing (then only info[0] is written); bit 2 the hashes exceed hash_capacity or the flag bytes
 * flag_capacity (the per-block arrays and info are written, no hash and no flag is).  -1 for a missing pointer or k == 0, -2
 * when the offsets decrease somewhere (nothing written).  A touched tree's levels are formed once, tree by tree. */
VKMR_API int vkmr_host_cpu_forest_merkleblocks(const vkmr_digest* digests, const uint64_t* offsets, uint32_t ntrees, const uint32_t* trees,
                                               const uint64_t* indices, uint32_t k, uint32_t* block_trees, uint64_t* block_counts,
                                               uint64_t* bit_counts, uint64_t* hash_starts, uint64_t* byte_starts, vkmr_digest* hashes,
                                               uint64_t hash_capacity, uint8_t* flags, uint64_t flag_capacity, uint64_t* info);

/* The receiver's side of one partial Merkle tree: Bitcoin Core's CPartialMerkleTree::ExtractMatches (TraverseAndExtract) under
 * this project's height h = max(1, ceil(log2 count)).  `hashes` [nhashes] and the flag bytes [nbytes] are one block of
 * vkmr_hip_forest_merkleblocks_async; on 0 root_out is the root they fold to, matched_idx_out / matched_hash_out (room for
 * nhashes entries each) the matched leaves in ascending order and *nmatched_out their number.  The caller compares the root
 * with the one it trusts.  Refusals, nothing written: -1 a missing pointer, -2 count == 0, -3 more hashes than leaves, -4 fewer
 * flag bits than hashes, -5 a flag or a hash read past the end, -6 not all hashes used, -7 the flags used do not end in the last
 * byte, -8 a right child that exists and equals its left (CVE-2012-2459: [a, b, c, c] has the root of [a, b, c]).  Padding bits
 * are not inspected, as in Core. */
VKMR_API int vkmr_host_cpu_merkleblock_extract(uint64_t count, const vkmr_digest* hashes, uint64_t nhashes, const uint8_t* flag_bytes,
                                               uint64_t nbytes, vkmr_digest* root_out, uint64_t* matched_idx_out, vkmr_digest* matched_hash_out,
                                               uint64_t* nmatched_out);

/* ---- sorted trees: order, lower bound, absence proofs (vkmr_hip_forest_sorted_async and its neighbours), for a party
 * without a GPU.  A forest is its leaves and offsets; one tree is a forest of one (offsets {0, count}).  Each returns -1 for a
 * missing pointer and 1 when the offsets decrease somewhere or end behind `total`; nothing is written then. ---- */

/* first_bad[t] = the lowest i in [1, c_t) with !(leaf[i-1] < leaf[i]), or UINT64_MAX; info: status 0, trees not sorted, trees whose
 * first offence is an equal pair, pairs compared. */
VKMR_API int vkmr_host_cpu_forest_sorted(const vkmr_digest* digests, uint64_t total, const uint64_t* offsets, uint32_t ntrees, uint64_t* first_bad,
                                         uint64_t* info);

/* indices[q] = the lower bound of queries[q] in tree trees[q] by the plan's loop, found[q] = 1 when the leaf there is the query;
 * UINT64_MAX and 0 for a tree >= ntrees. */
VKMR_API int vkmr_host_cpu_forest_lower_bound(const vkmr_digest* digests, uint64_t total, const uint64_t* offsets, uint32_t ntrees,
                                              const uint32_t* trees, const vkmr_digest* queries, uint32_t Q, uint64_t* indices, uint32_t* found);

/* The absence proofs of vkmr_hip_forest_absence_async, with no stored forest: the levels of a tree are built from its leaves, once
 * per tree however many queries name it.  2, and nothing written, when `stride` is below the height of a tree that a query names. */
VKMR_API int vkmr_host_cpu_forest_absence(const vkmr_digest* digests, uint64_t total, const uint64_t* offsets, uint32_t ntrees, const uint32_t* trees,
                                          const vkmr_digest* queries, uint32_t Q, uint32_t stride, uint64_t* indices, vkmr_digest* neighbours,
                                          vkmr_digest* main_row, vkmr_digest* low_row, uint32_t* heights);

/* verdict[q] of vkmr_hip_verify_forest_absence_async: the plan's verdict() over the CPU's node hash. */
VKMR_API int vkmr_host_cpu_verify_absence(const vkmr_digest* queries, const uint32_t* trees, const uint64_t* indices, const vkmr_digest* neighbours,
                                          const vkmr_digest* main_row, const vkmr_digest* low_row, const uint32_t* heights, uint32_t Q,
                                          uint32_t stride, const vkmr_digest* roots, const uint64_t* counts, uint32_t ntrees, uint32_t* verdict);

/* ---- sorted trees: every leaf between two digests, proved complete (vkmr_hip_forest_range_async and its neighbours) ---- */

/* The range proofs of vkmr_hip_forest_range_async, with no stored forest: the levels of a tree are built from its leaves, once per tree.
 * firsts[Q], leaf_starts[Q + 1], leaves (leaves_capacity cells), the two rows of Q x stride cells, heights[Q] and info[0..4) = status,
 * leaves carried, queries refused, leaves in range, as the device writes them; status bit 0 (no leaf written) when the leaves carried
 * exceed leaves_capacity, the only limit.  -1 for a missing pointer, 1 for offsets that are no forest's, 2 when `stride` is below the
 * height of a tree that a query names; nothing is written then. */
VKMR_API int vkmr_host_cpu_forest_range(const vkmr_digest* digests, uint64_t total, const uint64_t* offsets, uint32_t ntrees, const uint32_t* trees,
                                        const vkmr_digest* lo, const vkmr_digest* hi, uint32_t Q, uint32_t stride, uint64_t* firsts,
                                        uint64_t* leaf_starts, vkmr_digest* leaves, uint64_t leaves_capacity, vkmr_digest* left_row,
                                        vkmr_digest* right_row, uint32_t* heights, uint64_t* info);

/* The same for one tree over digests[0 .. count): every query names it, no heights. */
VKMR_API int vkmr_host_cpu_tree_range(const vkmr_digest* digests, uint64_t count, const vkmr_digest* lo, const vkmr_digest* hi, uint32_t Q,
                                      uint32_t stride, uint64_t* firsts, uint64_t* leaf_starts, vkmr_digest* leaves, uint64_t leaves_capacity,
                                      vkmr_digest* left_row, vkmr_digest* right_row, uint64_t* info);

/* verdict[q], in_first[q], in_count[q] of vkmr_hip_verify_forest_range_async: range_plan.hpp's verdict() over the CPU's node hash. */
VKMR_API int vkmr_host_cpu_verify_range(const uint32_t* trees, const vkmr_digest* lo, const vkmr_digest* hi, const uint64_t* firsts,
                                        const uint64_t* leaf_starts, const vkmr_digest* leaves, uint64_t nleaves, const vkmr_digest* left_row,
                                        const vkmr_digest* right_row, const uint32_t* heights, uint32_t Q, uint32_t stride,
                                        const vkmr_digest* roots, const uint64_t* counts, uint32_t ntrees, uint32_t* verdict, uint64_t* in_first,
                                        uint64_t* in_count);

/* ---- the leaves of a forest sorted tree by tree, by the rule of vkmr_hip_forest_sort_leaves_async ---- */

/* For every tree t the leaves at cells [offsets[t], offsets[t+1]) of digests_in, in increasing digest order (equal digests in input
 * order: std::stable_sort under absence_plan.hpp's less), at the same cells of digests_out; order_out[j] (may be NULL) the flat cell
 * of digests_in that lies at cell j.  info[0..4) as the device writes it: status (bit 0 the offsets, bit 1 a tree above max_count;
 * nothing else is written then), n, m counted with leafsort_plan.hpp's key, the leaves equal to an earlier leaf of their tree.  The
 * one difference: there is no tie limit, bit 2 is never set and the leaves are always sorted.  -1 for a missing pointer or total >=
 * 2^32; ntrees == 0 does nothing. */
VKMR_API int vkmr_host_cpu_forest_sort_leaves(const vkmr_digest* digests_in, uint64_t total, const uint64_t* offsets, uint32_t ntrees,
                                              uint64_t max_count, vkmr_digest* digests_out, uint32_t* order_out, uint64_t* info);

/* The same for one tree over digests_in[0 .. count): total = max_count = count. */
VKMR_API int vkmr_host_cpu_tree_sort_leaves(const vkmr_digest* digests_in, uint64_t count, vkmr_digest* digests_out, uint32_t* order_out,
                                            uint64_t* info);

/* ---- two sorted forests merged tree by tree, by the rule of vkmr_hip_forest_merge_leaves_async ---- */

/* A two-pointer merge per tree under absence_plan.hpp's less: op 0 union, 1 difference, 2 intersection of the strictly increasing
 * trees of A (a_digests, a_total, a_offsets) with the non-decreasing trees of B.  out_offsets[ntrees + 1], out_digests (out_capacity
 * cells), origin_out (may be NULL; bit 63: a cell of B) and info[0..4) = status, n_out, matches, repeats as the device writes them,
 * with the same status bits 0 to 4; with a nonzero status only info is written.  -1 for a missing pointer or op > 2; ntrees == 0
 * does nothing. */
VKMR_API int vkmr_host_cpu_forest_merge_leaves(const vkmr_digest* a_digests, uint64_t a_total, const uint64_t* a_offsets,
                                               const vkmr_digest* b_digests, uint64_t b_total, const uint64_t* b_offsets, uint32_t ntrees,
                                               uint32_t op, vkmr_digest* out_digests, uint64_t out_capacity, uint64_t* out_offsets,
                                               uint64_t* origin_out, uint64_t* info);

/* The same for one tree a side, a_digests[0 .. a_count) and b_digests[0 .. b_count): no offsets, n_out in info[1]. */
VKMR_API int vkmr_host_cpu_tree_merge_leaves(const vkmr_digest* a_digests, uint64_t a_count, const vkmr_digest* b_digests, uint64_t b_count,
                                             uint32_t op, vkmr_digest* out_digests, uint64_t out_capacity, uint64_t* origin_out, uint64_t* info);

/* ---- packing (stream_pack.cpp; in libvkmr_host.so and libvkmr_pipeline.so) ---- */

/* One-shot form for bindings: packs the whole buffer (final = true).  Returns the
 * number of strings, or -1 when a buffer was too small. */
VKMR_API int64_t vkmr_host_pack_lines(const uint8_t* buf, uint64_t len, uint32_t* data, uint64_t data_capacity_words, vkmr_metadata* meta,
                                      uint64_t meta_capacity, uint64_t* words_used, uint64_t* bytes_total);

/* The same with the portable (memchr per line) splitter forced, and the line counter of the parallel packer's first
 * pass in both forms: lets the tests hold the AVX2 forms against the portable ones on the same input. */
VKMR_API int64_t vkmr_host_pack_lines_portable(const uint8_t* buf, uint64_t len, uint32_t* data, uint64_t data_capacity_words, vkmr_metadata* meta,
                                               uint64_t meta_capacity, uint64_t* words_used, uint64_t* bytes_total);

/* out[0..4] = strings, words, bytes, empties, too_long; which: 0 = the form the packer uses on this CPU, 1 = portable */
VKMR_API void vkmr_host_count_lines(const uint8_t* buf, uint64_t len, int which, uint64_t* out);

/* The indexed two-pass form on one buffer (every line, the last one terminated or not), placed at data[first_word ...):
 * which as above.  Returns the number of strings, or -1 when a buffer was too small; out[0..3] = words, bytes, empties,
 * lines indexed. */
VKMR_API int64_t vkmr_host_pack_indexed(const uint8_t* buf, uint64_t len, uint32_t* data, uint64_t first_word, uint64_t data_capacity_words,
                                        vkmr_metadata* meta, uint64_t meta_capacity, int which, uint64_t* out);

/* CopyAndCountLines on one buffer: out[0..1] = newlines, empties; which as above. */
VKMR_API void vkmr_host_copy_and_count(const uint8_t* buf, uint64_t len, uint8_t* dst, int after_newline, int which, uint64_t* out);

/* A prefix split with capacity limits and `final` unset, as the stream processor calls it: out[0..4] = consumed, strings,
 * words, bytes, empties; which as above. */
VKMR_API void vkmr_host_pack_prefix(const uint8_t* buf, uint64_t len, int final, uint32_t* data, uint64_t first_word, uint64_t data_capacity_words,
                                    vkmr_metadata* meta, uint64_t meta_capacity, int which, uint64_t* out);

/* ---- the rndm generator (rndm_stream.cpp) ---- */

/* First n values of rand() after srand(seed) (test hook). */
VKMR_API void vkmr_host_rndm_rand(uint32_t seed, int32_t* out, uint64_t n);

/* Stateful form: the stream of `rndm seed * maxlen` produced batch after batch (a packed batch
 * addresses at most 2^32 words, so long-string workloads need several). */
VKMR_API void* vkmr_host_rndm_open(uint32_t seed);
VKMR_API void vkmr_host_rndm_close(void* h);

/* Next `count` strings of the stream into a fresh packed batch (metadata starts at word 0). */
VKMR_API int64_t vkmr_host_rndm_next(void* h, uint64_t count, uint32_t maxlen, uint32_t* data, uint64_t data_capacity_words, vkmr_metadata* meta,
                                     uint64_t* words_used);

/* Generates the strings of `rndm seed count maxlen` directly in the packed batch
 * layout (Batch::Push, reference src/vkmr/Batches.cpp:64-121): string i starts at the
 * word after string i-1, `start` is a word index, bytes past `size` in the last word
 * are zero.  Returns the number of strings written (== count) or -1 when the data
 * buffer is too small; *words_used receives the packed length in words. */
VKMR_API int64_t vkmr_host_rndm_pack(uint32_t seed, uint64_t count, uint32_t maxlen, uint32_t* data, uint64_t data_capacity_words,
                                     vkmr_metadata* meta, uint64_t* words_used);

/* ---- the pipeline (packed_pipeline.cpp; libvkmr_pipeline.so, which needs libvkmr_hip.so) ---- */

/* device: a HIP device index, or -1 for every device ("hip:all").  strings_per_batch: how many strings one map launch
 * takes (the batch pool is sized for it); slice_log2: digests per slice, 0 = chosen from the devices.
 * root_hex: 65 bytes.  seconds: the timed part (first Map to the root on the host).  Returns 0, or -1 on failure. */
VKMR_API int vkmr_host_pipeline_packed(int device, const uint32_t* data, uint64_t words, const vkmr_metadata* meta, uint64_t count,
                                       uint64_t strings_per_batch, uint32_t slice_log2, char* root_hex, double* seconds);

/* The front end on text in memory: the non-empty lines of text[0,len) -- a line ends at '\n' or at len; '\r' is kept
 * (Input::Get, reference src/vkmr/Inputs.cpp:75-101) -- through the parallel packer, pinned batches, Mappings, Reductions and
 * the combine, exactly as `vkmr hip:<n> < file` runs them, span by span (span_bytes at a time; 0 = the 32 MiB of vkmr_main).
 * device: a HIP device index, or -1 for every device ("hip:all").  root_hex: 65 bytes; all zero-length when the text holds no
 * string (the reference prints no root then).  items / bytes: strings added and their payload bytes.  seconds: from the
 * first span to the root on the host (the reference's stopwatch).  Returns 0, or -1 on failure. */
VKMR_API int vkmr_host_pipeline_text(int device, const char* text, uint64_t len, uint64_t span_bytes, char* root_hex, uint64_t* items,
                                     uint64_t* bytes, double* seconds);

#ifdef __cplusplus
}
#endif
#endif /* VKMR_HOST_H */
