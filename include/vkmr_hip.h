/*
 * vkmr_hip.h -- C ABI of the MI355X (gfx950) Merkle-root engine.
 *
 * This is the drop-in boundary: everything the reference's host code asked of
 * Vulkan for the map -> reduce -> combine hot path, as plain
 * C entry points over hand-written HIP kernels.  No C++ types, no exceptions, no
 * torch types.  Every function returns a vkmr_status (0 = ok, negative = error,
 * VKMR_NOT_READY = 1 from vkmr_hip_event_query only) and writes results through
 * out-pointers; vkmr_hip_last_error() gives the text of the last failure on the
 * calling thread.
 *
 * Each entry point cites the reference interface it replaces (file:line relative
 * to the reference tree).  INTEGRATION.md shows the binding a maintainer of the
 * reference would add.
 *
 * Threading: one host thread may drive any number of devices; every call that
 * takes `dev` selects that device itself.  Calls on one instance are not
 * re-entrant across threads (same as the reference, which is single-threaded).
 *
 * Ownership: buffers passed to an *_async call stay owned by the caller and must
 * stay alive until an event recorded after the call on the same stream has
 * completed (reference: a Batch is freed when its Mapping retires,
 * src/vkmr/Mappings.cpp:328-329; a Slice when its Reduction retires,
 * src/vkmr/Reductions.cpp:663).
 *
 * Scratch buffers: every entry point with a `scratch_dev` parameter names the size function that sizes it, and all of them
 * keep one contract, so that a caller may recycle one scratch across calls.  (1) What the scratch holds on entry does not
 * matter: the call clears or writes whatever it reads, and the result is the same from zeros, from 0xFF or from another call's
 * leftovers.  (2) The call reads and writes only the bytes the size function named for its arguments, from scratch_dev on.
 * (3) The next call may take the same scratch on the same stream with no wait in between: the stream orders them.  Calls on
 * different streams need a scratch each.  scratch_dev must be 16-byte aligned -- 8-byte for vkmr_hip_forest_find_async and
 * vkmr_hip_tree_find_async -- and no stricter alignment is ever needed; the size functions return whole multiples of that
 * alignment, except vkmr_hip_multiproof_scratch_bytes and vkmr_hip_sizes_scratch_bytes, which return the bare layout in whole
 * 4-byte words.  tests/scratch_cases.py holds a row per such entry point.
 */
#ifndef VKMR_HIP_H
#define VKMR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VKMR_API __attribute__((visibility("default")))

/* ---- status ------------------------------------------------------------- */
typedef int vkmr_status;
#define VKMR_OK            0
#define VKMR_NOT_READY     1   /* vkmr_hip_event_query: work still in flight (VK_NOT_READY) */
#define VKMR_ERR_INVALID  (-1) /* bad argument (null pointer, count/height mismatch, ...)   */
#define VKMR_ERR_NO_DEVICE (-2)
#define VKMR_ERR_OOM      (-3) /* VK_ERROR_OUT_OF_DEVICE_MEMORY / _HOST_MEMORY              */
#define VKMR_ERR_HIP      (-4) /* any other HIP runtime failure                              */
#define VKMR_ERR_COMM     (-5) /* RCCL failure, or librccl could not be loaded               */

/* ---- wire structs: identical layout to the reference's device structs ---- */

/* One packed input string.  Replaces VkSha256Metadata, src/common/SHA-256defs.h:51-54:
 * `start` is a 32-bit WORD index into the packed data buffer, `size` is in BYTES. */
typedef struct vkmr_metadata { uint32_t start; uint32_t size; } vkmr_metadata;

/* One digest cell.  Replaces VkSha256Result, src/common/SHA-256defs.h:47-49: eight
 * words holding the VALUES H[0..7], so raw little-endian memory is byte-swapped per
 * word relative to the canonical digest. */
typedef struct vkmr_digest { uint32_t data[8]; } vkmr_digest;

typedef struct vkmr_stream_s* vkmr_stream;   /* replaces VkQueue + VkCommandBuffer      */
typedef struct vkmr_event_s*  vkmr_event;    /* replaces VkFence and the timestamp pair */

/* ---- devices (replaces VkSha256D's enumeration, src/vkmr/SHA-256vk.cpp:38-171) ---- */
VKMR_API vkmr_status vkmr_hip_device_count(int* count);
/* Marketing name of device `dev` (VkPhysicalDeviceProperties::deviceName). */
VKMR_API vkmr_status vkmr_hip_device_name(int dev, char* buf, size_t buflen);
/* Free/total HBM in bytes (ComputeDevice::AvailableMemoryTypes budgets,
 * src/vkmr/Devices.h:184-245; used for slice sizing, src/vkmr/Slices.h:421-454). */
VKMR_API vkmr_status vkmr_hip_device_mem_info(int dev, size_t* free_bytes, size_t* total_bytes);
/* Compute-unit count and wavefront width (64 on gfx950); the reference reads
 * subgroupSize here, src/vkmr/Reductions.cpp:749-770. */
VKMR_API vkmr_status vkmr_hip_device_geometry(int dev, int* compute_units, int* wavefront);

/* ---- memory --------------------------------------------------------------- */
/* Pinned, zero-filled host buffer for a Batch's data / metadata (Batch::Buffer,
 * src/vkmr/Batches.cpp:196-237: host-visible + coherent, memset 0). */
VKMR_API vkmr_status vkmr_hip_host_alloc(size_t bytes, void** out);
VKMR_API vkmr_status vkmr_hip_host_free(void* p);
/* Device-local buffer: a Slice of digests (Slices::New, src/vkmr/Slices.h:297-384)
 * or the HBM landing zone of a batch. */
VKMR_API vkmr_status vkmr_hip_device_alloc(int dev, size_t bytes, void** out);
VKMR_API vkmr_status vkmr_hip_device_free(int dev, void* p);
VKMR_API vkmr_status vkmr_hip_memset_async(int dev, vkmr_stream s, void* dst, int value, size_t bytes);
VKMR_API vkmr_status vkmr_hip_memcpy_h2d_async(int dev, vkmr_stream s, void* dst_dev, const void* src_host, size_t bytes);
/* Used for the 32-byte root read-back (vkCmdCopyBuffer slice[0] -> host buffer,
 * src/vkmr/Reductions.cpp:537-540) and by tests to fetch digests. */
VKMR_API vkmr_status vkmr_hip_memcpy_d2h_async(int dev, vkmr_stream s, void* dst_host, const void* src_dev, size_t bytes);

/* ---- streams and events ---------------------------------------------------- */
/* A stream orders the ops submitted to it (the compute->compute barriers of
 * src/vkmr/Reductions.cpp:506-519 come for free).  ComputeDevice::Queue round-robin,
 * src/vkmr/Devices.cpp:525-538. */
VKMR_API vkmr_status vkmr_hip_stream_create(int dev, vkmr_stream* out);
VKMR_API vkmr_status vkmr_hip_stream_destroy(int dev, vkmr_stream s);
/* Start-up work, done when the caller wants it rather than inside its first copy and first launch: the library's
 * kernels are loaded onto the device and the stream's queue comes up (VKMR_WARM_KERNELS: one launch of the map kernel on
 * a four-byte string), the copy engine comes up (VKMR_WARM_COPY: one host-to-device copy of `copy_bytes` from pinned
 * memory on the stream -- the engine's set-up depends on the size: give the size of the copies to come, at least 256);
 * returns when both are done.  The reference pays the same at start-up, outside its stopwatch: ComputeDevice builds its
 * shader modules and compute pipelines before run() begins (src/vkmr/Devices.cpp:225-280, Shaders.cpp:20-40).
 * Optional: without it the first vkmr_hip_memcpy_h2d_async and the first launch take the time (20 + 15 ms on MI355X,
 * profiles/r03_frontend_phases.txt). */
#define VKMR_WARM_KERNELS 1u
#define VKMR_WARM_COPY 2u
VKMR_API vkmr_status vkmr_hip_warm_up(int dev, vkmr_stream s, unsigned what, size_t copy_bytes);
VKMR_API vkmr_status vkmr_hip_stream_sync(int dev, vkmr_stream s);
VKMR_API vkmr_status vkmr_hip_event_create(int dev, vkmr_event* out);
VKMR_API vkmr_status vkmr_hip_event_destroy(int dev, vkmr_event e);
VKMR_API vkmr_status vkmr_hip_event_record(int dev, vkmr_event e, vkmr_stream s);
/* vkGetFenceStatus (src/vkmr/Mappings.cpp:322, Reductions.cpp:642): VKMR_OK or VKMR_NOT_READY. */
VKMR_API vkmr_status vkmr_hip_event_query(int dev, vkmr_event e);
/* vkWaitForFences (src/vkmr/Mappings.cpp:362, Reductions.cpp:686). */
VKMR_API vkmr_status vkmr_hip_event_wait(int dev, vkmr_event e);
/* Make stream `s` wait for `e` (cross-stream ordering; no Vulkan counterpart needed
 * in the single-queue reference). */
VKMR_API vkmr_status vkmr_hip_stream_wait_event(int dev, vkmr_stream s, vkmr_event e);
/* QueryPoolTimer::ElapsedMillis, src/vkmr/QueryPoolTimers.cpp:52-93. */
VKMR_API vkmr_status vkmr_hip_event_elapsed_ms(int dev, vkmr_event begin, vkmr_event end, float* ms);

/* ---- the hot path ---------------------------------------------------------- */

/*
 * MAP: digests[i] = SHA-256(SHA-256(string i)) for i in [0,count).
 * Replaces Mapping::Dispatch + shader entry `_SHA_256_N_`
 * (src/vkmr/Mappings.cpp:135-232, src/shaders/SHA-256.comp:177-304).
 *   data_dev    packed words in HBM, layout of Batch::Push (src/vkmr/Batches.cpp:64-121)
 *   data_words  number of valid 32-bit words in data_dev (bounds every load)
 *   meta_dev    count entries; string i occupies bytes [4*start, 4*start+size)
 *   out_dev     count digest cells (a sub-slice, src/vkmr/Slices.h:145-187)
 * Deliberate differences from the shader: bounds test is `>=`
 * (Q4), tail bytes of the last word are masked to `size` (Q3), the 64-bit length
 * uses size>>29 for the high word.  size == 0 hashes the empty string.  A string whose
 * metadata runs past data_words is cut at the end of the buffer (bounded work for
 * corrupt metadata; the shader would read out of bounds).
 */
VKMR_API vkmr_status vkmr_hip_map_async(int dev, vkmr_stream s,
                                        const uint32_t* data_dev, uint64_t data_words,
                                        const vkmr_metadata* meta_dev, uint32_t count,
                                        vkmr_digest* out_dev);

/*
 * REDUCE: sub-tree root of `count` digests through exactly `height` levels of
 * node = SHA-256d(left || right), an unpaired node being paired with itself at
 * every level, including after the count has collapsed to one.
 * Replaces Reduction::Apply + ReductionBySubgroup::GetCommandBuffer + shader entry
 * `_SHA_256_2_BE_`/`_VKMR_BY_SUBGROUP_` (src/vkmr/Reductions.cpp:147-216, :433-547,
 * src/shaders/SHA-256.comp:308-391).  The caller chooses `height` exactly as the
 * reference chooses `applicable` (src/vkmr/Reductions.cpp:471): log2(capacity) for
 * every slice when the stream spans several slices, ceil(log2(count)) (at least 1:
 * a lone leaf is hashed with itself, the CPU backend's rule)
 * for a single slice.  Requires ceil(count / 2^height) == 1.
 *   digests_dev  count cells, read only (the reference reduces in place)
 *   scratch_dev  vkmr_hip_reduce_scratch_bytes(count) bytes of device memory; the size function is an
 *                upper bound for EVERY run of at most `count` digests, so scratch sized for a slice's
 *                capacity serves any shorter slice (may be NULL for count <= 128); 16-byte aligned, see "Scratch buffers"
 *   root_dev     one cell in device memory receiving the root
 * height is at most 63.
 */
VKMR_API vkmr_status vkmr_hip_reduce_async(int dev, vkmr_stream s,
                                           const vkmr_digest* digests_dev, uint64_t count, uint32_t height,
                                           void* scratch_dev, vkmr_digest* root_dev);
VKMR_API size_t vkmr_hip_reduce_scratch_bytes(uint64_t count);

/*
 * METADATA FROM SIZES.  The strings of a batch lie back to back (string i + 1 starts on the word after string i:
 * Batch::Push, src/vkmr/Batches.cpp:64-121), so entry i is {first_word + sum over j < i of ceil(size[j] / 4), size[i]}:
 * what the reference's host code computes while it appends (WordCount, Batches.cpp:182-187).  A caller that feeds the
 * device over PCIe may send the 16-bit sizes (2 bytes per string instead of 8) and have the entries written in device
 * memory, where vkmr_hip_map_async reads them.  Every size must be below 65 536 (send the entries themselves otherwise).
 *   sizes_dev    count sizes, 16-byte aligned
 *   scratch_dev  vkmr_hip_sizes_scratch_bytes(count) bytes, 16-byte aligned (see "Scratch buffers")
 *   meta_dev     count entries, 16-byte aligned, written
 */
VKMR_API vkmr_status vkmr_hip_metadata_from_sizes_async(int dev, vkmr_stream s, const uint16_t* sizes_dev, uint32_t count,
                                                        uint32_t first_word, void* scratch_dev, vkmr_metadata* meta_dev);
VKMR_API size_t vkmr_hip_sizes_scratch_bytes(uint32_t count);

/*
 * REDUCE, several slices at once: `nslices` consecutive slices of `capacity` digests
 * each (a power of two), the last holding `count_last` <= capacity, all reduced
 * through `height` levels by the same launches; roots_dev[k] receives slice k's
 * root.  This is Instance::Root's loop "for every remaining slice Reduce(...)"
 * (src/vkmr/SHA-256vk.cpp:301-311) issued as one operation, so that the
 * latency-bound tops of the sub-trees run side by side instead of one after the
 * other.  Same per-slice contract as vkmr_hip_reduce_async.  scratch_dev needs
 * vkmr_hip_reduce_slices_scratch_bytes(capacity, nslices) bytes, 16-byte aligned (see "Scratch buffers").
 */
VKMR_API vkmr_status vkmr_hip_reduce_slices_async(int dev, vkmr_stream s,
                                                  const vkmr_digest* digests_dev, uint32_t nslices,
                                                  uint64_t capacity, uint64_t count_last, uint32_t height,
                                                  void* scratch_dev, vkmr_digest* roots_dev);
VKMR_API size_t vkmr_hip_reduce_slices_scratch_bytes(uint64_t capacity, uint32_t nslices);

/*
 * PROOF (the reference's own "to do", README.md:118-120): the authentication path of
 * leaf `index` in exactly the tree vkmr_hip_reduce_async(count, height) computes.
 * siblings_dev[l], l = 0..height-1, receives the node the path node is hashed with at
 * level l: its left or right neighbour (bit l of `index` says which side the path node
 * is on: 0 = path node left), or the path node itself where it has no right sibling
 * (duplicate-last rule).  Folding the leaf digest with the siblings from l = 0 upwards
 * gives the root, which is also written to root_dev (may be NULL).  For a stream that
 * spans several slices the caller chains two proofs: this one inside the slice
 * (height = log2 capacity) and one over the slice roots.  Each sibling is the root of
 * the neighbouring sub-tree of 2^l leaves and is computed with the same kernels as the
 * reduction (total work: about one more reduction of the slice).
 * scratch_dev: vkmr_hip_reduce_scratch_bytes(count) bytes, 16-byte aligned (see "Scratch buffers").
 */
VKMR_API vkmr_status vkmr_hip_proof_async(int dev, vkmr_stream s,
                                          const vkmr_digest* digests_dev, uint64_t count, uint32_t height,
                                          uint64_t index, void* scratch_dev,
                                          vkmr_digest* siblings_dev, vkmr_digest* root_dev);

/*
 * REDUCE + PROOFS in one pass -- the reference's to-do as it words it: "for an indicated leaf,
 * allocate a buffer to hold and write out the intermediate values during reduction"
 * (README.md:118-120).  Exactly vkmr_hip_reduce_async (same launches, same root) with the
 * kernels' proof-writing instantiations: the lane that hashes the pair a path node belongs to
 * stores the other node of that pair.  indices[0..k): leaf indices (< count), k <= 16, read on
 * the host at call time.  siblings_dev[q * height + l] = sibling of indices[q]'s path node at
 * level l, as vkmr_hip_proof_async defines it; no extra hash is computed, the reduction's time
 * does not change measurably.  vkmr_hip_proof_async is kept as the independent cross-check.  scratch_dev: as vkmr_hip_reduce_async
 * takes it, 16-byte aligned (see "Scratch buffers").
 */
VKMR_API vkmr_status vkmr_hip_reduce_proofs_async(int dev, vkmr_stream s,
                                                  const vkmr_digest* digests_dev, uint64_t count, uint32_t height,
                                                  void* scratch_dev, vkmr_digest* root_dev,
                                                  const uint64_t* indices, uint32_t k, vkmr_digest* siblings_dev);

/*
 * One tree level per launch, one lane per pair: the reference's non-subgroup
 * reduction (BasicReduction, src/vkmr/Reductions.cpp:257-409; shader :393-434).
 * Kept as an independent cross-check of vkmr_hip_reduce_async; same contract.
 * scratch_dev needs vkmr_hip_reduce_levels_scratch_bytes(count) bytes, 16-byte aligned (see "Scratch buffers").
 */
VKMR_API vkmr_status vkmr_hip_reduce_levels_async(int dev, vkmr_stream s,
                                                  const vkmr_digest* digests_dev, uint64_t count, uint32_t height,
                                                  void* scratch_dev, vkmr_digest* root_dev);
VKMR_API size_t vkmr_hip_reduce_levels_scratch_bytes(uint64_t count);

/*
 * STORED TREE (the reference's proof "to do", README.md:118-120, for any number of leaves): every level of the tree
 * vkmr_hip_reduce_async(count, height) computes, kept in HBM.  Level 0 is digests_dev itself (not copied); tree_dev
 * holds levels 1..height back to back: level l has n_l = ceil(count / 2^l) cells and starts at cell
 * sum over 1 <= j < l of n_j.  Node j of level l = SHA-256d(L[l-1][2j] || L[l-1][min(2j+1, n_{l-1}-1)]) (duplicate-last
 * rule, also after the count has collapsed to one: the last-slice rule), so the last cell of tree_dev is the root that
 * vkmr_hip_reduce_async writes.  Same height contract as every reduce; height == 0 (count == 1) writes nothing (the root
 * is the leaf) and tree_dev may then be NULL.  One launch of the levels kernel per level: about the cost of
 * vkmr_hip_reduce_levels_async.
 *   tree_dev  vkmr_hip_tree_bytes(count, height) bytes of device memory
 * vkmr_hip_tree_bytes returns 0 for count == 0 or height > 63.
 */
VKMR_API size_t vkmr_hip_tree_bytes(uint64_t count, uint32_t height);
VKMR_API vkmr_status vkmr_hip_reduce_tree_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev,
                                                uint64_t count, uint32_t height, vkmr_digest* tree_dev);

/*
 * PROOFS FROM THE STORED TREE (README.md:118-120): a gather, no hash.  digests_dev and tree_dev as written by
 * vkmr_hip_reduce_tree_async(count, height); indices_dev: k leaf indices in DEVICE memory (k any value up to 2^32 - 1).
 * siblings_dev[q * height + l] (k * height cells, indexed in 64 bits) = L[l][s] with p = indices[q] >> l, s = p ^ 1, or
 * s = p where p ^ 1 >= n_l -- exactly vkmr_hip_proof_async's siblings and the layout of vkmr_hip_reduce_proofs_async.
 * The host cannot check indices that live on the device: an index >= count gets `height` all-zero cells.
 * k == 0 does nothing; height == 0 writes nothing.
 */
VKMR_API vkmr_status vkmr_hip_tree_proofs_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev,
                                                const vkmr_digest* tree_dev, uint64_t count, uint32_t height,
                                                const uint64_t* indices_dev, uint32_t k, vkmr_digest* siblings_dev);

/*
 * BATCH VERIFICATION (the reference has no counterpart: it neither writes nor checks proofs).  One lane per proof: leaf
 * leaves_dev[q] is folded with siblings_dev[q * height + l], l = 0..height-1, as vkmr_host_cpu_fold_proof does (bit l of
 * indices_dev[q] set: node = SHA-256d(sibling || node), else SHA-256d(node || sibling)).  ok_dev[q] = 1 when
 * indices_dev[q] < 2^height and the fold equals roots_dev[nroots == 1 ? 0 : q], else 0.
 *   height 1..63; nroots 1 (every proof against one root) or k (a root per proof); all buffers in device memory.
 * A proof shows membership AT A POSITION, not the number of leaves: under the duplicate-last rule the last node of an
 * odd level is its own sibling, so a tree over an odd number n of leaves and one over n + 1 leaves whose last leaf
 * repeats the n-th have the same root (the known ambiguity of Bitcoin-style trees).  Callers that need the count commit to it elsewhere.
 * k == 0 does nothing.
 */
VKMR_API vkmr_status vkmr_hip_verify_proofs_async(int dev, vkmr_stream s, const vkmr_digest* leaves_dev,
                                                  const uint64_t* indices_dev, const vkmr_digest* siblings_dev,
                                                  uint32_t k, uint32_t height, const vkmr_digest* roots_dev,
                                                  uint32_t nroots, uint32_t* ok_dev);

/*
 * UPDATE LEAVES OF THE STORED TREE (the reference has no counterpart: its trees are rebuilt).  digests_dev and tree_dev
 * as written by vkmr_hip_reduce_tree_async(count, height); level 0 is the caller's digests buffer and this call writes
 * into it.  indices_dev[0..k) and leaves_dev[0..k) in DEVICE memory: the indices strictly increasing and < count (the
 * host cannot check them; the device does, see status_dev).  On success digests_dev[indices[q]] = leaves[q] for every q,
 * and every ancestor of those leaves is hashed again by the rule of the stored tree (duplicate-last, also after the
 * count has collapsed to one), so every cell equals what a fresh vkmr_hip_reduce_tree_async over the updated leaves
 * writes.  No other cell is written.  Work: sum over l = 1..height of |unique(indices >> l)| node hashes, one launch
 * per level.
 *   status_dev  one uint32_t in device memory, always written: 0 when the update was applied; bit 0 set if an index
 *               was >= count, bit 1 if the indices were not strictly increasing (out of order or repeated).  When it
 *               is nonzero NOTHING in the leaves or the tree has changed.
 * k == 0 does nothing whatever the other arguments; height == 0 (count == 1) writes only the leaf, and tree_dev may then
 * be NULL.  Stream-ordered: a proof gather or verify enqueued after it on the same stream sees the new tree.
 */
VKMR_API vkmr_status vkmr_hip_tree_update_async(int dev, vkmr_stream s, vkmr_digest* digests_dev, vkmr_digest* tree_dev,
                                                uint64_t count, uint32_t height, const uint64_t* indices_dev,
                                                const vkmr_digest* leaves_dev, uint32_t k, uint32_t* status_dev);

/*
 * MULTIPROOF FROM THE STORED TREE (the reference has no counterpart): ONE proof for k leaves of one tree -- the proved
 * leaves, their positions and the nodes that cannot be recomputed from them, each once -- instead of k independent proofs
 * whose paths merge on the way up.  digests_dev and tree_dev as written by vkmr_hip_reduce_tree_async(count, height);
 * indices_dev[0..k) in DEVICE memory, strictly increasing and < count (the rule of vkmr_hip_tree_update_async; the device
 * checks it).  Let A_0 = the indices and A_{l+1} = unique(A_l >> 1).  For l = 0..height-1 in this order, and inside a level
 * for p in A_l ascending: nothing when p ^ 1 is in A_l (the verifier computes that node itself), else ONE node, L[l][p ^ 1],
 * or L[l][p] where p ^ 1 >= n_l (the cell vkmr_hip_tree_proofs_async puts there).  nodes_dev receives these M = sum of m_l
 * cells in that order.  m_l <= min(k, n_{l+1}): vkmr_hip_multiproof_max_nodes returns the bound
 * sum over l < height of min(k, ceil(count / 2^(l+1))) cells (0 for count == 0 or height > 63).  For k == 1 the multiproof is
 * the single proof: M == height, the cells of vkmr_hip_tree_proofs_async.  A gather, no hash.
 *   scratch_dev     vkmr_hip_multiproof_scratch_bytes(k, height) bytes of device memory, 16-byte aligned (0 for k == 0 or
 *                   height > 63; one size serves the gather and the verifier below)
 *   nodes_capacity  cells nodes_dev can hold; nodes_dev may be NULL when it is 0
 *   info_dev        2 + height uint64_t in device memory.  info_dev[0] = status, always written: 0 done; bit 0 an index
 *                   >= count, bit 1 indices not strictly increasing (both as vkmr_hip_tree_update_async defines them; then
 *                   nothing else of the caller's is written: info_dev[1..] keep what they held and must not be read);
 *                   bit 2 M > nodes_capacity (then info_dev[1] and the counts are written and valid and no node is, so the
 *                   caller can allocate and call again).  info_dev[1] = M, info_dev[2 + l] = m_l.
 * k == 0 does nothing whatever the other arguments; height == 0 (count == 1) writes the status and M = 0, and tree_dev,
 * scratch_dev and nodes_dev may then be NULL.  Stream-ordered like the other tree calls: a multiproof gathered after an
 * update on the same stream proves the new tree.
 */
VKMR_API size_t vkmr_hip_multiproof_max_nodes(uint64_t count, uint32_t height, uint32_t k);
VKMR_API size_t vkmr_hip_multiproof_scratch_bytes(uint32_t k, uint32_t height);
VKMR_API vkmr_status vkmr_hip_tree_multiproof_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev,
                                                    const vkmr_digest* tree_dev, uint64_t count, uint32_t height,
                                                    const uint64_t* indices_dev, uint32_t k, void* scratch_dev,
                                                    vkmr_digest* nodes_dev, uint64_t nodes_capacity, uint64_t* info_dev);

/*
 * MULTIPROOF VERIFICATION: one root, one answer.  leaves_dev[0..k) are the proved leaves, indices_dev[0..k) their
 * positions, nodes_dev[0..m) the multiproof in the order above; never `count`: whether p ^ 1 is in A_l follows from the
 * indices alone, and a duplicated last node arrives as an ordinary node of the proof.  cur_0[p] = the leaf of p.  For each
 * level, for each P in A_{l+1} ascending: of the children 2P and 2P + 1, those in A_l come from cur_l and a missing one is
 * the next unread node; cur_{l+1}[P] = SHA-256d(left || right).  ok_dev[0] = 1 iff the indices are strictly increasing and
 * < 2^height, exactly m nodes are consumed and cur_height[0] equals root_dev[0]; else 0.  Work: sum over l = 1..height of
 * |A_l| node hashes, one launch per level.  The leaves are not overwritten.
 *   height 1..63; scratch_dev: vkmr_hip_multiproof_scratch_bytes(k, height) bytes, 16-byte aligned; nodes_dev may be NULL
 *   when m == 0; all buffers in device memory.
 * As with vkmr_hip_verify_proofs_async, this shows membership AT POSITIONS, not the number of leaves: the known ambiguity
 * of duplicate-last trees is unchanged.  k == 0 does nothing.  vkmr_host_cpu_verify_multiproof (libvkmr_host.so) applies the
 * same rule on the CPU, for a receiver without a GPU.
 */
VKMR_API vkmr_status vkmr_hip_verify_multiproof_async(int dev, vkmr_stream s, const vkmr_digest* leaves_dev,
                                                      const uint64_t* indices_dev, uint32_t k, uint32_t height,
                                                      const vkmr_digest* nodes_dev, uint64_t m, const vkmr_digest* root_dev,
                                                      void* scratch_dev, uint32_t* ok_dev);

/*
 * FOREST (the reference has no counterpart: it reduces one stream to one root): the roots of `ntrees` independent trees of
 * unequal size in ONE call -- the blocks of a chain, the files of an index, the accounts of a state.  digests_dev holds
 * `total` cells, the leaves of all trees back to back; offsets_dev is ntrees + 1 uint64_t in DEVICE memory and tree t is
 * cells [offsets[t], offsets[t+1]), c_t of them.  roots_dev[t] receives what vkmr_hip_reduce_async(c_t, h_t) writes with
 * h_t = max(1, ceil(log2 c_t)): the single-slice rule (duplicate-last at every level, a lone leaf hashed with itself once).
 * An empty tree (c_t == 0) gets an all-zero cell and is not an error.
 *   max_count    the caller's upper bound on every c_t (at least 1; a value above `total` is treated as `total`).  It
 *                fixes the number of levels, and so the launches, without the host reading the offsets: one launch per
 *                level, max(1, ceil(log2 max_count)) of them, one lane per node of the whole forest at that level.  The
 *                launch sequence depends on (total, ntrees, max_count) only and never grows with ntrees.
 *   status_dev   one uint32_t in device memory, always written: 0 when done.  The host cannot check offsets that live on
 *                the device; the device does, before any root is written: bit 0 set if the offsets decrease somewhere or
 *                offsets[ntrees] > total, bit 1 if some c_t > max_count.  When it is nonzero NO cell of roots_dev is
 *                written (the rule of vkmr_hip_tree_update_async).
 *   scratch_dev  vkmr_hip_forest_scratch_bytes(total, ntrees) bytes of device memory, 16-byte aligned:
 *                32 * ((total >> 1) + (total >> 2) + 2 * ntrees), an upper bound for EVERY forest of at most `total`
 *                leaves in at most `ntrees` trees; 0 for ntrees == 0.
 * ntrees == 0 does nothing whatever the other arguments.  total == 0 with ntrees > 0 is allowed (every tree empty) and
 * digests_dev may then be NULL.  Stream-ordered: no allocation, no host synchronisation, no host read of device data.
 * vkmr_host_cpu_forest_roots (libvkmr_host.so) applies the same rule on the CPU, for a receiver without a GPU.
 */
VKMR_API size_t vkmr_hip_forest_scratch_bytes(uint64_t total, uint32_t ntrees);
VKMR_API vkmr_status vkmr_hip_reduce_forest_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev, uint64_t total,
                                                  const uint64_t* offsets_dev, uint32_t ntrees, uint64_t max_count,
                                                  void* scratch_dev, vkmr_digest* roots_dev, uint32_t* status_dev);

/*
 * STORED FOREST: vkmr_hip_reduce_forest_async with every level kept in HBM, so that the forest can hand out proofs.  Same
 * contract, same device-side checks and same launches (the status word zeroed, the check, one launch per level); there is
 * no scratch argument.  With H = max(1, ceil(log2 min(max_count, total))) levels and cells(l) = (total >> l) + ntrees:
 * level 0 is digests_dev itself (not copied); level l = 1..H has a buffer of cells(l) cells that starts at cell
 * sum over 1 <= j < l of cells(j) of forest_dev, and node j of tree t's level l is cell (offsets[t] >> l) + t + j of it, for
 * l < h_t.  Level h_t of tree t is its root and goes to roots_dev[t] as in vkmr_hip_reduce_forest_async (an empty tree: an
 * all-zero cell).  Cells of a level buffer that are not a node of some tree at that level are unspecified; nothing reads
 * them.  A nonzero status writes no root, and the forest is then not to be used.
 *   forest_dev  vkmr_hip_forest_tree_bytes(total, ntrees, max_count) bytes of device memory, 16-byte aligned:
 *               32 * sum over l = 1..H of cells(l); 0 for ntrees == 0 or max_count == 0.
 * ntrees == 0 does nothing whatever the other arguments.
 */
VKMR_API size_t vkmr_hip_forest_tree_bytes(uint64_t total, uint32_t ntrees, uint64_t max_count);
VKMR_API vkmr_status vkmr_hip_reduce_forest_tree_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev, uint64_t total,
                                                       const uint64_t* offsets_dev, uint32_t ntrees, uint64_t max_count,
                                                       vkmr_digest* forest_dev, vkmr_digest* roots_dev, uint32_t* status_dev);

/*
 * MUTATED TREES (CVE-2012-2459): the duplicate-last tree lets different leaf lists share a root -- [a, b, c] and
 * [a, b, c, c]; [a, b, c, d, e, f] and [a, b, c, d, e, f, e, f] -- so a root alone does not commit to the leaf list.  The
 * two builds above, with Bitcoin Core's ComputeMerkleRoot(hashes, &mutated) formed in the same launches, the level kept:
 * mutated_dev[t] (ntrees uint64_t in device memory) gets bit l set iff level l of tree t (n_l = ceil(c_t / 2^l) nodes,
 * 0 <= l < h_t) holds a j with 2j + 1 < n_l and node 2j equal to node 2j + 1: a pair in which BOTH nodes exist.  The last
 * node of an odd level, hashed with itself, is no such pair; an empty tree and a tree of one leaf get 0.  A caller who wants
 * Bitcoin Core's bool tests mutated[t] != 0.  A mutated tree is not refused: its root is written like any other.
 * Contract, device-side checks, status bits, scratch / forest layout and the launches are those of
 * vkmr_hip_reduce_forest_async and vkmr_hip_reduce_forest_tree_async (the status word zeroed, the check, one launch per
 * level; each level launch compares the two children it has loaded for the hash), plus one memset of mutated_dev in the same
 * sequence; the roots, and every cell of the stored forest, are the plain build's.  A nonzero status leaves mutated_dev all
 * zero and writes no root.  ntrees == 0 does nothing whatever the other arguments.  Refused on the host (VKMR_ERR_INVALID)
 * with ntrees > 0, before any HIP call: what the plain build refuses, and a NULL mutated_dev.
 * vkmr_host_cpu_forest_mutated (libvkmr_host.so) applies the same rule on the CPU, for a receiver without a GPU.
 */
VKMR_API vkmr_status vkmr_hip_reduce_forest_mutated_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev, uint64_t total,
                                                          const uint64_t* offsets_dev, uint32_t ntrees, uint64_t max_count,
                                                          void* scratch_dev, vkmr_digest* roots_dev, uint64_t* mutated_dev,
                                                          uint32_t* status_dev);
VKMR_API vkmr_status vkmr_hip_reduce_forest_tree_mutated_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev, uint64_t total,
                                                               const uint64_t* offsets_dev, uint32_t ntrees, uint64_t max_count,
                                                               vkmr_digest* forest_dev, vkmr_digest* roots_dev, uint64_t* mutated_dev,
                                                               uint32_t* status_dev);

/*
 * THE MASKS OF A STORED FOREST, formed again from its levels as they are now: for a forest whose leaves have changed through
 * vkmr_hip_forest_update_async, which rehashes paths and compares nothing.  digests_dev and forest_dev as written by
 * vkmr_hip_reduce_forest_tree_async (or its flagged twin); the call TRUSTS that offsets_dev, total, ntrees and max_count are
 * those of that build and that the build reported status 0 (the rule of vkmr_hip_forest_proofs_async).  mutated_dev gets
 * what vkmr_hip_reduce_forest_tree_mutated_async over the present leaves would write.  A compare, no hash: every level below
 * the roots is read once.  Launches, all on the caller's stream: mutated_dev zeroed, then one launch per level,
 * H = max(1, ceil(log2 min(max_count, total))) of them, with the build's grid; no allocation, no host read of device data.
 * Refused on the host (VKMR_ERR_INVALID) with ntrees > 0: a NULL pointer (digests_dev may be NULL when total == 0),
 * max_count == 0, total > 2^58.  ntrees == 0 does nothing whatever the other arguments.
 * Stream-ordered: a scan enqueued after an update on the same stream sees the new forest.
 */
VKMR_API vkmr_status vkmr_hip_forest_tree_mutated_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev,
                                                        const vkmr_digest* forest_dev, uint64_t total, const uint64_t* offsets_dev,
                                                        uint32_t ntrees, uint64_t max_count, uint64_t* mutated_dev);

/*
 * PROOFS FROM THE STORED FOREST ("is leaf i in tree t?"): a gather, no hash.  digests_dev and forest_dev as written by
 * vkmr_hip_reduce_forest_tree_async; the call TRUSTS that offsets_dev, total, ntrees and max_count are those of that build
 * and that the build reported status 0 -- it checks no offset again and follows them into the forest.  Query q is leaf
 * indices_dev[q] (its index inside its tree) of tree trees_dev[q]; both arrays live in DEVICE memory, in any order, repeats
 * allowed.  With H as above, the stride of a forest's proofs:
 *   heights_dev[q]           = h_t = max(1, ceil(log2 c_t))
 *   siblings_dev[q * H + l]  for l < h_t: the cell vkmr_hip_tree_proofs_async gives for a tree built over tree t's leaves
 *                            alone, L_t[l][p ^ 1] with p = index >> l, or L_t[l][p] where p ^ 1 >= n_l; all-zero for l >= h_t
 * (k * H cells, indexed in 64 bits).  The host cannot check queries that live on the device: trees[q] >= ntrees or
 * indices[q] >= c_t (so every query into an empty tree) gets height 0 and H all-zero cells, the rule of
 * vkmr_hip_tree_proofs_async for a bad index.  k == 0 does nothing.
 * vkmr_host_cpu_forest_proofs (libvkmr_host.so) applies the same rule on the CPU, for a sender without a GPU.
 */
VKMR_API vkmr_status vkmr_hip_forest_proofs_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev,
                                                  const vkmr_digest* forest_dev, uint64_t total, const uint64_t* offsets_dev,
                                                  uint32_t ntrees, uint64_t max_count, const uint32_t* trees_dev,
                                                  const uint64_t* indices_dev, uint32_t k, vkmr_digest* siblings_dev,
                                                  uint32_t* heights_dev);

/*
 * BATCH VERIFICATION OF FOREST PROOFS: vkmr_hip_verify_proofs_async for proofs of unequal height against the roots of a
 * forest.  One lane per proof.  ok_dev[q] = 1 iff 1 <= heights_dev[q] <= stride, indices_dev[q] < 2^heights_dev[q],
 * trees_dev[q] < ntrees, and leaves_dev[q] folded with siblings_dev[q * stride + l], l = 0..heights_dev[q]-1, as
 * vkmr_host_cpu_fold_proof does equals roots_dev[trees_dev[q]]; else 0.  Cells at l >= heights_dev[q] are never read.
 *   stride 1..63 (the H of vkmr_hip_forest_proofs_async, or any layout with at least the tallest proof's cells per proof);
 *   roots_dev: ntrees cells; all buffers in device memory.
 * The counts and the offsets of the forest are not arguments: a proof shows membership AT A POSITION of the tree whose root
 * it names, not the number of leaves, as stated at vkmr_hip_verify_proofs_async.  A wavefront works until its tallest proof
 * is folded.  k == 0 does nothing.
 */
VKMR_API vkmr_status vkmr_hip_verify_forest_proofs_async(int dev, vkmr_stream s, const vkmr_digest* leaves_dev,
                                                         const uint32_t* trees_dev, const uint64_t* indices_dev,
                                                         const vkmr_digest* siblings_dev, const uint32_t* heights_dev,
                                                         uint32_t k, uint32_t stride, const vkmr_digest* roots_dev,
                                                         uint32_t ntrees, uint32_t* ok_dev);

/*
 * LEAF UPDATES OF THE STORED FOREST: vkmr_hip_tree_update_async for a forest.  digests_dev, forest_dev and roots_dev as
 * written by vkmr_hip_reduce_forest_tree_async; the call TRUSTS that offsets_dev, total, ntrees and max_count are those of
 * that build and that the build reported status 0 (the rule of vkmr_hip_forest_proofs_async).  Entry q sets leaf
 * indices_dev[q] (its index inside its tree) of tree trees_dev[q] to leaves_dev[q]; all three arrays live in DEVICE memory,
 * and the (tree, index) pairs are strictly increasing in lexicographic order with index < c_t.  Every ancestor of an
 * updated leaf is rehashed once, in its tree's own cells: sum over l >= 1 of the distinct (tree, index >> l) pairs with
 * l <= h_t node hashes, and the root of every touched tree is written to roots_dev[t].
 *   status_dev  one uint32_t in device memory, always written: 0 when the update was applied; bit 0 set if a tree was
 *               >= ntrees or an index >= c_t (so for every entry into an empty tree), bit 1 if the pairs were not strictly
 *               increasing (out of order or repeated).  When it is nonzero NOTHING of the caller's has changed: no leaf,
 *               no cell of forest_dev, no root.
 * After status 0 every cell of the leaves, of forest_dev and of roots_dev equals what a fresh
 * vkmr_hip_reduce_forest_tree_async over the updated leaves writes; cells that a build never writes are not written here
 * either, nor are the roots of trees no entry names.  Launches, all on the caller's stream: the status word zeroed, the
 * check, the leaves, then one launch of k lanes per level, H = max(1, ceil(log2 min(max_count, total))) of them; never a
 * launch per tree, no allocation, no host read of device data.  Refused on the host (VKMR_ERR_INVALID) with k > 0: a NULL
 * pointer, ntrees == 0 or total == 0, max_count == 0, total > 2^58.  k == 0 does nothing whatever the other arguments.
 * Stream-ordered: a proof gather or verify enqueued after it on the same stream sees the new forest.
 */
VKMR_API vkmr_status vkmr_hip_forest_update_async(int dev, vkmr_stream s, vkmr_digest* digests_dev, vkmr_digest* forest_dev,
                                                  uint64_t total, const uint64_t* offsets_dev, uint32_t ntrees,
                                                  uint64_t max_count, const uint32_t* trees_dev, const uint64_t* indices_dev,
                                                  const vkmr_digest* leaves_dev, uint32_t k, vkmr_digest* roots_dev,
                                                  uint32_t* status_dev);

/*
 * MULTIPROOF FROM THE STORED FOREST: ONE compact proof for k leaves of MANY trees -- the matching transactions of many
 * blocks, sampled files of an index, batches from many accounts -- instead of k independent vkmr_hip_forest_proofs_async
 * proofs of H cells each whose paths merge on the way up.  digests_dev and forest_dev as written by
 * vkmr_hip_reduce_forest_tree_async; the call TRUSTS that offsets_dev, total, ntrees and max_count are those of that build and
 * that the build reported status 0 (the rule of vkmr_hip_forest_proofs_async).  Entry q is leaf indices_dev[q] (uint64, its
 * index inside its tree) of tree trees_dev[q] (uint32); both arrays live in DEVICE memory and the (tree, index) pairs are
 * strictly increasing in lexicographic order with tree < ntrees and index < c_t: the rule of vkmr_hip_forest_update_async,
 * checked on the device with the same status bits.  With h_t = max(1, ceil(log2 c_t)), H = max(1, ceil(log2 min(max_count,
 * total))) the forest's stride, and for tree t A_0(t) = its indices and A_{l+1}(t) = unique(A_l(t) >> 1): for l = 0..H-1 in
 * this order, inside a level for t ascending over the trees with l < h_t, inside a tree for p in A_l(t) ascending: nothing
 * when p ^ 1 is in A_l(t), else ONE node, L_t[l][p ^ 1], or L_t[l][p] where p ^ 1 >= n_l (the cell
 * vkmr_hip_forest_proofs_async puts there).  Neighbours in another tree never count as siblings; a tree of one leaf emits
 * the leaf itself.  The order is level-major over the WHOLE forest; restricted to one tree the nodes are that tree's
 * vkmr_hip_tree_multiproof_async multiproof, level by level.  nodes_dev receives these M = sum of m_l cells in that order.
 * Each emitted node belongs to one parent of a live tree, so m_l <= min(k, (total >> (l+1)) + ntrees):
 * vkmr_hip_forest_multiproof_max_nodes returns the sum of that bound over l < H (0 for total == 0, ntrees == 0 or
 * max_count == 0).  A gather, no hash.
 *   scratch_dev     vkmr_hip_forest_multiproof_scratch_bytes(k, H) bytes of device memory (a multiple of 16), 16-byte aligned (0 for k == 0 or
 *                   stride > 63; one size serves the gather and the verifier below)
 *   nodes_capacity  cells nodes_dev can hold; nodes_dev may be NULL when it is 0
 *   heights_dev     k uint32_t: heights_dev[q] = h of entry q's tree, as in vkmr_hip_forest_proofs_async
 *   info_dev        2 + H uint64_t in device memory.  info_dev[0] = status, always written: 0 done; bit 0 a tree >= ntrees or
 *                   an index >= c_t, bit 1 pairs not strictly increasing (both as vkmr_hip_forest_update_async defines them;
 *                   then nothing else of the caller's is written: heights_dev, nodes_dev and info_dev[1..] keep what they
 *                   held); bit 2 M > nodes_capacity (then the heights, info_dev[1] and the counts are written and valid and
 *                   no node is, so the caller can allocate and call again).  info_dev[1] = M, info_dev[2 + l] = m_l over
 *                   the whole forest.
 * Launches, all on the caller's stream: the status zeroed, the check, the heights, the ranking of
 * vkmr_hip_tree_multiproof_async with height := H, one gather of H x k lanes; never a launch per tree, no allocation, no host
 * read of device data.  Refused on the host (VKMR_ERR_INVALID) with k > 0: a NULL pointer, ntrees == 0 or total == 0,
 * max_count == 0, total > 2^58, scratch_dev not 16-byte aligned.  k == 0 does nothing whatever the other arguments.
 * Stream-ordered: a multiproof gathered after an update on the same stream proves the new forest.
 * vkmr_host_cpu_forest_multiproof (libvkmr_host.so) applies the same rule on the CPU, for a sender without a GPU.
 */
VKMR_API size_t vkmr_hip_forest_multiproof_max_nodes(uint64_t total, uint32_t ntrees, uint64_t max_count, uint32_t k);
VKMR_API size_t vkmr_hip_forest_multiproof_scratch_bytes(uint32_t k, uint32_t stride);
VKMR_API vkmr_status vkmr_hip_forest_multiproof_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev,
                                                      const vkmr_digest* forest_dev, uint64_t total, const uint64_t* offsets_dev,
                                                      uint32_t ntrees, uint64_t max_count, const uint32_t* trees_dev,
                                                      const uint64_t* indices_dev, uint32_t k, void* scratch_dev,
                                                      vkmr_digest* nodes_dev, uint64_t nodes_capacity, uint32_t* heights_dev,
                                                      uint64_t* info_dev);

/*
 * FOREST MULTIPROOF VERIFICATION: many roots, one answer.  leaves_dev[0..k) are the proved leaves, (trees_dev[q],
 * indices_dev[q]) their positions, heights_dev[q] the height of entry q's tree, nodes_dev[0..m) the multiproof in the order
 * above; never the counts or the offsets of the forest.  ok_dev[0] = 1 iff the pairs are strictly increasing, every tree
 * < ntrees, 1 <= heights_dev[q] <= stride, indices_dev[q] < 2^heights_dev[q], the entries of one tree carry one height, the
 * indices and heights imply exactly m nodes, and for every tree that some entry names the fold equals roots_dev[t]; else 0.
 * The fold is vkmr_hip_verify_multiproof_async's rule tree by tree, through heights_dev levels, a missing child being the
 * next unread node in the order above.  Roots of trees no entry names are not read.  Work: the distinct (tree, index >> l)
 * pairs with 1 <= l <= h_t node hashes, one launch of k lanes per level l < stride.  The leaves are not overwritten.
 *   stride 1..63 (the H of vkmr_hip_forest_multiproof_async, or anything at least the tallest tree's height); roots_dev:
 *   ntrees cells; scratch_dev: vkmr_hip_forest_multiproof_scratch_bytes(k, stride) bytes, 16-byte aligned; nodes_dev may be
 *   NULL when m == 0; all buffers in device memory.
 * As with vkmr_hip_verify_proofs_async, this shows membership AT POSITIONS, not the number of leaves: the known ambiguity
 * of duplicate-last trees is unchanged.  k == 0 does nothing.  vkmr_host_cpu_verify_forest_multiproof (libvkmr_host.so)
 * applies the same rule on the CPU, for a receiver without a GPU.
 */
VKMR_API vkmr_status vkmr_hip_verify_forest_multiproof_async(int dev, vkmr_stream s, const vkmr_digest* leaves_dev,
                                                             const uint32_t* trees_dev, const uint64_t* indices_dev,
                                                             const uint32_t* heights_dev, uint32_t k, uint32_t stride,
                                                             const vkmr_digest* nodes_dev, uint64_t m,
                                                             const vkmr_digest* roots_dev, uint32_t ntrees, void* scratch_dev,
                                                             uint32_t* ok_dev);

/*
 * APPLYING A MULTIPROOF (the reference has no counterpart): a party that holds ONLY THE ROOTS follows leaf updates.  The
 * primary replaces k leaves (vkmr_hip_forest_update_async) and sends the multiproof it gathered BEFORE the update, the old
 * and the new leaves and the counts; the follower checks the old leaves against its roots and folds the new leaves up the
 * same paths, and its roots advance without a leaf of the forest ever reaching it.  The forest form; the tree form is the
 * same with one tree, one `count` and one `height`.
 *   old_leaves_dev, new_leaves_dev   k cells each: the leaves at the entries before and after the update
 *   trees_dev, indices_dev, nodes_dev, m, roots_dev, ntrees, stride   as vkmr_hip_verify_forest_multiproof_async takes them
 *   counts_dev      k uint64_t in device memory: counts_dev[q] = c_t of entry q's tree.  Heights are not passed: the device
 *                   derives h = max(1, ceil(log2 c)).  The tree call takes `count` and `height`, height 1..63 with
 *                   2^height >= count, which may lie above the minimal one as in vkmr_hip_reduce_tree_async.
 *   scratch_dev     vkmr_hip_apply_multiproof_scratch_bytes(k, stride or height) bytes of device memory, 16-byte aligned: the
 *                   verifier's scratch in whole 16-byte units, then a second array of k cells, a second array of k uint32_t
 *                   and k uint32_t of heights, each part starting on 16 bytes (0 for k == 0 or levels > 63)
 *   new_roots_dev   ntrees cells (the tree call: one); may be roots_dev itself, so that a replica's roots advance in place:
 *                   the old roots are last read before the first new root is written
 * ok_dev[0] = 1 iff every count is >= 1, indices_dev[q] < counts_dev[q], the entries of one tree carry one count (status bit
 * 3, as for unequal heights) and vkmr_hip_verify_forest_multiproof_async would answer 1 for (old_leaves_dev, trees_dev,
 * indices_dev, the heights derived from the counts, stride, nodes_dev, m, roots_dev); else 0.  In the tree call a count of 0
 * or above 2^height answers 0.  No condition is added on the node consumed at a duplicate position: with honest counts the old
 * fold already fails when it is wrong.
 * THE NEW SIDE.  The same fold runs over new_leaves_dev with one change.  The verifier never learns a count -- a duplicated
 * last node arrives as an ordinary node of the proof -- which is sound for checking and wrong for applying: where a path node
 * is the last node of an odd level, the proof carries that node's OLD value as its own sibling.  So for a left child p of tree
 * t's level l whose sibling is not among the entries, when p + 1 >= n_l(t) = ceil(c_t / 2^l) the proof's node is still
 * consumed, but the new side's right operand is the new side's own value of p.  Everywhere else both sides take the same node.
 * When ok is 1 the cell new_roots_dev[t] of every tree that some entry names receives the new root; cells of trees no entry
 * names are never written; when ok is 0 nothing is written.  ok == 1 means: the new roots are those of the forest with these
 * counts, the old roots, and the new leaves at these positions.  The counts are no more authenticated by a root than they
 * ever were: the ambiguity of duplicate-last trees named above is unchanged, and the `mutated` calls exist for it.
 * Work: two node hashes per distinct (tree, index >> l) pair with 1 <= l <= h_t, over the verifier's loads plus one cell.
 * Launches, all on the caller's stream and a function of (k, stride) alone: the status zeroed and ok set, the heights and
 * count checks, the verifier's check, masks and ranking, one launch of 2 x k lanes per level, the verifier's finish, one
 * commit; no allocation, no host synchronisation, no host read of device data.  Refused on the host (VKMR_ERR_INVALID) with
 * k > 0: a NULL pointer (nodes_dev may be NULL when m == 0), stride or height outside 1..63, scratch_dev not 16-byte aligned.
 * k == 0 does nothing.  vkmr_host_cpu_apply_multiproof and vkmr_host_cpu_apply_forest_multiproof (libvkmr_host.so) apply the
 * same two rules on the CPU, for a follower without a GPU.
 */
VKMR_API size_t vkmr_hip_apply_multiproof_scratch_bytes(uint32_t k, uint32_t levels);
VKMR_API vkmr_status vkmr_hip_apply_multiproof_async(int dev, vkmr_stream s, const vkmr_digest* old_leaves_dev,
                                                     const vkmr_digest* new_leaves_dev, const uint64_t* indices_dev, uint32_t k,
                                                     uint64_t count, uint32_t height, const vkmr_digest* nodes_dev, uint64_t m,
                                                     const vkmr_digest* root_dev, void* scratch_dev, uint32_t* ok_dev,
                                                     vkmr_digest* new_root_dev);
VKMR_API vkmr_status vkmr_hip_apply_forest_multiproof_async(int dev, vkmr_stream s, const vkmr_digest* old_leaves_dev,
                                                            const vkmr_digest* new_leaves_dev, const uint32_t* trees_dev,
                                                            const uint64_t* indices_dev, const uint64_t* counts_dev, uint32_t k,
                                                            uint32_t stride, const vkmr_digest* nodes_dev, uint64_t m,
                                                            const vkmr_digest* roots_dev, uint32_t ntrees, void* scratch_dev,
                                                            uint32_t* ok_dev, vkmr_digest* new_roots_dev);

/*
 * FIND LEAVES BY DIGEST ("where is this hash?"; the reference has no counterpart): the step from a digest a caller holds -- a
 * txid, a file hash, an account key -- to the position every call above takes.  digests_dev, total, offsets_dev and ntrees
 * as in vkmr_hip_reduce_forest_async; the call TRUSTS the offsets as vkmr_hip_forest_proofs_async does (non-decreasing,
 * offsets[ntrees] <= total).  It reads level 0 alone and needs no stored level, so it also serves a caller who only ever
 * reduced.  queries_dev[0..k) are digests in DEVICE memory, in any order, repeats allowed.  The answer to query q is the LOWEST
 * flat position p with offsets[0] <= p < offsets[ntrees] and digests_dev[p] == queries_dev[q] on all 32 bytes, reported as
 *   trees_dev[q]   = t, the one tree with offsets[t] <= p < offsets[t+1] (an empty tree is never named)
 *   indices_dev[q] = p - offsets[t]
 * and as trees_dev[q] = 0xFFFFFFFF, indices_dev[q] = 0xFFFFFFFFFFFFFFFF when there is no such p.  Equal leaves may exist
 * (Bitcoin's chain holds two txids that each appear in two blocks): the lowest position wins, whatever the scheduling.  Inner
 * nodes, roots and the duplicated last node of an odd level are not leaves, and cells of digests_dev outside
 * [offsets[0], offsets[ntrees]) belong to no tree: none of them is ever found.  The two output arrays are what
 * vkmr_hip_forest_proofs_async takes, with no host step in between: a found query gets its proof there, an unfound one (a
 * tree >= ntrees) height 0 and all-zero cells.
 *   scratch_dev  vkmr_hip_find_scratch_bytes(k) bytes of device memory, 8-byte aligned: T slots of 8 bytes, T the smallest
 *                power of two >= max(64, 2k), then 8k + 4k bytes, the sum rounded up to 16.  The call sets it itself.
 * The queries are put into an open-addressed table in the scratch and the leaves are streamed past it ONCE, each read once,
 * whatever k: the time is that of reading 32 * total bytes plus the table's traffic.  The table holds queries only, so the
 * length of a probe walk depends on the caller's own queries, never on the forest's leaves.
 * Launches, all on the caller's stream: one memset of the scratch, the insert (k lanes), the scan (a grid sized from the
 * device's compute units; none when total == 0), the resolve (k lanes).  They depend on (total, k) only and never grow with
 * ntrees; no allocation, no host synchronisation, no host read of device data.
 * k == 0 does nothing whatever the other arguments.  ntrees == 0 or total == 0 with k > 0 writes "not found" for every
 * query; digests_dev may then be NULL (and offsets_dev when ntrees == 0).  Refused on the host (VKMR_ERR_INVALID) with k > 0,
 * before any HIP call: a NULL pointer that is needed, total above 2^58, scratch_dev not 8-byte aligned.
 * Stream-ordered: a lookup enqueued after an update on the same stream sees the new leaves.
 * vkmr_host_cpu_forest_find (libvkmr_host.so) applies the same rule on the CPU, for a party without a GPU.
 */
VKMR_API size_t vkmr_hip_find_scratch_bytes(uint32_t k);
VKMR_API vkmr_status vkmr_hip_forest_find_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev, uint64_t total,
                                                const uint64_t* offsets_dev, uint32_t ntrees,
                                                const vkmr_digest* queries_dev, uint32_t k, void* scratch_dev,
                                                uint32_t* trees_dev, uint64_t* indices_dev);
/*
 * The same lookup in ONE tree, the leaves being cells [0, count) of digests_dev: indices_dev[q] = the lowest index whose leaf
 * equals queries_dev[q], or UINT64_MAX when there is none -- which vkmr_hip_tree_proofs_async already treats as a bad index
 * (all-zero cells).  Same scratch, launches and refusals (count above 2^58); count == 0 writes "not found" for every query
 * and digests_dev may then be NULL.  vkmr_host_cpu_tree_find is the CPU's.
 */
VKMR_API vkmr_status vkmr_hip_tree_find_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev, uint64_t count,
                                              const vkmr_digest* queries_dev, uint32_t k, void* scratch_dev,
                                              uint64_t* indices_dev);

/*
 * SORT AND DEDUP LEAF ENTRIES (the reference has no counterpart): the step from entries in CALL order -- what
 * vkmr_hip_forest_find_async writes, "not found" markers in between, or a caller's own batch -- to the strictly increasing
 * (tree, index) pairs that vkmr_hip_forest_update_async, vkmr_hip_forest_multiproof_async and their tree twins require, with
 * no entry and no digest going through the host.  total, offsets_dev and ntrees as in vkmr_hip_reduce_forest_async; the call
 * TRUSTS the offsets as vkmr_hip_forest_find_async does.  trees_dev[0..k), indices_dev[0..k) are the entries, in device
 * memory, in any order, repeats allowed.  Entry q is VALID iff trees_dev[q] < ntrees and indices_dev[q] < c_t; its key is the
 * flat position offsets[t] + index < total, whose order is the lexicographic order of the pairs.  Every entry is exactly one of
 *   a survivor                                                      info_dev[0] = n
 *   find's "not found" marker (trees_dev[q] == 0xFFFFFFFF), left out   info_dev[1]
 *   out of range (any other entry that is not valid), left out      info_dev[2]
 *   an earlier repeat of a pair that occurs again later, left out   info_dev[3]
 * so info_dev[0] + [1] + [2] + [3] == k.  info_dev: 4 uint64_t of device memory, always written when k > 0.
 * Cells [0, n) of trees_out_dev, indices_out_dev: the distinct valid pairs, strictly increasing -- exactly what the four
 * calls above accept.  order_out_dev[j] (uint32) is the LARGEST q whose pair equals output pair j: the last occurrence wins,
 * so the result is a function of the input alone, whatever the scheduling.  Cells at and behind n are unspecified.  The
 * outputs (k cells each) must not overlap the inputs or the scratch.  n stays on the device and the next call takes its k
 * on the host: the caller reads info_dev back (32 bytes), as with vkmr_hip_forest_multiproof_async's info_dev.
 *   scratch_dev  vkmr_hip_sort_entries_scratch_bytes(total, k) bytes of device memory, 16-byte aligned (layout:
 *                csrc/sort_plan.hpp: ping-pong keys and payloads, 24 k bytes, the histograms, the ranking words).
 * A stable LSD radix sort of (key, q), 8 bits per pass over bit_length(total) bits -- one pass for total < 256, at most 8 --
 * then the last pair of every run of equal keys is kept.  Launches, all on the caller's stream: two memsets, the keys, three
 * per pass (histogram, scan, scatter), the flags, three ranking launches, the emit.  They depend on (total, k) only; no
 * allocation, no host synchronisation, no host read of device data; no kernel waits for another workgroup.
 * k == 0 does nothing whatever the other arguments.  ntrees == 0 or total == 0 with k > 0 writes n = 0 and counts every entry
 * in info_dev[1] or info_dev[2]; offsets_dev may be NULL when ntrees == 0.  Refused on the host (VKMR_ERR_INVALID) with k > 0,
 * before any HIP call: a NULL pointer that is needed, total above 2^58, scratch_dev not 16-byte aligned.
 * vkmr_host_cpu_forest_sort_entries (libvkmr_host.so) applies the same rule on the CPU.
 */
VKMR_API size_t vkmr_hip_sort_entries_scratch_bytes(uint64_t total, uint32_t k);
VKMR_API vkmr_status vkmr_hip_forest_sort_entries_async(int dev, vkmr_stream s, uint64_t total, const uint64_t* offsets_dev,
                                                        uint32_t ntrees, const uint32_t* trees_dev, const uint64_t* indices_dev,
                                                        uint32_t k, void* scratch_dev, uint32_t* trees_out_dev,
                                                        uint64_t* indices_out_dev, uint32_t* order_out_dev, uint64_t* info_dev);
/*
 * The same for ONE tree of `count` leaves: every entry is in tree 0, the key is the index, the marker is indices_dev[q] ==
 * UINT64_MAX (what vkmr_hip_tree_find_async writes), out of range is any other index >= count.  Same scratch
 * (vkmr_hip_sort_entries_scratch_bytes(count, k)), launches and refusals (count above 2^58); count == 0 writes n = 0.
 * vkmr_host_cpu_tree_sort_entries is the CPU's.
 */
VKMR_API vkmr_status vkmr_hip_tree_sort_entries_async(int dev, vkmr_stream s, uint64_t count, const uint64_t* indices_dev,
                                                      uint32_t k, void* scratch_dev, uint64_t* indices_out_dev,
                                                      uint32_t* order_out_dev, uint64_t* info_dev);
/*
 * GATHER DIGESTS: dst_dev[j] = src_dev[order_dev[j]], j < n -- the payload of a sorted batch (new leaves, proved leaves)
 * brought into the order of the sorted entries, order_dev being the sort's order_out_dev and n its info_dev[0].  One launch
 * of n lanes on the caller's stream.  Every order_dev[j] must be a cell of src_dev (the sort's are < k); dst_dev must not
 * overlap src_dev.  n == 0 does nothing; a NULL pointer with n > 0 is refused on the host.
 */
VKMR_API vkmr_status vkmr_hip_gather_digests_async(int dev, vkmr_stream s, const vkmr_digest* src_dev, const uint32_t* order_dev,
                                                   uint32_t n, vkmr_digest* dst_dev);

/*
 * DIFF TWO STORED FORESTS ("which leaves differ?"; the reference has no counterpart): two replicas of one shape -- a node and
 * its snapshot, a primary and a follower, a state before and after a batch -- and the leaves in which they differ, found from
 * the roots down.  A (digests_a_dev, forest_a_dev, roots_a_dev) and B (digests_b_dev, forest_b_dev, roots_b_dev) are two
 * stored forests built by vkmr_hip_reduce_forest_tree_async (or its flagged twin), and kept by vkmr_hip_forest_update_async,
 * over the SAME offsets_dev, total, ntrees and max_count, both with status 0; the call TRUSTS this as
 * vkmr_hip_forest_proofs_async trusts its offsets.  The answer is every (t, i) with i < c_t whose leaf differs between A and B
 * on any of the 32 bytes, as strictly increasing pairs in cells [0, n) of trees_out_dev (uint32) and indices_out_dev (uint64)
 * -- exactly what vkmr_hip_forest_update_async and vkmr_hip_forest_multiproof_async take -- and, when leaves_b_out_dev is not
 * NULL, B's leaf at each of those positions in cells [0, n) of it: diff -> update of A with k = n makes A equal to B, diff ->
 * multiproof on B proves exactly what changed.  Cells of the leaves outside [offsets[0], offsets[ntrees]) are no leaves and are
 * never compared; cells of a level buffer that are no node of a tree ("STORED FOREST": unspecified) are never read.
 * The walk is a descent, never a scan of level 0.  Step 0 compares roots_a[t] with roots_b[t]; the frontier is the trees whose
 * roots differ, each as node 0 of its level h_t = max(1, ceil(log2 c_t)) (an empty tree never enters).  Steps 1..H, H the
 * forest's stride: an entry (t, p) at level l >= 1 compares the children 2p and 2p + 1 of p, nodes of tree t's level l - 1, in
 * both forests and emits each differing child, in child order; node 2p + 1 exists only below ceil(c_t / 2^(l - 1)), so the
 * duplicated last node of an odd level is no second child; an entry already at level 0 (a tree shorter than H) is carried
 * forward.  Emission keeps order, so the frontier is sorted by (t, p) at every step and after step H it is the answer: no
 * sort follows and the result does not depend on scheduling.  The work and the traffic are those of the changed paths (at
 * most 128 bytes per compared node), not of the forest.  Two facts the call relies on: in consistent forests a differing node
 * has a differing child, so the frontier never shrinks on the way down and is at most n at every step -- a frontier that
 * outgrows `capacity` at any step proves n > capacity, and the call stops there; and EQUAL NODES ARE TAKEN TO COVER EQUAL
 * LEAVES (anything else is a SHA-256d collision) -- both sides having the same counts, the duplicate-last ambiguity of
 * CVE-2012-2459 (two leaf lists of different length under one root) does not arise.
 *   capacity   cells of each output; 0 is legal, the outputs may then be NULL: identical forests give n = 0, anything else bit 2
 *   info_dev   4 uint64_t of device memory, always written when ntrees > 0:
 *     [0] status: 0 done; bit 2 (value 4): more than `capacity` leaves differ -- the outputs are then unspecified, nothing
 *         outside their `capacity` cells is touched, and [1] is the size of the frontier that overflowed, a lower bound of n
 *     [1] n
 *     [2] the trees whose roots differ
 *     [3] the nodes whose children were compared: for a completed call exactly the distinct ancestors (t, l, i >> l),
 *         1 <= l <= h_t, of the differing leaves -- the descent visited the changed paths and nothing else
 *   scratch_dev  vkmr_hip_diff_scratch_bytes(capacity) bytes of device memory, 16-byte aligned (layout: csrc/diff_plan.hpp:
 *                two ping-pong frontiers of 12 bytes an entry, two mask bits per entry, their ranking words, a header)
 * Cells [0, n) of the outputs hold the answer, cells at and behind n are unspecified; the outputs must not overlap the inputs
 * or the scratch.  n stays on the device: the caller reads info_dev back (32 bytes) before the update or multiproof that
 * takes it as k, as with vkmr_hip_forest_sort_entries_async.
 * Launches, all on the caller's stream: one memset; step 0 is a count of differing roots per workgroup, one ranking launch
 * and the emit; every later step the mask (one lane per frontier entry), the three ranking launches of
 * vkmr_hip_forest_multiproof_async with one level, and the emit -- the last one writes the outputs and info_dev.  The grids
 * are sized from min(capacity, the nodes that far below the roots), so the top steps launch a handful of lanes.  The launches
 * are a function of (total, ntrees, max_count, capacity) alone; no allocation, no host synchronisation, no host read of device
 * data; no kernel waits for another workgroup, and no entry is appended through a counter in memory.
 * ntrees == 0 does nothing.  Refused on the host (VKMR_ERR_INVALID) with ntrees > 0, before any HIP call: a NULL pointer that
 * is needed (the leaves when total > 0, both forests, both roots, the offsets, the scratch, info_dev, the two entry outputs
 * when capacity > 0), max_count == 0, total above 2^58, scratch_dev not 16-byte aligned.
 * Stream-ordered: a diff enqueued behind an update on the same stream sees the updated forest.
 */
VKMR_API size_t vkmr_hip_diff_scratch_bytes(uint32_t capacity);
VKMR_API vkmr_status vkmr_hip_forest_diff_async(int dev, vkmr_stream s, const vkmr_digest* digests_a_dev,
                                                const vkmr_digest* forest_a_dev, const vkmr_digest* roots_a_dev,
                                                const vkmr_digest* digests_b_dev, const vkmr_digest* forest_b_dev,
                                                const vkmr_digest* roots_b_dev, uint64_t total, const uint64_t* offsets_dev,
                                                uint32_t ntrees, uint64_t max_count, void* scratch_dev, uint32_t* trees_out_dev,
                                                uint64_t* indices_out_dev, vkmr_digest* leaves_b_out_dev, uint32_t capacity,
                                                uint64_t* info_dev);
/*
 * The same for two stored TREES (vkmr_hip_reduce_tree_async) of one `count` and `height`: the root is the last cell of the
 * tree buffer (the leaf itself for height 0), every entry is in tree 0 and indices_out_dev alone carries the answer; info_dev[2]
 * is 1 when the roots differ.  Same scratch, counters and launches (step 0 is one lane); H = height, which may be above the
 * count's own, as everywhere.  count == 0 does nothing.  Refused on the host: a NULL pointer that is needed (the tree buffers
 * only when height > 0), a height that does not reduce count to one node -- as vkmr_hip_tree_proofs_async refuses it --, count
 * above 2^58, scratch_dev not 16-byte aligned.
 */
VKMR_API vkmr_status vkmr_hip_tree_diff_async(int dev, vkmr_stream s, const vkmr_digest* digests_a_dev,
                                              const vkmr_digest* tree_a_dev, const vkmr_digest* digests_b_dev,
                                              const vkmr_digest* tree_b_dev, uint64_t count, uint32_t height, void* scratch_dev,
                                              uint64_t* indices_out_dev, vkmr_digest* leaves_b_out_dev, uint32_t capacity,
                                              uint64_t* info_dev);

/*
 * AUDIT A STORED FOREST IN PLACE ("which nodes are not the hash of their children?"; the reference has no counterpart): the
 * fsck of what vkmr_hip_reduce_forest_tree_async built and the update calls rewrote.  With S(0, i) leaf i of tree t, and S(l, j)
 * for 1 <= l <= h_t = max(1, ceil(log2 c_t)) the STORED cell of node j of tree t's level l -- roots_dev[t] for l == h_t, else
 * cell stored_level_base(l) + pos_l(t) + j of forest_dev -- node (t, l, j) is BAD when
 *     S(l, j) != hash_pair(S(l - 1, 2j), S(l - 1, right_child(j, n_{l-1}))),
 * the children as they are stored NOW, not as a rebuild would make them.  An empty tree has one checkable node, (t, 1, 0), bad
 * when roots_dev[t] is not all zero.  So one flipped inner cell gives two bad nodes (the cell and its parent), a flipped root or
 * leaf one, and an inner node replaced with every ancestor rehashed consistently exactly one.  No bad node <=> the levels and
 * roots are cell for cell what a rebuild from the current leaves would write (induction over the levels).  Cells of a level
 * buffer that are no node of a tree are never read and never reported.
 *   masks_dev      ntrees uint64_t: bit l - 1 of masks_dev[t] set when level l of tree t holds a bad node (mutated_dev's shape)
 *   bad_trees_dev, bad_levels_dev (uint32_t), bad_nodes_dev (uint64_t)   `capacity` cells each: the bad nodes in strictly
 *                  increasing (level, tree, node) order, the first `capacity` of them; nothing is written behind the list or
 *                  behind `capacity`
 *   capacity       0 is legal, the three lists and scratch_dev may then be NULL: masks and counters only, one launch per level
 *   info_dev       4 uint64_t of device memory, always written when ntrees > 0:
 *     [0] status: bits 0 and 1 are vkmr_hip_reduce_forest_async's (offsets decreasing or past `total`; a tree above max_count):
 *         nothing is audited, the masks are all zero and no entry is written; bit 2 (value 4): capacity > 0 and more than
 *         `capacity` nodes are bad -- the first `capacity` entries are there
 *     [1] the bad nodes, the true count also above `capacity`
 *     [2] the trees with a nonzero mask
 *     [3] the nodes checked: every node of levels 1 .. h_t of every tree, one for an empty tree
 *   scratch_dev    vkmr_hip_audit_scratch_bytes(total, ntrees, capacity) bytes of device memory, 16-byte aligned; 0 bytes for
 *                  capacity == 0 (layout: csrc/audit_plan.hpp -- one ballot word per wavefront of cells and its ranking words)
 * READ ONLY: the leaves, the levels, the roots and the offsets are byte for byte what they were.  The work is the build's: one
 * hash per node, 96 bytes read for the build's 64 read and 32 written, and no second copy of anything.
 * Launches, all on the caller's stream: the memsets, the offsets check, one launch per level 1 .. H with the build's grid; with
 * capacity > 0 the three ranking launches of vkmr_hip_forest_multiproof_async over all the levels' ballot words as one level,
 * then one emit launch per level.  They are a function of (total, ntrees, max_count, capacity) alone; no allocation, no host
 * synchronisation, no host read of device data; no kernel waits for another workgroup, and no entry is appended through a
 * counter in memory.  ntrees == 0 does nothing.  Refused on the host (VKMR_ERR_INVALID) with ntrees > 0, before any HIP call: a
 * NULL pointer that is needed (the leaves when total > 0, the forest, the roots, the offsets, the masks, info_dev; the scratch
 * and the three lists when capacity > 0), max_count == 0, total above 2^58, scratch_dev not 16-byte aligned, and with
 * capacity > 0 a level of more than 2^32 - 1 cells (the masks-only form has no such limit).
 * vkmr_host_cpu_forest_audit (libvkmr_host.so) applies the same rule on the CPU.
 */
VKMR_API size_t vkmr_hip_audit_scratch_bytes(uint64_t total, uint32_t ntrees, uint32_t capacity);
VKMR_API vkmr_status vkmr_hip_forest_audit_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev,
                                                 const vkmr_digest* forest_dev, const vkmr_digest* roots_dev, uint64_t total,
                                                 const uint64_t* offsets_dev, uint32_t ntrees, uint64_t max_count,
                                                 void* scratch_dev, uint64_t* masks_dev, uint32_t* bad_trees_dev,
                                                 uint32_t* bad_levels_dev, uint64_t* bad_nodes_dev, uint32_t capacity,
                                                 uint64_t* info_dev);
/*
 * The same for one stored TREE (vkmr_hip_reduce_tree_async): levels 1 .. height, the root inside tree_dev; a lone-node level
 * above ceil(log2 count) must be hash(a, a) of the node below.  Every entry is in tree 0: bad_levels_dev and bad_nodes_dev carry
 * the list, and info_dev[2] is the tree's own level mask.  scratch_dev: vkmr_hip_audit_scratch_bytes(count, 1, capacity).
 * count == 0 does nothing; height 0 (one leaf) has no node to check and leaves info_dev all zero.  Refused on the host: a NULL
 * pointer that is needed, a height that does not reduce count to one node, count above 2^58, scratch_dev not 16-byte aligned,
 * and with capacity > 0 a level of more than 2^32 - 1 cells.  vkmr_host_cpu_tree_audit is the CPU's.
 */
VKMR_API vkmr_status vkmr_hip_tree_audit_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev,
                                               const vkmr_digest* tree_dev, uint64_t count, uint32_t height, void* scratch_dev,
                                               uint32_t* bad_levels_dev, uint64_t* bad_nodes_dev, uint32_t capacity,
                                               uint64_t* info_dev);

/*
 * STORED FORESTS THAT GROW: trees appended into room reserved at the build, and the last trees dropped again.  Node j of tree
 * t's level l is cell (offsets[t] >> l) + t + j of that level's buffer: it depends on tree t's own offset and number alone, so
 * nothing behind tree t moves it.  A forest built (vkmr_hip_reduce_forest_tree_async) with empty trees at its end and with
 * offsets[ntrees] < total therefore has its level buffers laid out for its CAPACITY -- `total` leaves, `ntrees` trees, none
 * above max_count -- and appending is filling the next empty trees: the work is that of the new trees alone, every earlier
 * cell stays where it is, and the grown forest is byte for byte one the build could have written, which every call above takes.
 *   total, ntrees, max_count   those of the build (the capacity), TRUSTED as vkmr_hip_forest_update_async trusts them
 *   first_tree, used           trees first_tree .. ntrees - 1 are empty and used == offsets[first_tree] == .. == offsets[ntrees];
 *                              host values, so that every grid is sized without reading device memory; checked on the device
 *   new_offsets_dev            m + 1 uint64_t in device memory, relative to `used`: new_offsets[0] == 0, none decreasing,
 *                              new_offsets[m] == n_leaves; new tree j holds leaves [new_offsets[j], new_offsets[j + 1])
 *   leaves_dev                 the n_leaves new leaves in device memory; leaves_dev == digests_dev + used says that they are in
 *                              place already (vkmr_hip_map_async writes at an output offset) and no copy is launched
 *   mutated_dev                NULL, or the ntrees masks of the flagged builds: those of the m new trees are zeroed and formed in
 *                              the same launches (each level compares the two children it loads); no other mask is touched
 *   status_dev                 one uint32_t in device memory, always written: 0 when the trees were appended; bit 0 set if the
 *                              new offsets decrease, do not start at 0 or do not end at n_leaves; bit 1 if a new count is above
 *                              max_count; bit 2 (value 4) if some offsets[t] != used for first_tree <= t <= ntrees.  When it is
 *                              nonzero NOTHING of the caller's has changed: no leaf cell (but those the caller put in place
 *                              itself), no offset, no cell of forest_dev, no root, no mask.
 * After status 0 the leaves lie at cells [used, used + n_leaves), offsets[first_tree + j] = used + new_offsets[j] for
 * 1 <= j <= m, every later offset up to offsets[ntrees] is used + n_leaves, and the levels and roots of trees first_tree ..
 * first_tree + m - 1 are written: every cell of the leaves, forest_dev, roots_dev and offsets_dev equals what a fresh
 * vkmr_hip_reduce_forest_tree_async over the resulting offsets writes; cells a build never writes are not written here either.
 * Launches, all on the caller's stream: the status word zeroed, one check (the new offsets and the placement), the leaves unless
 * in place, the offsets (which zeroes the new trees' masks too), then one launch per level, H = max(1, ceil(log2 min(max_count,
 * total))) of them, level l over the cells [pos_l(used, first_tree), pos_l(used + n_leaves, first_tree + m)) alone, never a
 * level's whole buffer; no launch per tree, no allocation, no host read of device data.  Refused on the host (VKMR_ERR_INVALID)
 * with m > 0, before any HIP call: a NULL pointer (leaves_dev may be NULL when n_leaves == 0, mutated_dev always),
 * first_tree + m > ntrees, used + n_leaves > total, max_count == 0, total > 2^58.  m == 0 does nothing whatever the other
 * arguments.  Stream-ordered: a proof gather enqueued after it on the same stream sees the new trees.
 */
VKMR_API vkmr_status vkmr_hip_forest_append_async(int dev, vkmr_stream s, vkmr_digest* digests_dev, vkmr_digest* forest_dev,
                                                  uint64_t total, uint64_t* offsets_dev, uint32_t ntrees, uint64_t max_count,
                                                  uint32_t first_tree, uint64_t used, const vkmr_digest* leaves_dev,
                                                  uint64_t n_leaves, const uint64_t* new_offsets_dev, uint32_t m,
                                                  vkmr_digest* roots_dev, uint64_t* mutated_dev, uint32_t* status_dev);
/*
 * The inverse, for a reorganisation (drop the last trees, then append others): for keep_trees <= t < ntrees,
 * offsets[t + 1] = offsets[keep_trees] and roots_dev[t] all zero -- one launch, no hash.  The cells of the level buffers are left
 * as they are: they belong to no tree any more and nothing reads them.  Afterwards the forest is what a build over the shortened
 * offsets writes, in every cell such a build writes.  keep_trees == ntrees does nothing; keep_trees > ntrees, or a NULL pointer
 * with keep_trees < ntrees, is refused on the host.
 */
VKMR_API vkmr_status vkmr_hip_forest_truncate_async(int dev, vkmr_stream s, uint64_t* offsets_dev, uint32_t ntrees,
                                                    uint32_t keep_trees, vkmr_digest* roots_dev);
/*
 * The same at the other end, for a window that loses its oldest trees: for t < drop_trees, offsets[t] = offsets[drop_trees],
 * roots_dev[t] all zero and, with mutated_dev (the ntrees masks, or NULL), mutated_dev[t] = 0 -- one launch, one lane per
 * dropped tree, no hash; offsets[drop_trees] is read and never written.  Trees 0 .. drop_trees - 1 are then empty trees at the
 * offset where tree drop_trees begins: pos_l stays strictly increasing (neighbouring dropped trees are one cell apart), every
 * tree from drop_trees on keeps its offset and its NUMBER and so every cell of its own, and the forest is what a build over the
 * new offsets writes (offsets[0] > 0 is a forest every call above takes), in every cell such a build writes.  The leaves and
 * level cells in front belong to no tree any more; offsets do not decrease, so they cannot be used again in place --
 * vkmr_hip_forest_copy_trees_async into another forest reclaims them.  drop_trees == 0 does nothing; drop_trees > ntrees, or a
 * NULL offsets_dev or roots_dev with drop_trees > 0, is refused on the host before any HIP call.  Stream-ordered.
 */
VKMR_API vkmr_status vkmr_hip_forest_drop_front_async(int dev, vkmr_stream s, uint64_t* offsets_dev, uint32_t ntrees,
                                                      uint32_t drop_trees, vkmr_digest* roots_dev, uint64_t* mutated_dev);

/*
 * STORED TREES COPIED INTO ANOTHER FOREST: repack a forest whose reserve is used up or whose front was dropped, delete trees from
 * the middle, merge two forests, split one -- without hashing.  A stored tree at another offset, under another number or in
 * another forest has the same nodes; only their cells differ, and differently per level, because (offset >> l) does not commute
 * with a shift of the offset.  So the call is vkmr_hip_forest_append_async with "hash the two children" replaced by "copy the
 * node": 32 bytes read and 32 written per cell.
 *   src_*                      a stored forest (vkmr_hip_reduce_forest_tree_async, grown or not), TRUSTED as every reader trusts
 *                              it: src_digests_dev its leaves, src_forest_dev its levels, src_total / src_ntrees / src_max_count
 *                              its capacity, src_offsets_dev its src_ntrees + 1 offsets, src_roots_dev its roots;
 *                              src_mutated_dev NULL or its src_ntrees masks
 *   sel_dev                    m uint32_t in device memory: destination tree first_tree + j becomes source tree sel[j]; any
 *                              order, repeats and empty trees allowed
 *   n_leaves, new_offsets_dev  as append's (m + 1 uint64_t relative to `used`, from 0 to n_leaves): host values and their
 *                              prefix sums, which the host forms from the counts it knows; checked on the device against the
 *                              source's own offsets
 *   dst_*, first_tree, used    append's arguments: the destination's leaves, levels, capacity, offsets and roots; trees
 *                              first_tree .. dst_ntrees - 1 are empty at `used`.  dst_mutated_dev NULL or its dst_ntrees masks:
 *                              those of the m new trees are copied from src_mutated_dev, or zeroed when that is NULL
 *   status_dev                 one uint32_t in device memory, always written: 0 when the trees were copied; append's bits --
 *                              bit 0: the new offsets decrease, do not start at 0 or do not end at n_leaves; bit 1: a count
 *                              above dst_max_count; bit 2 (value 4): some dst offsets[t] != used for first_tree <= t <=
 *                              dst_ntrees -- and bit 3 (value 8): some sel[j] >= src_ntrees, or new count j is not the count of
 *                              source tree sel[j].  An unchecked sel[j] is never followed into the source's offsets.  When it
 *                              is nonzero NOTHING of the destination has changed.
 * After status 0 every cell of the destination's leaves, dst_forest_dev, dst_roots_dev and dst_offsets_dev that a fresh
 * vkmr_hip_reduce_forest_tree_async over the resulting offsets writes holds what that build writes, and no other cell is
 * written (a tree's last level is kept in the roots alone, here as there).  Launches, all on the caller's stream: the status
 * word zeroed, one check, the offsets (append's own kernel, which zeroes the new trees' masks too), then one launch per level
 * l = 0 .. H_d = max(1, ceil(log2 min(dst_max_count, dst_total))), level 0 being the leaves, each over the cells
 * [pos_l(used, first_tree), pos_l(used + n_leaves, first_tree + m)) alone, one lane per destination cell; no launch per tree, no
 * allocation, no host read of device data, no hash.  Refused on the host (VKMR_ERR_INVALID) with m > 0, before any HIP call: a
 * NULL pointer (the two mask arrays may be NULL, the two leaves buffers when n_leaves == 0), first_tree + m > dst_ntrees,
 * used + n_leaves > dst_total, either max_count == 0, either total > 2^58, and dst_digests_dev == src_digests_dev, dst_forest_dev == src_forest_dev, dst_offsets_dev ==
 * src_offsets_dev or dst_roots_dev == src_roots_dev: a copy inside one forest is not offered.  Buffers that overlap in part
 * are the caller's business: the call does not look for them, and the result is then undefined.  m == 0 does nothing whatever
 * the other arguments.  Stream-ordered: a proof gather enqueued after it on the same stream sees the copied trees.
 */
VKMR_API vkmr_status vkmr_hip_forest_copy_trees_async(int dev, vkmr_stream s, const vkmr_digest* src_digests_dev,
                                                      const vkmr_digest* src_forest_dev, uint64_t src_total,
                                                      const uint64_t* src_offsets_dev, uint32_t src_ntrees, uint64_t src_max_count,
                                                      const vkmr_digest* src_roots_dev, const uint64_t* src_mutated_dev,
                                                      const uint32_t* sel_dev, uint32_t m, uint64_t n_leaves,
                                                      const uint64_t* new_offsets_dev, vkmr_digest* dst_digests_dev,
                                                      vkmr_digest* dst_forest_dev, uint64_t dst_total, uint64_t* dst_offsets_dev,
                                                      uint32_t dst_ntrees, uint64_t dst_max_count, uint32_t first_tree, uint64_t used,
                                                      vkmr_digest* dst_roots_dev, uint64_t* dst_mutated_dev, uint32_t* status_dev);

/*
 * THE OPEN TREE GROWS OR SHRINKS BY LEAVES, at its right edge: a block still collecting transactions, the newest file of an
 * index, a log kept as one tree (a forest of one tree built with a reserve).  The open tree is the last tree in use: every
 * tree behind it is empty.  Its cells do not move -- node j of its level l is cell (offsets[tree] >> l) + tree + j whatever its
 * count -- so taking n more leaves, or dropping the last r, rehashes only the nodes whose value changes: those from
 * min(count, new count) >> l on at level l, at most (n >> l) + 2 of them; where the old or the new tree has a single node at
 * level l the range starts at node 0, because the build keeps a tree's last level in roots_dev alone (growing 2 -> 3 must form
 * a cell never stored; shrinking 3 -> 2 must carry an inner cell to roots_dev).
 *   total, ntrees, max_count   those of the build (the capacity), TRUSTED as vkmr_hip_forest_update_async trusts them, and
 *                              with them the offsets of the trees in front of `tree`, which the build checked
 *   tree, count, used          the open tree, its leaves now, the leaves in use: offsets[tree] + count == used ==
 *                              offsets[tree + 1] == .. == offsets[ntrees]; host values, so that every grid is sized without
 *                              reading device memory; checked on the device
 *   leaves_dev                 (extend) the n_leaves new leaves in device memory; leaves_dev == digests_dev + used says that they
 *                              are in place already (vkmr_hip_map_async writes at an output offset) and no copy is launched
 *   r                          (shrink) the leaves dropped from the end; their cells are free again and are not written
 *   mutated_dev                NULL, or the ntrees masks of the flagged builds: the open tree's is zeroed and formed again
 *                              from the whole tree (a compare without a hash behind each level: an old right-edge pair may have
 *                              set a bit that must clear, so the edge alone cannot say); no other mask is touched
 *   status_dev                 one uint32_t in device memory, always written, in vkmr_hip_forest_append_async's numbering:
 *                              0 when done; bit 2 (value 4) if offsets[tree] + count != used or some offsets[t] != used for
 *                              tree < t <= ntrees.  When it is nonzero NOTHING of the caller's has changed: no leaf cell (but
 *                              those the caller put in place itself), no offset, no cell of forest_dev, no root, no mask.
 * After status 0 offsets[t + 1] is offsets[tree] + the new count for every t >= tree, and every cell of the leaves, forest_dev,
 * roots_dev and offsets_dev that a fresh vkmr_hip_reduce_forest_tree_async over those offsets writes holds what it writes (a
 * tree shrunk to no leaf: the zero root).  Cells such a build does not write -- those of dropped nodes -- keep what they held.
 * Launches, all on the caller's stream: the status word zeroed, one check, the leaves unless in place (extend), the offsets
 * (which zeroes the mask too), then at most one launch per level, H = max(1, ceil(log2 min(max_count, total))) of them, level
 * l over the dirty nodes alone, never a level's whole buffer, and none where there is no dirty node (and with mutated_dev the
 * compare behind it, over the one tree); no launch per node, no allocation, no host read of device data.  Refused on the host
 * (VKMR_ERR_INVALID), before any HIP call: a NULL pointer (mutated_dev may always be NULL), tree >= ntrees, count + n_leaves
 * > max_count, used + n_leaves > total, r > count, count > used, used > total, max_count == 0, total > 2^58.  n_leaves == 0 or
 * r == 0 does nothing whatever the other arguments.  Stream-ordered: a proof gather enqueued after it on the same stream sees
 * the new leaves.  The host advances its own count and used by n_leaves, or takes r from both.
 */
VKMR_API vkmr_status vkmr_hip_forest_extend_async(int dev, vkmr_stream s, vkmr_digest* digests_dev, vkmr_digest* forest_dev,
                                                  uint64_t total, uint64_t* offsets_dev, uint32_t ntrees, uint64_t max_count,
                                                  uint32_t tree, uint64_t count, uint64_t used, const vkmr_digest* leaves_dev,
                                                  uint64_t n_leaves, vkmr_digest* roots_dev, uint64_t* mutated_dev, uint32_t* status_dev);
VKMR_API vkmr_status vkmr_hip_forest_shrink_async(int dev, vkmr_stream s, vkmr_digest* digests_dev, vkmr_digest* forest_dev,
                                                  uint64_t total, uint64_t* offsets_dev, uint32_t ntrees, uint64_t max_count,
                                                  uint32_t tree, uint64_t count, uint64_t used, uint64_t r, vkmr_digest* roots_dev,
                                                  uint64_t* mutated_dev, uint32_t* status_dev);

/*
 * FRONTIERS: A HOLDER OF THE ROOTS ALONE FOLLOWS TREES THAT GROW.  vkmr_hip_apply_forest_multiproof_async lets a follower keep up
 * with leaf updates; the calls above let the primary's trees grow.  A follower of a growing tree needs no witness at all: a
 * duplicate-last tree of c leaves is determined, for every future extension, by its FRONTIER -- the count c and one PEAK per
 * set bit l of c, node (c >> l) - 1 of level l, the root of a complete subtree of 2^l leaves that no later leaf changes.  A
 * frontier is `stride` digests per tree (1 <= stride <= 64), cell l for bit l of the count; the cell of a clear bit is never
 * read and always written as zero, so that two frontiers of equal trees compare byte for byte.  c == 0 is a tree not yet
 * begun (every cell zero): appending a tree and extending the open tree are the same call.
 *   counts_dev, peaks_dev      T counts (uint64_t) and T x stride digests in device memory
 * ROOT OF A FRONTIER.  c == 0: the all-zero root.  Else, with no carry to begin with, for l = 0 .. H(c) - 1,
 * H(c) = max(1, ceil(log2 c)): where bit l of c is set carry = node_hash(P_l, carry if there is one, else P_l); else where
 * there is a carry carry = node_hash(carry, carry).  The root is the carry, or P_H(c) when there is none (c a power of two, at
 * least 2).  A tree of one leaf: node_hash(leaf, leaf), as everywhere in this library.
 *
 * vkmr_hip_forest_frontier_async: the frontiers of every tree of a stored forest, as vkmr_hip_forest_proofs_async takes it
 * (digests_dev, forest_dev, total, offsets_dev, ntrees, max_count: those of the build, trusted in the same way) with its
 * roots_dev, which holds the peak of a tree whose count is a power of two.  counts_out_dev[t] and the stride cells of
 * peaks_out_dev behind t * stride are written for every tree; one launch, a lane per cell, no hash.  Refused: a NULL pointer,
 * what vkmr_hip_forest_proofs_async refuses of the forest, stride outside 1..64, and a stride below the bits of
 * min(max_count, total) (a tree the build allows would lose a peak).  ntrees == 0 does nothing.
 *
 * vkmr_hip_frontier_roots_async: roots_out_dev[q] = the root of frontier q by the rule above, T of them, one launch, a lane
 * per tree and at most 63 node hashes in it.  A count above 2^58 or of more bits than stride reads no peak and gives the zero
 * root.  vkmr_hip_verify_frontier_async: the same walk compared with roots_dev[q]: ok_dev[q] (uint32_t) = 1 when equal, else 0
 * (0 for such a count).  This is how a follower ADOPTS a frontier it is sent under roots it already trusts: a peak or a
 * count that was changed gives another root.  The roots authenticate the frontier as far as SHA-256d binds a root to its
 * tree; nothing else is checked.  Refused: a NULL pointer, stride outside 1..64.  T == 0 does nothing.
 *
 * vkmr_hip_frontier_extend_async: T frontiers each take new leaves; the new roots and the new frontiers come out.
 *   leaves_dev, total_new      the new leaves of all trees back to back, in device memory (may be NULL when total_new == 0)
 *   offsets_dev                T + 1 offsets into them: tree q takes n_q = offsets[q+1] - offsets[q] leaves; in device memory
 *                              and CHECKED there (below).  n_q == 0: the tree keeps its frontier and still gets its root
 *   max_new                    the caller's bound on n_q, checked
 *   scratch_dev                vkmr_hip_frontier_extend_scratch_bytes(total_new, T) bytes, 16-byte aligned: two level buffers of
 *                              (total_new >> 1) + 2 T digests and 64 T staging cells
 *   new_counts_dev, new_peaks_dev   T counts and T x stride digests; MAY BE counts_dev and peaks_dev: the frontiers then
 *                              advance in place.  Cells of clear bits are written as zero
 *   roots_dev                  T digests: the root of every tree after the call (zero for a tree still without a leaf)
 *   status_dev                 one uint32_t, always written: 0 when done; bit 0 (1) offsets that decrease, offsets[0] != 0 or
 *                              offsets[T] != total_new; bit 1 (2) n_q > max_new; bit 2 (4) a new count above 2^58; bit 3 (8) a
 *                              new count of more bits than stride.  When it is nonzero NOTHING of the caller's is written:
 *                              no count, no peak, no root (scratch is).
 * Level l >= 1 forms, of tree q going from c to c2 = c + n_q leaves, the nodes c >> l .. ceil(c2 / 2^l) - 1, at most
 * (n_q >> l) + 2 of them, from the nodes the level below formed (the new leaves for l == 1) and ONE old value, the peak
 * P_(l-1) where bit l - 1 of c is set; no other cell of the frontier is read and no stored level exists.  Launches, all on the
 * caller's stream: the status word zeroed, one check, one launch per level for ALL trees, min(stride, 58) of them (level l:
 * (total_new >> l) + 2 T lanes), and one commit that writes the counts and the peaks behind the last level; never a launch
 * per tree, no allocation, no host read of device data.  Refused on the host (VKMR_ERR_INVALID), before any HIP call: a NULL
 * pointer, stride outside 1..64, total_new above 2^58, scratch off the 16-byte grid, more cells than a launch takes.
 * T == 0 does nothing.  vkmr_host_cpu_frontier_roots, vkmr_host_cpu_frontier_extend and vkmr_host_cpu_forest_frontier
 * (libvkmr_host.so) apply the same rules on the CPU, for a follower without a GPU.  Not offered: shrinking a frontier (the
 * dropped peaks are gone; the primary must send them).
 */
VKMR_API vkmr_status vkmr_hip_forest_frontier_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev, const vkmr_digest* forest_dev,
                                                    uint64_t total, const uint64_t* offsets_dev, uint32_t ntrees, uint64_t max_count,
                                                    const vkmr_digest* roots_dev, uint32_t stride, uint64_t* counts_out_dev,
                                                    vkmr_digest* peaks_out_dev);
VKMR_API vkmr_status vkmr_hip_frontier_roots_async(int dev, vkmr_stream s, const uint64_t* counts_dev, const vkmr_digest* peaks_dev,
                                                   uint32_t stride, uint32_t T, vkmr_digest* roots_out_dev);
VKMR_API vkmr_status vkmr_hip_verify_frontier_async(int dev, vkmr_stream s, const uint64_t* counts_dev, const vkmr_digest* peaks_dev,
                                                    uint32_t stride, uint32_t T, const vkmr_digest* roots_dev, uint32_t* ok_dev);
VKMR_API size_t vkmr_hip_frontier_extend_scratch_bytes(uint64_t total_new, uint32_t T);
VKMR_API vkmr_status vkmr_hip_frontier_extend_async(int dev, vkmr_stream s, const uint64_t* counts_dev, const vkmr_digest* peaks_dev,
                                                    uint32_t stride, uint32_t T, const vkmr_digest* leaves_dev, uint64_t total_new,
                                                    const uint64_t* offsets_dev, uint64_t max_new, void* scratch_dev,
                                                    uint64_t* new_counts_dev, vkmr_digest* new_peaks_dev, vkmr_digest* roots_dev,
                                                    uint32_t* status_dev);

/*
 * CONSISTENCY PROOFS: A HOLDER OF TWO ROOTS CHECKS THAT A TREE ONLY GREW.  A monitor, a light client or an auditor of a log
 * holds the root a tree had at c leaves, is handed the root it has at c2 >= c leaves, and must decide whether the first c leaves
 * are still the ones it trusted -- without the c2 - c leaves between.  The proof is two rows of `stride` digests (1 <= stride
 * <= 64), read from the stored levels of the NEW tree without a hash.  With l0 the lowest set bit of c >= 1 and the notation of
 * the block above:
 *   peaks    cell l = P_l of the OLD count for every set bit l of c (a complete node never changes): a frontier of count c
 *   rights   for l0 <= l < H(c2) the walk from P_l0 to the new root stands on node j = (c >> l0) - 1 of level l0 and on
 *            j = c >> l above it.  Where l == l0 or bit l of c is clear j is a left child, and cell l holds node j + 1 of the
 *            new tree's level l when that node exists (j + 1 < ceil(c2 / 2^l)); where bit l of c is set above l0, j is a right
 *            child whose left sibling is P_l, so no cell is needed
 * Every other cell of both rows is zero and is never read, so that two proofs of one claim compare byte for byte.
 * THE CHECK.  The root of the frontier (c, peaks), by the rule above, must be the old root.  Then acc = P_l0 and for
 * l = l0 .. H(c2) - 1: a left child gives acc = node_hash(acc, rights[l] if node j + 1 exists, else acc), a right child
 * acc = node_hash(P_l, acc); acc must be the new root.  Both must hold: the SAME peaks serve both walks, which is what binds
 * the old tree into the new one.  c == c2 runs through the same rule.  c == 0: ok exactly when the old root is all zero (any
 * tree extends one not yet begun), nothing else is read.  ok = 0 without reading a cell: c > c2, c2 > 2^58, c2 of more bits
 * than stride.  At most H(c) + H(c2) node hashes a query.
 *
 * vkmr_hip_forest_consistency_async: the proofs of Q queries out of a stored forest, taken as vkmr_hip_forest_frontier_async
 * takes it (digests_dev .. max_count: those of the build, trusted in the same way; roots_dev holds every level of a single node).
 *   trees_dev, old_counts_dev  Q queries (tree, old count) in device memory, CHECKED there; a tree in any order and as often as
 *                              wanted: a log serves many followers at different counts
 *   new_counts_out_dev         Q counts: the count the tree of query q has now
 *   peaks_out_dev, rights_out_dev   Q x stride digests each; EVERY cell is written, zeros included
 *   status_dev                 one uint32_t, always written: 0 when done; bit 0 (1) a tree index >= ntrees; bit 1 (2) an old
 *                              count above the tree's count (so a tree dropped from the front, count 0, proves nothing but
 *                              c == 0, and a tree that shrank below c is refused); bit 2 (4) a current count of more bits than
 *                              stride.  When it is nonzero NOTHING of the caller's is written: no count, no cell.
 * Level 0 is the leaves; level l >= 1 of two nodes at least is cell (offsets[t] >> l) + t + node of stored level l; a level of a
 * single node is roots_dev[t] (only the seed P_l0 when c == c2 == 2^l0 lies there).  Launches, all on the caller's stream: the
 * status word zeroed, one check (a lane per query), one gather (a lane per (query, cell), at most two loads, no hash); never a
 * launch per tree or per query, no allocation, no host read of device data.  Refused on the host (VKMR_ERR_INVALID), before
 * any HIP call: a NULL pointer, and what vkmr_hip_forest_frontier_async refuses.  Q == 0 does nothing.
 *
 * vkmr_hip_verify_consistency_async: the check above, a lane per query in one launch; ok_dev[q] (uint32_t) = 1 when proof q
 * (old_counts_dev[q], new_counts_dev[q], the stride cells of peaks_dev and rights_dev behind q * stride) holds under
 * old_roots_dev[q] and new_roots_dev[q], else 0.  No stored level, no scratch: what a monitor runs.  The roots are per query;
 * the caller indexes its own tables by tree.  Refused: a NULL pointer, stride outside 1..64.  Q == 0 does nothing.
 * The peaks row with the old counts IS a frontier: vkmr_hip_frontier_roots_async over it names every tree's root as of its old
 * count again, and a follower that fell behind adopts it under the old root it trusts and goes on with
 * vkmr_hip_frontier_extend_async.  vkmr_host_cpu_forest_consistency and vkmr_host_cpu_verify_consistency (libvkmr_host.so)
 * apply the same rules on the CPU.  Inclusion proofs as of an earlier count: vkmr_hip_forest_proofs_at_async, below.
 */
VKMR_API vkmr_status vkmr_hip_forest_consistency_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev, const vkmr_digest* forest_dev,
                                                       uint64_t total, const uint64_t* offsets_dev, uint32_t ntrees, uint64_t max_count,
                                                       const vkmr_digest* roots_dev, const uint32_t* trees_dev, const uint64_t* old_counts_dev,
                                                       uint32_t Q, uint32_t stride, uint64_t* new_counts_out_dev, vkmr_digest* peaks_out_dev,
                                                       vkmr_digest* rights_out_dev, uint32_t* status_dev);
VKMR_API vkmr_status vkmr_hip_verify_consistency_async(int dev, vkmr_stream s, const uint64_t* old_counts_dev, const uint64_t* new_counts_dev,
                                                       const vkmr_digest* peaks_dev, const vkmr_digest* rights_dev, uint32_t stride, uint32_t Q,
                                                       const vkmr_digest* old_roots_dev, const vkmr_digest* new_roots_dev, uint32_t* ok_dev);

/*
 * INCLUSION PROOFS AS OF AN EARLIER COUNT: "LEAF i WAS IN THE TREE I TRUSTED".  The other half of the append-only pair for a log
 * that serves checkpoints: a client holds the root tree t had at c leaves and asks for the proof of leaf i < c under THAT root,
 * while the tree has grown to c2 >= c leaves.  An EPOCH is (tree, old count); a log serves many queries at few epochs.  With the
 * notation of the two blocks above, l0 the lowest set bit of c >= 1:
 *   a node s of level l of the old tree with (s + 1) << l <= c is COMPLETE: no later leaf changes it, so it is node s of level l
 *   of the new tree -- a leaf, cell (offsets[t] >> l) + t + s of stored level l, or roots_dev[t] where the level has one node;
 *   a level l0 < l <= H(c) of the old tree has one other node, its last: E_l = node_hash(P_(l-1), E_(l-1)) where bit l - 1 of c
 *   is set (E_(l-1) replaced by P_(l-1) itself for l - 1 == l0), else node_hash(E_(l-1), E_(l-1)) -- the carry of the frontier's
 *   root walk, the peaks P_l read from the new tree as the consistency gather reads them;
 *   the old root is E_H(c); for c a power of two of at least 2 it is node 0 of level H(c) of the new tree, without a hash; for
 *   c == 1 it is node_hash(leaf, leaf).  H(c) - l0 node hashes an epoch (none for a power of two), NONE per query.
 * The proof of leaf i < c has H(c) cells: cell l is node s = j ^ 1 of the old tree's level l for j = i >> l, or j itself where
 * j ^ 1 >= ceil(c / 2^l) -- the stored node when complete, else E_l.
 *
 * vkmr_hip_forest_proofs_at_async: the stored forest as vkmr_hip_forest_consistency_async takes it (digests_dev .. roots_dev).
 *   epoch_trees_dev, epoch_counts_dev   E epochs (uint32 tree, uint64 old count) in device memory, CHECKED there
 *   epochs_dev, indices_dev    k queries: leaf indices_dev[q] (uint64) as of epoch epochs_dev[q] (uint32)
 *   edges_out_dev              E x stride digests: cell l of epoch e is E_l for l0 < l < H(c) when the epoch hashes, every other
 *                              cell zero; EVERY cell is written
 *   old_roots_out_dev          E digests: the root of epoch e's tree as of its count; all zero for c == 0
 *   siblings_dev, heights_dev  k x stride digests and k uint32: heights_dev[q] = H(c), cells l < H(c) as above, cells above zero.
 *                              A query with epochs_dev[q] >= E or indices_dev[q] >= c -- every query into an epoch of c == 0 --
 *                              gets height 0 and zero cells: vkmr_hip_forest_proofs_async's rule for a bad index, not a status bit
 *   status_dev                 one uint32_t, always written: 0 when done, else the bits of vkmr_hip_forest_consistency_async
 *                              over the epochs: bit 0 (1) a tree index >= ntrees; bit 1 (2) an old count above the tree's count
 *                              now; bit 2 (4) a current count of more bits than stride.  When it is nonzero NOTHING of the
 *                              caller's is written: no edge, no root, no proof, no height.
 * VERIFYING.  There is no new verifier: the output is exactly what vkmr_hip_verify_forest_proofs_async takes with
 * trees_dev := epochs_dev, roots_dev := old_roots_out_dev (or the roots the client trusts, in the order of the epochs) and
 * ntrees := E; on the CPU every proof folds with vkmr_host_cpu_fold_proof.
 * Launches, all on the caller's stream: the status word zeroed, one check (a lane per epoch), one edge launch (a lane per epoch,
 * the hashes of its right edge through one node hash), one gather (a lane per (query, level): one load, from the stored forest
 * or from the edge row, and one store; no hash); never a launch per tree, epoch or query, no allocation, no scratch to size, no
 * host read of device data.  Refused on the host (VKMR_ERR_INVALID), before any HIP call: a NULL pointer (the four query buffers
 * may be NULL when k == 0), stride outside 1..63 (the verifier's range), and what vkmr_hip_forest_consistency_async refuses of
 * the forest.  E == 0 does nothing.  k == 0 with E > 0 is valid: the edges and the old roots alone, "the root of tree t as of
 * count c".  vkmr_host_cpu_forest_proofs_at (libvkmr_host.so) applies the same rules on the CPU.  Not offered: multiproofs as of
 * an earlier count.
 */
VKMR_API vkmr_status vkmr_hip_forest_proofs_at_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev, const vkmr_digest* forest_dev,
                                                     uint64_t total, const uint64_t* offsets_dev, uint32_t ntrees, uint64_t max_count,
                                                     const vkmr_digest* roots_dev, const uint32_t* epoch_trees_dev, const uint64_t* epoch_counts_dev,
                                                     uint32_t E, const uint32_t* epochs_dev, const uint64_t* indices_dev, uint32_t k, uint32_t stride,
                                                     vkmr_digest* edges_out_dev, vkmr_digest* old_roots_out_dev, vkmr_digest* siblings_dev,
                                                     uint32_t* heights_dev, uint32_t* status_dev);

/*
 * PARTIAL MERKLE TREES IN BIP37 ORDER: the form Bitcoin software reads for "these transactions are in this block" -- the partial
 * Merkle tree of a `merkleblock` message, Bitcoin Core's CPartialMerkleTree -- ONE per named tree of a stored forest, built on the
 * device in one call: a wallet rescan or a filter match over many blocks.  digests_dev, forest_dev, total, offsets_dev, ntrees,
 * max_count and the k entries (trees_dev[q], indices_dev[q]) are those of vkmr_hip_forest_multiproof_async: device memory, the
 * pairs strictly increasing, tree < ntrees, index < c_t, checked on the device into the same status bits 0 and 1.
 * THE RULE, for a tree of c >= 1 leaves: h = max(1, ceil(log2 c)), w(l) = ceil(c / 2^l) the nodes of level l, A_0 the tree's
 * matched indices, A_{l+1} = unique(A_l >> 1).  visit(h, 0) starts the walk; visit(l, p) appends the flag f = (p in A_l); if
 * l == 0 or !f it appends the hash of stored node (l, p); otherwise visit(l - 1, 2p), then visit(l - 1, 2p + 1) only if
 * 2p + 1 < w(l - 1).  Flag number i is bit i & 7 of byte i >> 3; padding bits are 0.  For c >= 2 the flags and hashes are byte
 * for byte what Bitcoin Core's TraverseAndBuild writes.  THE LONE LEAF: for c == 1 the rule gives two flags and one hash, and the
 * root is hash_pair(leaf, leaf); Bitcoin has one flag and the txid as the root.  It is not special-cased: this engine's root of
 * such a tree is not Bitcoin's anyway.  Against the multiproof: the matched leaves themselves are carried, and nothing is where
 * the multiproof puts a node in as its own sibling (the duplicate-last edge): hashes = k_t + the tree's multiproof nodes - those
 * emitted at such an edge.
 * Outputs, B the number of distinct trees named, b over them in ascending order (the per-block arrays have room for k entries,
 * the two starts for k + 1):
 *   block_trees_dev[b]   uint32: the tree of block b          block_counts_dev[b]  uint64: c_t
 *   bit_counts_dev[b]    uint64: the flags of block b
 *   hash_starts_dev[b]   uint64: the first hash of block b in hashes_dev; [B] their number
 *   byte_starts_dev[b]   uint64: the first flag byte of block b in flags_dev (every block starts on a byte); [B] their number
 *   hashes_dev           hash_capacity vkmr_digest cells, tree-major, each block in the visit order above
 *   flags_dev            flag_capacity bytes, 4-byte aligned; every byte in [0, byte_starts_dev[B]) is written whole
 *   info_dev             4 uint64: [0] status, [1] B, [2] the hashes, [3] the flag bytes
 * Status: bits 0 and 1 as above -- then nothing else of the caller's is written; bit 2 when the hashes exceed hash_capacity or the
 * flag bytes flag_capacity -- then the per-block arrays and info_dev are written and valid, no hash and no flag is, and the caller
 * can allocate and call again.  Nothing behind the used hashes and bytes is touched.  vkmr_hip_forest_merkleblocks_max_hashes
 * (<= k + vkmr_hip_forest_multiproof_max_nodes) and _max_flag_bytes (per tree flags <= 2 * hashes + h, a byte of padding a
 * block) bound them from the forest's shape; scratch_dev is vkmr_hip_forest_merkleblocks_scratch_bytes(k, H) bytes, 16-byte
 * aligned, H the forest's stride (the tree's height for the twin).
 * No walk on the device: what the walk appends between one matched leaf and the next is a closed form of the two indices
 * (csrc/merkleblock_plan.hpp), so a prefix sum over the entries places everything.  Launches, all on the caller's stream: the
 * status zeroed, the check, then nine kernels whatever k, B and H are (sums, starts, places; byte sums, starts, places; the flag
 * words zeroed, the emit of H x k lanes, the flag bytes out); never a launch per tree or per level, no allocation, no host read
 * of device data; every kernel behind the check reads the status first; flags of neighbouring small trees share 32-bit words and
 * are set with atomicOr.  No kernel hashes.  Refused on the host (VKMR_ERR_INVALID) with k > 0: what
 * vkmr_hip_forest_multiproof_async refuses, and a flags_dev off the 4-byte grid.  k == 0 does nothing.  Stream-ordered behind
 * updates.  vkmr_hip_tree_merkleblock_async is the same for ONE stored tree (vkmr_hip_reduce_tree_async) with
 * height == max(1, ceil(log2 count)) -- any other height is refused: B is 1 and block_trees_dev[0] is 0.
 * vkmr_host_cpu_forest_merkleblocks (libvkmr_host.so) applies the same rule on the CPU; vkmr_host_cpu_merkleblock_extract is the
 * receiver's side, Bitcoin Core's TraverseAndExtract under this height, with its CVE-2012-2459 check.  Not offered: a batched
 * verifier on the device -- the receiver of a merkleblock is a light client.
 */
VKMR_API size_t vkmr_hip_forest_merkleblocks_max_hashes(uint64_t total, uint32_t ntrees, uint64_t max_count, uint32_t k);
VKMR_API size_t vkmr_hip_forest_merkleblocks_max_flag_bytes(uint64_t total, uint32_t ntrees, uint64_t max_count, uint32_t k);
VKMR_API size_t vkmr_hip_forest_merkleblocks_scratch_bytes(uint32_t k, uint32_t stride);
VKMR_API vkmr_status vkmr_hip_forest_merkleblocks_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev, const vkmr_digest* forest_dev,
                                                        uint64_t total, const uint64_t* offsets_dev, uint32_t ntrees, uint64_t max_count,
                                                        const uint32_t* trees_dev, const uint64_t* indices_dev, uint32_t k, void* scratch_dev,
                                                        uint32_t* block_trees_dev, uint64_t* block_counts_dev, uint64_t* bit_counts_dev,
                                                        uint64_t* hash_starts_dev, uint64_t* byte_starts_dev, vkmr_digest* hashes_dev,
                                                        uint64_t hash_capacity, uint8_t* flags_dev, uint64_t flag_capacity, uint64_t* info_dev);
VKMR_API vkmr_status vkmr_hip_tree_merkleblock_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev, const vkmr_digest* tree_dev,
                                                     uint64_t count, uint32_t height, const uint64_t* indices_dev, uint32_t k, void* scratch_dev,
                                                     uint32_t* block_trees_dev, uint64_t* block_counts_dev, uint64_t* bit_counts_dev,
                                                     uint64_t* hash_starts_dev, uint64_t* byte_starts_dev, vkmr_digest* hashes_dev,
                                                     uint64_t hash_capacity, uint8_t* flags_dev, uint64_t flag_capacity, uint64_t* info_dev);

/*
 * SORTED TREES (the reference has no counterpart): "this digest is NO leaf", proved to a holder of the roots and the counts.  Every
 * proof above says that something IS in a tree; the one "no", vkmr_hip_forest_find_async's not-found pair, is visible only to who
 * holds every leaf.  A tree whose leaves are strictly increasing gives the provable one: x is absent exactly when two ADJACENT
 * leaves straddle it, or it lies below leaf 0 or above the last leaf, and the inclusion proofs of those neighbours prove it under
 * the root.  The rules, csrc/absence_plan.hpp:
 *   order        a < b compares data[0], then data[1], .. data[7] as UNSIGNED 32-bit values: the byte order of the canonical digest
 *   sorted       leaf[i-1] < leaf[i] for every 1 <= i < c; equal neighbours offend as well
 *   lower bound  lo = 0, hi = c; while lo < hi: mid = lo + (hi - lo) / 2; leaf[mid] < x ? lo = mid + 1 : hi = mid.  The answer is
 *                lo, on a sorted tree the number of leaves below x; fixed as a loop, so an unsorted tree still has one answer
 * digests_dev, total, offsets_dev, ntrees as in vkmr_hip_reduce_forest_async, TRUSTED as vkmr_hip_forest_find_async trusts them; no
 * leaf load leaves [offsets[0], min(offsets[ntrees], total)).  All four calls are stream-ordered on the caller's stream, allocate
 * nothing, need no scratch and read no device data on the host; every index and offset is 64-bit.  Refused on the host
 * (VKMR_ERR_INVALID), before any HIP call: a NULL pointer that is needed, a count above 2^58, a buffer off its grid (16 bytes for
 * digests, 8 for uint64_t, 4 for uint32_t) and what each call names below.
 *
 * IS IT SORTED: one read-only pass over level 0, 32 bytes a leaf, no stored level needed.
 *   first_bad_dev[t]  ntrees uint64_t: the lowest i in [1, c_t) with !(leaf[i-1] < leaf[i]), or UINT64_MAX.  A descent across the
 *                     boundary of two trees is no offence.
 *   info_dev          four uint64_t: [0] status (bit 0: the offsets decrease somewhere or end behind total; the rest is then
 *                     not to be used), [1] trees not sorted, [2] those whose first offence is an EQUAL pair, [3] pairs compared
 * Launches: two memsets, the scan (a lane per cell; none below two cells) and a lane per tree.  ntrees == 0 does nothing.  The
 * one-tree twin takes the leaves as cells [0, count) of digests_dev; first_bad_dev is then one uint64_t; count == 0 is fine.
 * This pass is what tests vkmr_hip_forest_sort_leaves_async below.
 */
VKMR_API vkmr_status vkmr_hip_forest_sorted_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev, uint64_t total,
                                                  const uint64_t* offsets_dev, uint32_t ntrees, uint64_t* first_bad_dev, uint64_t* info_dev);
VKMR_API vkmr_status vkmr_hip_tree_sorted_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev, uint64_t count,
                                                uint64_t* first_bad_dev, uint64_t* info_dev);
/*
 * LOWER BOUND: Q queries (trees_dev[q], queries_dev[q]) in DEVICE memory, one lane a query running the loop above:
 *   indices_out_dev[q] = i, found_out_dev[q] = 1 when leaf i exists and equals the query, else 0
 * and UINT64_MAX, 0 for a tree >= ntrees.  The tree need not be sorted for the call to answer; the answer then means what the
 * loop makes of it.  On a sorted tree the number of leaves in [x, y) is the difference of two queries: range counts come free.
 * No stored level is needed.  Q == 0 does nothing.
 */
VKMR_API vkmr_status vkmr_hip_forest_lower_bound_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev, uint64_t total,
                                                       const uint64_t* offsets_dev, uint32_t ntrees, const uint32_t* trees_dev,
                                                       const vkmr_digest* queries_dev, uint32_t Q, uint64_t* indices_out_dev,
                                                       uint32_t* found_out_dev);
VKMR_API vkmr_status vkmr_hip_tree_lower_bound_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev, uint64_t count,
                                                     const vkmr_digest* queries_dev, uint32_t Q, uint64_t* indices_out_dev,
                                                     uint32_t* found_out_dev);
/*
 * ABSENCE PROOFS out of a stored forest (digests_dev, forest_dev, total, offsets_dev, ntrees, max_count: those of the build,
 * trusted as vkmr_hip_forest_proofs_async trusts them): the lower bound, then a gather.  No hash.  For query q, i its lower bound
 * in tree t of c leaves and H(c) = max(1, ceil(log2 c)), 0 for c == 0:
 *   indices_out_dev[q]         i
 *   neighbours_out_dev[2q]     pred = leaf i - 1, a zero cell when i == 0;   [2q + 1]  succ = leaf i, a zero cell when i == c
 *   heights_out_dev[q]         H(c)
 *   main_out_dev[q * stride + l]  the plain inclusion proof (vkmr_hip_forest_proofs_async's cells) of the ANCHOR: leaf i when
 *                              i < c, else leaf c - 1; zero for l >= H(c)
 *   low_out_dev[q * stride + l]   only when 0 < i < c, with top = ctz(i): the sibling of leaf i - 1 at the levels l < top; zero
 *                              from top up.  The bits of i - 1 below top are ones, so these are left siblings and all exist.
 * This is the compact form: above top the two paths are one, and the node of leaf i - 1 at level top IS main[top].  A tree
 * >= ntrees gets height 0, index UINT64_MAX and zero cells; a tree without a leaf index 0, height 0 and zero cells.  Every cell
 * of every output is written.  Launches: a lane per query, then a lane per (query, level).  Refused: stride 0, above 63 or below
 * the forest's H = max(1, ceil(log2 min(max_count, total))).  Q == 0 does nothing.  The one-tree twin reads a tree stored by
 * vkmr_hip_reduce_tree_async with height == max(1, ceil(log2 count)) -- any other is refused --; its stride is that height, and it
 * writes no heights.  A query that IS a leaf gets the same cells: succ is then the query, and the check below says "present".
 */
VKMR_API vkmr_status vkmr_hip_forest_absence_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev, const vkmr_digest* forest_dev,
                                                   uint64_t total, const uint64_t* offsets_dev, uint32_t ntrees, uint64_t max_count,
                                                   const uint32_t* trees_dev, const vkmr_digest* queries_dev, uint32_t Q, uint32_t stride,
                                                   uint64_t* indices_out_dev, vkmr_digest* neighbours_out_dev, vkmr_digest* main_out_dev,
                                                   vkmr_digest* low_out_dev, uint32_t* heights_out_dev);
VKMR_API vkmr_status vkmr_hip_tree_absence_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev, const vkmr_digest* tree_dev,
                                                 uint64_t count, uint32_t height, const vkmr_digest* queries_dev, uint32_t Q,
                                                 uint64_t* indices_out_dev, vkmr_digest* neighbours_out_dev, vkmr_digest* main_out_dev,
                                                 vkmr_digest* low_out_dev);
/*
 * THE CHECK of Q absence proofs against roots_dev[ntrees] and counts_dev[ntrees], one lane a proof.  verdict_dev[q] is
 *   0 not proven, 1 absent, proven, 2 present, proven
 * by these steps, with t, i, pred, succ, the rows and height as above and c = counts_dev[t]:
 *   1. 0 when t >= ntrees;  2. 0 when height != H(c) (or above stride, or c above 2^58);  3. 0 when i > c
 *   4. c == 0: 1 exactly when the root is all zero
 *   5. i < c and x == succ: succ folded through the main row (vkmr_host_cpu_fold_proof, index i); 2 when that is the root.  pred
 *      and the low row are not looked at
 *   6. else pred < x is required when i > 0, and x < succ when i < c
 *   7. the anchor (succ when i < c, else pred, at index min(i, c - 1)) folded through the main row must be the root
 *   8. when 0 < i < c: pred folded through low[0 .. top) as a right child at every level must equal main[top]
 *   9. 1 when all of it holds
 * Cells of the low row at or above top, and of either row at or above the height, are never read.  The cost is H + top node
 * hashes a proof where two plain proofs take 2 H; over random gaps the mean top is about 1.  SOUNDNESS: the verdict binds under a
 * root COMMITTED OVER A SORTED TREE -- two adjacent leaves of an unsorted tree may straddle a digest that is a leaf elsewhere.
 * Who holds the leaves checks that with vkmr_hip_forest_sorted_async; a light client trusts whoever signed the root for it.
 * Refused: stride 0 or above 63.  Q == 0 does nothing.  The one-tree twin checks against one root and one count, the same for
 * every proof; its stride is `height`, refused unless height == H(count) (0 for count == 0, when the rows may be NULL).
 * vkmr_host_cpu_forest_sorted, vkmr_host_cpu_forest_lower_bound, vkmr_host_cpu_forest_absence and vkmr_host_cpu_verify_absence
 * (libvkmr_host.so) apply the same rules on the CPU, for a party without a GPU.
 */
VKMR_API vkmr_status vkmr_hip_verify_forest_absence_async(int dev, vkmr_stream s, const vkmr_digest* queries_dev, const uint32_t* trees_dev,
                                                          const uint64_t* indices_dev, const vkmr_digest* neighbours_dev,
                                                          const vkmr_digest* main_dev, const vkmr_digest* low_dev, const uint32_t* heights_dev,
                                                          uint32_t Q, uint32_t stride, const vkmr_digest* roots_dev, const uint64_t* counts_dev,
                                                          uint32_t ntrees, uint32_t* verdict_dev);
VKMR_API vkmr_status vkmr_hip_verify_absence_async(int dev, vkmr_stream s, const vkmr_digest* queries_dev, const uint64_t* indices_dev,
                                                   const vkmr_digest* neighbours_dev, const vkmr_digest* main_dev, const vkmr_digest* low_dev,
                                                   uint32_t Q, uint32_t height, const vkmr_digest* root_dev, uint64_t count,
                                                   uint32_t* verdict_dev);

/*
 * RANGE PROOFS: "here is EVERY leaf of tree t between lo and hi, and none was left out", for a holder of the roots and counts of
 * sorted trees.  The rules, csrc/range_plan.hpp.  A query is (trees_dev[q], lo_dev[q], hi_dev[q]): a tree and a CLOSED interval of
 * digests in the order above; the all-zero and the all-ones digest say "from the start" and "to the end".  For tree t of c leaves,
 * H = H(c):
 *   i0 = the lower bound of lo;  i1 = the upper bound of hi (the lower bound, + 1 when the leaf there is hi)
 *   the RUN is leaves [a, b]: a = i0 > 0 ? i0 - 1 : 0, b = i1 < c ? i1 : c - 1, m = b - a + 1 >= 1 -- the leaves in the range and the
 *   neighbour on either side that fences them, where there is one; an empty range carries its fence alone (one or two leaves)
 *   c == 0: first 0, m 0.  t >= ntrees or hi < lo: the query is REFUSED, first UINT64_MAX, m 0, height 0; the check answers 0
 * THE GATHER (no hash; four small launches, a lane per carried leaf, a lane per (query, level)) writes
 *   firsts_out_dev[q]       a
 *   leaf_starts_out_dev     Q + 1 words: the exclusive prefix over m, formed in 64 bits; [Q] is the leaves carried
 *   leaves_out_dev          the runs back to back: cells [leaf_starts[q], leaf_starts[q + 1]) are leaves a .. b of the tree
 *   left_out_dev, right_out_dev   Q x stride cells each: left[l] = node (a >> l) - 1 of level l when (a >> l) is odd, right[l] = node
 *                           (b >> l) + 1 when (b >> l) is even and that node exists (< ceil(c / 2^l)); zero cells otherwise and from H
 *                           up.  The duplicate of a level's last node is NOT carried: the check duplicates by the count, as BIP37
 *                           does, so that the count binds the right edge.  Every cell of both rows is written
 *   heights_out_dev[q]      H (the forest call only)
 *   info_dev[0..4)          status, leaves carried, queries refused, leaves in range
 * Status bit 0: the leaves carried exceed leaves_capacity.  firsts, leaf_starts, the heights, the rows and info are valid then,
 * info[1] is the true total, NO leaf is written; the caller allocates and calls again (leaves_capacity 0, leaves_out_dev NULL, is
 * the counting call).  Nothing at or behind cell leaf_starts[Q] of leaves_out_dev is touched.  scratch_dev:
 * vkmr_hip_range_scratch_bytes(0, Q) bytes, 16-byte aligned.  Refused as vkmr_hip_forest_absence_async refuses: a NULL pointer, a
 * buffer off its grid, stride 0, above 63 or below the forest's H.  Q == 0 does nothing.  The one-tree twin reads one stored tree
 * (vkmr_hip_reduce_tree_async; count >= 1, height == H(count), which is its stride) and writes no heights.
 */
VKMR_API size_t vkmr_hip_range_scratch_bytes(uint64_t nleaves, uint32_t Q);
VKMR_API vkmr_status vkmr_hip_forest_range_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev, const vkmr_digest* forest_dev, uint64_t total,
                                                 const uint64_t* offsets_dev, uint32_t ntrees, uint64_t max_count, const uint32_t* trees_dev,
                                                 const vkmr_digest* lo_dev, const vkmr_digest* hi_dev, uint32_t Q, uint32_t stride, void* scratch_dev,
                                                 uint64_t* firsts_out_dev, uint64_t* leaf_starts_out_dev, vkmr_digest* leaves_out_dev,
                                                 uint64_t leaves_capacity, vkmr_digest* left_out_dev, vkmr_digest* right_out_dev,
                                                 uint32_t* heights_out_dev, uint64_t* info_dev);
VKMR_API vkmr_status vkmr_hip_tree_range_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev, const vkmr_digest* tree_dev, uint64_t count,
                                               uint32_t height, const vkmr_digest* lo_dev, const vkmr_digest* hi_dev, uint32_t Q, void* scratch_dev,
                                               uint64_t* firsts_out_dev, uint64_t* leaf_starts_out_dev, vkmr_digest* leaves_out_dev,
                                               uint64_t leaves_capacity, vkmr_digest* left_out_dev, vkmr_digest* right_out_dev, uint64_t* info_dev);
/*
 * THE CHECK of Q range proofs against roots_dev[ntrees] and counts_dev[ntrees]; nleaves is the cells of leaves_dev, at least
 * leaf_starts[Q].  With t, a, the rows and the height as above, m = leaf_starts[q + 1] - leaf_starts[q] and c = counts_dev[t],
 * verdict_dev[q] is 0 when
 *   t >= ntrees;  height != H(c), or above stride;  c > 2^58;  a + m > c;  hi < lo;  m == 0 with c > 0
 * and c == 0 is proven empty exactly when m == 0 and the root is all zero.  Otherwise it is 1 when all of this holds:
 *   1. the carried leaves are strictly increasing
 *   2. leaf[a] < lo, or a == 0;   3. leaf[b] > hi, or b == c - 1          (the fences)
 *   4. leaf[a + 1] >= lo when m >= 2 and leaf[a] < lo; leaf[b - 1] <= hi when m >= 2 and leaf[b] > hi   (the canonical shape)
 *   5. THE FOLD: the nodes of level l are [a >> l, b >> l]; parent p takes its left child 2p from left[l] when 2p < (a >> l), its
 *      right child 2p + 1 from right[l] when 2p + 1 > (b >> l) and 2p + 1 < ceil(c / 2^l), and the left child again when 2p + 1 does
 *      not exist.  After H levels the one node left must be the root.
 * in_first_dev[q], in_count_dev[q]: the leaves of the run that lie in [lo, hi], as an index into the tree and a number; both 0 when
 * the verdict is 0.  The position is bound: every left / right decision is taken from a, m and c, and no row cell is read that the
 * rule does not name (the zero cells, and the cells at or above H, never).  leaf_starts that is no non-decreasing sequence ending at
 * or below nleaves proves nothing: every verdict is 0.  SOUNDNESS: as with absence, the verdict binds under a root COMMITTED OVER A
 * SORTED TREE.  The launches: a lane per query and a lane per leaf for the refusals, then ONE LAUNCH PER LEVEL (`stride` of them)
 * with a lane per node of all ranges, then a lane per query.  scratch_dev: vkmr_hip_range_scratch_bytes(nleaves, Q) bytes, 16-byte
 * aligned (0 for Q == 0 or nleaves above 2^58).  Refused: stride 0 or above 63, a NULL pointer, a buffer off its grid.  Q == 0 does
 * nothing.  The one-tree twin checks against one root and one count; its stride is `height`, refused unless height == H(count) (0 for
 * count == 0, when the rows may be NULL).  vkmr_host_cpu_forest_range, vkmr_host_cpu_tree_range and vkmr_host_cpu_verify_range
 * (libvkmr_host.so) apply the same rules on the CPU.
 */
VKMR_API vkmr_status vkmr_hip_verify_forest_range_async(int dev, vkmr_stream s, const uint32_t* trees_dev, const vkmr_digest* lo_dev,
                                                        const vkmr_digest* hi_dev, const uint64_t* firsts_dev, const uint64_t* leaf_starts_dev,
                                                        const vkmr_digest* leaves_dev, uint64_t nleaves, const vkmr_digest* left_dev,
                                                        const vkmr_digest* right_dev, const uint32_t* heights_dev, uint32_t Q, uint32_t stride,
                                                        const vkmr_digest* roots_dev, const uint64_t* counts_dev, uint32_t ntrees, void* scratch_dev,
                                                        uint32_t* verdict_dev, uint64_t* in_first_dev, uint64_t* in_count_dev);
VKMR_API vkmr_status vkmr_hip_verify_range_async(int dev, vkmr_stream s, const vkmr_digest* lo_dev, const vkmr_digest* hi_dev,
                                                 const uint64_t* firsts_dev, const uint64_t* leaf_starts_dev, const vkmr_digest* leaves_dev,
                                                 uint64_t nleaves, const vkmr_digest* left_dev, const vkmr_digest* right_dev, uint32_t Q,
                                                 uint32_t height, const vkmr_digest* root_dev, uint64_t count, void* scratch_dev,
                                                 uint32_t* verdict_dev, uint64_t* in_first_dev, uint64_t* in_count_dev);

/*
 * SORT THE LEAVES of a forest, tree by tree, on the device: what makes a sorted tree out of a set of digests without a trip
 * through the host.  A stable segmented sort of 32-byte digests: for every tree t the leaves at cells [offsets[t], offsets[t+1])
 * of digests_in_dev are written to the SAME cells of digests_out_dev in increasing order -- the order above (word 0 first, every
 * word unsigned) --, equal digests in their input order.  total, offsets_dev, ntrees, max_count as in vkmr_hip_reduce_forest_async.
 *   order_out_dev[j]  for offsets[0] <= j < offsets[ntrees]: the flat cell of digests_in_dev that now lies at cell j of
 *                     digests_out_dev (uint32; `total` cells; may be NULL).  order_out_dev + offsets[0] is what
 *                     vkmr_hip_gather_digests_async takes, so that a payload (values, string numbers) follows the leaves.
 *   info_dev          4 uint64_t, always written when ntrees > 0: [0] status, [1] n, the leaves sorted (0 with status bit 0),
 *                     [2] m, the leaves that tie with a neighbour on the sort key, [3] the leaves equal in all 32 bytes to an
 *                     earlier leaf of their tree (0 with a nonzero status).  A tree with [3] > 0 cannot be strictly increasing;
 *                     the call sorts it all the same and says so.
 * Cells outside [offsets[0], offsets[ntrees]) of both outputs are never touched.  Status bits, checked on the device before
 * anything is written, as the forest build does: bit 0 the offsets decrease somewhere or offsets[ntrees] > total; bit 1 some
 * tree holds more than max_count leaves; bit 2 m > VKMR_LEAFSORT_MAX_TIES (csrc/leafsort_plan.hpp; [2] still holds m).  With a
 * nonzero status no cell of digests_out_dev or order_out_dev is written.
 * HOW (csrc/leafsort_plan.hpp): one stable LSD radix sort, csrc/sort_plan.hpp's passes of 8 bits, of the 64-bit keys
 *   (tree << P) | (the digest's first 64 bits >> (64 - P)),  P = min(64 - bit_length(ntrees - 1), 2 * bit_length(max_count) + 8)
 * over `total` elements -- element i is cell offsets[0] + i, the elements behind the last leaf carry an all-ones sentinel --, so
 * ceil((bit_length(ntrees - 1) + P) / 8) <= 8 passes; then the few leaves whose key equals a neighbour's are placed inside their
 * run of equal keys by all 256 bits.  That last step costs at most MAX_TIES^2 compares whatever the input: a crafted batch with
 * more ties is refused (bit 2) and goes through vkmr_host_cpu_forest_sort_leaves, which has no limit.  Among hashed leaves about
 * n / (512 * max_count) tie.
 *   scratch_dev  vkmr_hip_sort_leaves_scratch_bytes(total) bytes of device memory, 16-byte aligned: about 29.3 bytes a cell (24 for
 *                the ping-pong keys and positions, 4 for dest, the rest histograms); 0 for total == 0, when it may be NULL
 * Launches, all on the caller's stream: two memsets, the check, the keys, three per pass, the ties, the place, the emit.  They
 * depend on (total, ntrees, max_count) alone; no allocation, no host synchronisation, no host read of device data; no kernel
 * waits for another workgroup; atomics only count.  ntrees == 0 does nothing.  total == 0 with ntrees > 0 writes n = 0 (and the
 * status of the offsets).  Refused on the host (VKMR_ERR_INVALID), before any HIP call: a NULL pointer that is needed, total >=
 * 2^32 (positions are uint32), scratch_dev not 16-byte aligned, the `total` cells of digests_out_dev overlapping those of
 * digests_in_dev or the scratch.
 * The one-tree twin sorts cells [0, count): total = max_count = count, no offsets, status bit 2 alone; order_out_dev may be NULL.
 * vkmr_host_cpu_forest_sort_leaves / vkmr_host_cpu_tree_sort_leaves (libvkmr_host.so) are the CPU's, without the tie limit.
 */
VKMR_API size_t vkmr_hip_sort_leaves_scratch_bytes(uint64_t total);
VKMR_API vkmr_status vkmr_hip_forest_sort_leaves_async(int dev, vkmr_stream s, const vkmr_digest* digests_in_dev, uint64_t total,
                                                       const uint64_t* offsets_dev, uint32_t ntrees, uint64_t max_count, void* scratch_dev,
                                                       vkmr_digest* digests_out_dev, uint32_t* order_out_dev, uint64_t* info_dev);
VKMR_API vkmr_status vkmr_hip_tree_sort_leaves_async(int dev, vkmr_stream s, const vkmr_digest* digests_in_dev, uint64_t count,
                                                     void* scratch_dev, vkmr_digest* digests_out_dev, uint32_t* order_out_dev,
                                                     uint64_t* info_dev);

/*
 * MERGE two sorted forests over the same ntrees, tree by tree, on the device: what inserts leaves into sorted trees, removes them
 * and says which are held in common, in one streaming pass and with equal digests kept once.  A is a_digests_dev, a_total,
 * a_offsets_dev[ntrees + 1] and B is b_digests_dev, b_total, b_offsets_dev[ntrees + 1], both laid out as
 * vkmr_hip_reduce_forest_async takes them; the order is the one above (word 0 first, every word unsigned).  Every tree of A must
 * be strictly increasing; every tree of B non-decreasing -- equal neighbours, which vkmr_hip_forest_sort_leaves_async leaves
 * behind, count once.  Tree t of the output, by op:
 *   0 union          the distinct digests of A_t and B_t, increasing; a digest in both is A's cell
 *   1 difference     the leaves of A_t that equal no leaf of B_t
 *   2 intersection   the leaves of A_t that equal some leaf of B_t
 *   out_offsets_dev   ntrees + 1 uint64_t, out_offsets[0] = 0: what the forest builds take as it is
 *   out_digests_dev   the output trees back to back at cells [0, out_offsets[ntrees]); out_capacity cells; the cells at or behind
 *                     out_offsets[ntrees] are never touched
 *   origin_out_dev    (may be NULL) out_capacity uint64_t: the flat input cell that lies at output cell j, bit 63 set when it is a
 *                     cell of B, so that a payload can follow
 *   info_dev          4 uint64_t, always written when ntrees > 0: [0] status, [1] n_out, [2] matches, the distinct digests of B
 *                     that equal a leaf of A in their tree, [3] repeats, the leaves of B equal to their predecessor in their tree.
 *                     [2] and [3] do not depend on op; n_out = nA + nB - matches - repeats (union), nA - matches (difference),
 *                     matches (intersection).  [1..3] are 0 when one of the status bits 0 to 3 is set.
 * Status bits, all formed on the device before any cell of out_digests_dev, origin_out_dev or out_offsets_dev is written; with a
 * nonzero status none of those is written: bit 0 A's offsets decrease somewhere or end behind a_total; bit 1 the same for B; bit 2
 * some tree of A is not strictly increasing; bit 3 some tree of B decreases somewhere; bit 4 n_out > out_capacity ([1] still holds
 * n_out, so that the caller can call again).  out_capacity = nA + nB for union, nA for the other two, never sees bit 4.
 * HOW (csrc/merge_plan.hpp): a lane per leaf of B runs the lower bound's loop in A_t and compares with its predecessor; a kept
 * leaf counts at A's slot "in front of element lb" (an atomic add that only counts), a match marks it; one exclusive prefix over
 * the slots and B's keep flags (sort_scan_kernel as it is, two launches) makes every destination a closed form; then a lane per leaf
 * of A and, for union, of B does one 32-byte load and one 32-byte store.  The elements are numbered from offsets[0]: the work
 * follows (a_total, b_total, ntrees), never where the forests lie in their buffers.
 *   scratch_dev  vkmr_hip_merge_leaves_scratch_bytes(a_total, b_total, ntrees) bytes, 16-byte aligned: about 4 bytes a cell of A
 *                and 8 a cell of B (ntrees does not enter today's layout); 0 when the call would be refused for its size
 * Launches, all on the caller's stream: two memsets, the two offsets checks, the order of A, the marks of B, two scans, the emit;
 * no allocation, no host synchronisation, no host read of device data; no kernel waits for another workgroup.  ntrees == 0 does
 * nothing.  Empty trees on either side, an empty A and an empty B are fine and still write the offsets and info.  Refused on the
 * host (VKMR_ERR_INVALID), before any HIP call: a NULL pointer that is needed (the digests of a side with no cell and
 * out_digests_dev with out_capacity == 0 are not), op > 2, a_total + b_total + 2 >= 2^32 (the scan carries uint32 sums), a
 * digest buffer or the scratch off its 16-byte grid, a uint64_t buffer off its 8-byte grid, the out_capacity cells of
 * out_digests_dev overlapping either input or the scratch.
 * The one-tree twin merges cells [0, a_count) with cells [0, b_count): no offsets, n_out in info[1] alone, status bits 2, 3 and 4.
 * vkmr_host_cpu_forest_merge_leaves / vkmr_host_cpu_tree_merge_leaves (libvkmr_host.so) are the CPU's.
 */
VKMR_API size_t vkmr_hip_merge_leaves_scratch_bytes(uint64_t a_total, uint64_t b_total, uint32_t ntrees);
VKMR_API vkmr_status vkmr_hip_forest_merge_leaves_async(int dev, vkmr_stream s, const vkmr_digest* a_digests_dev, uint64_t a_total,
                                                        const uint64_t* a_offsets_dev, const vkmr_digest* b_digests_dev, uint64_t b_total,
                                                        const uint64_t* b_offsets_dev, uint32_t ntrees, uint32_t op, void* scratch_dev,
                                                        vkmr_digest* out_digests_dev, uint64_t out_capacity, uint64_t* out_offsets_dev,
                                                        uint64_t* origin_out_dev, uint64_t* info_dev);
VKMR_API vkmr_status vkmr_hip_tree_merge_leaves_async(int dev, vkmr_stream s, const vkmr_digest* a_digests_dev, uint64_t a_count,
                                                      const vkmr_digest* b_digests_dev, uint64_t b_count, uint32_t op, void* scratch_dev,
                                                      vkmr_digest* out_digests_dev, uint64_t out_capacity, uint64_t* origin_out_dev,
                                                      uint64_t* info_dev);

/*
 * COMBINE:duplicate-last Merkle root over n >= 1 slice roots given in slice order, always
 * at least one level -- the rule of CpuSha256D::Root that the reference applies to the slice
 * roots on the CPU (CpuSha256DforReductions, src/vkmr/Reductions.cpp:56-69, :703-712).  Here
 * the roots stay in HBM (where the reductions or the gather below left them) and the combine is
 * one more launch on the caller's stream: no allocation, no synchronisation.  For n == 1 the
 * reference prints the slice root itself (src/vkmr/Reductions.cpp:692-701); callers do the same
 * and do not call combine.
 *   scratch_dev  vkmr_hip_reduce_scratch_bytes(n) bytes, 16-byte aligned (see "Scratch buffers"); may be NULL for n <= 128
 */
VKMR_API vkmr_status vkmr_hip_combine_async(int dev, vkmr_stream s, const vkmr_digest* roots_dev, uint32_t n,
                                            void* scratch_dev, vkmr_digest* root_dev);

/* ---- multi-GPU: slices sharded over devices, ONE gather of the sub-tree roots --------------
 *
 * The reference drives one device and collects slice roots on the host: each Reduction copies
 * its 32-byte root into a host-visible buffer (src/vkmr/Reductions.cpp:125-145, :537-540) and
 * ReductionsImpl::WaitFor feeds them, in slice order, to CpuSha256DforReductions (:56-69,
 * :703-712).  With slices sharded over the GPUs of a node that collection is a single RCCL
 * all-gather over xGMI (32 bytes per slice), after which any rank holds every root and runs
 * vkmr_hip_combine_async.  Two ways to form the communicator: one process driving every GPU
 * (the C++ front end's "hip:all"), or one process per GPU (bench.py under torch.distributed.run;
 * the 128-byte id travels over whatever channel the host program already has).
 * librccl is loaded on the first communicator, never by single-GPU runs.
 */
typedef struct vkmr_comm_s* vkmr_comm;
#define VKMR_COMM_ID_BYTES 128   /* sizeof(ncclUniqueId) */

/* One process, ndev devices: rank i of the communicator is devs[i]. */
VKMR_API vkmr_status vkmr_hip_comm_init_all(const int* devs, int ndev, vkmr_comm* out);
/* One process per device: rank 0 creates the id, every rank joins with the same id. */
VKMR_API vkmr_status vkmr_hip_comm_create_id(void* id /* VKMR_COMM_ID_BYTES */);
VKMR_API vkmr_status vkmr_hip_comm_init_rank(int dev, const void* id, int nranks, int rank, vkmr_comm* out);
VKMR_API vkmr_status vkmr_hip_comm_destroy(vkmr_comm c);
/* Ranks in the communicator and how many of them this process drives. */
VKMR_API vkmr_status vkmr_hip_comm_size(vkmr_comm c, int* nranks, int* nlocal);

/*
 * GATHER: every rank contributes `per_rank` roots; when the call has completed on streams[i],
 * all_dev[i] (nranks * per_rank cells) holds rank r's roots at [r * per_rank, (r + 1) * per_rank).
 * The three arrays have one entry per LOCAL rank (one entry in a one-process-per-GPU program).
 * Ranks with fewer roots pad to per_rank; the padding is never read by the combine.
 * Issued as one ncclAllGather per local rank (grouped), enqueued on the given streams: ordered
 * after the reductions that produce roots_dev[i] when those ran on the same stream.
 */
VKMR_API vkmr_status vkmr_hip_gather_roots_async(vkmr_comm c, const vkmr_stream* streams,
                                                 const vkmr_digest* const* roots_dev, uint32_t per_rank,
                                                 vkmr_digest* const* all_dev);

/*
 * Reorders gathered roots into slice order when slices were dealt round-robin (slice k on rank
 * (k-1) % nranks, Slices::New -- the reference numbers slices 1, 2, ... in stream order,
 * src/vkmr/Slices.h:371): out[k] = gathered[(k % nranks) * per_rank + k / nranks], k < total.
 * With one slice per rank (bench.py) the gathered order already is the slice order.
 */
VKMR_API vkmr_status vkmr_hip_roots_in_slice_order_async(int dev, vkmr_stream s, const vkmr_digest* gathered_dev,
                                                         uint32_t nranks, uint32_t per_rank, uint32_t total,
                                                         vkmr_digest* out_dev);

/* Canonical lower-case hex of a digest cell (hash_to_string + print_bytes,
 * src/vkmr/SHA-256plus.cpp:453-469, src/vkmr/Debug.cpp:38-46).  hex holds 65 bytes. */
VKMR_API void vkmr_hip_digest_hex(const vkmr_digest* d, char* hex);

/* ---- diagnostics ----------------------------------------------------------- */
VKMR_API const char* vkmr_hip_last_error(void);
/* What the LAST vkmr_hip_map_async of this process launched (kernel instantiation, fetch mode, tile), the reduction
 * kernels, and " build=<id>": the identity of the kernel sources and build parameters this library was made from
 * (vk_merkle_roots_amd/build.py: source_id) -- profile records are matched against it (profiles/pmc_latest.json). */
VKMR_API const char* vkmr_hip_kernel_info(void);
/* Which RCCL the communicators are bound to: the shared object ncclAllGather lives in and ncclGetVersion, e.g.
 * "rccl=/opt/rocm/lib/librccl.so.1 version=22703"; "rccl=not loaded" before the first communicator.  A process that
 * carries PyTorch must show torch's copy here, not a second one (csrc/comm_rccl.hpp). */
VKMR_API const char* vkmr_hip_comm_info(void);

#ifdef __cplusplus
}
#endif
#endif /* VKMR_HIP_H */
