// vkmr_hip.hip -- HIP kernels (gfx950) and the C ABI of include/vkmr_hip.h.
//
// Kernels (headers beside this file)
//   map_kernel.hpp      map_kernel             SHA-256d of every packed string      (SHA-256.comp:177-304)
//   reduce_kernels.hpp  reduce_pass_kernel     streaming sub-tree collapse per wave (SHA-256.comp:325-391)
//                       reduce_collapse_kernel / reduce_tail_kernel   the latency-bound top, __shfl_down
//                       reduce_level_kernel    one level per launch, cross-check    (SHA-256.comp:393-434); builds the stored tree
//   entries.hpp         what one stored tree and a stored forest differ in (entries, cells), and one body per operation they share
//   tree_kernels.hpp    tree_proofs_kernel     proofs gathered from the stored tree (README.md:118-120)
//                       verify_proofs_kernel   batch proof verification, one lane per proof (no reference counterpart)
//                       tree_update_*_kernel   leaf updates: check, store the leaves, rehash the dirty nodes level by level
//                       multiproof_*_kernel, tree_multiproof_gather_kernel, verify_multiproof_*_kernel   one proof for k leaves:
//                                              rank the nodes to emit, gather them; fold leaves and nodes level by level
//                       tree_apply_*_kernel   the new root from the old root: the verifier's fold of the old leaves and, in
//                                              the same launches (grid.y = the side), the fold of the new leaves; one commit
//   forest_kernels.hpp  forest_check_kernel, forest_level_kernel   roots of many trees of unequal size: one lane per node of the
//                                              whole forest, level by level (no reference counterpart); builds the stored forest
//                       forest_level_mutated_kernel, forest_scan_mutated_kernel   the same level with the mutation flag (equal
//                                              sibling pairs, CVE-2012-2459) formed beside the hash, and the flag alone from stored levels
//                       forest_append_*_kernel, forest_truncate_kernel   trees appended into the room a stored forest was built
//                                              with (the level body again, over the new trees' cells alone), the last trees dropped
//   forest_copy_kernels.hpp  forest_drop_front_kernel, forest_copy_*_kernel   the oldest trees dropped (offsets alone), stored trees
//                                              copied into another forest cell by cell: no hash
//                       forest_extend_*_kernel   the last tree in use grown or shrunk by leaves: the level body once more, over
//                                              the nodes of its right edge alone
//   frontier_kernels.hpp  frontier_*_kernel     trees followed by their frontiers alone (a count and one peak per set bit): the
//                                              new roots and frontiers from the new leaves, the root of a frontier, the frontier
//                                              of a stored tree
//   consistency_kernels.hpp  consistency_*_kernel   consistency proofs: the peaks of an earlier count and the right neighbours of
//                                              the walk from them to the root gathered from a stored forest (no hash), and the
//                                              verifier's two root walks, one lane per query (rules: consistency_plan.hpp)
//   proofs_at_kernels.hpp  proofs_at_*_kernel   inclusion proofs as of an earlier count: the old tree's right edge hashed once per
//                                              epoch (one lane each, one hash_pair), then a gather without a hash, one lane per
//                                              (query, level) (rules: proofs_at_plan.hpp)
//   merkleblock_kernels.hpp  merkleblock_*_kernel   partial Merkle trees in BIP37 order, one per named tree: the groups of the
//                                              entries summed, placed by two prefix sums (entries, blocks), then one lane per
//                                              (entry, level) copies at most three nodes and sets one flag; no hash, no walk
//                                              (the closed form and the sizes: merkleblock_plan.hpp)
//   absence_kernels.hpp  *_sorted_*_kernel, *_lower_bound_kernel, *_absence_*_kernel   sorted trees: one pass over level 0 for the first
//                                              pair out of order per tree, the lower bound of a digest, the two neighbours and their
//                                              compact pair of proofs gathered (no hash), and the verdict absent / present, one lane
//                                              per proof through one hash_pair (rules: absence_plan.hpp)
//   range_kernels.hpp  *_range_runs_kernel .. *_range_rows_kernel, *_range_heads_kernel .. *_range_verdict_kernel   sorted trees: every leaf
//                                              between two digests with the two rows that close its run (no hash), and the check that
//                                              none was left out: one launch per level, a lane per node of all ranges (rules: range_plan.hpp)
//   leafsort_kernels.hpp  *_leafsort_keys_kernel, *_leafsort_ties_kernel, *_leafsort_place_kernel, *_leafsort_emit_kernel   the leaves of a
//                                              forest sorted tree by tree in digest order: sort_kernels.hpp's radix passes over
//                                              (tree, digest prefix) keys, then the few ties placed by all 256 bits; no hash
//                                              (the key, the sentinel and the tie limit: leafsort_plan.hpp)
//   merge_kernels.hpp  *_merge_order_kernel, *_merge_mark_kernel, *_merge_emit_kernel   two sorted forests merged tree by tree (union,
//                                              difference, intersection): a lower bound per leaf of B, counts and marks at A's
//                                              slots, sort_scan_kernel over them, every leaf copied to a closed-form cell; no hash
//                                              (the slots and the placement: merge_plan.hpp)
//   forest_tree_kernels.hpp  forest_proofs_kernel          proofs gathered from the stored forest, one lane per (query, level)
//                            verify_forest_proofs_kernel   batch verification of proofs of unequal height, one lane per proof
//                            forest_update_*_kernel        leaf updates of the stored forest: tree_update_*'s bodies, a tree per entry
//                            forest_multiproof_*_kernel, verify_forest_multiproof_*_kernel   one proof for leaves of many trees:
//                                              the multiproof bodies and tree_kernels.hpp's ranking, a tree and a height per entry
//                            forest_apply_*_kernel   the new roots from the old roots: heights from the counts, the
//                                              verifier's launches on them, the level kernel twice as wide, one commit
//   find_kernels.hpp   find_insert_kernel, *_find_scan_kernel, *_find_resolve_kernel   lookup by digest: the queries in an open-addressed
//                                              table, every leaf streamed past it once, lowest position per query (sizes: find_plan.hpp)
//   sort_kernels.hpp    *_sort_keys_kernel, sort_histogram_kernel, sort_scan_kernel, sort_scatter_kernel, sort_flags_kernel, *_sort_emit_kernel,
//                                              gather_digests_kernel   leaf entries sorted and deduplicated: a stable LSD radix sort of
//                                              (flat position, q) pairs, the last of every run kept (sizes: sort_plan.hpp)
//   diff_kernels.hpp    *_diff_roots_count_kernel, *_diff_roots_emit_kernel, *_diff_mask_kernel, *_diff_emit_kernel   the leaves that differ
//                                              between two stored forests or trees of one shape: a descent from the roots, the frontier
//                                              ranked by the multiproof's ranking kernels at every step (steps and sizes: diff_plan.hpp)
//   audit_kernels.hpp   *_audit_level_kernel, *_audit_emit_kernel   the nodes of a stored forest or tree that are not the hash of their
//                                              stored children: the build's launches with a compare for the store, the bad nodes ranked
//                                              by the multiproof's ranking kernels (sizes: audit_plan.hpp)
//   sha256d_device.hpp  the SHA-256 round / compression building blocks, and the tree's: hash_parent, node_diff, store_node
//   merkle_math.hpp     the integer rules, no HIP types (ceil_shift, height, right_child, sibling): shared with host/ and tests/c
//   meta_kernels.hpp    sizes_*_kernel         metadata entries from 16-bit sizes   (Batches.cpp:64-121)
//
// Plans (no HIP types either: g++ compiles them, tests/c replays them, the test double sizes its scratch with them)
//   map_plan.hpp        the map kernel's fetch mode and tile for a batch
//   reduce_plan.hpp     the launch schedule of a slice reduction, height_ok, the chunks of a run of slices, the scratch sizes
//   tree_plan.hpp       the stored tree's level offsets, the multiproof node bound and scratch layout, the apply calls' scratch layout
//   forest_plan.hpp     where a forest's nodes lie, level by level; its scratch, stored size and multiproof node bound
//   find_plan.hpp       the lookup's scratch layout and scan grid
//   sort_plan.hpp       the entry sort's passes, tiles, histogram words and scratch layout
//   diff_plan.hpp       one step of a diff's descent, the bound on every step's frontier and the scratch layout
//   audit_plan.hpp      the ballot words of an audit's levels, the nodes it checks and the scratch layout
//   merkleblock_plan.hpp  what a BIP37 walk appends between two matched leaves, in closed form; the three size bounds, the scratch layout
//   range_plan.hpp      the run a closed interval of digests carries, the cells of its two rows, the check's steps and level layout
//   absence_plan.hpp    the order on digests, the lower bound's loop, the cells of an absence proof and the verdict of its check
//   leafsort_plan.hpp   the leaf sort's key and passes, its elements and sentinel, what a tie is, the tie limit and the scratch layout
//   merge_plan.hpp      the merge's slots, what a leaf of B does at its slot, where every leaf goes, the counts and the scratch layout
//
// Host side: plain launches on the caller's stream, each through launch() and so each checked; every argument refusal
// through refuse(__func__, why); no allocation, no sync inside the *_async entry points.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <stdlib.h>

#include <atomic>

#include "../../include/vkmr_hip.h"
#include "sha256d_device.hpp"

using vkmr_dev::Node;

#include "map_kernel.hpp"
#include "map_plan.hpp"
#include "meta_kernels.hpp"
#ifdef VKMR_EXPERIMENTS
#include "../../include/vkmr_hip_experiments.h"
#include "experiments/split_kernels.hpp"   // text -> packed batch on the device: measured, no gain, not shipped (include/vkmr_hip_experiments.h)
#endif
#include "reduce_kernels.hpp"
#include "reduce_plan.hpp"
#include "tree_plan.hpp"
#include "tree_kernels.hpp"
#include "forest_kernels.hpp"
#include "forest_copy_kernels.hpp"
#include "forest_tree_kernels.hpp"
#include "find_kernels.hpp"
#include "sort_kernels.hpp"
#include "diff_kernels.hpp"
#include "audit_kernels.hpp"
#include "frontier_kernels.hpp"
#include "consistency_kernels.hpp"
#include "proofs_at_kernels.hpp"
#include "merkleblock_kernels.hpp"
#include "absence_kernels.hpp"
#include "range_kernels.hpp"
#include "leafsort_kernels.hpp"
#include "merge_kernels.hpp"

// ============================================================================
// C ABI
// ============================================================================

static thread_local char g_err[512] = "";

static vkmr_status fail(vkmr_status code, const char* what, hipError_t e = hipSuccess)
{
    if (e != hipSuccess)
        snprintf(g_err, sizeof g_err, "%s: %s (%s)", what, hipGetErrorString(e), hipGetErrorName(e));
    else
        snprintf(g_err, sizeof g_err, "%s", what);
    return code;
}

static vkmr_status from_hip(hipError_t e, const char* what)
{
    if (e == hipSuccess) return VKMR_OK;
    (void)hipGetLastError();   // clear the sticky error
    if (e == hipErrorOutOfMemory) return fail(VKMR_ERR_OOM, what, e);
    if (e == hipErrorNoDevice || e == hipErrorInvalidDevice) return fail(VKMR_ERR_NO_DEVICE, what, e);
    return fail(VKMR_ERR_HIP, what, e);
}

// Return this vkmr_status unless it is VKMR_OK; VKMR_TRY: the same for a hipError_t.
#define VKMR_CHECK(expr)                                 \
    do {                                                 \
        const vkmr_status st__ = (expr);                 \
        if (st__ != VKMR_OK) return st__;                \
    } while (0)
#define VKMR_TRY(expr) VKMR_CHECK(from_hip((expr), #expr))

static inline hipStream_t S(vkmr_stream s) { return reinterpret_cast<hipStream_t>(s); }
static inline hipEvent_t E(vkmr_event e) { return reinterpret_cast<hipEvent_t>(e); }
// The ABI's digests (and raw scratch) as the kernels' nodes.
static inline const Node* nodes(const vkmr_digest* d) { return reinterpret_cast<const Node*>(d); }
static inline Node* nodes(vkmr_digest* d) { return reinterpret_cast<Node*>(d); }
static inline Node* nodes(void* p) { return static_cast<Node*>(p); }
// One lane per item in workgroups of 256: the workgroups, the grid (x for the items, y as given), and the most a launch takes.
static inline uint64_t groups_of(uint64_t items) { return (items + 255) / 256; }
static inline dim3 grid_of(uint64_t items, uint32_t y = 1) { return dim3((uint32_t)groups_of(items), y); }
static inline bool grid_too_large(uint64_t groups) { return groups > 0x7fffffffull; }
// A refusal in the words "<entry point>: <why>".  An entry point passes __func__; a helper that refuses on its behalf is given it.
static vkmr_status refuse(const char* who, const char* why)
{
    snprintf(g_err, sizeof g_err, "%s: %s", who, why);
    return VKMR_ERR_INVALID;
}

// One launch without dynamic LDS, checked.  The arguments convert to the kernel's own parameter types as in a plain call.
template <class T> struct as_declared { typedef T type; };
template <class... P>
static vkmr_status launch(void (*kernel)(P...), dim3 grid, dim3 block, hipStream_t stream, typename as_declared<P>::type... args)
{
    hipLaunchKernelGGL(kernel, grid, block, 0, stream, args...);
    return from_hip(hipGetLastError(), "hipGetLastError()");
}

extern "C" {

const char* vkmr_hip_last_error(void) { return g_err; }

#ifdef VKMR_STAMPS
// diagnostic build only: copies the stamp buffer out and clears it for the next launch
__attribute__((visibility("default"))) int vkmr_hip_debug_stamps(unsigned long long* out, int words)
{
    // The callers' streams are non-blocking ones: nothing orders them against the copy and the memset below (both on the
    // null stream) but these two device-wide waits.
    if (words < 0 || words > VKMR_STAMP_SLOTS * 8) return -1;
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps), sizeof(unsigned long long) * words) != hipSuccess) return -1;
    void* p = nullptr;
    if (hipGetSymbolAddress(&p, HIP_SYMBOL(g_stamps)) != hipSuccess) return -1;
    if (hipMemset(p, 0, sizeof(unsigned long long) * VKMR_STAMP_SLOTS * 8) != hipSuccess) return -1;
    return hipDeviceSynchronize() == hipSuccess ? 0 : -1;
}
#endif

const char* vkmr_hip_kernel_info(void);   // defined after the map entry point: it reports what the last launch chose

vkmr_status vkmr_hip_device_count(int* count)
{
    if (!count) return refuse(__func__, "null out pointer");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {   // no driver / no GPU: zero devices, like an empty Vulkan enumeration
        (void)hipGetLastError();
        *count = 0;
        fail(VKMR_OK, "hipGetDeviceCount", e);
        return VKMR_OK;
    }
    *count = n;
    return VKMR_OK;
}

vkmr_status vkmr_hip_device_name(int dev, char* buf, size_t buflen)
{
    if (!buf || buflen == 0) return refuse(__func__, "null buffer");
    hipDeviceProp_t p;
    VKMR_TRY(hipGetDeviceProperties(&p, dev));
    // some ROCm installs leave the marketing name empty: fall back to the ISA name
    snprintf(buf, buflen, "%s", p.name[0] ? p.name : p.gcnArchName);
    return VKMR_OK;
}

vkmr_status vkmr_hip_device_mem_info(int dev, size_t* free_bytes, size_t* total_bytes)
{
    if (!free_bytes || !total_bytes) return refuse(__func__, "null out pointer");
    VKMR_TRY(hipSetDevice(dev));
    VKMR_TRY(hipMemGetInfo(free_bytes, total_bytes));
    return VKMR_OK;
}

vkmr_status vkmr_hip_device_geometry(int dev, int* compute_units, int* wavefront)
{
    hipDeviceProp_t p;
    VKMR_TRY(hipGetDeviceProperties(&p, dev));
    if (compute_units) *compute_units = p.multiProcessorCount;
    if (wavefront) *wavefront = p.warpSize;
    return VKMR_OK;
}

vkmr_status vkmr_hip_host_alloc(size_t bytes, void** out)
{
    if (!out || bytes == 0) return refuse(__func__, "bad argument");
    void* p = nullptr;
    VKMR_TRY(hipHostMalloc(&p, bytes, hipHostMallocDefault));
    memset(p, 0, bytes);
    *out = p;
    return VKMR_OK;
}

vkmr_status vkmr_hip_host_free(void* p)
{
    if (!p) return VKMR_OK;
    VKMR_TRY(hipHostFree(p));
    return VKMR_OK;
}

vkmr_status vkmr_hip_device_alloc(int dev, size_t bytes, void** out)
{
    if (!out || bytes == 0) return refuse(__func__, "bad argument");
    VKMR_TRY(hipSetDevice(dev));
    void* p = nullptr;
    VKMR_TRY(hipMalloc(&p, bytes));
    *out = p;
    return VKMR_OK;
}

vkmr_status vkmr_hip_device_free(int dev, void* p)
{
    if (!p) return VKMR_OK;
    VKMR_TRY(hipSetDevice(dev));
    VKMR_TRY(hipFree(p));
    return VKMR_OK;
}

vkmr_status vkmr_hip_memset_async(int dev, vkmr_stream s, void* dst, int value, size_t bytes)
{
    if (!dst) return refuse(__func__, "null pointer");
    VKMR_TRY(hipSetDevice(dev));
    VKMR_TRY(hipMemsetAsync(dst, value, bytes, S(s)));
    return VKMR_OK;
}

vkmr_status vkmr_hip_memcpy_h2d_async(int dev, vkmr_stream s, void* dst_dev, const void* src_host, size_t bytes)
{
    if (!dst_dev || !src_host) return refuse(__func__, "null pointer");
    VKMR_TRY(hipSetDevice(dev));
    VKMR_TRY(hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, S(s)));
    return VKMR_OK;
}

vkmr_status vkmr_hip_memcpy_d2h_async(int dev, vkmr_stream s, void* dst_host, const void* src_dev, size_t bytes)
{
    if (!dst_host || !src_dev) return refuse(__func__, "null pointer");
    VKMR_TRY(hipSetDevice(dev));
    VKMR_TRY(hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, S(s)));
    return VKMR_OK;
}

vkmr_status vkmr_hip_stream_create(int dev, vkmr_stream* out)
{
    if (!out) return refuse(__func__, "null out pointer");
    VKMR_TRY(hipSetDevice(dev));
    hipStream_t s;
    VKMR_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *out = reinterpret_cast<vkmr_stream>(s);
    return VKMR_OK;
}

vkmr_status vkmr_hip_stream_destroy(int dev, vkmr_stream s)
{
    if (!s) return VKMR_OK;
    VKMR_TRY(hipSetDevice(dev));
    VKMR_TRY(hipStreamDestroy(S(s)));
    return VKMR_OK;
}

vkmr_status vkmr_hip_stream_sync(int dev, vkmr_stream s)
{
    VKMR_TRY(hipSetDevice(dev));
    VKMR_TRY(hipStreamSynchronize(S(s)));
    return VKMR_OK;
}

vkmr_status vkmr_hip_event_create(int dev, vkmr_event* out)
{
    if (!out) return refuse(__func__, "null out pointer");
    VKMR_TRY(hipSetDevice(dev));
    hipEvent_t e;
    VKMR_TRY(hipEventCreate(&e));
    *out = reinterpret_cast<vkmr_event>(e);
    return VKMR_OK;
}

vkmr_status vkmr_hip_event_destroy(int dev, vkmr_event e)
{
    if (!e) return VKMR_OK;
    VKMR_TRY(hipSetDevice(dev));
    VKMR_TRY(hipEventDestroy(E(e)));
    return VKMR_OK;
}

vkmr_status vkmr_hip_event_record(int dev, vkmr_event e, vkmr_stream s)
{
    if (!e) return refuse(__func__, "null event");
    VKMR_TRY(hipSetDevice(dev));
    VKMR_TRY(hipEventRecord(E(e), S(s)));
    return VKMR_OK;
}

vkmr_status vkmr_hip_event_query(int dev, vkmr_event e)
{
    if (!e) return refuse(__func__, "null event");
    VKMR_TRY(hipSetDevice(dev));
    hipError_t r = hipEventQuery(E(e));
    if (r == hipErrorNotReady) {
        (void)hipGetLastError();
        return VKMR_NOT_READY;
    }
    return from_hip(r, "hipEventQuery");
}

vkmr_status vkmr_hip_event_wait(int dev, vkmr_event e)
{
    if (!e) return refuse(__func__, "null event");
    VKMR_TRY(hipSetDevice(dev));
    VKMR_TRY(hipEventSynchronize(E(e)));
    return VKMR_OK;
}

vkmr_status vkmr_hip_stream_wait_event(int dev, vkmr_stream s, vkmr_event e)
{
    if (!e) return refuse(__func__, "null event");
    VKMR_TRY(hipSetDevice(dev));
    VKMR_TRY(hipStreamWaitEvent(S(s), E(e), 0));
    return VKMR_OK;
}

vkmr_status vkmr_hip_event_elapsed_ms(int dev, vkmr_event begin, vkmr_event end, float* ms)
{
    if (!begin || !end || !ms) return refuse(__func__, "null argument");
    VKMR_TRY(hipSetDevice(dev));
    VKMR_TRY(hipEventElapsedTime(ms, E(begin), E(end)));
    return VKMR_OK;
}

// ---- map ------------------------------------------------------------------------

// What the last vkmr_hip_map_async of this process chose (reported by vkmr_hip_kernel_info): a vkmr_map::Mode, or one of these.
enum { MAP_NONE = -1, MAP_EXPERIMENT = -2 };
static std::atomic<int> g_last_map_mode{MAP_NONE};       // diagnostics only; several host threads may drive different devices
static std::atomic<uint32_t> g_last_map_tile{0};

// The shipped fetch modes (csrc/map_kernel.hpp); which one a batch gets, and with which tile: map_plan.hpp.
// (spelled with every template argument: the names must read exactly as a profiler prints them, provenance.py)
#define VKMR_MAP_STAGED_KERNEL map_kernel<512, 1024, 17664, 0, false, 0>
#define VKMR_MAP_DIRECT512_KERNEL map_kernel<512, 2048, 64, 2, true, 0>
#define VKMR_MAP_DIRECT256_KERNEL map_kernel<256, 2048, 64, 2, true, 0>
#define VKMR_MAP_LONG512_KERNEL map_kernel<512, 2048, 64, 5, true, 0>
#define VKMR_MAP_LONG256_KERNEL map_kernel<256, 2048, 64, 5, true, 0>

using vkmr_map::direct_tile;
using vkmr_map::staged_tile;
using vkmr_map::tiles_of;

#ifdef VKMR_EXPERIMENTS
#include "map_experiments.hpp"   // tools build only: VKMR_MAP_VARIANT / _FIT / _TILE / _DYNLDS and the non-shipped instantiations
#endif

vkmr_status vkmr_hip_map_async(int dev, vkmr_stream s, const uint32_t* data_dev, uint64_t data_words,
                               const vkmr_metadata* meta_dev, uint32_t count, vkmr_digest* out_dev)
{
    if (count == 0) return VKMR_OK;
    if (!meta_dev || !out_dev || (!data_dev && data_words != 0)) return refuse(__func__, "null pointer");
    VKMR_TRY(hipSetDevice(dev));
    Node* out = nodes(out_dev);
#ifdef VKMR_EXPERIMENTS
    if (vkmr_map_experiment(S(s), data_dev, data_words, meta_dev, count, out, vkmr_map::avg_words(data_words, count))) {
        g_last_map_mode = MAP_EXPERIMENT;
        VKMR_TRY(hipGetLastError());
        return VKMR_OK;
    }
#endif
    const vkmr_map::Plan p = vkmr_map::plan(data_words, count);
    const dim3 grid(tiles_of(count, p.tile));
    g_last_map_mode = p.mode;
    g_last_map_tile = p.tile;
    switch (p.mode) {
        case vkmr_map::LONG512: return launch(VKMR_MAP_LONG512_KERNEL, grid, dim3(512), S(s), data_dev, data_words, meta_dev, count, out, p.tile);
        case vkmr_map::LONG256: return launch(VKMR_MAP_LONG256_KERNEL, grid, dim3(256), S(s), data_dev, data_words, meta_dev, count, out, p.tile);
        case vkmr_map::DIRECT512: return launch(VKMR_MAP_DIRECT512_KERNEL, grid, dim3(512), S(s), data_dev, data_words, meta_dev, count, out, p.tile);
        case vkmr_map::DIRECT256: return launch(VKMR_MAP_DIRECT256_KERNEL, grid, dim3(256), S(s), data_dev, data_words, meta_dev, count, out, p.tile);
        case vkmr_map::STAGED: break;
    }
    return launch(VKMR_MAP_STAGED_KERNEL, grid, dim3(512), S(s), data_dev, data_words, meta_dev, count, out, p.tile);
}

// ---- metadata from sizes (meta_kernels.hpp) ---------------------------------------------------------------------------
size_t vkmr_hip_sizes_scratch_bytes(uint32_t count)
{
    return ((size_t)(((uint64_t)count + VKMR_SIZES_BLOCK - 1) / VKMR_SIZES_BLOCK) + 1u) * sizeof(uint32_t);
}

vkmr_status vkmr_hip_metadata_from_sizes_async(int dev, vkmr_stream s, const uint16_t* sizes_dev, uint32_t count, uint32_t first_word,
                                               void* scratch_dev, vkmr_metadata* meta_dev)
{
    if (count == 0) return VKMR_OK;
    if (!sizes_dev || !scratch_dev || !meta_dev) return refuse(__func__, "null pointer");
    if ((reinterpret_cast<uintptr_t>(sizes_dev) & 15u) || (reinterpret_cast<uintptr_t>(meta_dev) & 15u))
        return refuse(__func__, "sizes and metadata must be 16-byte aligned");
    VKMR_TRY(hipSetDevice(dev));
    const uint32_t nblocks = (uint32_t)(((uint64_t)count + VKMR_SIZES_BLOCK - 1) / VKMR_SIZES_BLOCK);
    uint32_t* blocks = static_cast<uint32_t*>(scratch_dev);
    VKMR_CHECK(launch(sizes_block_words_kernel, dim3(nblocks), dim3(VKMR_SIZES_THREADS), S(s), sizes_dev, count, blocks));
    VKMR_CHECK(launch(sizes_block_starts_kernel, dim3(1), dim3(VKMR_SIZES_THREADS), S(s), blocks, nblocks, first_word));
    return launch(sizes_expand_kernel, dim3(nblocks), dim3(VKMR_SIZES_THREADS), S(s), sizes_dev, count, blocks, meta_dev);
}

#ifdef VKMR_EXPERIMENTS
// ---- text -> packed batch (split_kernels.hpp) ---------------------------------------------------------------------------
namespace {
struct SplitScratch { uint32_t *blk_count, *blk_after, *wblocks; vkmr_split::Line* lines; size_t bytes; };
SplitScratch split_scratch(void* base, uint32_t text_bytes, uint32_t meta_capacity)
{
    auto up = [](size_t n) { return (n + 255u) & ~(size_t)255u; };
    const size_t nb = ((size_t)text_bytes + VKMR_SPLIT_BLOCK - 1) / VKMR_SPLIT_BLOCK + 1, nwb = ((size_t)meta_capacity + VKMR_SIZES_BLOCK - 1) / VKMR_SIZES_BLOCK + 1;
    char* p = static_cast<char*>(base);
    SplitScratch sc;
    sc.blk_count = reinterpret_cast<uint32_t*>(p); p += up(nb * 4);
    sc.blk_after = reinterpret_cast<uint32_t*>(p); p += up(nb * 4);
    sc.wblocks = reinterpret_cast<uint32_t*>(p); p += up(nwb * 4);
    sc.lines = reinterpret_cast<vkmr_split::Line*>(p); p += up((size_t)meta_capacity * sizeof(vkmr_split::Line));
    sc.bytes = (size_t)(p - static_cast<char*>(base));
    return sc;
}
}  // namespace

size_t vkmr_hip_split_scratch_bytes(uint32_t text_bytes, uint32_t meta_capacity) { return split_scratch(nullptr, text_bytes, meta_capacity).bytes; }

vkmr_status vkmr_hip_split_text_async(int dev, vkmr_stream s, const uint8_t* text_dev, uint32_t text_bytes, void* scratch_dev, uint32_t* data_dev,
                                      uint64_t data_capacity_words, vkmr_metadata* meta_dev, uint32_t meta_capacity, uint32_t* result_dev)
{
    if (!result_dev) return refuse(__func__, "null result pointer");
    VKMR_TRY(hipSetDevice(dev));
    VKMR_TRY(hipMemsetAsync(result_dev, 0, 3 * sizeof(uint32_t), S(s)));
    if (text_bytes == 0) return VKMR_OK;
    if (!text_dev || !scratch_dev || !data_dev || !meta_dev || meta_capacity == 0)
        return refuse(__func__, "null pointer");
    if ((reinterpret_cast<uintptr_t>(text_dev) & 15u) || text_bytes > 0xFFFFFFE0u)
        return refuse(__func__, "the text must be 16-byte aligned and shorter than 4 GiB");
    const SplitScratch sc = split_scratch(scratch_dev, text_bytes, meta_capacity);
    const uint32_t nb = (uint32_t)(((uint64_t)text_bytes + VKMR_SPLIT_BLOCK - 1) / VKMR_SPLIT_BLOCK);
    const uint32_t nwb = (uint32_t)(((uint64_t)meta_capacity + VKMR_SIZES_BLOCK - 1) / VKMR_SIZES_BLOCK);
    const dim3 text_grid(nb), text_block(VKMR_SPLIT_THREADS), lines_grid(nwb), lines_block(VKMR_SIZES_THREADS);
    VKMR_CHECK(launch(split_count_kernel, text_grid, text_block, S(s), text_dev, text_bytes, sc.blk_count, sc.blk_after));
    VKMR_CHECK(launch(split_scan_kernel, dim3(1), text_block, S(s), sc.blk_count, sc.blk_after, nb, result_dev));
    VKMR_CHECK(launch(split_lines_kernel, text_grid, text_block, S(s), text_dev, text_bytes, sc.blk_count, sc.blk_after, sc.lines, meta_capacity, result_dev));
    VKMR_CHECK(launch(split_block_words_kernel, lines_grid, lines_block, S(s), sc.lines, result_dev, meta_capacity, sc.wblocks));
    VKMR_CHECK(launch(sizes_block_starts_kernel, dim3(1), lines_block, S(s), sc.wblocks, nwb, 0));
    VKMR_CHECK(launch(split_expand_kernel, lines_grid, lines_block, S(s), sc.lines, result_dev, meta_capacity, sc.wblocks, meta_dev));
    return launch(split_pack_kernel, dim3((meta_capacity + 255u) / 256u), dim3(256), S(s), text_dev, sc.lines, meta_dev, result_dev, meta_capacity, data_dev, data_capacity_words);
}
#endif   // VKMR_EXPERIMENTS

// See the header: the first copy and the first launch of a process, taken out of the caller's pipeline.
vkmr_status vkmr_hip_warm_up(int dev, vkmr_stream s, unsigned what, size_t copy_bytes)
{
    VKMR_TRY(hipSetDevice(dev));
    if (!(what & (VKMR_WARM_KERNELS | VKMR_WARM_COPY))) return VKMR_OK;
    // one pinned and one device block, of 256 bytes at least: metadata {word 0, 4 bytes} at 0, the string's word at 64, its digest at 128
    const size_t bytes = (what & VKMR_WARM_COPY) && copy_bytes > 256 ? copy_bytes : 256;
    void *h = nullptr, *d = nullptr;
    hipError_t e = hipHostMalloc(&h, bytes, hipHostMallocDefault);
    if (e == hipSuccess) e = hipMalloc(&d, bytes);
    if (e == hipSuccess) {
        memset(h, 0, 256);
        static_cast<uint32_t*>(h)[1] = 4u;
        if (what & VKMR_WARM_COPY) e = hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, S(s));
        else e = hipMemsetAsync(d, 0, 256, S(s));
    }
    vkmr_status launched = VKMR_OK;
    if (e == hipSuccess && (what & VKMR_WARM_KERNELS))
        launched = launch(VKMR_MAP_STAGED_KERNEL, dim3(1), dim3(512), S(s), static_cast<const uint32_t*>(d) + 16, 1, static_cast<const vkmr_metadata*>(d), 1,
                          nodes(d) + 4, 1024);
    if (e == hipSuccess && launched == VKMR_OK) e = hipStreamSynchronize(S(s));
    if (d) (void)hipFree(d);
    if (h) (void)hipHostFree(h);
    VKMR_CHECK(launched);
    VKMR_TRY(e);
    return VKMR_OK;
}

#define VKMR_STR2(x) #x
#define VKMR_STR(x) VKMR_STR2(x)
const char* vkmr_hip_kernel_info(void)
{
    static thread_local char buf[512];
    const char* map = "map=(no launch yet; staged: " VKMR_STR((VKMR_MAP_STAGED_KERNEL)) ")";
    switch (g_last_map_mode.load()) {
        case vkmr_map::STAGED: map = "map=" VKMR_STR((VKMR_MAP_STAGED_KERNEL)) " LDS-staged tiles sorted by block count"; break;
        case vkmr_map::DIRECT512: map = "map=" VKMR_STR((VKMR_MAP_DIRECT512_KERNEL)) " per-lane 16-byte loads"; break;
        case vkmr_map::DIRECT256: map = "map=" VKMR_STR((VKMR_MAP_DIRECT256_KERNEL)) " per-lane 16-byte loads, short launch"; break;
        case vkmr_map::LONG512: map = "map=" VKMR_STR((VKMR_MAP_LONG512_KERNEL)) " per-lane 16-byte loads, two blocks per trip"; break;
        case vkmr_map::LONG256: map = "map=" VKMR_STR((VKMR_MAP_LONG256_KERNEL)) " per-lane 16-byte loads, two blocks per trip, short launch"; break;
#ifdef VKMR_EXPERIMENTS
        case MAP_EXPERIMENT: map = "map=EXPERIMENT (VKMR_MAP_VARIANT; not a product build)"; break;
#endif
        default: break;
    }
#ifndef VKMR_BUILD_ID
#define VKMR_BUILD_ID "unknown"
#endif
    snprintf(buf, sizeof buf, "%s tile=%u reduce=reduce_pass_kernel(m<=%d)+reduce_collapse_kernel+reduce_tail_kernel(<=%d nodes) build=" VKMR_BUILD_ID, map,
             g_last_map_tile.load(), VKMR_PASS_MAXM, VKMR_TAIL_MAX);
    return buf;
}

// ---- reduce ---------------------------------------------------------------------

using vkmr_plan::ceil_shift;
using vkmr_plan::next_step;
typedef vkmr_plan::Step ReduceStep;
using vkmr_plan::STEP_BULK;
using vkmr_plan::STEP_COLLAPSE;
using vkmr_plan::STEP_TAIL;

using vkmr_plan::height_ok;

size_t vkmr_hip_reduce_scratch_bytes(uint64_t count)
{
    // ping-pong: outputs of step 1 and step 2 (later steps are smaller), for ANY run of at
    // most `count` nodes -- see vkmr_plan::cells_upper_bound
    return (size_t)vkmr_plan::cells_upper_bound(count, 1) * sizeof(vkmr_digest);
}

// Reduces `nslices` slices (n_full nodes each, the last n_last) through `height`
// levels each; slice k's root goes to roots[k].  The step sequence is that of a full
// slice; a shorter last slice rides along (its surplus wavefronts exit at once).
static vkmr_status reduce_launch(const char* who, hipStream_t stream, const Node* digests, uint32_t nslices, uint64_t n_full, uint64_t n_last,
                                 uint32_t height, Node* scratch, Node* roots, const ProofArgs* proofs = nullptr)
{
    const Node* in = digests;
    uint64_t n = n_full, nl = n_last, in_stride = n_full;
    uint32_t left = height;
    Node* bufA = scratch;
    Node* bufB = nullptr;
    const bool prove = proofs && proofs->k > 0;   // the kernels that also write the siblings of the proofs' path nodes (reduce_kernels.hpp)
    for (int pass = 0;; ++pass) {
        const ReduceStep st = next_step(n, left, nslices);
        const uint32_t level0 = height - left;     // tree level of this launch's input nodes
        SliceGeom g;
        g.n_full = n; g.n_last = nl; g.in_stride = in_stride; g.nslices = nslices;
        if (st.kind == STEP_TAIL) {
            g.out_stride = 1;
            if (prove) return launch(reduce_tail_proofs_kernel, dim3(1, nslices), dim3(64), stream, in, g, left, roots, *proofs, level0);
            return launch(reduce_tail_kernel, dim3(1, nslices), dim3(64), stream, in, g, left, roots);
        }
        Node* out;
        if (pass == 0) {
            out = bufA;
            bufB = bufA + st.n_out * nslices;
        } else {
            out = (pass & 1) ? bufB : bufA;
        }
        g.out_stride = st.n_out;
        if (st.kind == STEP_BULK) {
            const uint32_t m = st.levels - 1u;
            const uint64_t waves = ceil_shift(n, 7 + m);
            const uint64_t grid = (waves + VKMR_PASS_WAVES - 1) / VKMR_PASS_WAVES;
            if (grid_too_large(grid)) return refuse(who, "slice too large");
            const dim3 pgrid((uint32_t)grid, nslices), pblock(VKMR_PASS_WAVES * 64);
            VKMR_CHECK(prove ? launch(reduce_pass_proofs_kernel, pgrid, pblock, stream, in, g, out, m, *proofs, level0)
                             : launch(reduce_pass_kernel, pgrid, pblock, stream, in, g, out, m));
        } else {
            const uint64_t cwaves = ceil_shift(n, 7);
            const dim3 cgrid((uint32_t)((cwaves + VKMR_COLLAPSE_WAVES - 1) / VKMR_COLLAPSE_WAVES), nslices);
            const dim3 cblock(VKMR_COLLAPSE_WAVES * 64);
            VKMR_CHECK(prove ? launch(reduce_collapse_proofs_kernel, cgrid, cblock, stream, in, g, st.levels, out, *proofs, level0)
                             : launch(reduce_collapse_kernel, cgrid, cblock, stream, in, g, st.levels, out));
        }
        in = out;
        in_stride = st.n_out;
        n = st.n_out;
        nl = ceil_shift(nl, st.levels);
        left -= st.levels;
    }
}

vkmr_status vkmr_hip_reduce_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev, uint64_t count,
                                  uint32_t height, void* scratch_dev, vkmr_digest* root_dev)
{
    if (!digests_dev || !root_dev) return refuse(__func__, "null pointer");
    if (!height_ok(count, height))
        return refuse(__func__, "height does not reduce count to one node");
    if (count > VKMR_TAIL_MAX && !scratch_dev) return refuse(__func__, "null scratch");
    VKMR_TRY(hipSetDevice(dev));
    return reduce_launch(__func__, S(s), nodes(digests_dev), 1, count, count, height, nodes(scratch_dev), nodes(root_dev));
}

// ---- proof ----------------------------------------------------------------------

vkmr_status vkmr_hip_proof_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev, uint64_t count, uint32_t height,
                                 uint64_t index, void* scratch_dev, vkmr_digest* siblings_dev, vkmr_digest* root_dev)
{
    if (!digests_dev || !siblings_dev) return refuse(__func__, "null pointer");
    if (!height_ok(count, height)) return refuse(__func__, "height does not reduce count to one node");
    if (index >= count) return refuse(__func__, "index out of range");
    if (count > VKMR_TAIL_MAX && !scratch_dev) return refuse(__func__, "null scratch");
    VKMR_TRY(hipSetDevice(dev));
    const Node* leaves = nodes(digests_dev);
    Node* sib = nodes(siblings_dev);
    for (uint32_t l = 0; l < height; ++l) {
        // level l has cl nodes; q is the partner of the path node (or the path node itself at the ragged right edge)
        const uint64_t cl = (l >= 64) ? 1 : ceil_shift(count, l);
        const uint64_t q = vkmr_math::sibling((l >= 64) ? 0 : (index >> l), cl);
        // node q of level l = root of the sub-tree over leaves [q * 2^l, min((q + 1) * 2^l, count)), l levels
        const uint64_t lo = (l >= 64) ? 0 : (q << l);
        uint64_t n = (l >= 63) ? count - lo : ((count - lo < (1ull << l)) ? count - lo : (1ull << l));
        if (l == 0) {
            VKMR_TRY(hipMemcpyAsync(sib, leaves + lo, sizeof(Node), hipMemcpyDeviceToDevice, S(s)));
        } else {
            VKMR_CHECK(reduce_launch(__func__, S(s), leaves + lo, 1, n, n, l, nodes(scratch_dev), sib + l));
        }
    }
    if (root_dev)
        return reduce_launch(__func__, S(s), leaves, 1, count, count, height, nodes(scratch_dev), nodes(root_dev));
    return VKMR_OK;
}

// The reduction of vkmr_hip_reduce_async that ALSO writes the Merkle proofs of `k` leaves while it runs (the reference's to-do,
// README.md:118-120): siblings_dev[q * height + l] = the sibling of leaf indices[q]'s path node at level l.  Same launches, same
// root, no extra hash (reduce_kernels.hpp: note_siblings); vkmr_hip_proof_async stays as the independent cross-check.
vkmr_status vkmr_hip_reduce_proofs_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev, uint64_t count, uint32_t height, void* scratch_dev,
                                         vkmr_digest* root_dev, const uint64_t* indices, uint32_t k, vkmr_digest* siblings_dev)
{
    if (k == 0) return vkmr_hip_reduce_async(dev, s, digests_dev, count, height, scratch_dev, root_dev);
    if (!digests_dev || !root_dev || !indices || !siblings_dev) return refuse(__func__, "null pointer");
    if (k > VKMR_MAX_PROOFS) return refuse(__func__, "more than 16 proofs in one reduction");
    if (!height_ok(count, height)) return refuse(__func__, "height does not reduce count to one node");
    if (count > VKMR_TAIL_MAX && !scratch_dev) return refuse(__func__, "null scratch");
    ProofArgs pa;
    pa.k = k;
    pa.height = height;
    pa.sib = nodes(siblings_dev);
    for (uint32_t q = 0; q < VKMR_MAX_PROOFS; ++q) pa.index[q] = 0;
    for (uint32_t q = 0; q < k; ++q) {
        if (indices[q] >= count) return refuse(__func__, "index out of range");
        pa.index[q] = indices[q];
    }
    VKMR_TRY(hipSetDevice(dev));
    if (height == 0) {   // one node, no level: the root is the node (reduce_tail_kernel), no sibling exists
        return reduce_launch(__func__, S(s), nodes(digests_dev), 1, count, count, height, nodes(scratch_dev), nodes(root_dev));
    }
    return reduce_launch(__func__, S(s), nodes(digests_dev), 1, count, count, height, nodes(scratch_dev), nodes(root_dev), &pa);
}

vkmr_status vkmr_hip_reduce_slices_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev, uint32_t nslices,
                                         uint64_t capacity, uint64_t count_last, uint32_t height, void* scratch_dev,
                                         vkmr_digest* roots_dev)
{
    if (!digests_dev || !roots_dev || nslices == 0) return refuse(__func__, "bad argument");
    if (count_last == 0 || count_last > capacity)
        return refuse(__func__, "bad slice geometry");
    if (!height_ok(nslices == 1 ? count_last : capacity, height))
        return refuse(__func__, "height does not reduce a slice to one node");
    if (capacity > VKMR_TAIL_MAX && !scratch_dev) return refuse(__func__, "null scratch");
    VKMR_TRY(hipSetDevice(dev));
    const vkmr_plan::SliceChunks chunks = vkmr_plan::slice_chunks(nslices);   // at most 32768 slices per launch sequence
    const Node* digests = nodes(digests_dev);
    Node* roots = nodes(roots_dev);
    const uint64_t n_full = (nslices == 1) ? count_last : capacity;
    for (uint32_t c = 0; c < chunks.count(); ++c) {
        const uint32_t first = chunks.first(c);
        const bool has_last = (c + 1 == chunks.count());
        VKMR_CHECK(reduce_launch(__func__, S(s), digests + (uint64_t)first * capacity, chunks.size(c), n_full, has_last ? count_last : capacity, height,
                                 nodes(scratch_dev), roots + first));
    }
    return VKMR_OK;
}

size_t vkmr_hip_reduce_slices_scratch_bytes(uint64_t capacity, uint32_t nslices)
{
    return (size_t)vkmr_plan::slices_scratch_cells(capacity, nslices) * sizeof(vkmr_digest);
}

size_t vkmr_hip_reduce_levels_scratch_bytes(uint64_t count)
{
    return (size_t)vkmr_plan::levels_scratch_cells(count) * sizeof(vkmr_digest);
}

// Level lv + 1 from level lv, lv = 0..height-1, one reduce_level_kernel launch each; dst(lv) is where level lv + 1 goes.
// Shared by the levels cross-check (ping-pong scratch, root last) and the stored tree (every level kept).
extern "C++" {   // a template inside the C block
template <class Dst>
static vkmr_status levels_launch(const char* who, hipStream_t stream, const Node* in, uint64_t count, uint32_t height, Dst dst)
{
    uint64_t n = count;
    for (uint32_t lv = 0; lv < height; ++lv) {
        const uint64_t pairs = ceil_shift(n, 1);
        Node* out = dst(lv);
        if (grid_too_large(groups_of(pairs))) return refuse(who, "slice too large");
        VKMR_CHECK(launch(reduce_level_kernel, grid_of(pairs), dim3(256), stream, in, n, out));
        in = out;
        n = pairs;
    }
    return VKMR_OK;
}
}

vkmr_status vkmr_hip_reduce_levels_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev, uint64_t count,
                                         uint32_t height, void* scratch_dev, vkmr_digest* root_dev)
{
    if (!digests_dev || !root_dev || !scratch_dev)
        return refuse(__func__, "null pointer");
    if (!height_ok(count, height))
        return refuse(__func__, "height does not reduce count to one node");
    VKMR_TRY(hipSetDevice(dev));
    Node* bufA = nodes(scratch_dev);
    Node* bufB = bufA + vkmr_plan::levels_second_buffer(count);
    Node* root = nodes(root_dev);
    VKMR_CHECK(levels_launch(__func__, S(s), nodes(digests_dev), count, height,
                             [=](uint32_t lv) { return (lv + 1 == height) ? root : ((lv & 1) ? bufB : bufA); }));
    if (height == 0) VKMR_TRY(hipMemcpyAsync(root_dev, digests_dev, sizeof(vkmr_digest), hipMemcpyDeviceToDevice, S(s)));
    return VKMR_OK;
}

// ---- stored tree: build, gather proofs, verify (tree_kernels.hpp) -------------------------------------------------------

// Start cell of every level 1..height inside the tree buffer, as the kernels take it (tree_plan.hpp).
static TreeLevels tree_levels(uint64_t count, uint32_t height)
{
    TreeLevels lv;
    vkmr_tree::levels(count, height, lv.off);
    return lv;
}

size_t vkmr_hip_tree_bytes(uint64_t count, uint32_t height)
{
    if (count == 0 || height > 63) return 0;
    return (size_t)vkmr_tree::cells(count, height) * sizeof(vkmr_digest);
}

vkmr_status vkmr_hip_reduce_tree_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev, uint64_t count, uint32_t height,
                                       vkmr_digest* tree_dev)
{
    if (!digests_dev || (!tree_dev && height > 0)) return refuse(__func__, "null pointer");
    if (!height_ok(count, height))
        return refuse(__func__, "height does not reduce count to one node");
    if (height == 0) return VKMR_OK;   // one leaf, no level: the root is the leaf
    const TreeLevels lv = tree_levels(count, height);
    VKMR_TRY(hipSetDevice(dev));
    Node* tree = nodes(tree_dev);
    return levels_launch(__func__, S(s), nodes(digests_dev), count, height, [&](uint32_t l) { return tree + lv.off[l + 1]; });
}

vkmr_status vkmr_hip_tree_proofs_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev, const vkmr_digest* tree_dev, uint64_t count,
                                       uint32_t height, const uint64_t* indices_dev, uint32_t k, vkmr_digest* siblings_dev)
{
    if (k == 0) return VKMR_OK;
    if (!digests_dev || (!tree_dev && height > 0) || !indices_dev || !siblings_dev)
        return refuse(__func__, "null pointer");
    if (!height_ok(count, height))
        return refuse(__func__, "height does not reduce count to one node");
    if (height == 0) return VKMR_OK;   // no level, no sibling
    const TreeLevels lv = tree_levels(count, height);
    const uint64_t total = (uint64_t)k * height;
    if (grid_too_large(groups_of(total))) return refuse(__func__, "too many proofs in one call");
    VKMR_TRY(hipSetDevice(dev));
    return launch(tree_proofs_kernel, grid_of(total), dim3(256), S(s), nodes(digests_dev), nodes(tree_dev), lv, count, height, indices_dev, total,
                  nodes(siblings_dev));
}

vkmr_status vkmr_hip_verify_proofs_async(int dev, vkmr_stream s, const vkmr_digest* leaves_dev, const uint64_t* indices_dev,
                                         const vkmr_digest* siblings_dev, uint32_t k, uint32_t height, const vkmr_digest* roots_dev,
                                         uint32_t nroots, uint32_t* ok_dev)
{
    if (k == 0) return VKMR_OK;
    if (!leaves_dev || !indices_dev || !siblings_dev || !roots_dev || !ok_dev)
        return refuse(__func__, "null pointer");
    if (height == 0 || height > 63) return refuse(__func__, "height must be 1..63");
    if (nroots != 1 && nroots != k) return refuse(__func__, "nroots must be 1 or k");
    VKMR_TRY(hipSetDevice(dev));
    return launch(verify_proofs_kernel, grid_of(k), dim3(256), S(s), nodes(leaves_dev), indices_dev, nodes(siblings_dev), k, height, nodes(roots_dev),
                  nroots == 1 ? 0 : 1, ok_dev);
}

vkmr_status vkmr_hip_tree_update_async(int dev, vkmr_stream s, vkmr_digest* digests_dev, vkmr_digest* tree_dev, uint64_t count,
                                       uint32_t height, const uint64_t* indices_dev, const vkmr_digest* leaves_dev, uint32_t k,
                                       uint32_t* status_dev)
{
    if (k == 0) return VKMR_OK;
    if (!digests_dev || (!tree_dev && height > 0) || !indices_dev || !leaves_dev || !status_dev)
        return refuse(__func__, "null pointer");
    if (!height_ok(count, height))
        return refuse(__func__, "height does not reduce count to one node");
    const TreeLevels lv = tree_levels(count, height);
    const dim3 grid = grid_of(k);
    Node* digests = nodes(digests_dev);
    Node* tree = nodes(tree_dev);
    VKMR_TRY(hipSetDevice(dev));
    VKMR_TRY(hipMemsetAsync(status_dev, 0, sizeof(uint32_t), S(s)));
    VKMR_CHECK(launch(tree_update_check_kernel, grid, dim3(256), S(s), indices_dev, k, count, status_dev));
    VKMR_CHECK(launch(tree_update_leaves_kernel, grid, dim3(256), S(s), digests, indices_dev, nodes(leaves_dev), k, status_dev));
    for (uint32_t l = 1; l <= height; ++l) {   // level l from level l - 1, which the previous launch finished
        const Node* in = (l == 1) ? digests : tree + lv.off[l - 1];
        VKMR_CHECK(launch(tree_update_level_kernel, grid, dim3(256), S(s), in, ceil_shift(count, l - 1), tree + lv.off[l], indices_dev, k, l, status_dev));
    }
    return VKMR_OK;
}

// ---- multiproofs: one proof for k leaves of one stored tree (tree_kernels.hpp) ----------------------------------------------

size_t vkmr_hip_multiproof_max_nodes(uint64_t count, uint32_t height, uint32_t k)
{
    if (count == 0 || height > 63) return 0;
    return (size_t)vkmr_tree::multiproof_max_nodes(count, height, k);
}

using vkmr_tree::MultiproofLayout;
using vkmr_tree::multiproof_layout;
static_assert(sizeof(vkmr_digest) == vkmr_tree::CELL_BYTES && sizeof(Node) == vkmr_tree::CELL_BYTES, "tree_plan.hpp counts cells of 32 bytes");

size_t vkmr_hip_multiproof_scratch_bytes(uint32_t k, uint32_t height)
{
    if (k == 0 || height > 63) return 0;
    return multiproof_layout(k, height).bytes;
}

// The parts of a multiproof call's scratch_dev as the kernels take them.  (Integer arithmetic: a tree of one leaf has no
// scratch, and none of these is then used.)
struct MultiproofScratch {
    Node* cell;
    uint64_t *mask, *word_start, *block, *hdr;
    uint32_t* end;
    MultiproofScratch(void* scratch_dev, const MultiproofLayout& L)
    {
        const uintptr_t at = reinterpret_cast<uintptr_t>(scratch_dev);
        cell = reinterpret_cast<Node*>(at + L.cell);
        mask = reinterpret_cast<uint64_t*>(at + L.mask);
        word_start = reinterpret_cast<uint64_t*>(at + L.word_start);
        block = reinterpret_cast<uint64_t*>(at + L.block);
        hdr = reinterpret_cast<uint64_t*>(at + L.hdr);
        end = reinterpret_cast<uint32_t*>(at + L.end);
    }
};

// The ranking launches every multiproof call shares, behind its own check and masks kernel: block sums, block starts, word
// starts.  `levels` is one tree's height or a forest's stride; limit / exact as multiproof_block_starts_kernel takes them.
// `hdr` is the call's header: the caller's info_dev in a gather, the scratch's own in a verification.
static vkmr_status multiproof_rank_launch(hipStream_t stream, uint32_t levels, const MultiproofLayout& L, const MultiproofScratch& sc, uint64_t* hdr,
                                          uint64_t limit, uint32_t exact)
{
    const dim3 wgrid((uint32_t)L.blocks, levels), wblock(VKMR_MP_BLOCK_WORDS);
    VKMR_CHECK(launch(multiproof_block_sums_kernel, wgrid, wblock, stream, sc.mask, L.words, L.blocks, sc.block));
    VKMR_CHECK(launch(multiproof_block_starts_kernel, dim3(1), dim3(256), stream, sc.block, L.blocks, levels, limit, exact, hdr));
    return launch(multiproof_word_starts_kernel, wgrid, wblock, stream, sc.mask, L.words, L.blocks, sc.block, hdr, sc.word_start);
}

// The single tree's check and flags in front of the ranking: the index check into hdr[0] with `count` as its bound, then the
// masks.  A tree of one leaf (height 0) has no level to rank: the check alone, and M = 0.
static vkmr_status tree_multiproof_rank_launch(hipStream_t stream, const uint64_t* indices_dev, uint32_t k, uint64_t count, uint32_t height,
                                               const MultiproofLayout& L, const MultiproofScratch& sc, uint64_t* hdr, uint64_t limit, uint32_t exact)
{
    VKMR_TRY(hipMemsetAsync(hdr, 0, (height == 0 ? 2 : 1) * sizeof(uint64_t), stream));
    VKMR_CHECK(launch(tree_update_check_kernel, grid_of(k), dim3(256), stream, indices_dev, k, count, reinterpret_cast<uint32_t*>(hdr)));
    if (height == 0) return VKMR_OK;
    VKMR_CHECK(launch(multiproof_masks_kernel, grid_of(k), dim3(256), stream, indices_dev, k, height, L.words, hdr, sc.mask));
    return multiproof_rank_launch(stream, height, L, sc, hdr, limit, exact);
}

vkmr_status vkmr_hip_tree_multiproof_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev, const vkmr_digest* tree_dev, uint64_t count,
                                           uint32_t height, const uint64_t* indices_dev, uint32_t k, void* scratch_dev, vkmr_digest* nodes_dev,
                                           uint64_t nodes_capacity, uint64_t* info_dev)
{
    if (k == 0) return VKMR_OK;
    if (!digests_dev || !indices_dev || !info_dev || (height > 0 && (!tree_dev || !scratch_dev)) || (!nodes_dev && nodes_capacity > 0))
        return refuse(__func__, "null pointer");
    if (!height_ok(count, height)) return refuse(__func__, "height does not reduce count to one node");
    const TreeLevels lv = tree_levels(count, height);
    const MultiproofLayout L = multiproof_layout(k, height);
    const MultiproofScratch sc(scratch_dev, L);
    VKMR_TRY(hipSetDevice(dev));
    VKMR_CHECK(tree_multiproof_rank_launch(S(s), indices_dev, k, count, height, L, sc, info_dev, nodes_capacity, 0u));
    if (height == 0) return VKMR_OK;
    return launch(tree_multiproof_gather_kernel, grid_of(k, height), dim3(256), S(s), nodes(digests_dev), nodes(tree_dev), lv, count, indices_dev, k, L.words,
                  sc.mask, sc.word_start, info_dev, nodes(nodes_dev));
}

vkmr_status vkmr_hip_verify_multiproof_async(int dev, vkmr_stream s, const vkmr_digest* leaves_dev, const uint64_t* indices_dev, uint32_t k,
                                             uint32_t height, const vkmr_digest* nodes_dev, uint64_t m, const vkmr_digest* root_dev,
                                             void* scratch_dev, uint32_t* ok_dev)
{
    if (k == 0) return VKMR_OK;
    if (!leaves_dev || !indices_dev || !root_dev || !scratch_dev || !ok_dev || (!nodes_dev && m > 0)) return refuse(__func__, "null pointer");
    if (height == 0 || height > 63) return refuse(__func__, "height must be 1..63");
    const MultiproofLayout L = multiproof_layout(k, height);
    const MultiproofScratch sc(scratch_dev, L);
    VKMR_TRY(hipSetDevice(dev));
    // the index check with 2^height as the bound: bit 0 an index outside the tree, bit 1 not strictly increasing; exact: M == m
    VKMR_CHECK(tree_multiproof_rank_launch(S(s), indices_dev, k, 1ull << height, height, L, sc, sc.hdr, m, 1u));
    const dim3 grid = grid_of(k);
    for (uint32_t l = 0; l < height; ++l)   // level l + 1 from level l, which the previous launch finished
        VKMR_CHECK(launch(verify_multiproof_level_kernel, grid, dim3(256), S(s), l == 0 ? nodes(leaves_dev) : sc.cell, sc.cell, sc.end, indices_dev, k, l,
                          L.words, sc.mask, sc.word_start, nodes(nodes_dev), sc.hdr));
    return launch(verify_multiproof_finish_kernel, dim3(1), dim3(64), S(s), sc.cell, nodes(root_dev), sc.hdr, ok_dev);
}

// ---- applying a multiproof: the new root from the old root, the old and the new leaves (tree_kernels.hpp) ------------------

using vkmr_tree::ApplyLayout;
using vkmr_tree::apply_layout;

size_t vkmr_hip_apply_multiproof_scratch_bytes(uint32_t k, uint32_t levels)
{
    if (k == 0 || levels > 63) return 0;
    return apply_layout(k, levels).bytes;
}

// What an apply call's scratch_dev holds behind the verifier's parts: side 1's cells and ends, the derived heights.
struct ApplyScratch {
    MultiproofScratch mp;
    Node* cell1;
    uint32_t *end1, *heights;
    ApplyScratch(void* scratch_dev, const ApplyLayout& A) : mp(scratch_dev, A.mp)
    {
        const uintptr_t at = reinterpret_cast<uintptr_t>(scratch_dev);
        cell1 = reinterpret_cast<Node*>(at + A.cell1);
        end1 = reinterpret_cast<uint32_t*>(at + A.end1);
        heights = reinterpret_cast<uint32_t*>(at + A.heights);
    }
};

vkmr_status vkmr_hip_apply_multiproof_async(int dev, vkmr_stream s, const vkmr_digest* old_leaves_dev, const vkmr_digest* new_leaves_dev,
                                            const uint64_t* indices_dev, uint32_t k, uint64_t count, uint32_t height, const vkmr_digest* nodes_dev,
                                            uint64_t m, const vkmr_digest* root_dev, void* scratch_dev, uint32_t* ok_dev, vkmr_digest* new_root_dev)
{
    if (k == 0) return VKMR_OK;
    if (!old_leaves_dev || !new_leaves_dev || !indices_dev || !root_dev || !scratch_dev || !ok_dev || !new_root_dev || (!nodes_dev && m > 0))
        return refuse(__func__, "null pointer");
    if (height == 0 || height > 63) return refuse(__func__, "height must be 1..63");
    if (reinterpret_cast<uintptr_t>(scratch_dev) & 15u) return refuse(__func__, "scratch must be 16-byte aligned");
    const ApplyLayout A = apply_layout(k, height);
    const ApplyScratch sc(scratch_dev, A);
    VKMR_TRY(hipSetDevice(dev));
    // the verifier's check with the count as the bound: bit 0 an index that is no leaf.  A count of 0 has no leaf, and one
    // above 2^height is none this height can hold: the bound 0 refuses every index.  exact: M == m
    const uint64_t bound = count <= (1ull << height) ? count : 0ull;
    VKMR_CHECK(tree_multiproof_rank_launch(S(s), indices_dev, k, bound, height, A.mp, sc.mp, sc.mp.hdr, m, 1u));
    const dim3 grid = grid_of(k, 2);
    for (uint32_t l = 0; l < height; ++l)   // level l + 1 from level l on both sides, which the previous launch finished
        VKMR_CHECK(launch(tree_apply_level_kernel, grid, dim3(256), S(s), l == 0 ? nodes(old_leaves_dev) : sc.mp.cell,
                          l == 0 ? nodes(new_leaves_dev) : sc.cell1, sc.mp.cell, sc.cell1, sc.mp.end, sc.end1, indices_dev, count, k, l, A.mp.words,
                          sc.mp.mask, sc.mp.word_start, nodes(nodes_dev), sc.mp.hdr));
    VKMR_CHECK(launch(verify_multiproof_finish_kernel, dim3(1), dim3(64), S(s), sc.mp.cell, nodes(root_dev), sc.mp.hdr, ok_dev));
    return launch(tree_apply_commit_kernel, dim3(1), dim3(64), S(s), sc.cell1, ok_dev, nodes(new_root_dev));
}

// ---- forest: the roots of many trees of unequal size (forest_kernels.hpp, forest_plan.hpp) ---------------------------------

size_t vkmr_hip_forest_scratch_bytes(uint64_t total, uint32_t ntrees)
{
    // two ping-pong level buffers: ((total >> 1) + ntrees) + ((total >> 2) + ntrees) cells -- vkmr_forest::scratch_cells
    return (size_t)vkmr_forest::scratch_cells(total, ntrees) * sizeof(vkmr_digest);
}

// The launches of the forest builds: the status word zeroed, the check, then level l from level l - 1 for l = 1 .. levels.
// level(l) is where level l >= 1 is kept: one of two alternating buffers (the roots alone are wanted) or a buffer of its own
// (the stored forest).  With mutated_dev (the flagged builds; null in the plain ones) the masks are zeroed in the same
// sequence and every level is forest_level_mutated_kernel's: the same launches, grids and buffers.
extern "C++" {   // a template inside the C block
template <class LevelBuffer>
static vkmr_status forest_launch(const char* who, int dev, vkmr_stream s, const vkmr_digest* digests_dev, uint64_t total, const uint64_t* offsets_dev,
                                 uint32_t ntrees, uint64_t max_count, const void* buffer_dev, vkmr_digest* roots_dev, uint64_t* mutated_dev,
                                 uint32_t* status_dev, LevelBuffer level)
{
    if ((!digests_dev && total > 0) || !offsets_dev || !buffer_dev || !roots_dev || !status_dev) return refuse(who, "null pointer");
    if (max_count == 0) return refuse(who, "max_count must be at least 1");
    if (reinterpret_cast<uintptr_t>(buffer_dev) & 15u) return refuse(who, "the level buffer must be 16-byte aligned");
    if (total > (1ull << 58) || grid_too_large(groups_of(vkmr_forest::level_cells(total, ntrees, 1)))) return refuse(who, "forest too large");
    if (max_count > total) max_count = total;
    const uint32_t levels = vkmr_forest::launches(total, max_count);
    const Node* digests = nodes(digests_dev);
    Node* roots = nodes(roots_dev);
    VKMR_TRY(hipSetDevice(dev));
    VKMR_TRY(hipMemsetAsync(status_dev, 0, sizeof(uint32_t), S(s)));
    if (mutated_dev) VKMR_TRY(hipMemsetAsync(mutated_dev, 0, sizeof(uint64_t) * ntrees, S(s)));
    VKMR_CHECK(launch(forest_check_kernel, grid_of(ntrees), dim3(256), S(s), offsets_dev, ntrees, total, max_count, status_dev));
    for (uint32_t l = 1; l <= levels; ++l) {   // level l from level l - 1, which the previous launch finished
        const Node* in = (l == 1) ? digests : level(l - 1);
        const uint64_t cells = vkmr_forest::level_cells(total, ntrees, l);
        VKMR_CHECK(mutated_dev ? launch(forest_level_mutated_kernel, grid_of(cells), dim3(256), S(s), in, offsets_dev, ntrees, l, cells, level(l), roots,
                                        reinterpret_cast<unsigned long long*>(mutated_dev), status_dev)
                               : launch(forest_level_kernel, grid_of(cells), dim3(256), S(s), in, offsets_dev, ntrees, l, cells, level(l), roots, status_dev));
    }
    return VKMR_OK;
}
}  // extern "C++"

vkmr_status vkmr_hip_reduce_forest_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev, uint64_t total, const uint64_t* offsets_dev,
                                         uint32_t ntrees, uint64_t max_count, void* scratch_dev, vkmr_digest* roots_dev, uint32_t* status_dev)
{
    if (ntrees == 0) return VKMR_OK;
    Node* scratch = nodes(scratch_dev);
    return forest_launch(__func__, dev, s, digests_dev, total, offsets_dev, ntrees, max_count, scratch_dev, roots_dev, nullptr,
                         status_dev, [&](uint32_t l) { return scratch + vkmr_forest::level_base(total, ntrees, l); });
}

vkmr_status vkmr_hip_reduce_forest_mutated_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev, uint64_t total, const uint64_t* offsets_dev,
                                                 uint32_t ntrees, uint64_t max_count, void* scratch_dev, vkmr_digest* roots_dev,
                                                 uint64_t* mutated_dev, uint32_t* status_dev)
{
    if (ntrees == 0) return VKMR_OK;
    if (!mutated_dev) return refuse(__func__, "null pointer");
    Node* scratch = nodes(scratch_dev);
    return forest_launch(__func__, dev, s, digests_dev, total, offsets_dev, ntrees, max_count, scratch_dev, roots_dev,
                         mutated_dev, status_dev, [&](uint32_t l) { return scratch + vkmr_forest::level_base(total, ntrees, l); });
}

// ---- stored forest: every level kept, proofs gathered from it, proofs of unequal height verified (forest_tree_kernels.hpp) ----

size_t vkmr_hip_forest_tree_bytes(uint64_t total, uint32_t ntrees, uint64_t max_count)
{
    if (ntrees == 0 || max_count == 0) return 0;
    return (size_t)vkmr_forest::stored_cells(total, ntrees, vkmr_forest::launches(total, max_count)) * sizeof(vkmr_digest);
}

vkmr_status vkmr_hip_reduce_forest_tree_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev, uint64_t total, const uint64_t* offsets_dev,
                                              uint32_t ntrees, uint64_t max_count, vkmr_digest* forest_dev, vkmr_digest* roots_dev,
                                              uint32_t* status_dev)
{
    if (ntrees == 0) return VKMR_OK;
    Node* forest = nodes(forest_dev);
    return forest_launch(__func__, dev, s, digests_dev, total, offsets_dev, ntrees, max_count, forest_dev, roots_dev,
                         nullptr, status_dev, [&](uint32_t l) { return forest + vkmr_forest::stored_level_base(total, ntrees, l); });
}

vkmr_status vkmr_hip_reduce_forest_tree_mutated_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev, uint64_t total,
                                                      const uint64_t* offsets_dev, uint32_t ntrees, uint64_t max_count, vkmr_digest* forest_dev,
                                                      vkmr_digest* roots_dev, uint64_t* mutated_dev, uint32_t* status_dev)
{
    if (ntrees == 0) return VKMR_OK;
    if (!mutated_dev) return refuse(__func__, "null pointer");
    Node* forest = nodes(forest_dev);
    return forest_launch(__func__, dev, s, digests_dev, total, offsets_dev, ntrees, max_count, forest_dev,
                         roots_dev, mutated_dev, status_dev, [&](uint32_t l) { return forest + vkmr_forest::stored_level_base(total, ntrees, l); });
}

// What the stored forest's entry points refuse alike, behind their null-pointer test, in the order each tests it: a forest
// without a leaf where the call needs one (`no_leaf` says why; null: an empty forest is fine), no max_count, too many leaves,
// scratch off the 16-byte grid (null: none to test), more entries than a launch takes.
static vkmr_status forest_args_check(const char* who, uint64_t total, uint32_t ntrees, uint64_t max_count, uint32_t k, const char* no_leaf,
                                     const void* scratch_dev)
{
    if (no_leaf && (ntrees == 0 || total == 0)) return refuse(who, no_leaf);
    if (max_count == 0) return refuse(who, "max_count must be at least 1");
    if (total > (1ull << 58)) return refuse(who, "forest too large");
    if (reinterpret_cast<uintptr_t>(scratch_dev) & 15u) return refuse(who, "scratch must be 16-byte aligned");
    if (grid_too_large(groups_of(k))) return refuse(who, "too many entries in one call");
    return VKMR_OK;
}

// First cell of the buffer of every level 1..H inside the stored forest (base[0] = 0, unused), as the kernels take it.
static ForestLevels forest_levels(uint64_t total, uint32_t ntrees, uint32_t H)
{
    ForestLevels lv;
    for (uint32_t l = 0; l < VKMR_TREE_MAX_LEVELS; ++l) lv.base[l] = (l >= 1 && l <= H) ? vkmr_forest::stored_level_base(total, ntrees, l) : 0;
    return lv;
}

// The masks of a stored forest, formed again from its levels as they are now (behind updates): the memset, then one launch per
// level with the build's grid; level l - 1 is read, nothing but the masks is written.
vkmr_status vkmr_hip_forest_tree_mutated_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev, const vkmr_digest* forest_dev, uint64_t total,
                                               const uint64_t* offsets_dev, uint32_t ntrees, uint64_t max_count, uint64_t* mutated_dev)
{
    if (ntrees == 0) return VKMR_OK;
    if ((!digests_dev && total > 0) || !forest_dev || !offsets_dev || !mutated_dev) return refuse(__func__, "null pointer");
    VKMR_CHECK(forest_args_check(__func__, total, ntrees, max_count, 0, nullptr, nullptr));
    if (grid_too_large(groups_of(vkmr_forest::level_cells(total, ntrees, 1)))) return refuse(__func__, "forest too large");
    const uint32_t H = vkmr_forest::launches(total, max_count);   // <= 58
    const Node* digests = nodes(digests_dev);
    const Node* forest = nodes(forest_dev);
    VKMR_TRY(hipSetDevice(dev));
    VKMR_TRY(hipMemsetAsync(mutated_dev, 0, sizeof(uint64_t) * ntrees, S(s)));
    for (uint32_t l = 1; l <= H; ++l) {
        const Node* in = (l == 1) ? digests : forest + vkmr_forest::stored_level_base(total, ntrees, l - 1);
        const uint64_t cells = vkmr_forest::level_cells(total, ntrees, l);
        VKMR_CHECK(launch(forest_scan_mutated_kernel, grid_of(cells), dim3(256), S(s), in, offsets_dev, ntrees, l, cells,
                          reinterpret_cast<unsigned long long*>(mutated_dev)));
    }
    return VKMR_OK;
}

vkmr_status vkmr_hip_forest_proofs_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev, const vkmr_digest* forest_dev, uint64_t total,
                                         const uint64_t* offsets_dev, uint32_t ntrees, uint64_t max_count, const uint32_t* trees_dev,
                                         const uint64_t* indices_dev, uint32_t k, vkmr_digest* siblings_dev, uint32_t* heights_dev)
{
    if (k == 0) return VKMR_OK;
    if ((!digests_dev && total > 0) || !forest_dev || !offsets_dev || !trees_dev || !indices_dev || !siblings_dev || !heights_dev)
        return refuse(__func__, "null pointer");
    VKMR_CHECK(forest_args_check(__func__, total, ntrees, max_count, k, nullptr, nullptr));
    const uint32_t H = vkmr_forest::launches(total, max_count);   // <= 58
    const ForestLevels lv = forest_levels(total, ntrees, H);
    const uint64_t cells = (uint64_t)k * H;
    if (grid_too_large(groups_of(cells))) return refuse(__func__, "too many proofs in one call");
    VKMR_TRY(hipSetDevice(dev));
    return launch(forest_proofs_kernel, grid_of(cells), dim3(256), S(s), nodes(digests_dev), nodes(forest_dev), lv, offsets_dev, ntrees, H, trees_dev,
                  indices_dev, cells, nodes(siblings_dev), heights_dev);
}

vkmr_status vkmr_hip_verify_forest_proofs_async(int dev, vkmr_stream s, const vkmr_digest* leaves_dev, const uint32_t* trees_dev,
                                                const uint64_t* indices_dev, const vkmr_digest* siblings_dev, const uint32_t* heights_dev,
                                                uint32_t k, uint32_t stride, const vkmr_digest* roots_dev, uint32_t ntrees, uint32_t* ok_dev)
{
    if (k == 0) return VKMR_OK;
    if (!leaves_dev || !trees_dev || !indices_dev || !siblings_dev || !heights_dev || !roots_dev || !ok_dev)
        return refuse(__func__, "null pointer");
    if (stride == 0 || stride > 63) return refuse(__func__, "stride must be 1..63");
    VKMR_TRY(hipSetDevice(dev));
    return launch(verify_forest_proofs_kernel, grid_of(k), dim3(256), S(s), nodes(leaves_dev), trees_dev, indices_dev, nodes(siblings_dev), heights_dev, k,
                  stride, nodes(roots_dev), ntrees, ok_dev);
}

// ---- leaf updates of the stored forest (forest_tree_kernels.hpp) -----------------------------------------------------------

vkmr_status vkmr_hip_forest_update_async(int dev, vkmr_stream s, vkmr_digest* digests_dev, vkmr_digest* forest_dev, uint64_t total,
                                         const uint64_t* offsets_dev, uint32_t ntrees, uint64_t max_count, const uint32_t* trees_dev,
                                         const uint64_t* indices_dev, const vkmr_digest* leaves_dev, uint32_t k, vkmr_digest* roots_dev,
                                         uint32_t* status_dev)
{
    if (k == 0) return VKMR_OK;
    if (!digests_dev || !forest_dev || !offsets_dev || !trees_dev || !indices_dev || !leaves_dev || !roots_dev || !status_dev)
        return refuse(__func__, "null pointer");
    VKMR_CHECK(forest_args_check(__func__, total, ntrees, max_count, k, "a forest without a leaf has none to update", nullptr));
    const uint32_t H = vkmr_forest::launches(total, max_count);   // <= 58
    const dim3 grid = grid_of(k);
    Node* digests = nodes(digests_dev);
    Node* forest = nodes(forest_dev);
    Node* roots = nodes(roots_dev);
    VKMR_TRY(hipSetDevice(dev));
    VKMR_TRY(hipMemsetAsync(status_dev, 0, sizeof(uint32_t), S(s)));
    VKMR_CHECK(launch(forest_update_check_kernel, grid, dim3(256), S(s), offsets_dev, ntrees, trees_dev, indices_dev, k, status_dev));
    VKMR_CHECK(launch(forest_update_leaves_kernel, grid, dim3(256), S(s), digests, offsets_dev, trees_dev, indices_dev, nodes(leaves_dev), k, status_dev));
    for (uint32_t l = 1; l <= H; ++l) {   // level l from level l - 1, which the previous launch finished
        const Node* in = (l == 1) ? digests : forest + vkmr_forest::stored_level_base(total, ntrees, l - 1);
        VKMR_CHECK(launch(forest_update_level_kernel, grid, dim3(256), S(s), in, forest + vkmr_forest::stored_level_base(total, ntrees, l), roots, offsets_dev,
                          trees_dev, indices_dev, k, l, status_dev));
    }
    return VKMR_OK;
}

// ---- stored forests that grow: trees appended into reserved room, the last trees dropped (forest_kernels.hpp) ----------------

vkmr_status vkmr_hip_forest_append_async(int dev, vkmr_stream s, vkmr_digest* digests_dev, vkmr_digest* forest_dev, uint64_t total,
                                         uint64_t* offsets_dev, uint32_t ntrees, uint64_t max_count, uint32_t first_tree, uint64_t used,
                                         const vkmr_digest* leaves_dev, uint64_t n_leaves, const uint64_t* new_offsets_dev, uint32_t m,
                                         vkmr_digest* roots_dev, uint64_t* mutated_dev, uint32_t* status_dev)
{
    if (m == 0) return VKMR_OK;
    if (!digests_dev || !forest_dev || !offsets_dev || (!leaves_dev && n_leaves > 0) || !new_offsets_dev || !roots_dev || !status_dev)
        return refuse(__func__, "null pointer");
    if (first_tree > ntrees || m > ntrees - first_tree) return refuse(__func__, "more trees than the forest has room for");
    if (used > total || n_leaves > total - used) return refuse(__func__, "more leaves than the forest has room for");
    VKMR_CHECK(forest_args_check(__func__, total, ntrees, max_count, 0, nullptr, nullptr));
    if (grid_too_large(groups_of(n_leaves))) return refuse(__func__, "too many leaves in one call");
    const uint32_t H = vkmr_forest::launches(total, max_count);   // <= 58: the build's, so every level buffer is where the build put it
    const uint32_t end_tree = first_tree + m, behind = ntrees - first_tree;
    Node* digests = nodes(digests_dev);
    Node* forest = nodes(forest_dev);
    Node* roots = nodes(roots_dev);
    unsigned long long* mutated = reinterpret_cast<unsigned long long*>(mutated_dev);
    VKMR_TRY(hipSetDevice(dev));
    VKMR_TRY(hipMemsetAsync(status_dev, 0, sizeof(uint32_t), S(s)));
    // a lane per offset from first_tree to ntrees: behind + 1 of them, and m <= behind new trees among them
    VKMR_CHECK(launch(forest_append_check_kernel, grid_of((uint64_t)behind + 1), dim3(256), S(s), offsets_dev, ntrees, first_tree, used, new_offsets_dev,
                      m, n_leaves, max_count, status_dev));
    if (n_leaves > 0 && leaves_dev != digests_dev + used)   // not yet in place
        VKMR_CHECK(launch(forest_append_leaves_kernel, grid_of(n_leaves), dim3(256), S(s), digests, used, nodes(leaves_dev), n_leaves, status_dev));
    // the offsets, and the masks of the new trees zeroed in the same launch: a memset could not read the status word
    VKMR_CHECK(launch(forest_append_offsets_kernel, grid_of(behind), dim3(256), S(s), offsets_dev, ntrees, first_tree, used, new_offsets_dev, m, mutated,
                      status_dev));
    for (uint32_t l = 1; l <= H; ++l) {   // level l from level l - 1, over the new trees' cells alone
        const Node* in = (l == 1) ? digests : forest + vkmr_forest::stored_level_base(total, ntrees, l - 1);
        Node* out = forest + vkmr_forest::stored_level_base(total, ntrees, l);
        const uint64_t base = vkmr_forest::append_first_cell(used, first_tree, l), end = vkmr_forest::append_end_cell(used + n_leaves, end_tree, l);
        VKMR_CHECK(mutated ? launch(forest_append_level_flagged_kernel, grid_of(end - base), dim3(256), S(s), in, offsets_dev, end_tree, l, base, end, out, roots,
                                    mutated, status_dev)
                           : launch(forest_append_level_kernel, grid_of(end - base), dim3(256), S(s), in, offsets_dev, end_tree, l, base, end, out, roots,
                                    status_dev));
    }
    return VKMR_OK;
}

vkmr_status vkmr_hip_forest_truncate_async(int dev, vkmr_stream s, uint64_t* offsets_dev, uint32_t ntrees, uint32_t keep_trees, vkmr_digest* roots_dev)
{
    if (keep_trees > ntrees) return refuse(__func__, "more trees to keep than the forest has");
    if (keep_trees == ntrees) return VKMR_OK;
    if (!offsets_dev || !roots_dev) return refuse(__func__, "null pointer");
    VKMR_TRY(hipSetDevice(dev));
    return launch(forest_truncate_kernel, grid_of(ntrees - keep_trees), dim3(256), S(s), offsets_dev, ntrees, keep_trees, nodes(roots_dev));
}

// ---- forests that slide: the oldest trees dropped, stored trees copied into another forest (forest_copy_kernels.hpp) ----------

vkmr_status vkmr_hip_forest_drop_front_async(int dev, vkmr_stream s, uint64_t* offsets_dev, uint32_t ntrees, uint32_t drop_trees,
                                             vkmr_digest* roots_dev, uint64_t* mutated_dev)
{
    if (drop_trees > ntrees) return refuse(__func__, "more trees to drop than the forest has");
    if (drop_trees == 0) return VKMR_OK;
    if (!offsets_dev || !roots_dev) return refuse(__func__, "null pointer");
    VKMR_TRY(hipSetDevice(dev));
    return launch(forest_drop_front_kernel, grid_of(drop_trees), dim3(256), S(s), offsets_dev, drop_trees, nodes(roots_dev),
                  reinterpret_cast<unsigned long long*>(mutated_dev));
}

vkmr_status vkmr_hip_forest_copy_trees_async(int dev, vkmr_stream s, const vkmr_digest* src_digests_dev, const vkmr_digest* src_forest_dev,
                                             uint64_t src_total, const uint64_t* src_offsets_dev, uint32_t src_ntrees, uint64_t src_max_count,
                                             const vkmr_digest* src_roots_dev, const uint64_t* src_mutated_dev, const uint32_t* sel_dev, uint32_t m,
                                             uint64_t n_leaves, const uint64_t* new_offsets_dev, vkmr_digest* dst_digests_dev,
                                             vkmr_digest* dst_forest_dev, uint64_t dst_total, uint64_t* dst_offsets_dev, uint32_t dst_ntrees,
                                             uint64_t dst_max_count, uint32_t first_tree, uint64_t used, vkmr_digest* dst_roots_dev,
                                             uint64_t* dst_mutated_dev, uint32_t* status_dev)
{
    if (m == 0) return VKMR_OK;
    if (((!src_digests_dev || !dst_digests_dev) && n_leaves > 0) || !src_forest_dev || !src_offsets_dev || !src_roots_dev || !sel_dev ||
        !new_offsets_dev || !dst_forest_dev || !dst_offsets_dev || !dst_roots_dev || !status_dev)
        return refuse(__func__, "null pointer");
    if (first_tree > dst_ntrees || m > dst_ntrees - first_tree) return refuse(__func__, "more trees than the forest has room for");
    if (used > dst_total || n_leaves > dst_total - used) return refuse(__func__, "more leaves than the forest has room for");
    VKMR_CHECK(forest_args_check(__func__, src_total, src_ntrees, src_max_count, 0, nullptr, nullptr));
    VKMR_CHECK(forest_args_check(__func__, dst_total, dst_ntrees, dst_max_count, 0, nullptr, nullptr));
    if ((dst_digests_dev && dst_digests_dev == src_digests_dev) || dst_forest_dev == src_forest_dev || dst_offsets_dev == src_offsets_dev || dst_roots_dev == src_roots_dev)
        return refuse(__func__, "a copy inside one forest is not offered");
    if (grid_too_large(groups_of(n_leaves))) return refuse(__func__, "too many leaves in one call");
    const uint32_t H = vkmr_forest::launches(dst_total, dst_max_count);   // <= 58: the destination's build's
    const uint32_t H_src = vkmr_forest::launches(src_total, src_max_count);
    const uint32_t end_tree = first_tree + m, behind = dst_ntrees - first_tree;
    Node* roots = nodes(dst_roots_dev);
    unsigned long long* mutated = reinterpret_cast<unsigned long long*>(dst_mutated_dev);
    const unsigned long long* src_mutated = reinterpret_cast<const unsigned long long*>(src_mutated_dev);
    VKMR_TRY(hipSetDevice(dev));
    VKMR_TRY(hipMemsetAsync(status_dev, 0, sizeof(uint32_t), S(s)));
    VKMR_CHECK(launch(forest_copy_check_kernel, grid_of((uint64_t)behind + 1), dim3(256), S(s), dst_offsets_dev, dst_ntrees, first_tree, used,
                      new_offsets_dev, m, n_leaves, dst_max_count, sel_dev, src_offsets_dev, src_ntrees, status_dev));
    // append's own: the destination offsets, and the masks of the new trees zeroed in the same launch
    VKMR_CHECK(launch(forest_append_offsets_kernel, grid_of(behind), dim3(256), S(s), dst_offsets_dev, dst_ntrees, first_tree, used, new_offsets_dev, m,
                      mutated, status_dev));
    for (uint32_t l = 0; l <= H; ++l) {   // level l of the new trees from level l of their source trees: a cell is copied at l < height(c) <= H_src only
        const Node* src = (l == 0) ? nodes(src_digests_dev) : nodes(src_forest_dev) + vkmr_forest::stored_level_base(src_total, src_ntrees, l < H_src ? l : H_src);
        Node* dst = (l == 0) ? nodes(dst_digests_dev) : nodes(dst_forest_dev) + vkmr_forest::stored_level_base(dst_total, dst_ntrees, l);
        const uint64_t base = vkmr_forest::append_first_cell(used, first_tree, l), end = vkmr_forest::append_end_cell(used + n_leaves, end_tree, l);
        if (end == base) continue;        // level 0 of trees that are all empty
        VKMR_CHECK(launch(forest_copy_level_kernel, grid_of(end - base), dim3(256), S(s), src, src_offsets_dev, nodes(src_roots_dev), src_mutated, sel_dev,
                          dst_offsets_dev, first_tree, end_tree, l, base, end, dst, roots, mutated, status_dev));
    }
    return VKMR_OK;
}

// ---- the open tree of a stored forest grown or shrunk by leaves, at its right edge (forest_kernels.hpp) ----------------------

// Both calls behind their own refusals: tree `tree` at offset used - count goes from `count` to `new_count` leaves; `n_new`
// leaves of leaves_dev are copied behind `used` first unless they lie there already (0 when shrinking).
static vkmr_status forest_edge(const char* who, int dev, vkmr_stream s, vkmr_digest* digests_dev, vkmr_digest* forest_dev, uint64_t total,
                               uint64_t* offsets_dev, uint32_t ntrees, uint64_t max_count, uint32_t tree, uint64_t count, uint64_t used,
                               const vkmr_digest* leaves_dev, uint64_t n_new, uint64_t new_count, vkmr_digest* roots_dev, uint64_t* mutated_dev,
                               uint32_t* status_dev)
{
    if (!digests_dev || !forest_dev || !offsets_dev || !roots_dev || !status_dev) return refuse(who, "null pointer");
    if (tree >= ntrees) return refuse(who, "no such tree");
    if (count > used || used > total) return refuse(who, "more leaves in use than the forest holds");
    VKMR_CHECK(forest_args_check(who, total, ntrees, max_count, 0, nullptr, nullptr));
    if (grid_too_large(groups_of(n_new))) return refuse(who, "too many leaves in one call");
    const uint32_t H = vkmr_forest::launches(total, max_count);   // the build's, so every level buffer is where the build put it
    const uint32_t end_tree = tree + 1u, behind = ntrees - tree;
    const uint64_t o = used - count;
    Node* digests = nodes(digests_dev);
    Node* forest = nodes(forest_dev);
    Node* roots = nodes(roots_dev);
    unsigned long long* mutated = reinterpret_cast<unsigned long long*>(mutated_dev);
    VKMR_TRY(hipSetDevice(dev));
    VKMR_TRY(hipMemsetAsync(status_dev, 0, sizeof(uint32_t), S(s)));
    // a lane per offset from `tree` to ntrees: behind + 1 of them
    VKMR_CHECK(launch(forest_extend_check_kernel, grid_of((uint64_t)behind + 1), dim3(256), S(s), offsets_dev, ntrees, tree, count, used, status_dev));
    if (n_new > 0 && leaves_dev != digests_dev + used)   // not yet in place
        VKMR_CHECK(launch(forest_append_leaves_kernel, grid_of(n_new), dim3(256), S(s), digests, used, nodes(leaves_dev), n_new, status_dev));
    VKMR_CHECK(launch(forest_extend_offsets_kernel, grid_of(behind), dim3(256), S(s), offsets_dev, ntrees, tree, o + new_count, mutated, status_dev));
    for (uint32_t l = 1; l <= H; ++l) {   // level l from level l - 1, over the dirty nodes of the open tree's right edge alone
        const Node* in = (l == 1) ? digests : forest + vkmr_forest::stored_level_base(total, ntrees, l - 1);
        Node* out = forest + vkmr_forest::stored_level_base(total, ntrees, l);
        const uint64_t base = vkmr_forest::extend_first_cell(o, tree, count, new_count, l), end = vkmr_forest::extend_end_cell(o, tree, new_count, l);
        if (end > base)   // empty where the edge ends on a node boundary, and above the new tree's root
            VKMR_CHECK(launch(forest_extend_level_kernel, grid_of(end - base), dim3(256), S(s), in, offsets_dev, end_tree, l, base, end, out, roots,
                              status_dev));
        const uint64_t whole = vkmr_forest::pos(o, tree, l);
        if (mutated && new_count > 0 && end > whole)   // the mask again from the whole tree: level l - 1 is final behind launch l - 1
            VKMR_CHECK(launch(forest_extend_scan_kernel, grid_of(end - whole), dim3(256), S(s), in, offsets_dev, end_tree, l, whole, end, mutated,
                              status_dev));
    }
    return VKMR_OK;
}

vkmr_status vkmr_hip_forest_extend_async(int dev, vkmr_stream s, vkmr_digest* digests_dev, vkmr_digest* forest_dev, uint64_t total,
                                         uint64_t* offsets_dev, uint32_t ntrees, uint64_t max_count, uint32_t tree, uint64_t count, uint64_t used,
                                         const vkmr_digest* leaves_dev, uint64_t n_leaves, vkmr_digest* roots_dev, uint64_t* mutated_dev,
                                         uint32_t* status_dev)
{
    if (n_leaves == 0) return VKMR_OK;
    if (!leaves_dev) return refuse(__func__, "null pointer");
    if (count > max_count || n_leaves > max_count - count) return refuse(__func__, "the tree would pass max_count");
    if (used > total || n_leaves > total - used) return refuse(__func__, "more leaves than the forest has room for");
    return forest_edge(__func__, dev, s, digests_dev, forest_dev, total, offsets_dev, ntrees, max_count, tree, count, used, leaves_dev, n_leaves,
                       count + n_leaves, roots_dev, mutated_dev, status_dev);
}

vkmr_status vkmr_hip_forest_shrink_async(int dev, vkmr_stream s, vkmr_digest* digests_dev, vkmr_digest* forest_dev, uint64_t total,
                                         uint64_t* offsets_dev, uint32_t ntrees, uint64_t max_count, uint32_t tree, uint64_t count, uint64_t used,
                                         uint64_t r, vkmr_digest* roots_dev, uint64_t* mutated_dev, uint32_t* status_dev)
{
    if (r == 0) return VKMR_OK;
    if (r > count) return refuse(__func__, "more leaves to drop than the tree has");
    return forest_edge(__func__, dev, s, digests_dev, forest_dev, total, offsets_dev, ntrees, max_count, tree, count, used, nullptr, 0, count - r,
                       roots_dev, mutated_dev, status_dev);
}

// ---- trees followed by their frontiers alone (frontier_kernels.hpp, frontier_plan.hpp) ----------------------------------------

static vkmr_status frontier_args_check(const char* who, uint32_t stride, uint32_t T)
{
    if (stride == 0 || stride > VKMR_FRONTIER_MAX_STRIDE) return refuse(who, "stride must be 1..64");
    if (grid_too_large(groups_of((uint64_t)T * VKMR_FRONTIER_MAX_STRIDE))) return refuse(who, "too many trees in one call");
    return VKMR_OK;
}

vkmr_status vkmr_hip_forest_frontier_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev, const vkmr_digest* forest_dev, uint64_t total,
                                           const uint64_t* offsets_dev, uint32_t ntrees, uint64_t max_count, const vkmr_digest* roots_dev,
                                           uint32_t stride, uint64_t* counts_out_dev, vkmr_digest* peaks_out_dev)
{
    if (ntrees == 0) return VKMR_OK;
    if ((!digests_dev && total > 0) || !forest_dev || !offsets_dev || !roots_dev || !counts_out_dev || !peaks_out_dev)
        return refuse(__func__, "null pointer");
    VKMR_CHECK(forest_args_check(__func__, total, ntrees, max_count, 0, nullptr, nullptr));
    VKMR_CHECK(frontier_args_check(__func__, stride, ntrees));
    if (vkmr_frontier::bit_length(max_count < total ? max_count : total) > stride) return refuse(__func__, "a tree of max_count leaves has more peaks than stride");
    const ForestLevels lv = forest_levels(total, ntrees, vkmr_forest::launches(total, max_count));
    VKMR_TRY(hipSetDevice(dev));
    return launch(frontier_gather_kernel, grid_of((uint64_t)ntrees * stride), dim3(256), S(s), nodes(digests_dev), nodes(forest_dev), lv, offsets_dev, ntrees,
                  nodes(roots_dev), stride, counts_out_dev, nodes(peaks_out_dev));
}

// Both forms of the root walk: the roots written, or compared with `want_dev` into ok_dev.
static vkmr_status frontier_roots(const char* who, int dev, vkmr_stream s, const uint64_t* counts_dev, const vkmr_digest* peaks_dev, uint32_t stride,
                                  uint32_t T, vkmr_digest* roots_out_dev, const vkmr_digest* want_dev, uint32_t* ok_dev)
{
    if (T == 0) return VKMR_OK;
    if (!counts_dev || !peaks_dev || (!roots_out_dev && !want_dev) || (want_dev && !ok_dev)) return refuse(who, "null pointer");
    VKMR_CHECK(frontier_args_check(who, stride, T));
    VKMR_TRY(hipSetDevice(dev));
    return launch(frontier_roots_kernel, grid_of(T), dim3(256), S(s), counts_dev, nodes(peaks_dev), stride, T, nodes(roots_out_dev), nodes(want_dev), ok_dev);
}

vkmr_status vkmr_hip_frontier_roots_async(int dev, vkmr_stream s, const uint64_t* counts_dev, const vkmr_digest* peaks_dev, uint32_t stride, uint32_t T,
                                          vkmr_digest* roots_out_dev)
{
    if (T != 0 && !roots_out_dev) return refuse(__func__, "null pointer");
    return frontier_roots(__func__, dev, s, counts_dev, peaks_dev, stride, T, roots_out_dev, nullptr, nullptr);
}

vkmr_status vkmr_hip_verify_frontier_async(int dev, vkmr_stream s, const uint64_t* counts_dev, const vkmr_digest* peaks_dev, uint32_t stride, uint32_t T,
                                           const vkmr_digest* roots_dev, uint32_t* ok_dev)
{
    if (T != 0 && (!roots_dev || !ok_dev)) return refuse(__func__, "null pointer");
    return frontier_roots(__func__, dev, s, counts_dev, peaks_dev, stride, T, nullptr, roots_dev, ok_dev);
}

size_t vkmr_hip_frontier_extend_scratch_bytes(uint64_t total_new, uint32_t T)
{
    if (total_new > vkmr_frontier::max_count()) return 0;
    return (size_t)vkmr_frontier::scratch_cells(total_new, T) * sizeof(vkmr_digest);
}

vkmr_status vkmr_hip_frontier_extend_async(int dev, vkmr_stream s, const uint64_t* counts_dev, const vkmr_digest* peaks_dev, uint32_t stride, uint32_t T,
                                           const vkmr_digest* leaves_dev, uint64_t total_new, const uint64_t* offsets_dev, uint64_t max_new,
                                           void* scratch_dev, uint64_t* new_counts_dev, vkmr_digest* new_peaks_dev, vkmr_digest* roots_dev,
                                           uint32_t* status_dev)
{
    if (T == 0) return VKMR_OK;
    if (!counts_dev || !peaks_dev || (!leaves_dev && total_new > 0) || !offsets_dev || !scratch_dev || !new_counts_dev || !new_peaks_dev || !roots_dev ||
        !status_dev)
        return refuse(__func__, "null pointer");
    VKMR_CHECK(frontier_args_check(__func__, stride, T));
    if (total_new > vkmr_frontier::max_count()) return refuse(__func__, "too many leaves in one call");
    if (reinterpret_cast<uintptr_t>(scratch_dev) & 15u) return refuse(__func__, "scratch must be 16-byte aligned");
    if (grid_too_large(groups_of(vkmr_frontier::level_cells(total_new, T, 1)))) return refuse(__func__, "too many leaves in one call");
    Node* scratch = nodes(scratch_dev);
    Node* staging = scratch + vkmr_frontier::staging_base(total_new, T);
    VKMR_TRY(hipSetDevice(dev));
    VKMR_TRY(hipMemsetAsync(status_dev, 0, sizeof(uint32_t), S(s)));
    VKMR_CHECK(launch(frontier_check_kernel, grid_of(T), dim3(256), S(s), counts_dev, offsets_dev, T, total_new, max_new, stride, status_dev));
    const uint32_t H = vkmr_frontier::launches(stride);
    for (uint32_t l = 1; l <= H; ++l) {   // level l of every tree's extension from level l - 1: one launch for all trees
        const Node* in = (l == 1) ? nodes(leaves_dev) : scratch + vkmr_frontier::level_base(total_new, T, l - 1);
        const uint64_t cells = vkmr_frontier::level_cells(total_new, T, l);
        VKMR_CHECK(launch(frontier_level_kernel, grid_of(cells), dim3(256), S(s), in, counts_dev, nodes(peaks_dev), stride, offsets_dev, T, l, cells,
                          scratch + vkmr_frontier::level_base(total_new, T, l), staging, nodes(roots_dev), status_dev));
    }
    // a wavefront per tree: four trees a workgroup
    return launch(frontier_commit_kernel, dim3((uint32_t)(((uint64_t)T + 3) / 4)), dim3(256), S(s), counts_dev, nodes(peaks_dev), stride, offsets_dev, T,
                  nodes(leaves_dev), staging, new_counts_dev, nodes(new_peaks_dev), nodes(roots_dev), status_dev);
}

// ---- consistency proofs (consistency_kernels.hpp, consistency_plan.hpp) ----------------------------------------------------------

vkmr_status vkmr_hip_forest_consistency_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev, const vkmr_digest* forest_dev, uint64_t total,
                                              const uint64_t* offsets_dev, uint32_t ntrees, uint64_t max_count, const vkmr_digest* roots_dev,
                                              const uint32_t* trees_dev, const uint64_t* old_counts_dev, uint32_t Q, uint32_t stride,
                                              uint64_t* new_counts_out_dev, vkmr_digest* peaks_out_dev, vkmr_digest* rights_out_dev, uint32_t* status_dev)
{
    if (Q == 0) return VKMR_OK;
    if ((!digests_dev && total > 0) || !forest_dev || !offsets_dev || !roots_dev || !trees_dev || !old_counts_dev || !new_counts_out_dev ||
        !peaks_out_dev || !rights_out_dev || !status_dev)
        return refuse(__func__, "null pointer");
    VKMR_CHECK(forest_args_check(__func__, total, ntrees, max_count, 0, nullptr, nullptr));
    VKMR_CHECK(frontier_args_check(__func__, stride, Q));
    if (vkmr_frontier::bit_length(max_count < total ? max_count : total) > stride) return refuse(__func__, "a tree of max_count leaves has more bits than stride");
    const ForestLevels lv = forest_levels(total, ntrees, vkmr_forest::launches(total, max_count));
    VKMR_TRY(hipSetDevice(dev));
    VKMR_TRY(hipMemsetAsync(status_dev, 0, sizeof(uint32_t), S(s)));
    VKMR_CHECK(launch(consistency_check_kernel, grid_of(Q), dim3(256), S(s), offsets_dev, ntrees, trees_dev, old_counts_dev, Q, stride, status_dev));
    return launch(consistency_gather_kernel, grid_of((uint64_t)Q * stride), dim3(256), S(s), nodes(digests_dev), nodes(forest_dev), lv, offsets_dev,
                  nodes(roots_dev), trees_dev, old_counts_dev, Q, stride, new_counts_out_dev, nodes(peaks_out_dev), nodes(rights_out_dev), status_dev);
}

vkmr_status vkmr_hip_verify_consistency_async(int dev, vkmr_stream s, const uint64_t* old_counts_dev, const uint64_t* new_counts_dev,
                                              const vkmr_digest* peaks_dev, const vkmr_digest* rights_dev, uint32_t stride, uint32_t Q,
                                              const vkmr_digest* old_roots_dev, const vkmr_digest* new_roots_dev, uint32_t* ok_dev)
{
    if (Q == 0) return VKMR_OK;
    if (!old_counts_dev || !new_counts_dev || !peaks_dev || !rights_dev || !old_roots_dev || !new_roots_dev || !ok_dev) return refuse(__func__, "null pointer");
    VKMR_CHECK(frontier_args_check(__func__, stride, Q));
    VKMR_TRY(hipSetDevice(dev));
    return launch(consistency_fold_kernel, grid_of(Q), dim3(256), S(s), old_counts_dev, new_counts_dev, nodes(peaks_dev), nodes(rights_dev), stride, Q,
                  nodes(old_roots_dev), nodes(new_roots_dev), ok_dev);
}

// ---- inclusion proofs as of an earlier count (proofs_at_kernels.hpp, proofs_at_plan.hpp) ---------------------------------------

vkmr_status vkmr_hip_forest_proofs_at_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev, const vkmr_digest* forest_dev, uint64_t total,
                                            const uint64_t* offsets_dev, uint32_t ntrees, uint64_t max_count, const vkmr_digest* roots_dev,
                                            const uint32_t* epoch_trees_dev, const uint64_t* epoch_counts_dev, uint32_t E, const uint32_t* epochs_dev,
                                            const uint64_t* indices_dev, uint32_t k, uint32_t stride, vkmr_digest* edges_out_dev,
                                            vkmr_digest* old_roots_out_dev, vkmr_digest* siblings_dev, uint32_t* heights_dev, uint32_t* status_dev)
{
    if (E == 0) return VKMR_OK;
    if ((!digests_dev && total > 0) || !forest_dev || !offsets_dev || !roots_dev || !epoch_trees_dev || !epoch_counts_dev || !edges_out_dev ||
        !old_roots_out_dev || !status_dev || (k > 0 && (!epochs_dev || !indices_dev || !siblings_dev || !heights_dev)))
        return refuse(__func__, "null pointer");
    VKMR_CHECK(forest_args_check(__func__, total, ntrees, max_count, 0, nullptr, nullptr));
    if (stride == 0 || stride > 63) return refuse(__func__, "stride must be 1..63");
    VKMR_CHECK(frontier_args_check(__func__, stride, E));
    if (grid_too_large(groups_of((uint64_t)k * stride))) return refuse(__func__, "too many proofs in one call");
    if (vkmr_frontier::bit_length(max_count < total ? max_count : total) > stride) return refuse(__func__, "a tree of max_count leaves has more bits than stride");
    const ForestLevels lv = forest_levels(total, ntrees, vkmr_forest::launches(total, max_count));
    VKMR_TRY(hipSetDevice(dev));
    VKMR_TRY(hipMemsetAsync(status_dev, 0, sizeof(uint32_t), S(s)));
    VKMR_CHECK(launch(proofs_at_check_kernel, grid_of(E), dim3(256), S(s), offsets_dev, ntrees, epoch_trees_dev, epoch_counts_dev, E, stride, status_dev));
    VKMR_CHECK(launch(proofs_at_edge_kernel, grid_of(E), dim3(256), S(s), nodes(digests_dev), nodes(forest_dev), lv, offsets_dev, nodes(roots_dev),
                      epoch_trees_dev, epoch_counts_dev, E, stride, nodes(edges_out_dev), nodes(old_roots_out_dev), status_dev));
    if (k == 0) return VKMR_OK;                  // the edges and the old roots alone: the root of tree t as of count c
    return launch(proofs_at_gather_kernel, grid_of((uint64_t)k * stride), dim3(256), S(s), nodes(digests_dev), nodes(forest_dev), lv, offsets_dev,
                  nodes(roots_dev), epoch_trees_dev, epoch_counts_dev, E, epochs_dev, indices_dev, k, stride, nodes(edges_out_dev), nodes(siblings_dev),
                  heights_dev, status_dev);
}

// ---- sorted trees: order, lower bound, absence proofs (absence_kernels.hpp, absence_plan.hpp) -----------------------------------

static inline bool off_grid(const void* p, uintptr_t grid) { return (reinterpret_cast<uintptr_t>(p) & (grid - 1u)) != 0; }

// Both sortedness passes, on the caller's stream: first_bad set to "none", the counters zeroed, the scan (no launch below two
// cells), the finish.  offsets_dev null: one tree over [0, cells).
static vkmr_status sorted_launch(const char* who, int dev, vkmr_stream s, const vkmr_digest* digests_dev, uint64_t cells, const uint64_t* offsets_dev,
                                 uint32_t ntrees, uint64_t* first_bad_dev, uint64_t* info_dev)
{
    if (cells > (1ull << 58)) return refuse(who, "too many leaves");
    if (off_grid(digests_dev, 16) || off_grid(first_bad_dev, 8) || off_grid(info_dev, 8) || off_grid(offsets_dev, 8)) return refuse(who, "misaligned buffer");
    if (grid_too_large(groups_of(cells)) || grid_too_large(groups_of(ntrees))) return refuse(who, "too many leaves for one call");
    unsigned long long* first_bad = reinterpret_cast<unsigned long long*>(first_bad_dev);
    unsigned long long* info = reinterpret_cast<unsigned long long*>(info_dev);
    VKMR_TRY(hipSetDevice(dev));
    VKMR_TRY(hipMemsetAsync(first_bad_dev, 0xFF, sizeof(uint64_t) * (size_t)ntrees, S(s)));
    VKMR_TRY(hipMemsetAsync(info_dev, 0, 4 * sizeof(uint64_t), S(s)));
    if (cells >= 2) {
        VKMR_CHECK(offsets_dev ? launch(forest_sorted_scan_kernel, grid_of(cells - 1), dim3(256), S(s), nodes(digests_dev), offsets_dev, ntrees, cells, first_bad)
                               : launch(tree_sorted_scan_kernel, grid_of(cells - 1), dim3(256), S(s), nodes(digests_dev), cells, first_bad));
    }
    if (offsets_dev) return launch(forest_sorted_finish_kernel, grid_of(ntrees), dim3(256), S(s), nodes(digests_dev), offsets_dev, ntrees, cells, first_bad, info);
    return launch(tree_sorted_finish_kernel, dim3(1), dim3(64), S(s), nodes(digests_dev), cells, first_bad, info);
}

vkmr_status vkmr_hip_forest_sorted_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev, uint64_t total, const uint64_t* offsets_dev,
                                         uint32_t ntrees, uint64_t* first_bad_dev, uint64_t* info_dev)
{
    if (ntrees == 0) return VKMR_OK;
    if ((!digests_dev && total > 0) || !offsets_dev || !first_bad_dev || !info_dev) return refuse(__func__, "null pointer");
    return sorted_launch(__func__, dev, s, digests_dev, total, offsets_dev, ntrees, first_bad_dev, info_dev);
}

vkmr_status vkmr_hip_tree_sorted_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev, uint64_t count, uint64_t* first_bad_dev,
                                       uint64_t* info_dev)
{
    if ((!digests_dev && count > 0) || !first_bad_dev || !info_dev) return refuse(__func__, "null pointer");
    return sorted_launch(__func__, dev, s, digests_dev, count, nullptr, 1, first_bad_dev, info_dev);
}

vkmr_status vkmr_hip_forest_lower_bound_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev, uint64_t total, const uint64_t* offsets_dev,
                                              uint32_t ntrees, const uint32_t* trees_dev, const vkmr_digest* queries_dev, uint32_t Q,
                                              uint64_t* indices_out_dev, uint32_t* found_out_dev)
{
    if (Q == 0) return VKMR_OK;
    if (!trees_dev || !queries_dev || !indices_out_dev || !found_out_dev || (ntrees > 0 && !offsets_dev) || (ntrees > 0 && total > 0 && !digests_dev))
        return refuse(__func__, "null pointer");
    if (total > (1ull << 58)) return refuse(__func__, "too many leaves");
    if (off_grid(digests_dev, 16) || off_grid(queries_dev, 16) || off_grid(offsets_dev, 8) || off_grid(indices_out_dev, 8) || off_grid(trees_dev, 4) ||
        off_grid(found_out_dev, 4))
        return refuse(__func__, "misaligned buffer");
    if (grid_too_large(groups_of(Q))) return refuse(__func__, "too many queries in one call");
    VKMR_TRY(hipSetDevice(dev));
    return launch(forest_lower_bound_kernel, grid_of(Q), dim3(256), S(s), nodes(digests_dev), offsets_dev, ntrees, total, trees_dev, nodes(queries_dev), Q,
                  indices_out_dev, found_out_dev);
}

vkmr_status vkmr_hip_tree_lower_bound_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev, uint64_t count, const vkmr_digest* queries_dev,
                                            uint32_t Q, uint64_t* indices_out_dev, uint32_t* found_out_dev)
{
    if (Q == 0) return VKMR_OK;
    if (!queries_dev || !indices_out_dev || !found_out_dev || (count > 0 && !digests_dev)) return refuse(__func__, "null pointer");
    if (count > (1ull << 58)) return refuse(__func__, "too many leaves");
    if (off_grid(digests_dev, 16) || off_grid(queries_dev, 16) || off_grid(indices_out_dev, 8) || off_grid(found_out_dev, 4))
        return refuse(__func__, "misaligned buffer");
    if (grid_too_large(groups_of(Q))) return refuse(__func__, "too many queries in one call");
    VKMR_TRY(hipSetDevice(dev));
    return launch(tree_lower_bound_kernel, grid_of(Q), dim3(256), S(s), nodes(digests_dev), count, nodes(queries_dev), Q, indices_out_dev, found_out_dev);
}

// What the two gathers and the two checks refuse of their proof buffers alike: a missing one, one off its grid, too many cells.
static vkmr_status absence_buffers_check(const char* who, const void* queries, const void* indices, const void* neighbours, const void* main_row,
                                         const void* low_row, uint32_t Q, uint32_t stride)
{
    if (!queries || !indices || !neighbours || (stride > 0 && (!main_row || !low_row))) return refuse(who, "null pointer");
    if (off_grid(queries, 16) || off_grid(neighbours, 16) || off_grid(main_row, 16) || off_grid(low_row, 16) || off_grid(indices, 8))
        return refuse(who, "misaligned buffer");
    if (grid_too_large(groups_of((uint64_t)Q * (stride ? stride : 1u)))) return refuse(who, "too many proofs in one call");
    return VKMR_OK;
}

vkmr_status vkmr_hip_forest_absence_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev, const vkmr_digest* forest_dev, uint64_t total,
                                          const uint64_t* offsets_dev, uint32_t ntrees, uint64_t max_count, const uint32_t* trees_dev,
                                          const vkmr_digest* queries_dev, uint32_t Q, uint32_t stride, uint64_t* indices_out_dev,
                                          vkmr_digest* neighbours_out_dev, vkmr_digest* main_out_dev, vkmr_digest* low_out_dev, uint32_t* heights_out_dev)
{
    if (Q == 0) return VKMR_OK;
    if ((!digests_dev && total > 0) || !forest_dev || !offsets_dev || !trees_dev || !heights_out_dev) return refuse(__func__, "null pointer");
    if (stride == 0 || stride > 63) return refuse(__func__, "stride must be 1..63");
    VKMR_CHECK(absence_buffers_check(__func__, queries_dev, indices_out_dev, neighbours_out_dev, main_out_dev, low_out_dev, Q, stride));
    VKMR_CHECK(forest_args_check(__func__, total, ntrees, max_count, Q, nullptr, nullptr));
    if (off_grid(digests_dev, 16) || off_grid(forest_dev, 16) || off_grid(offsets_dev, 8) || off_grid(trees_dev, 4) || off_grid(heights_out_dev, 4))
        return refuse(__func__, "misaligned buffer");
    const uint32_t H = vkmr_forest::launches(total, max_count);   // <= 58
    if (stride < H) return refuse(__func__, "stride is below the forest's levels");
    const ForestLevels lv = forest_levels(total, ntrees, H);
    VKMR_TRY(hipSetDevice(dev));
    VKMR_CHECK(launch(forest_absence_entries_kernel, grid_of(Q), dim3(256), S(s), nodes(digests_dev), offsets_dev, ntrees, total, trees_dev,
                      nodes(queries_dev), Q, indices_out_dev, nodes(neighbours_out_dev), heights_out_dev));
    return launch(forest_absence_rows_kernel, grid_of((uint64_t)Q * stride), dim3(256), S(s), nodes(digests_dev), nodes(forest_dev), lv, offsets_dev, ntrees,
                  total, trees_dev, indices_out_dev, Q, stride, nodes(main_out_dev), nodes(low_out_dev));
}

vkmr_status vkmr_hip_tree_absence_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev, const vkmr_digest* tree_dev, uint64_t count,
                                        uint32_t height, const vkmr_digest* queries_dev, uint32_t Q, uint64_t* indices_out_dev,
                                        vkmr_digest* neighbours_out_dev, vkmr_digest* main_out_dev, vkmr_digest* low_out_dev)
{
    if (Q == 0) return VKMR_OK;
    if (!digests_dev || !tree_dev) return refuse(__func__, "null pointer");
    if (count == 0 || count > (1ull << 58) || height != vkmr_math::height(count)) return refuse(__func__, "height must be max(1, ceil(log2 count))");
    VKMR_CHECK(absence_buffers_check(__func__, queries_dev, indices_out_dev, neighbours_out_dev, main_out_dev, low_out_dev, Q, height));
    if (off_grid(digests_dev, 16) || off_grid(tree_dev, 16)) return refuse(__func__, "misaligned buffer");
    const TreeLevels lv = tree_levels(count, height);
    VKMR_TRY(hipSetDevice(dev));
    VKMR_CHECK(launch(tree_absence_entries_kernel, grid_of(Q), dim3(256), S(s), nodes(digests_dev), count, nodes(queries_dev), Q, indices_out_dev,
                      nodes(neighbours_out_dev)));
    return launch(tree_absence_rows_kernel, grid_of((uint64_t)Q * height), dim3(256), S(s), nodes(digests_dev), nodes(tree_dev), lv, count, indices_out_dev, Q,
                  height, nodes(main_out_dev), nodes(low_out_dev));
}

vkmr_status vkmr_hip_verify_forest_absence_async(int dev, vkmr_stream s, const vkmr_digest* queries_dev, const uint32_t* trees_dev,
                                                 const uint64_t* indices_dev, const vkmr_digest* neighbours_dev, const vkmr_digest* main_dev,
                                                 const vkmr_digest* low_dev, const uint32_t* heights_dev, uint32_t Q, uint32_t stride,
                                                 const vkmr_digest* roots_dev, const uint64_t* counts_dev, uint32_t ntrees, uint32_t* verdict_dev)
{
    if (Q == 0) return VKMR_OK;
    if (!trees_dev || !heights_dev || !verdict_dev || (ntrees > 0 && (!roots_dev || !counts_dev))) return refuse(__func__, "null pointer");
    if (stride == 0 || stride > 63) return refuse(__func__, "stride must be 1..63");
    VKMR_CHECK(absence_buffers_check(__func__, queries_dev, indices_dev, neighbours_dev, main_dev, low_dev, Q, stride));
    if (off_grid(roots_dev, 16) || off_grid(counts_dev, 8) || off_grid(trees_dev, 4) || off_grid(heights_dev, 4) || off_grid(verdict_dev, 4))
        return refuse(__func__, "misaligned buffer");
    VKMR_TRY(hipSetDevice(dev));
    return launch(forest_absence_fold_kernel, grid_of(Q), dim3(256), S(s), nodes(queries_dev), trees_dev, indices_dev, nodes(neighbours_dev), nodes(main_dev),
                  nodes(low_dev), heights_dev, Q, stride, nodes(roots_dev), counts_dev, ntrees, verdict_dev);
}

vkmr_status vkmr_hip_verify_absence_async(int dev, vkmr_stream s, const vkmr_digest* queries_dev, const uint64_t* indices_dev,
                                          const vkmr_digest* neighbours_dev, const vkmr_digest* main_dev, const vkmr_digest* low_dev, uint32_t Q,
                                          uint32_t height, const vkmr_digest* root_dev, uint64_t count, uint32_t* verdict_dev)
{
    if (Q == 0) return VKMR_OK;
    if (!root_dev || !verdict_dev) return refuse(__func__, "null pointer");
    if (height > 63 || height != vkmr_absence::height(count)) return refuse(__func__, "height must be max(1, ceil(log2 count)), 0 for no leaf");
    VKMR_CHECK(absence_buffers_check(__func__, queries_dev, indices_dev, neighbours_dev, main_dev, low_dev, Q, height));
    if (off_grid(root_dev, 16) || off_grid(verdict_dev, 4)) return refuse(__func__, "misaligned buffer");
    VKMR_TRY(hipSetDevice(dev));
    return launch(tree_absence_fold_kernel, grid_of(Q), dim3(256), S(s), nodes(queries_dev), indices_dev, nodes(neighbours_dev), nodes(main_dev),
                  nodes(low_dev), Q, height, nodes(root_dev), count, verdict_dev);
}

// ---- sorted trees: every leaf between two digests, proved complete (range_kernels.hpp, range_plan.hpp) ----------------------------

size_t vkmr_hip_range_scratch_bytes(uint64_t nleaves, uint32_t Q)
{
    if (Q == 0 || nleaves > (1ull << 58)) return 0;
    return (size_t)vkmr_range::layout(nleaves, Q).bytes;
}

namespace {
// The parts of a range call's scratch_dev as the kernels take them.
struct RangeScratch {
    uint32_t *bad, *ok;
    uint64_t* sums;
    Node *tops, *odd, *even;
    RangeScratch(void* scratch_dev, const vkmr_range::Layout& L)
    {
        const uintptr_t at = reinterpret_cast<uintptr_t>(scratch_dev);
        bad = reinterpret_cast<uint32_t*>(at);
        sums = reinterpret_cast<uint64_t*>(at + L.sums);
        ok = reinterpret_cast<uint32_t*>(at + L.ok);
        tops = reinterpret_cast<Node*>(at + L.tops);
        odd = reinterpret_cast<Node*>(at + L.odd);
        even = reinterpret_cast<Node*>(at + L.even);
    }
};

// What the two gathers and the two checks refuse of their proof buffers alike: a missing one, one off its grid, too many cells.
vkmr_status range_buffers_check(const char* who, const void* lo, const void* hi, const void* firsts, const void* leaf_starts, const void* leaves,
                                uint64_t nleaves, const void* left_row, const void* right_row, const void* scratch, uint32_t Q, uint32_t stride)
{
    if (!lo || !hi || !firsts || !leaf_starts || !scratch || (nleaves > 0 && !leaves) || (stride > 0 && (!left_row || !right_row)))
        return refuse(who, "null pointer");
    if (off_grid(lo, 16) || off_grid(hi, 16) || off_grid(leaves, 16) || off_grid(left_row, 16) || off_grid(right_row, 16) || off_grid(firsts, 8) ||
        off_grid(leaf_starts, 8))
        return refuse(who, "misaligned buffer");
    if (off_grid(scratch, 16)) return refuse(who, "scratch must be 16-byte aligned");
    if (nleaves > (1ull << 58)) return refuse(who, "too many leaves");
    if (grid_too_large(groups_of((uint64_t)Q + 1)) || grid_too_large(groups_of(vkmr_range::level_cells(nleaves, Q, 0))))
        return refuse(who, "too many leaves or queries in one call");
    return VKMR_OK;
}
}  // namespace

vkmr_status vkmr_hip_forest_range_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev, const vkmr_digest* forest_dev, uint64_t total,
                                        const uint64_t* offsets_dev, uint32_t ntrees, uint64_t max_count, const uint32_t* trees_dev,
                                        const vkmr_digest* lo_dev, const vkmr_digest* hi_dev, uint32_t Q, uint32_t stride, void* scratch_dev,
                                        uint64_t* firsts_out_dev, uint64_t* leaf_starts_out_dev, vkmr_digest* leaves_out_dev, uint64_t leaves_capacity,
                                        vkmr_digest* left_out_dev, vkmr_digest* right_out_dev, uint32_t* heights_out_dev, uint64_t* info_dev)
{
    if (Q == 0) return VKMR_OK;
    if ((!digests_dev && total > 0) || !forest_dev || !offsets_dev || !trees_dev || !heights_out_dev || !info_dev) return refuse(__func__, "null pointer");
    if (stride == 0 || stride > 63) return refuse(__func__, "stride must be 1..63");
    VKMR_CHECK(range_buffers_check(__func__, lo_dev, hi_dev, firsts_out_dev, leaf_starts_out_dev, leaves_out_dev, leaves_capacity, left_out_dev,
                                   right_out_dev, scratch_dev, Q, stride));
    VKMR_CHECK(forest_args_check(__func__, total, ntrees, max_count, Q, nullptr, nullptr));
    if (off_grid(digests_dev, 16) || off_grid(forest_dev, 16) || off_grid(offsets_dev, 8) || off_grid(trees_dev, 4) || off_grid(heights_out_dev, 4) ||
        off_grid(info_dev, 8))
        return refuse(__func__, "misaligned buffer");
    const uint32_t H = vkmr_forest::launches(total, max_count);   // <= 58
    if (stride < H) return refuse(__func__, "stride is below the forest's levels");
    const ForestLevels lv = forest_levels(total, ntrees, H);
    const vkmr_range::Layout L = vkmr_range::layout(0, Q);
    const RangeScratch sc(scratch_dev, L);
    unsigned long long* info = reinterpret_cast<unsigned long long*>(info_dev);
    const dim3 qgrid((uint32_t)L.groups), qblock(VKMR_RANGE_THREADS);
    VKMR_TRY(hipSetDevice(dev));
    VKMR_TRY(hipMemsetAsync(info_dev, 0, 4 * sizeof(uint64_t), S(s)));
    VKMR_CHECK(launch(forest_range_runs_kernel, qgrid, qblock, S(s), nodes(digests_dev), offsets_dev, ntrees, total, trees_dev, nodes(lo_dev), nodes(hi_dev),
                      Q, firsts_out_dev, leaf_starts_out_dev, heights_out_dev, sc.sums, info));
    VKMR_CHECK(launch(range_starts_kernel, dim3(1), qblock, S(s), sc.sums, L.groups, leaves_capacity, info));
    VKMR_CHECK(launch(range_places_kernel, qgrid, qblock, S(s), sc.sums, Q, leaf_starts_out_dev));
    if (leaves_capacity > 0)
        VKMR_CHECK(launch(forest_range_leaves_kernel, grid_of(leaves_capacity), dim3(256), S(s), nodes(digests_dev), offsets_dev, ntrees, total, trees_dev, Q,
                          firsts_out_dev, leaf_starts_out_dev, info, nodes(leaves_out_dev)));
    return launch(forest_range_rows_kernel, grid_of(Q, stride), dim3(256), S(s), nodes(digests_dev), nodes(forest_dev), lv, offsets_dev, ntrees, total,
                  trees_dev, firsts_out_dev, leaf_starts_out_dev, Q, stride, nodes(left_out_dev), nodes(right_out_dev));
}

vkmr_status vkmr_hip_tree_range_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev, const vkmr_digest* tree_dev, uint64_t count,
                                      uint32_t height, const vkmr_digest* lo_dev, const vkmr_digest* hi_dev, uint32_t Q, void* scratch_dev,
                                      uint64_t* firsts_out_dev, uint64_t* leaf_starts_out_dev, vkmr_digest* leaves_out_dev, uint64_t leaves_capacity,
                                      vkmr_digest* left_out_dev, vkmr_digest* right_out_dev, uint64_t* info_dev)
{
    if (Q == 0) return VKMR_OK;
    if (!digests_dev || !tree_dev || !info_dev) return refuse(__func__, "null pointer");
    if (count == 0 || count > (1ull << 58) || height != vkmr_math::height(count)) return refuse(__func__, "height must be max(1, ceil(log2 count))");
    VKMR_CHECK(range_buffers_check(__func__, lo_dev, hi_dev, firsts_out_dev, leaf_starts_out_dev, leaves_out_dev, leaves_capacity, left_out_dev,
                                   right_out_dev, scratch_dev, Q, height));
    if (off_grid(digests_dev, 16) || off_grid(tree_dev, 16) || off_grid(info_dev, 8)) return refuse(__func__, "misaligned buffer");
    const TreeLevels lv = tree_levels(count, height);
    const vkmr_range::Layout L = vkmr_range::layout(0, Q);
    const RangeScratch sc(scratch_dev, L);
    unsigned long long* info = reinterpret_cast<unsigned long long*>(info_dev);
    const dim3 qgrid((uint32_t)L.groups), qblock(VKMR_RANGE_THREADS);
    VKMR_TRY(hipSetDevice(dev));
    VKMR_TRY(hipMemsetAsync(info_dev, 0, 4 * sizeof(uint64_t), S(s)));
    VKMR_CHECK(launch(tree_range_runs_kernel, qgrid, qblock, S(s), nodes(digests_dev), count, nodes(lo_dev), nodes(hi_dev), Q, firsts_out_dev,
                      leaf_starts_out_dev, sc.sums, info));
    VKMR_CHECK(launch(range_starts_kernel, dim3(1), qblock, S(s), sc.sums, L.groups, leaves_capacity, info));
    VKMR_CHECK(launch(range_places_kernel, qgrid, qblock, S(s), sc.sums, Q, leaf_starts_out_dev));
    if (leaves_capacity > 0)
        VKMR_CHECK(launch(tree_range_leaves_kernel, grid_of(leaves_capacity), dim3(256), S(s), nodes(digests_dev), count, Q, firsts_out_dev,
                          leaf_starts_out_dev, info, nodes(leaves_out_dev)));
    return launch(tree_range_rows_kernel, grid_of(Q, height), dim3(256), S(s), nodes(digests_dev), nodes(tree_dev), lv, count, firsts_out_dev,
                  leaf_starts_out_dev, Q, height, nodes(left_out_dev), nodes(right_out_dev));
}

vkmr_status vkmr_hip_verify_forest_range_async(int dev, vkmr_stream s, const uint32_t* trees_dev, const vkmr_digest* lo_dev, const vkmr_digest* hi_dev,
                                               const uint64_t* firsts_dev, const uint64_t* leaf_starts_dev, const vkmr_digest* leaves_dev,
                                               uint64_t nleaves, const vkmr_digest* left_dev, const vkmr_digest* right_dev, const uint32_t* heights_dev,
                                               uint32_t Q, uint32_t stride, const vkmr_digest* roots_dev, const uint64_t* counts_dev, uint32_t ntrees,
                                               void* scratch_dev, uint32_t* verdict_dev, uint64_t* in_first_dev, uint64_t* in_count_dev)
{
    if (Q == 0) return VKMR_OK;
    if (!trees_dev || !heights_dev || !verdict_dev || !in_first_dev || !in_count_dev || (ntrees > 0 && (!roots_dev || !counts_dev)))
        return refuse(__func__, "null pointer");
    if (stride == 0 || stride > 63) return refuse(__func__, "stride must be 1..63");
    VKMR_CHECK(range_buffers_check(__func__, lo_dev, hi_dev, firsts_dev, leaf_starts_dev, leaves_dev, nleaves, left_dev, right_dev, scratch_dev, Q, stride));
    if (off_grid(roots_dev, 16) || off_grid(counts_dev, 8) || off_grid(trees_dev, 4) || off_grid(heights_dev, 4) || off_grid(verdict_dev, 4) ||
        off_grid(in_first_dev, 8) || off_grid(in_count_dev, 8))
        return refuse(__func__, "misaligned buffer");
    const vkmr_range::Layout L = vkmr_range::layout(nleaves, Q);
    const RangeScratch sc(scratch_dev, L);
    VKMR_TRY(hipSetDevice(dev));
    VKMR_TRY(hipMemsetAsync(scratch_dev, 0, 32, S(s)));
    VKMR_CHECK(launch(forest_range_heads_kernel, grid_of(Q), dim3(256), S(s), trees_dev, heights_dev, nodes(roots_dev), counts_dev, ntrees, nodes(lo_dev),
                      nodes(hi_dev), firsts_dev, leaf_starts_dev, nodes(leaves_dev), nleaves, Q, stride, sc.bad, sc.ok, in_first_dev, in_count_dev));
    if (nleaves >= 2) VKMR_CHECK(launch(range_order_kernel, grid_of(nleaves - 1), dim3(256), S(s), leaf_starts_dev, nodes(leaves_dev), nleaves, Q, sc.ok));
    for (uint32_t l = 0; l < stride; ++l) {      // level l + 1 from level l: odd levels in one buffer, even ones in the other
        const uint64_t cells = vkmr_range::level_cells(nleaves, Q, l + 1);
        VKMR_CHECK(launch(forest_range_level_kernel, grid_of(cells), dim3(256), S(s), trees_dev, heights_dev, counts_dev, ntrees, firsts_dev, leaf_starts_dev,
                          nodes(leaves_dev), nleaves, nodes(left_dev), nodes(right_dev), Q, stride, l, sc.bad, sc.ok, (l & 1u) ? sc.odd : sc.even,
                          (l & 1u) ? sc.even : sc.odd, sc.tops));
    }
    return launch(forest_range_verdict_kernel, grid_of(Q), dim3(256), S(s), trees_dev, heights_dev, nodes(roots_dev), counts_dev, ntrees, Q, sc.bad, sc.ok,
                  sc.tops, verdict_dev, in_first_dev, in_count_dev);
}

vkmr_status vkmr_hip_verify_range_async(int dev, vkmr_stream s, const vkmr_digest* lo_dev, const vkmr_digest* hi_dev, const uint64_t* firsts_dev,
                                        const uint64_t* leaf_starts_dev, const vkmr_digest* leaves_dev, uint64_t nleaves, const vkmr_digest* left_dev,
                                        const vkmr_digest* right_dev, uint32_t Q, uint32_t height, const vkmr_digest* root_dev, uint64_t count,
                                        void* scratch_dev, uint32_t* verdict_dev, uint64_t* in_first_dev, uint64_t* in_count_dev)
{
    if (Q == 0) return VKMR_OK;
    if (!root_dev || !verdict_dev || !in_first_dev || !in_count_dev) return refuse(__func__, "null pointer");
    if (height > 63 || height != vkmr_absence::height(count)) return refuse(__func__, "height must be max(1, ceil(log2 count)), 0 for no leaf");
    VKMR_CHECK(range_buffers_check(__func__, lo_dev, hi_dev, firsts_dev, leaf_starts_dev, leaves_dev, nleaves, left_dev, right_dev, scratch_dev, Q, height));
    if (off_grid(root_dev, 16) || off_grid(verdict_dev, 4) || off_grid(in_first_dev, 8) || off_grid(in_count_dev, 8))
        return refuse(__func__, "misaligned buffer");
    const vkmr_range::Layout L = vkmr_range::layout(nleaves, Q);
    const RangeScratch sc(scratch_dev, L);
    VKMR_TRY(hipSetDevice(dev));
    VKMR_TRY(hipMemsetAsync(scratch_dev, 0, 32, S(s)));
    VKMR_CHECK(launch(tree_range_heads_kernel, grid_of(Q), dim3(256), S(s), height, nodes(root_dev), count, nodes(lo_dev), nodes(hi_dev), firsts_dev,
                      leaf_starts_dev, nodes(leaves_dev), nleaves, Q, sc.bad, sc.ok, in_first_dev, in_count_dev));
    if (nleaves >= 2) VKMR_CHECK(launch(range_order_kernel, grid_of(nleaves - 1), dim3(256), S(s), leaf_starts_dev, nodes(leaves_dev), nleaves, Q, sc.ok));
    for (uint32_t l = 0; l < height; ++l) {
        const uint64_t cells = vkmr_range::level_cells(nleaves, Q, l + 1);
        VKMR_CHECK(launch(tree_range_level_kernel, grid_of(cells), dim3(256), S(s), height, count, firsts_dev, leaf_starts_dev, nodes(leaves_dev), nleaves,
                          nodes(left_dev), nodes(right_dev), Q, l, sc.bad, sc.ok, (l & 1u) ? sc.odd : sc.even, (l & 1u) ? sc.even : sc.odd, sc.tops));
    }
    return launch(tree_range_verdict_kernel, grid_of(Q), dim3(256), S(s), height, nodes(root_dev), count, Q, sc.bad, sc.ok, sc.tops, verdict_dev,
                  in_first_dev, in_count_dev);
}

// ---- partial Merkle trees in BIP37 order (merkleblock_kernels.hpp, merkleblock_plan.hpp) ----------------------------------------

size_t vkmr_hip_forest_merkleblocks_max_hashes(uint64_t total, uint32_t ntrees, uint64_t max_count, uint32_t k)
{
    if (total == 0 || ntrees == 0 || max_count == 0 || k == 0) return 0;
    return (size_t)vkmr_mb::max_hashes(total, ntrees, max_count, k);
}

size_t vkmr_hip_forest_merkleblocks_max_flag_bytes(uint64_t total, uint32_t ntrees, uint64_t max_count, uint32_t k)
{
    if (total == 0 || ntrees == 0 || max_count == 0 || k == 0) return 0;
    return (size_t)vkmr_mb::max_flag_bytes(total, ntrees, max_count, k);
}

size_t vkmr_hip_forest_merkleblocks_scratch_bytes(uint32_t k, uint32_t stride)
{
    if (k == 0 || stride == 0 || stride > 63) return 0;
    return vkmr_mb::layout(k, stride).bytes;
}

namespace {
// The parts of a merkleblock call's scratch_dev as the kernels take them.
struct MerkleblockScratch {
    uint64_t *flag_at, *hash_at, *sums, *bit_start, *byte_sums;
    uint32_t *block_of, *flag_words;
    MerkleblockScratch(void* scratch_dev, const vkmr_mb::Layout& L)
    {
        const uintptr_t at = reinterpret_cast<uintptr_t>(scratch_dev);
        flag_at = reinterpret_cast<uint64_t*>(at + L.flag_at);
        hash_at = reinterpret_cast<uint64_t*>(at + L.hash_at);
        block_of = reinterpret_cast<uint32_t*>(at + L.block_of);
        sums = reinterpret_cast<uint64_t*>(at + L.sums);
        bit_start = reinterpret_cast<uint64_t*>(at + L.bit_start);
        byte_sums = reinterpret_cast<uint64_t*>(at + L.byte_sums);
        flag_words = reinterpret_cast<uint32_t*>(at + L.flag_words);
    }
};

struct MerkleblockOutputs {
    uint32_t* block_trees;
    uint64_t *block_counts, *bit_counts, *hash_starts, *byte_starts;
    vkmr_digest* hashes;
    uint64_t hash_capacity;
    uint8_t* flags;
    uint64_t flag_capacity;
    uint64_t* info;
};

vkmr_status merkleblock_outputs_check(const char* who, const MerkleblockOutputs& o, const void* scratch_dev)
{
    if (!o.block_trees || !o.block_counts || !o.bit_counts || !o.hash_starts || !o.byte_starts || !o.info || !scratch_dev ||
        (!o.hashes && o.hash_capacity > 0) || (!o.flags && o.flag_capacity > 0))
        return refuse(who, "null pointer");
    if (reinterpret_cast<uintptr_t>(scratch_dev) & 15u) return refuse(who, "scratch must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(o.flags) & 3u) return refuse(who, "flags_dev must be 4-byte aligned");
    return VKMR_OK;
}

// The launches behind the index check, the same for one tree and for a forest but for the three kernels that read entries:
// `sums`, `places` and `emit` launch those with the caller's own arguments in front.
extern "C++" {
template <class Sums, class Places, class Emit>
vkmr_status merkleblock_launch(hipStream_t stream, uint32_t k, uint32_t stride, const vkmr_mb::Layout& L, const MerkleblockScratch& sc,
                               const MerkleblockOutputs& o, Sums sums, Places places, Emit emit)
{
    const dim3 egrid((uint32_t)L.groups), eblock(VKMR_MB_THREADS);
    VKMR_CHECK(sums(egrid, eblock));
    VKMR_CHECK(launch(merkleblock_starts_kernel, dim3(1), eblock, stream, sc.sums, L.groups, o.info, sc.bit_start, o.hash_starts));
    VKMR_CHECK(places(egrid, eblock));
    VKMR_CHECK(launch(merkleblock_byte_sums_kernel, egrid, eblock, stream, o.info, sc.bit_start, o.bit_counts, sc.byte_sums));
    VKMR_CHECK(launch(merkleblock_byte_starts_kernel, dim3(1), eblock, stream, sc.byte_sums, L.groups, o.hash_capacity, o.flag_capacity, o.info));
    VKMR_CHECK(launch(merkleblock_byte_places_kernel, dim3((uint32_t)(((uint64_t)k + 1 + VKMR_MB_THREADS - 1) / VKMR_MB_THREADS)), eblock, stream, o.info,
                      sc.bit_start, sc.byte_sums, o.byte_starts));
    // the flag words in use never exceed the scratch's (the plan's bound) nor, with status 0, the caller's capacity
    uint64_t words = (o.flag_capacity + 3) / 4;
    if (words > L.words) words = L.words;
    if (words == 0) words = 1;                   // no byte fits: the status is bit 2 and both kernels return at once
    VKMR_CHECK(launch(merkleblock_zero_kernel, grid_of(words), dim3(256), stream, o.info, sc.flag_words));
    VKMR_CHECK(emit(grid_of(k, stride), dim3(256)));
    return launch(merkleblock_flags_kernel, grid_of(words), dim3(256), stream, o.info, sc.flag_words, o.flags);
}
}  // extern "C++"
}  // namespace

vkmr_status vkmr_hip_forest_merkleblocks_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev, const vkmr_digest* forest_dev, uint64_t total,
                                               const uint64_t* offsets_dev, uint32_t ntrees, uint64_t max_count, const uint32_t* trees_dev,
                                               const uint64_t* indices_dev, uint32_t k, void* scratch_dev, uint32_t* block_trees_dev,
                                               uint64_t* block_counts_dev, uint64_t* bit_counts_dev, uint64_t* hash_starts_dev, uint64_t* byte_starts_dev,
                                               vkmr_digest* hashes_dev, uint64_t hash_capacity, uint8_t* flags_dev, uint64_t flag_capacity,
                                               uint64_t* info_dev)
{
    if (k == 0) return VKMR_OK;
    const MerkleblockOutputs o{block_trees_dev, block_counts_dev, bit_counts_dev, hash_starts_dev, byte_starts_dev, hashes_dev, hash_capacity, flags_dev,
                               flag_capacity, info_dev};
    if (!digests_dev || !forest_dev || !offsets_dev || !trees_dev || !indices_dev) return refuse(__func__, "null pointer");
    VKMR_CHECK(merkleblock_outputs_check(__func__, o, scratch_dev));
    VKMR_CHECK(forest_args_check(__func__, total, ntrees, max_count, k, "a forest without a leaf has none to match", scratch_dev));
    const uint32_t H = vkmr_forest::launches(total, max_count);   // <= 58
    const ForestLevels lv = forest_levels(total, ntrees, H);
    const vkmr_mb::Layout L = vkmr_mb::layout(k, H);
    const MerkleblockScratch sc(scratch_dev, L);
    hipStream_t stream = S(s);
    VKMR_TRY(hipSetDevice(dev));
    VKMR_TRY(hipMemsetAsync(info_dev, 0, sizeof(uint64_t), stream));
    VKMR_CHECK(launch(forest_update_check_kernel, grid_of(k), dim3(256), stream, offsets_dev, ntrees, trees_dev, indices_dev, k,
                      reinterpret_cast<uint32_t*>(info_dev)));
    return merkleblock_launch(
        stream, k, H, L, sc, o,
        [&](dim3 g, dim3 b) { return launch(merkleblock_forest_sums_kernel, g, b, stream, offsets_dev, trees_dev, indices_dev, k, L.groups, info_dev, sc.sums); },
        [&](dim3 g, dim3 b) {
            return launch(merkleblock_forest_places_kernel, g, b, stream, offsets_dev, trees_dev, indices_dev, k, L.groups, info_dev, sc.sums, sc.flag_at,
                          sc.hash_at, sc.block_of, sc.bit_start, block_trees_dev, block_counts_dev, hash_starts_dev);
        },
        [&](dim3 g, dim3 b) {
            return launch(merkleblock_forest_emit_kernel, g, b, stream, nodes(digests_dev), nodes(forest_dev), lv, offsets_dev, trees_dev, indices_dev, k,
                          info_dev, sc.flag_at, sc.hash_at, sc.block_of, sc.bit_start, byte_starts_dev, nodes(hashes_dev), sc.flag_words);
        });
}

vkmr_status vkmr_hip_tree_merkleblock_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev, const vkmr_digest* tree_dev, uint64_t count,
                                            uint32_t height, const uint64_t* indices_dev, uint32_t k, void* scratch_dev, uint32_t* block_trees_dev,
                                            uint64_t* block_counts_dev, uint64_t* bit_counts_dev, uint64_t* hash_starts_dev, uint64_t* byte_starts_dev,
                                            vkmr_digest* hashes_dev, uint64_t hash_capacity, uint8_t* flags_dev, uint64_t flag_capacity, uint64_t* info_dev)
{
    if (k == 0) return VKMR_OK;
    const MerkleblockOutputs o{block_trees_dev, block_counts_dev, bit_counts_dev, hash_starts_dev, byte_starts_dev, hashes_dev, hash_capacity, flags_dev,
                               flag_capacity, info_dev};
    if (!digests_dev || !tree_dev || !indices_dev) return refuse(__func__, "null pointer");
    VKMR_CHECK(merkleblock_outputs_check(__func__, o, scratch_dev));
    if (count == 0 || height == 0 || height > 63 || height != vkmr_math::height(count))
        return refuse(__func__, "height must be max(1, ceil(log2 count)): the walk starts at the tree's root");
    if (grid_too_large(groups_of(k))) return refuse(__func__, "too many entries in one call");
    const TreeLevels lv = tree_levels(count, height);
    const vkmr_mb::Layout L = vkmr_mb::layout(k, height);
    const MerkleblockScratch sc(scratch_dev, L);
    hipStream_t stream = S(s);
    VKMR_TRY(hipSetDevice(dev));
    VKMR_TRY(hipMemsetAsync(info_dev, 0, sizeof(uint64_t), stream));
    VKMR_CHECK(launch(tree_update_check_kernel, grid_of(k), dim3(256), stream, indices_dev, k, count, reinterpret_cast<uint32_t*>(info_dev)));
    return merkleblock_launch(
        stream, k, height, L, sc, o,
        [&](dim3 g, dim3 b) { return launch(merkleblock_tree_sums_kernel, g, b, stream, indices_dev, count, k, L.groups, info_dev, sc.sums); },
        [&](dim3 g, dim3 b) {
            return launch(merkleblock_tree_places_kernel, g, b, stream, indices_dev, count, k, L.groups, info_dev, sc.sums, sc.flag_at, sc.hash_at, sc.block_of,
                          sc.bit_start, block_trees_dev, block_counts_dev, hash_starts_dev);
        },
        [&](dim3 g, dim3 b) {
            return launch(merkleblock_tree_emit_kernel, g, b, stream, nodes(digests_dev), nodes(tree_dev), lv, count, indices_dev, k, info_dev, sc.flag_at,
                          sc.hash_at, sc.block_of, sc.bit_start, byte_starts_dev, nodes(hashes_dev), sc.flag_words);
        });
}

// ---- multiproofs inside the stored forest (forest_tree_kernels.hpp) ---------------------------------------------------------

size_t vkmr_hip_forest_multiproof_max_nodes(uint64_t total, uint32_t ntrees, uint64_t max_count, uint32_t k)
{
    if (total == 0 || ntrees == 0 || max_count == 0) return 0;
    return (size_t)vkmr_forest::multiproof_max_nodes(total, ntrees, max_count, k);
}

size_t vkmr_hip_forest_multiproof_scratch_bytes(uint32_t k, uint32_t stride)
{
    return (vkmr_hip_multiproof_scratch_bytes(k, stride) + 15u) & ~(size_t)15u;   // the single tree's layout with height := stride, in whole 16-byte units
}

vkmr_status vkmr_hip_forest_multiproof_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev, const vkmr_digest* forest_dev, uint64_t total,
                                             const uint64_t* offsets_dev, uint32_t ntrees, uint64_t max_count, const uint32_t* trees_dev,
                                             const uint64_t* indices_dev, uint32_t k, void* scratch_dev, vkmr_digest* nodes_dev,
                                             uint64_t nodes_capacity, uint32_t* heights_dev, uint64_t* info_dev)
{
    if (k == 0) return VKMR_OK;
    if (!digests_dev || !forest_dev || !offsets_dev || !trees_dev || !indices_dev || !scratch_dev || !heights_dev || !info_dev ||
        (!nodes_dev && nodes_capacity > 0))
        return refuse(__func__, "null pointer");
    VKMR_CHECK(forest_args_check(__func__, total, ntrees, max_count, k, "a forest without a leaf has none to prove", scratch_dev));
    const uint32_t H = vkmr_forest::launches(total, max_count);   // <= 58
    const ForestLevels lv = forest_levels(total, ntrees, H);
    const MultiproofLayout L = multiproof_layout(k, H);
    const MultiproofScratch sc(scratch_dev, L);
    const dim3 grid = grid_of(k);
    VKMR_TRY(hipSetDevice(dev));
    VKMR_TRY(hipMemsetAsync(info_dev, 0, sizeof(uint64_t), S(s)));
    VKMR_CHECK(launch(forest_update_check_kernel, grid, dim3(256), S(s), offsets_dev, ntrees, trees_dev, indices_dev, k, reinterpret_cast<uint32_t*>(info_dev)));
    VKMR_CHECK(launch(forest_multiproof_heights_kernel, grid, dim3(256), S(s), offsets_dev, trees_dev, k, info_dev, heights_dev));
    VKMR_CHECK(launch(forest_multiproof_masks_kernel, grid, dim3(256), S(s), trees_dev, indices_dev, heights_dev, k, H, L.words, info_dev, sc.mask));
    VKMR_CHECK(multiproof_rank_launch(S(s), H, L, sc, info_dev, nodes_capacity, 0u));
    return launch(forest_multiproof_gather_kernel, grid_of(k, H), dim3(256), S(s), nodes(digests_dev), nodes(forest_dev), lv, offsets_dev, trees_dev,
                  indices_dev, k, L.words, sc.mask, sc.word_start, info_dev, nodes(nodes_dev));
}

vkmr_status vkmr_hip_verify_forest_multiproof_async(int dev, vkmr_stream s, const vkmr_digest* leaves_dev, const uint32_t* trees_dev,
                                                    const uint64_t* indices_dev, const uint32_t* heights_dev, uint32_t k, uint32_t stride,
                                                    const vkmr_digest* nodes_dev, uint64_t m, const vkmr_digest* roots_dev, uint32_t ntrees,
                                                    void* scratch_dev, uint32_t* ok_dev)
{
    if (k == 0) return VKMR_OK;
    if (!leaves_dev || !trees_dev || !indices_dev || !heights_dev || !roots_dev || !scratch_dev || !ok_dev || (!nodes_dev && m > 0))
        return refuse(__func__, "null pointer");
    if (stride == 0 || stride > 63) return refuse(__func__, "stride must be 1..63");
    if (reinterpret_cast<uintptr_t>(scratch_dev) & 15u) return refuse(__func__, "scratch must be 16-byte aligned");
    const MultiproofLayout L = multiproof_layout(k, stride);
    const MultiproofScratch sc(scratch_dev, L);
    const dim3 grid = grid_of(k);
    VKMR_TRY(hipSetDevice(dev));
    VKMR_TRY(hipMemsetAsync(sc.hdr, 0, sizeof(uint64_t), S(s)));
    VKMR_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(ok_dev), 1, 1, S(s)));   // the finish kernel clears it
    VKMR_CHECK(launch(verify_forest_multiproof_check_kernel, grid, dim3(256), S(s), trees_dev, indices_dev, heights_dev, k, stride, ntrees,
                      reinterpret_cast<uint32_t*>(sc.hdr)));
    VKMR_CHECK(launch(forest_multiproof_masks_kernel, grid, dim3(256), S(s), trees_dev, indices_dev, heights_dev, k, stride, L.words, sc.hdr, sc.mask));
    VKMR_CHECK(multiproof_rank_launch(S(s), stride, L, sc, sc.hdr, m, 1u));   // exact: M == m
    for (uint32_t l = 0; l < stride; ++l)   // level l + 1 from level l, which the previous launch finished
        VKMR_CHECK(launch(verify_forest_multiproof_level_kernel, grid, dim3(256), S(s), l == 0 ? nodes(leaves_dev) : sc.cell, sc.cell, sc.end, trees_dev,
                          indices_dev, heights_dev, k, l, L.words, sc.mask, sc.word_start, nodes(nodes_dev), sc.hdr));
    return launch(verify_forest_multiproof_finish_kernel, grid, dim3(256), S(s), sc.cell, trees_dev, k, nodes(roots_dev), sc.hdr, ok_dev);
}

// ---- applying a forest multiproof: the new roots from the old roots, the old and the new leaves (forest_tree_kernels.hpp) ----

vkmr_status vkmr_hip_apply_forest_multiproof_async(int dev, vkmr_stream s, const vkmr_digest* old_leaves_dev, const vkmr_digest* new_leaves_dev,
                                                   const uint32_t* trees_dev, const uint64_t* indices_dev, const uint64_t* counts_dev, uint32_t k,
                                                   uint32_t stride, const vkmr_digest* nodes_dev, uint64_t m, const vkmr_digest* roots_dev,
                                                   uint32_t ntrees, void* scratch_dev, uint32_t* ok_dev, vkmr_digest* new_roots_dev)
{
    if (k == 0) return VKMR_OK;
    if (!old_leaves_dev || !new_leaves_dev || !trees_dev || !indices_dev || !counts_dev || !roots_dev || !scratch_dev || !ok_dev || !new_roots_dev ||
        (!nodes_dev && m > 0))
        return refuse(__func__, "null pointer");
    if (stride == 0 || stride > 63) return refuse(__func__, "stride must be 1..63");
    if (reinterpret_cast<uintptr_t>(scratch_dev) & 15u) return refuse(__func__, "scratch must be 16-byte aligned");
    const ApplyLayout A = apply_layout(k, stride);
    const ApplyScratch sc(scratch_dev, A);
    const MultiproofLayout& L = A.mp;
    const dim3 grid = grid_of(k);
    uint32_t* status = reinterpret_cast<uint32_t*>(sc.mp.hdr);
    VKMR_TRY(hipSetDevice(dev));
    VKMR_TRY(hipMemsetAsync(sc.mp.hdr, 0, sizeof(uint64_t), S(s)));
    VKMR_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(ok_dev), 1, 1, S(s)));   // the finish kernel clears it
    // the heights from the counts, then the verifier's own launches on them: no flag is computed a second way
    VKMR_CHECK(launch(forest_apply_heights_kernel, grid, dim3(256), S(s), trees_dev, indices_dev, counts_dev, k, sc.heights, status));
    VKMR_CHECK(launch(verify_forest_multiproof_check_kernel, grid, dim3(256), S(s), trees_dev, indices_dev, sc.heights, k, stride, ntrees, status));
    VKMR_CHECK(launch(forest_multiproof_masks_kernel, grid, dim3(256), S(s), trees_dev, indices_dev, sc.heights, k, stride, L.words, sc.mp.hdr, sc.mp.mask));
    VKMR_CHECK(multiproof_rank_launch(S(s), stride, L, sc.mp, sc.mp.hdr, m, 1u));   // exact: M == m
    for (uint32_t l = 0; l < stride; ++l)   // level l + 1 from level l on both sides, which the previous launch finished
        VKMR_CHECK(launch(forest_apply_level_kernel, grid_of(k, 2), dim3(256), S(s), l == 0 ? nodes(old_leaves_dev) : sc.mp.cell,
                          l == 0 ? nodes(new_leaves_dev) : sc.cell1, sc.mp.cell, sc.cell1, sc.mp.end, sc.end1, trees_dev, indices_dev, sc.heights,
                          counts_dev, k, l, L.words, sc.mp.mask, sc.mp.word_start, nodes(nodes_dev), sc.mp.hdr));
    VKMR_CHECK(launch(verify_forest_multiproof_finish_kernel, grid, dim3(256), S(s), sc.mp.cell, trees_dev, k, nodes(roots_dev), sc.mp.hdr, ok_dev));
    return launch(forest_apply_commit_kernel, grid, dim3(256), S(s), sc.cell1, trees_dev, k, ok_dev, nodes(new_roots_dev));
}

// ---- lookup by digest (find_kernels.hpp, find_plan.hpp) ---------------------------------------------------------------------

size_t vkmr_hip_find_scratch_bytes(uint32_t k) { return (size_t)vkmr_find::scratch_bytes(k); }

// Compute units of device `dev`, asked for once per device: the scan's grid is sized from it.
static vkmr_status compute_units_of(int dev, uint32_t* cus)
{
    static std::atomic<int> known[64];
    int n = (dev >= 0 && dev < 64) ? known[dev].load(std::memory_order_relaxed) : 0;
    if (n <= 0) {
        VKMR_TRY(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev));
        if (n <= 0) n = 1;
        if (dev >= 0 && dev < 64) known[dev].store(n, std::memory_order_relaxed);
    }
    *cus = (uint32_t)n;
    return VKMR_OK;
}

// The parts of a lookup's scratch_dev (find_plan.hpp) as the kernels take them.
struct FindScratch {
    unsigned long long *table, *best;
    uint32_t* rep;
    FindScratch(void* scratch_dev, uint32_t k)
    {
        char* at = static_cast<char*>(scratch_dev);
        table = reinterpret_cast<unsigned long long*>(at);
        best = reinterpret_cast<unsigned long long*>(at + vkmr_find::best_offset(k));
        rep = reinterpret_cast<uint32_t*>(at + vkmr_find::rep_offset(k));
    }
};

// The launches of both lookups, all on the caller's stream: the scratch set to 0xFF (every slot empty, every best position
// "none"), the queries inserted, the leaves scanned (no launch when there is no cell to scan), the answers resolved.  They
// depend on (cells, k) and the device alone.  trees_dev null: one tree over [0, cells), and no offsets.
static vkmr_status find_launch(const char* who, int dev, vkmr_stream s, const vkmr_digest* digests_dev, uint64_t cells, const uint64_t* offsets_dev,
                               uint32_t ntrees, const vkmr_digest* queries_dev, uint32_t k, void* scratch_dev, uint32_t* trees_dev,
                               uint64_t* indices_dev)
{
    if (cells > (1ull << 58)) return refuse(who, "too many leaves");
    if (reinterpret_cast<uintptr_t>(scratch_dev) & 7u) return refuse(who, "scratch must be 8-byte aligned");
    const uint64_t mask = vkmr_find::table_slots(k) - 1ull;
    const FindScratch sc(scratch_dev, k);
    uint32_t cus = 0;
    VKMR_TRY(hipSetDevice(dev));
    VKMR_CHECK(compute_units_of(dev, &cus));
    VKMR_TRY(hipMemsetAsync(scratch_dev, 0xFF, (size_t)vkmr_find::scratch_bytes(k), S(s)));
    VKMR_CHECK(launch(find_insert_kernel, grid_of(k), dim3(256), S(s), nodes(queries_dev), k, sc.table, mask, sc.rep));
    if (cells > 0) {
        const dim3 grid((uint32_t)vkmr_find::scan_groups(cells, cus)), block(VKMR_FIND_THREADS);
        VKMR_CHECK(trees_dev ? launch(forest_find_scan_kernel, grid, block, S(s), nodes(digests_dev), offsets_dev, ntrees, cells, nodes(queries_dev), sc.table,
                                      mask, sc.best)
                             : launch(tree_find_scan_kernel, grid, block, S(s), nodes(digests_dev), cells, nodes(queries_dev), sc.table, mask, sc.best));
    }
    if (trees_dev) return launch(forest_find_resolve_kernel, grid_of(k), dim3(256), S(s), offsets_dev, ntrees, cells, k, sc.best, sc.rep, trees_dev, indices_dev);
    return launch(tree_find_resolve_kernel, grid_of(k), dim3(256), S(s), cells, k, sc.best, sc.rep, indices_dev);
}

vkmr_status vkmr_hip_forest_find_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev, uint64_t total, const uint64_t* offsets_dev,
                                       uint32_t ntrees, const vkmr_digest* queries_dev, uint32_t k, void* scratch_dev, uint32_t* trees_dev,
                                       uint64_t* indices_dev)
{
    if (k == 0) return VKMR_OK;
    const bool leaves = ntrees > 0 && total > 0;       // without a tree or a cell nothing is read but the queries
    if (!queries_dev || !scratch_dev || !trees_dev || !indices_dev || (ntrees > 0 && !offsets_dev) || (leaves && !digests_dev))
        return refuse(__func__, "null pointer");
    // no tree: the kernels read no offset and scan an empty range; the launches stay those of (total, k)
    return find_launch(__func__, dev, s, digests_dev, total, offsets_dev, ntrees, queries_dev, k, scratch_dev, trees_dev, indices_dev);
}

vkmr_status vkmr_hip_tree_find_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev, uint64_t count, const vkmr_digest* queries_dev,
                                     uint32_t k, void* scratch_dev, uint64_t* indices_dev)
{
    if (k == 0) return VKMR_OK;
    if (!queries_dev || !scratch_dev || !indices_dev || (count > 0 && !digests_dev)) return refuse(__func__, "null pointer");
    return find_launch(__func__, dev, s, digests_dev, count, nullptr, 0, queries_dev, k, scratch_dev, nullptr, indices_dev);
}

// ---- leaf entries sorted and deduplicated (sort_kernels.hpp, sort_plan.hpp) -------------------------------------------------

static_assert(VKMR_SORT_RANK_BLOCK_WORDS == VKMR_MP_BLOCK_WORDS, "the survivors are ranked by the multiproof's ranking kernels");
static_assert(VKMR_SORT_THREADS == VKMR_SIZES_THREADS && VKMR_SORT_BINS == VKMR_SORT_THREADS, "one bin per lane, and block_exclusive's workgroup");

size_t vkmr_hip_sort_entries_scratch_bytes(uint64_t total, uint32_t k) { return vkmr_sort::scratch_bytes(total, k); }

// The parts of a sort's scratch_dev (sort_plan.hpp) as the kernels take them.
struct SortScratch {
    uint64_t *key[2], *mask, *word_start, *block, *hdr;
    uint32_t *val[2], *hist, *totals;
    SortScratch(void* scratch_dev, const vkmr_sort::Layout& L)
    {
        char* at = static_cast<char*>(scratch_dev);
        for (int b = 0; b < 2; ++b) {
            key[b] = reinterpret_cast<uint64_t*>(at + L.key[b]);
            val[b] = reinterpret_cast<uint32_t*>(at + L.val[b]);
        }
        hist = reinterpret_cast<uint32_t*>(at + L.hist);
        totals = reinterpret_cast<uint32_t*>(at + L.totals);
        mask = reinterpret_cast<uint64_t*>(at + L.mask);
        word_start = reinterpret_cast<uint64_t*>(at + L.word_start);
        block = reinterpret_cast<uint64_t*>(at + L.block);
        hdr = reinterpret_cast<uint64_t*>(at + L.hdr);
    }
};

// The launches of both sorts, all on the caller's stream: the counters and the ranking header zeroed, the keys, three launches
// per pass, the flags, the three ranking launches (one level), the emit.  They depend on (cells, k) alone.  trees_dev null:
// one tree over [0, cells), and no offsets.
static vkmr_status sort_launch(const char* who, int dev, vkmr_stream s, uint64_t cells, const uint64_t* offsets_dev, uint32_t ntrees,
                               const uint32_t* trees_dev, const uint64_t* indices_dev, uint32_t k, void* scratch_dev, uint32_t* trees_out_dev,
                               uint64_t* indices_out_dev, uint32_t* order_out_dev, uint64_t* info_dev)
{
    if (cells > vkmr_sort::MAX_TOTAL) return refuse(who, "too many leaves");
    if (reinterpret_cast<uintptr_t>(scratch_dev) & 15u) return refuse(who, "scratch must be 16-byte aligned");
    const vkmr_sort::Layout L = vkmr_sort::layout(k);
    const SortScratch sc(scratch_dev, L);
    const uint32_t passes = vkmr_sort::passes(cells);
    unsigned long long* info = reinterpret_cast<unsigned long long*>(info_dev);
    const dim3 lanes = grid_of(k), tiles((uint32_t)L.G), block(VKMR_SORT_THREADS);
    VKMR_TRY(hipSetDevice(dev));
    VKMR_TRY(hipMemsetAsync(info_dev, 0, 4 * sizeof(uint64_t), S(s)));
    VKMR_TRY(hipMemsetAsync(sc.hdr, 0, 4 * sizeof(uint64_t), S(s)));
    VKMR_CHECK(trees_dev ? launch(forest_sort_keys_kernel, lanes, dim3(256), S(s), offsets_dev, ntrees, cells, trees_dev, indices_dev, k, sc.key[0], sc.val[0], info)
                         : launch(tree_sort_keys_kernel, lanes, dim3(256), S(s), cells, indices_dev, k, sc.key[0], sc.val[0], info));
    for (uint32_t p = 0; p < passes; ++p) {   // pass p from buffer p & 1 into the other, which the previous launches are done with
        const uint32_t in = vkmr_sort::pass_input(p), out = in ^ 1u;
        VKMR_CHECK(launch(sort_histogram_kernel, tiles, block, S(s), sc.key[in], k, p, L.G, sc.hist));
        VKMR_CHECK(launch(sort_scan_kernel, dim3(VKMR_SORT_BINS), block, S(s), sc.hist, L.G, sc.totals));
        VKMR_CHECK(launch(sort_scatter_kernel, tiles, block, S(s), sc.key[in], sc.val[in], k, p, L.G, sc.hist, sc.totals, sc.key[out], sc.val[out]));
    }
    const uint32_t at = vkmr_sort::result_buffer(cells);
    VKMR_CHECK(launch(sort_flags_kernel, lanes, dim3(256), S(s), sc.key[at], k, cells, L.words, sc.mask));
    const dim3 wgrid((uint32_t)L.blocks, 1), wblock(VKMR_MP_BLOCK_WORDS);
    VKMR_CHECK(launch(multiproof_block_sums_kernel, wgrid, wblock, S(s), sc.mask, L.words, L.blocks, sc.block));
    VKMR_CHECK(launch(multiproof_block_starts_kernel, dim3(1), dim3(256), S(s), sc.block, L.blocks, 1u, ~0ull, 0u, sc.hdr));
    VKMR_CHECK(launch(multiproof_word_starts_kernel, wgrid, wblock, S(s), sc.mask, L.words, L.blocks, sc.block, sc.hdr, sc.word_start));
    if (trees_dev)
        return launch(forest_sort_emit_kernel, lanes, dim3(256), S(s), offsets_dev, ntrees, sc.key[at], sc.val[at], k, sc.mask, sc.word_start, sc.hdr,
                      trees_out_dev, indices_out_dev, order_out_dev, info_dev);
    return launch(tree_sort_emit_kernel, lanes, dim3(256), S(s), sc.key[at], sc.val[at], k, sc.mask, sc.word_start, sc.hdr, indices_out_dev, order_out_dev, info_dev);
}

vkmr_status vkmr_hip_forest_sort_entries_async(int dev, vkmr_stream s, uint64_t total, const uint64_t* offsets_dev, uint32_t ntrees,
                                               const uint32_t* trees_dev, const uint64_t* indices_dev, uint32_t k, void* scratch_dev,
                                               uint32_t* trees_out_dev, uint64_t* indices_out_dev, uint32_t* order_out_dev, uint64_t* info_dev)
{
    if (k == 0) return VKMR_OK;
    if (!trees_dev || !indices_dev || !scratch_dev || !trees_out_dev || !indices_out_dev || !order_out_dev || !info_dev || (ntrees > 0 && !offsets_dev))
        return refuse(__func__, "null pointer");
    // no tree: the kernels read no offset and every entry is a marker or outside; the launches stay those of (total, k)
    return sort_launch(__func__, dev, s, total, offsets_dev, ntrees, trees_dev, indices_dev, k, scratch_dev, trees_out_dev, indices_out_dev,
                       order_out_dev, info_dev);
}

vkmr_status vkmr_hip_tree_sort_entries_async(int dev, vkmr_stream s, uint64_t count, const uint64_t* indices_dev, uint32_t k, void* scratch_dev,
                                             uint64_t* indices_out_dev, uint32_t* order_out_dev, uint64_t* info_dev)
{
    if (k == 0) return VKMR_OK;
    if (!indices_dev || !scratch_dev || !indices_out_dev || !order_out_dev || !info_dev) return refuse(__func__, "null pointer");
    return sort_launch(__func__, dev, s, count, nullptr, 0, nullptr, indices_dev, k, scratch_dev, nullptr, indices_out_dev, order_out_dev, info_dev);
}

vkmr_status vkmr_hip_gather_digests_async(int dev, vkmr_stream s, const vkmr_digest* src_dev, const uint32_t* order_dev, uint32_t n,
                                          vkmr_digest* dst_dev)
{
    if (n == 0) return VKMR_OK;
    if (!src_dev || !order_dev || !dst_dev) return refuse(__func__, "null pointer");
    VKMR_TRY(hipSetDevice(dev));
    return launch(gather_digests_kernel, grid_of(n), dim3(256), S(s), nodes(src_dev), order_dev, n, nodes(dst_dev));
}

// ---- the leaves of a forest sorted tree by tree (leafsort_kernels.hpp, leafsort_plan.hpp) ------------------------------------

static_assert(VKMR_LEAFSORT_HEADER_WORDS == 4u, "status, m, repeats, the tie refusal");

size_t vkmr_hip_sort_leaves_scratch_bytes(uint64_t total) { return vkmr_leafsort::scratch_bytes(total); }

// [a, a + na) and [b, b + nb) share a byte.
static inline bool bytes_overlap(const void* a, uint64_t na, const void* b, uint64_t nb)
{
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    return na && nb && pa < pb + nb && pb < pa + na;
}

// The launches of both leaf sorts, all on the caller's stream: two memsets, the check (a forest's), the keys, three launches per
// pass, the ties, the place, the emit.  They depend on (total, ntrees, max_count) alone.  offsets_dev null: one tree over
// [0, total), nothing to check.
static vkmr_status leafsort_launch(const char* who, int dev, vkmr_stream s, const vkmr_digest* in_dev, uint64_t total, const uint64_t* offsets_dev,
                                   uint32_t ntrees, uint64_t max_count, void* scratch_dev, vkmr_digest* out_dev, uint32_t* order_out_dev,
                                   uint64_t* info_dev)
{
    if (total >= vkmr_leafsort::MAX_TOTAL) return refuse(who, "2^32 leaves or more: positions are 32-bit");
    if (total == 0) {   // no cell: nothing to sort, and the offsets are still checked
        VKMR_TRY(hipSetDevice(dev));
        VKMR_TRY(hipMemsetAsync(info_dev, 0, 4 * sizeof(uint64_t), S(s)));
        if (!offsets_dev) return VKMR_OK;
        return launch(forest_check_kernel, grid_of(ntrees), dim3(256), S(s), offsets_dev, ntrees, total, max_count, reinterpret_cast<uint32_t*>(info_dev));
    }
    if (!in_dev || !scratch_dev || !out_dev) return refuse(who, "null pointer");
    if (reinterpret_cast<uintptr_t>(scratch_dev) & 15u) return refuse(who, "scratch must be 16-byte aligned");
    const vkmr_leafsort::Layout L = vkmr_leafsort::layout(total);
    if (bytes_overlap(out_dev, 32u * total, in_dev, 32u * total) || bytes_overlap(out_dev, 32u * total, scratch_dev, L.bytes))
        return refuse(who, "the sorted leaves must not overlap the input or the scratch");
    const SortScratch sc(scratch_dev, L.sort);
    char* at = static_cast<char*>(scratch_dev);
    uint32_t* dest = reinterpret_cast<uint32_t*>(at + L.dest);
    uint64_t* hdr = reinterpret_cast<uint64_t*>(at + L.hdr);
    unsigned long long* counters = reinterpret_cast<unsigned long long*>(hdr);   // the same words, as atomicAdd takes them
    const vkmr_leafsort::Shape shape = vkmr_leafsort::shape(ntrees, max_count);
    const uint32_t passes = vkmr_leafsort::passes(shape), k = (uint32_t)total;
    const dim3 lanes = grid_of(k), tiles((uint32_t)L.sort.G), block(VKMR_SORT_THREADS);
    const Node *in = nodes(in_dev);
    VKMR_TRY(hipSetDevice(dev));
    VKMR_TRY(hipMemsetAsync(info_dev, 0, 4 * sizeof(uint64_t), S(s)));
    VKMR_TRY(hipMemsetAsync(hdr, 0, VKMR_LEAFSORT_HEADER_WORDS * sizeof(uint64_t), S(s)));
    if (offsets_dev) {
        VKMR_CHECK(launch(forest_check_kernel, grid_of(ntrees), dim3(256), S(s), offsets_dev, ntrees, total, max_count, reinterpret_cast<uint32_t*>(hdr)));
        VKMR_CHECK(launch(forest_leafsort_keys_kernel, lanes, dim3(256), S(s), offsets_dev, ntrees, in, k, shape.P, hdr, sc.key[0], sc.val[0]));
    } else {
        VKMR_CHECK(launch(tree_leafsort_keys_kernel, lanes, dim3(256), S(s), total, in, k, shape.P, hdr, sc.key[0], sc.val[0]));
    }
    for (uint32_t p = 0; p < passes; ++p) {   // pass p from buffer p & 1 into the other, which the previous launches are done with
        const uint32_t from = vkmr_sort::pass_input(p), to = from ^ 1u;
        VKMR_CHECK(launch(sort_histogram_kernel, tiles, block, S(s), sc.key[from], k, p, L.sort.G, sc.hist));
        VKMR_CHECK(launch(sort_scan_kernel, dim3(VKMR_SORT_BINS), block, S(s), sc.hist, L.sort.G, sc.totals));
        VKMR_CHECK(launch(sort_scatter_kernel, tiles, block, S(s), sc.key[from], sc.val[from], k, p, L.sort.G, sc.hist, sc.totals, sc.key[to], sc.val[to]));
    }
    const uint32_t r = vkmr_leafsort::result_buffer(shape);
    if (offsets_dev) {
        VKMR_CHECK(launch(forest_leafsort_ties_kernel, lanes, dim3(256), S(s), offsets_dev, ntrees, sc.key[r], counters));
        VKMR_CHECK(launch(forest_leafsort_place_kernel, lanes, dim3(256), S(s), offsets_dev, ntrees, in, sc.key[r], sc.val[r], counters, dest));
        return launch(forest_leafsort_emit_kernel, lanes, dim3(256), S(s), offsets_dev, ntrees, in, sc.val[r], dest, hdr, nodes(out_dev), order_out_dev, info_dev);
    }
    VKMR_CHECK(launch(tree_leafsort_ties_kernel, lanes, dim3(256), S(s), total, sc.key[r], counters));
    VKMR_CHECK(launch(tree_leafsort_place_kernel, lanes, dim3(256), S(s), total, in, sc.key[r], sc.val[r], counters, dest));
    return launch(tree_leafsort_emit_kernel, lanes, dim3(256), S(s), total, in, sc.val[r], dest, hdr, nodes(out_dev), order_out_dev, info_dev);
}

vkmr_status vkmr_hip_forest_sort_leaves_async(int dev, vkmr_stream s, const vkmr_digest* digests_in_dev, uint64_t total, const uint64_t* offsets_dev,
                                              uint32_t ntrees, uint64_t max_count, void* scratch_dev, vkmr_digest* digests_out_dev,
                                              uint32_t* order_out_dev, uint64_t* info_dev)
{
    if (ntrees == 0) return VKMR_OK;
    if (!offsets_dev || !info_dev) return refuse(__func__, "null pointer");
    return leafsort_launch(__func__, dev, s, digests_in_dev, total, offsets_dev, ntrees, max_count, scratch_dev, digests_out_dev, order_out_dev, info_dev);
}

vkmr_status vkmr_hip_tree_sort_leaves_async(int dev, vkmr_stream s, const vkmr_digest* digests_in_dev, uint64_t count, void* scratch_dev,
                                            vkmr_digest* digests_out_dev, uint32_t* order_out_dev, uint64_t* info_dev)
{
    if (!info_dev) return refuse(__func__, "null pointer");
    return leafsort_launch(__func__, dev, s, digests_in_dev, count, nullptr, 1u, count, scratch_dev, digests_out_dev, order_out_dev, info_dev);
}

// ---- two sorted forests merged tree by tree (merge_kernels.hpp, merge_plan.hpp) ---------------------------------------------

static_assert(VKMR_MERGE_HEADER_WORDS >= 5u, "status bits 2 and 3, matches, repeats, the two offsets checks");
static_assert(VKMR_MERGE_SCAN_ROW % VKMR_SORT_SCAN_SPAN == 0u, "a row is whole trips of sort_scan_kernel");

size_t vkmr_hip_merge_leaves_scratch_bytes(uint64_t a_total, uint64_t b_total, uint32_t) { return vkmr_merge::scratch_bytes(a_total, b_total); }

// The launches of both merges, all on the caller's stream: two memsets, the two offsets checks (a forest's), the order of A, the
// marks of B, the scan's two launches, the emit.  They depend on (a_total, b_total, ntrees, op) alone.  a_offsets_dev null: one
// tree a side at cell 0, nothing to check.
static vkmr_status merge_launch(const char* who, int dev, vkmr_stream s, const vkmr_digest* a_dev, uint64_t a_total, const uint64_t* a_offsets_dev,
                                const vkmr_digest* b_dev, uint64_t b_total, const uint64_t* b_offsets_dev, uint32_t ntrees, uint32_t op,
                                void* scratch_dev, vkmr_digest* out_dev, uint64_t out_capacity, uint64_t* out_offsets_dev, uint64_t* origin_out_dev,
                                uint64_t* info_dev)
{
    if (op > VKMR_MERGE_INTERSECTION) return refuse(who, "op is 0 (union), 1 (difference) or 2 (intersection)");
    if (!vkmr_merge::fits(a_total, b_total)) return refuse(who, "a_total + b_total + 2 must stay below 2^32: the scan's sums are 32-bit");
    if (!info_dev || !scratch_dev || (a_total && !a_dev) || (b_total && !b_dev) || (out_capacity && !out_dev)) return refuse(who, "null pointer");
    if ((reinterpret_cast<uintptr_t>(scratch_dev) | reinterpret_cast<uintptr_t>(a_dev) | reinterpret_cast<uintptr_t>(b_dev) |
         reinterpret_cast<uintptr_t>(out_dev)) & 15u)
        return refuse(who, "digests and scratch must be 16-byte aligned");
    if ((reinterpret_cast<uintptr_t>(a_offsets_dev) | reinterpret_cast<uintptr_t>(b_offsets_dev) | reinterpret_cast<uintptr_t>(out_offsets_dev) |
         reinterpret_cast<uintptr_t>(origin_out_dev) | reinterpret_cast<uintptr_t>(info_dev)) & 7u)
        return refuse(who, "uint64_t buffers must be 8-byte aligned");
    if (out_capacity > (~0ull >> 6)) return refuse(who, "out_capacity too large");
    const vkmr_merge::Layout L = vkmr_merge::layout(a_total, b_total);
    if (bytes_overlap(out_dev, 32u * out_capacity, a_dev, 32u * a_total) || bytes_overlap(out_dev, 32u * out_capacity, b_dev, 32u * b_total) ||
        bytes_overlap(out_dev, 32u * out_capacity, scratch_dev, L.bytes))
        return refuse(who, "the output cells must not overlap an input or the scratch");
    char* at = static_cast<char*>(scratch_dev);
    uint32_t* scan = reinterpret_cast<uint32_t*>(at + L.scan);
    uint32_t* tot = reinterpret_cast<uint32_t*>(at + L.tot);
    uint32_t* grand = reinterpret_cast<uint32_t*>(at + L.grand);
    uint32_t* pos0 = reinterpret_cast<uint32_t*>(at + L.pos0);
    unsigned long long* hdr = reinterpret_cast<unsigned long long*>(at + L.hdr);
    const Node *a = nodes(a_dev), *b = nodes(b_dev);
    const uint64_t emit_lanes = std::max<uint64_t>(a_total + (op == VKMR_MERGE_UNION ? b_total : 0ull), a_offsets_dev ? (uint64_t)ntrees + 1u : 1u);
    const dim3 block(256), scan_block(VKMR_SORT_THREADS);
    VKMR_TRY(hipSetDevice(dev));
    VKMR_TRY(hipMemsetAsync(at + L.scan, 0, L.tot - L.scan, S(s)));
    VKMR_TRY(hipMemsetAsync(hdr, 0, VKMR_MERGE_HEADER_WORDS * sizeof(uint64_t), S(s)));
    if (a_offsets_dev) {
        VKMR_CHECK(launch(forest_check_kernel, grid_of(ntrees), block, S(s), a_offsets_dev, ntrees, a_total, ~0ull, reinterpret_cast<uint32_t*>(hdr + 3)));
        VKMR_CHECK(launch(forest_check_kernel, grid_of(ntrees), block, S(s), b_offsets_dev, ntrees, b_total, ~0ull, reinterpret_cast<uint32_t*>(hdr + 4)));
        if (a_total > 1) VKMR_CHECK(launch(forest_merge_order_kernel, grid_of(a_total), block, S(s), a_offsets_dev, b_offsets_dev, ntrees, a, hdr));
        if (b_total) VKMR_CHECK(launch(forest_merge_mark_kernel, grid_of(b_total), block, S(s), a_offsets_dev, b_offsets_dev, ntrees, a, b, op, L.S, hdr, scan, pos0));
    } else {
        if (a_total > 1) VKMR_CHECK(launch(tree_merge_order_kernel, grid_of(a_total), block, S(s), a_total, b_total, a, hdr));
        if (b_total) VKMR_CHECK(launch(tree_merge_mark_kernel, grid_of(b_total), block, S(s), a_total, b_total, a, b, op, L.S, hdr, scan, pos0));
    }
    VKMR_CHECK(launch(sort_scan_kernel, dim3((uint32_t)L.rows), scan_block, S(s), scan, (uint64_t)VKMR_MERGE_SCAN_ROW, tot));
    VKMR_CHECK(launch(sort_scan_kernel, dim3(1), scan_block, S(s), tot, L.rows, grand));
    if (a_offsets_dev)
        return launch(forest_merge_emit_kernel, grid_of(emit_lanes), block, S(s), a_offsets_dev, b_offsets_dev, ntrees, a, b, op, a_total, b_total,
                      (const unsigned long long*)hdr, (const uint32_t*)scan, (const uint32_t*)tot, (const uint32_t*)pos0, out_capacity, nodes(out_dev),
                      out_offsets_dev, origin_out_dev, info_dev);
    return launch(tree_merge_emit_kernel, grid_of(emit_lanes), block, S(s), a_total, b_total, a, b, op, (const unsigned long long*)hdr, (const uint32_t*)scan,
                  (const uint32_t*)tot, (const uint32_t*)pos0, out_capacity, nodes(out_dev), origin_out_dev, info_dev);
}

vkmr_status vkmr_hip_forest_merge_leaves_async(int dev, vkmr_stream s, const vkmr_digest* a_digests_dev, uint64_t a_total, const uint64_t* a_offsets_dev,
                                               const vkmr_digest* b_digests_dev, uint64_t b_total, const uint64_t* b_offsets_dev, uint32_t ntrees,
                                               uint32_t op, void* scratch_dev, vkmr_digest* out_digests_dev, uint64_t out_capacity,
                                               uint64_t* out_offsets_dev, uint64_t* origin_out_dev, uint64_t* info_dev)
{
    if (ntrees == 0) return VKMR_OK;
    if (!a_offsets_dev || !b_offsets_dev || !out_offsets_dev) return refuse(__func__, "null pointer");
    return merge_launch(__func__, dev, s, a_digests_dev, a_total, a_offsets_dev, b_digests_dev, b_total, b_offsets_dev, ntrees, op, scratch_dev,
                        out_digests_dev, out_capacity, out_offsets_dev, origin_out_dev, info_dev);
}

vkmr_status vkmr_hip_tree_merge_leaves_async(int dev, vkmr_stream s, const vkmr_digest* a_digests_dev, uint64_t a_count, const vkmr_digest* b_digests_dev,
                                             uint64_t b_count, uint32_t op, void* scratch_dev, vkmr_digest* out_digests_dev, uint64_t out_capacity,
                                             uint64_t* origin_out_dev, uint64_t* info_dev)
{
    return merge_launch(__func__, dev, s, a_digests_dev, a_count, nullptr, b_digests_dev, b_count, nullptr, 1u, op, scratch_dev, out_digests_dev,
                        out_capacity, nullptr, origin_out_dev, info_dev);
}

// ---- the leaves that differ between two stored forests or trees (diff_kernels.hpp, diff_plan.hpp) ----------------------------

static_assert(VKMR_DIFF_RANK_BLOCK_WORDS == VKMR_MP_BLOCK_WORDS, "the frontier is ranked by the multiproof's ranking kernels");
static_assert(VKMR_DIFF_HEADER_WORDS >= 2 + 1 + 2, "the ranking's header of one level, then the diff's two counters");

size_t vkmr_hip_diff_scratch_bytes(uint32_t capacity) { return vkmr_diff::scratch_bytes(capacity); }

// The parts of a diff's scratch_dev (diff_plan.hpp) as the kernels take them.
struct DiffScratch {
    uint64_t *node[2], *mask, *word_start, *block, *hdr;
    uint32_t* tree[2];
    DiffScratch(void* scratch_dev, const vkmr_diff::Layout& L)
    {
        char* at = static_cast<char*>(scratch_dev);
        for (int b = 0; b < 2; ++b) {
            node[b] = reinterpret_cast<uint64_t*>(at + L.node[b]);
            tree[b] = reinterpret_cast<uint32_t*>(at + L.tree[b]);
        }
        mask = reinterpret_cast<uint64_t*>(at + L.mask);
        word_start = reinterpret_cast<uint64_t*>(at + L.word_start);
        block = reinterpret_cast<uint64_t*>(at + L.block);
        hdr = reinterpret_cast<uint64_t*>(at + L.hdr);
    }
};

// The ranking of one step's mask words: the multiproof's three launches with one level; more than `capacity` set bits is
// status bit 2, and everything behind reads the status first.
static vkmr_status diff_rank_launch(hipStream_t stream, const DiffScratch& sc, uint64_t words, uint32_t capacity)
{
    const uint64_t blocks = vkmr_diff::rank_blocks(words);
    const dim3 wgrid((uint32_t)blocks, 1), wblock(VKMR_MP_BLOCK_WORDS);
    VKMR_CHECK(launch(multiproof_block_sums_kernel, wgrid, wblock, stream, sc.mask, words, blocks, sc.block));
    VKMR_CHECK(launch(multiproof_block_starts_kernel, dim3(1), dim3(256), stream, sc.block, blocks, 1u, (uint64_t)capacity, 0u, sc.hdr));
    return launch(multiproof_word_starts_kernel, wgrid, wblock, stream, sc.mask, words, blocks, sc.block, sc.hdr, sc.word_start);
}

vkmr_status vkmr_hip_forest_diff_async(int dev, vkmr_stream s, const vkmr_digest* digests_a_dev, const vkmr_digest* forest_a_dev,
                                       const vkmr_digest* roots_a_dev, const vkmr_digest* digests_b_dev, const vkmr_digest* forest_b_dev,
                                       const vkmr_digest* roots_b_dev, uint64_t total, const uint64_t* offsets_dev, uint32_t ntrees, uint64_t max_count,
                                       void* scratch_dev, uint32_t* trees_out_dev, uint64_t* indices_out_dev, vkmr_digest* leaves_b_out_dev,
                                       uint32_t capacity, uint64_t* info_dev)
{
    if (ntrees == 0) return VKMR_OK;
    if (((!digests_a_dev || !digests_b_dev) && total > 0) || !forest_a_dev || !forest_b_dev || !roots_a_dev || !roots_b_dev || !offsets_dev ||
        !scratch_dev || !info_dev || ((!trees_out_dev || !indices_out_dev) && capacity > 0))
        return refuse(__func__, "null pointer");
    VKMR_CHECK(forest_args_check(__func__, total, ntrees, max_count, 0, nullptr, scratch_dev));
    const uint32_t H = vkmr_forest::launches(total, max_count);   // <= 58
    const ForestLevels lv = forest_levels(total, ntrees, H);
    const DiffScratch sc(scratch_dev, vkmr_diff::layout(capacity));
    const uint32_t steps = (capacity == 0 || total == 0) ? 0u : H;   // no room for an entry, or no leaf to differ: step 0 alone
    const dim3 roots(vkmr_diff::root_groups(ntrees)), block(VKMR_DIFF_THREADS);
    const uint64_t span = vkmr_diff::root_span(ntrees);
    const Node *da = nodes(digests_a_dev), *fa = nodes(forest_a_dev), *db = nodes(digests_b_dev), *fb = nodes(forest_b_dev);
    VKMR_TRY(hipSetDevice(dev));
    VKMR_TRY(hipMemsetAsync(sc.hdr, 0, VKMR_DIFF_HEADER_WORDS * sizeof(uint64_t), S(s)));
    VKMR_CHECK(launch(forest_diff_roots_count_kernel, roots, block, S(s), nodes(roots_a_dev), nodes(roots_b_dev), offsets_dev, ntrees, span, sc.block));
    VKMR_CHECK(launch(multiproof_block_starts_kernel, dim3(1), dim3(256), S(s), sc.block, (uint64_t)roots.x, 1u, (uint64_t)capacity, 0u, sc.hdr));
    VKMR_CHECK(launch(forest_diff_roots_emit_kernel, roots, block, S(s), nodes(roots_a_dev), nodes(roots_b_dev), offsets_dev, ntrees, span, sc.block, sc.hdr,
                      sc.tree[0], sc.node[0], info_dev, steps == 0 ? 1u : 0u));
    for (uint32_t step = 1; step <= steps; ++step) {   // frontier (step - 1) & 1 into the other, or into the outputs at the end
        const uint32_t in = (step - 1u) & 1u, out = in ^ 1u;
        const bool last = step == steps;
        const uint64_t bound = vkmr_diff::forest_frontier_bound(total, ntrees, capacity, step);   // >= 1
        const uint64_t words = vkmr_diff::mask_words(bound);
        VKMR_CHECK(launch(forest_diff_mask_kernel, grid_of(bound), block, S(s), da, fa, db, fb, lv, offsets_dev, ntrees, sc.tree[in], sc.node[in], step, words,
                          sc.hdr, sc.mask));
        VKMR_CHECK(diff_rank_launch(S(s), sc, words, capacity));
        VKMR_CHECK(launch(forest_diff_emit_kernel, grid_of(bound), block, S(s), db, offsets_dev, ntrees, sc.tree[in], sc.node[in], step, bound, sc.mask,
                          sc.word_start, sc.hdr, last ? trees_out_dev : sc.tree[out], last ? indices_out_dev : sc.node[out],
                          last ? nodes(leaves_b_out_dev) : (Node*)nullptr, info_dev, last ? 1u : 0u));
    }
    return VKMR_OK;
}

vkmr_status vkmr_hip_tree_diff_async(int dev, vkmr_stream s, const vkmr_digest* digests_a_dev, const vkmr_digest* tree_a_dev,
                                     const vkmr_digest* digests_b_dev, const vkmr_digest* tree_b_dev, uint64_t count, uint32_t height, void* scratch_dev,
                                     uint64_t* indices_out_dev, vkmr_digest* leaves_b_out_dev, uint32_t capacity, uint64_t* info_dev)
{
    if (count == 0) return VKMR_OK;
    if (!digests_a_dev || !digests_b_dev || (height > 0 && (!tree_a_dev || !tree_b_dev)) || !scratch_dev || !info_dev ||
        (!indices_out_dev && capacity > 0))
        return refuse(__func__, "null pointer");
    if (!height_ok(count, height)) return refuse(__func__, "height does not reduce count to one node");
    if (count > vkmr_diff::MAX_TOTAL) return refuse(__func__, "too many leaves");
    if (reinterpret_cast<uintptr_t>(scratch_dev) & 15u) return refuse(__func__, "scratch must be 16-byte aligned");
    const TreeLevels lv = tree_levels(count, height);
    const DiffScratch sc(scratch_dev, vkmr_diff::layout(capacity));
    const uint32_t steps = capacity == 0 ? 0u : height;
    const dim3 block(VKMR_DIFF_THREADS);
    const Node *da = nodes(digests_a_dev), *ta = nodes(tree_a_dev), *db = nodes(digests_b_dev), *tb = nodes(tree_b_dev);
    const uint64_t root_cell = lv.off[height];         // level `height` is one cell; height 0: the leaf, and this is not used
    VKMR_TRY(hipSetDevice(dev));
    VKMR_TRY(hipMemsetAsync(sc.hdr, 0, VKMR_DIFF_HEADER_WORDS * sizeof(uint64_t), S(s)));
    VKMR_CHECK(launch(tree_diff_roots_count_kernel, dim3(1), block, S(s), da, ta, db, tb, count, height, root_cell, sc.block));
    VKMR_CHECK(launch(multiproof_block_starts_kernel, dim3(1), dim3(256), S(s), sc.block, 1ull, 1u, (uint64_t)capacity, 0u, sc.hdr));
    // a tree of one leaf without a level: the root is the leaf, and step 0 writes the answer
    const bool leaf = height == 0 && capacity > 0;
    VKMR_CHECK(launch(tree_diff_roots_emit_kernel, dim3(1), block, S(s), da, ta, db, tb, count, height, root_cell, sc.block, sc.hdr,
                      leaf ? indices_out_dev : sc.node[0], leaf ? nodes(leaves_b_out_dev) : (Node*)nullptr, info_dev, steps == 0 ? 1u : 0u));
    for (uint32_t step = 1; step <= steps; ++step) {
        const uint32_t in = (step - 1u) & 1u, out = in ^ 1u;
        const bool last = step == steps;
        const uint32_t l = vkmr_diff::level_at(height, step);
        const uint64_t bound = vkmr_diff::tree_frontier_bound(count, height, capacity, step);      // >= 1
        const uint64_t words = vkmr_diff::mask_words(bound);
        VKMR_CHECK(launch(tree_diff_mask_kernel, grid_of(bound), block, S(s), da, ta, db, tb, count, height, vkmr_diff::tree_child_base(lv.off, l), sc.node[in],
                          step, words, sc.hdr, sc.mask));
        VKMR_CHECK(diff_rank_launch(S(s), sc, words, capacity));
        VKMR_CHECK(launch(tree_diff_emit_kernel, grid_of(bound), block, S(s), db, sc.node[in], step, bound, sc.mask, sc.word_start, sc.hdr,
                          last ? indices_out_dev : sc.node[out], last ? nodes(leaves_b_out_dev) : (Node*)nullptr, info_dev, last ? 1u : 0u));
    }
    return VKMR_OK;
}

// ---- the nodes of a stored forest or tree that are not the hash of their children (audit_kernels.hpp, audit_plan.hpp) -------------

static_assert(VKMR_AUDIT_RANK_BLOCK_WORDS == VKMR_MP_BLOCK_WORDS, "the ballot words are ranked by the multiproof's ranking kernels");
static_assert(VKMR_AUDIT_HEADER_WORDS >= 2 + 1, "the ranking's header of one level");
static_assert(VKMR_AUDIT_THREADS == 256u, "grid_of() counts workgroups of 256");

size_t vkmr_hip_audit_scratch_bytes(uint64_t total, uint32_t ntrees, uint32_t capacity) { return vkmr_audit::scratch_bytes(total, ntrees, capacity); }

// The parts of an audit's scratch_dev (audit_plan.hpp) as the kernels take them; all null for the masks-only form.
struct AuditScratch {
    uint64_t *mask, *word_start, *block, *hdr;
    AuditScratch(void* scratch_dev, const vkmr_audit::Layout& L, uint32_t capacity)
    {
        char* at = capacity ? static_cast<char*>(scratch_dev) : nullptr;
        mask = at ? reinterpret_cast<uint64_t*>(at + L.mask) : nullptr;
        word_start = at ? reinterpret_cast<uint64_t*>(at + L.word_start) : nullptr;
        block = at ? reinterpret_cast<uint64_t*>(at + L.block) : nullptr;
        hdr = at ? reinterpret_cast<uint64_t*>(at + L.hdr) : nullptr;
    }
};

// The ranking of the `words` ballot words a call left: the multiproof's three launches with one level and no limit -- the
// emit launches cut the list at `capacity` themselves, so that the first `capacity` entries are written also when there are more.
static vkmr_status audit_rank_launch(hipStream_t stream, const AuditScratch& sc, uint64_t words)
{
    const uint64_t blocks = vkmr_audit::rank_blocks(words);
    const dim3 wgrid((uint32_t)blocks, 1), wblock(VKMR_MP_BLOCK_WORDS);
    VKMR_CHECK(launch(multiproof_block_sums_kernel, wgrid, wblock, stream, sc.mask, words, blocks, sc.block));
    VKMR_CHECK(launch(multiproof_block_starts_kernel, dim3(1), dim3(256), stream, sc.block, blocks, 1u, ~0ull, 0u, sc.hdr));
    return launch(multiproof_word_starts_kernel, wgrid, wblock, stream, sc.mask, words, blocks, sc.block, sc.hdr, sc.word_start);
}

vkmr_status vkmr_hip_forest_audit_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev, const vkmr_digest* forest_dev, const vkmr_digest* roots_dev,
                                        uint64_t total, const uint64_t* offsets_dev, uint32_t ntrees, uint64_t max_count, void* scratch_dev,
                                        uint64_t* masks_dev, uint32_t* bad_trees_dev, uint32_t* bad_levels_dev, uint64_t* bad_nodes_dev, uint32_t capacity,
                                        uint64_t* info_dev)
{
    if (ntrees == 0) return VKMR_OK;
    if ((!digests_dev && total > 0) || !forest_dev || !roots_dev || !offsets_dev || !masks_dev || !info_dev ||
        (capacity > 0 && (!scratch_dev || !bad_trees_dev || !bad_levels_dev || !bad_nodes_dev)))
        return refuse(__func__, "null pointer");
    VKMR_CHECK(forest_args_check(__func__, total, ntrees, max_count, 0, nullptr, capacity ? scratch_dev : nullptr));
    const uint64_t cells1 = vkmr_forest::level_cells(total, ntrees, 1);
    if (grid_too_large(groups_of(cells1))) return refuse(__func__, "forest too large");
    if (capacity > 0 && cells1 > vkmr_audit::MAX_LIST_CELLS) return refuse(__func__, "a level of more than 2^32 - 1 cells cannot be listed: capacity must be 0");
    if (max_count > total) max_count = total;
    const uint32_t H = vkmr_forest::launches(total, max_count);   // <= 58
    const AuditScratch sc(scratch_dev, vkmr_audit::layout(total, ntrees, capacity), capacity);
    const Node *digests = nodes(digests_dev), *forest = nodes(forest_dev), *roots = nodes(roots_dev);
    const dim3 block(VKMR_AUDIT_THREADS);
    VKMR_TRY(hipSetDevice(dev));
    VKMR_TRY(hipMemsetAsync(info_dev, 0, 4 * sizeof(uint64_t), S(s)));
    VKMR_TRY(hipMemsetAsync(masks_dev, 0, sizeof(uint64_t) * ntrees, S(s)));
    if (capacity) VKMR_TRY(hipMemsetAsync(sc.hdr, 0, VKMR_AUDIT_HEADER_WORDS * sizeof(uint64_t), S(s)));
    VKMR_CHECK(launch(forest_check_kernel, grid_of(ntrees), dim3(256), S(s), offsets_dev, ntrees, total, max_count, reinterpret_cast<uint32_t*>(info_dev)));
    for (uint32_t l = 1; l <= H; ++l) {   // level l against level l - 1, both as they are stored
        const Node* in = (l == 1) ? digests : forest + vkmr_forest::stored_level_base(total, ntrees, l - 1);
        const uint64_t cells = vkmr_forest::level_cells(total, ntrees, l);
        VKMR_CHECK(launch(forest_audit_level_kernel, grid_of(cells), block, S(s), in, forest + vkmr_forest::stored_level_base(total, ntrees, l), roots,
                          offsets_dev, ntrees, l, cells, masks_dev, capacity ? sc.mask + vkmr_audit::forest_word_base(total, ntrees, l) : (uint64_t*)nullptr,
                          info_dev));
    }
    if (capacity == 0) return VKMR_OK;
    VKMR_CHECK(audit_rank_launch(S(s), sc, vkmr_audit::forest_word_base(total, ntrees, H + 1u)));
    for (uint32_t l = 1; l <= H; ++l) {
        const uint64_t cells = vkmr_forest::level_cells(total, ntrees, l), base = vkmr_audit::forest_word_base(total, ntrees, l);
        VKMR_CHECK(launch(forest_audit_emit_kernel, grid_of(cells), block, S(s), offsets_dev, ntrees, l, cells, sc.mask + base, sc.word_start + base,
                          bad_trees_dev, bad_levels_dev, bad_nodes_dev, capacity, info_dev, l == H ? 1u : 0u));
    }
    return VKMR_OK;
}

vkmr_status vkmr_hip_tree_audit_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev, const vkmr_digest* tree_dev, uint64_t count, uint32_t height,
                                      void* scratch_dev, uint32_t* bad_levels_dev, uint64_t* bad_nodes_dev, uint32_t capacity, uint64_t* info_dev)
{
    if (count == 0) return VKMR_OK;
    if (!digests_dev || (height > 0 && !tree_dev) || !info_dev || (capacity > 0 && (!scratch_dev || !bad_levels_dev || !bad_nodes_dev)))
        return refuse(__func__, "null pointer");
    if (!height_ok(count, height)) return refuse(__func__, "height does not reduce count to one node");
    if (count > (1ull << 58) || grid_too_large(groups_of(ceil_shift(count, 1)))) return refuse(__func__, "too many leaves");
    if (capacity > 0 && (reinterpret_cast<uintptr_t>(scratch_dev) & 15u)) return refuse(__func__, "scratch must be 16-byte aligned");
    if (capacity > 0 && ceil_shift(count, 1) > vkmr_audit::MAX_LIST_CELLS)
        return refuse(__func__, "a level of more than 2^32 - 1 cells cannot be listed: capacity must be 0");
    const TreeLevels lv = tree_levels(count, height);
    const AuditScratch sc(scratch_dev, vkmr_audit::layout(count, 1u, capacity), capacity);
    const Node *digests = nodes(digests_dev), *tree = nodes(tree_dev);
    const dim3 block(VKMR_AUDIT_THREADS);
    VKMR_TRY(hipSetDevice(dev));
    VKMR_TRY(hipMemsetAsync(info_dev, 0, 4 * sizeof(uint64_t), S(s)));
    if (height == 0) return VKMR_OK;   // one leaf, no level: the root is the leaf, and there is no node to check
    if (capacity) VKMR_TRY(hipMemsetAsync(sc.hdr, 0, VKMR_AUDIT_HEADER_WORDS * sizeof(uint64_t), S(s)));
    for (uint32_t l = 1; l <= height; ++l) {
        const uint64_t n_in = ceil_shift(count, l - 1), n_out = ceil_shift(count, l);
        VKMR_CHECK(launch(tree_audit_level_kernel, grid_of(n_out), block, S(s), l == 1 ? digests : tree + lv.off[l - 1], tree + lv.off[l], n_in, n_out, l,
                          capacity ? sc.mask + vkmr_audit::tree_word_base(count, l) : (uint64_t*)nullptr, info_dev));
    }
    if (capacity == 0) return VKMR_OK;
    VKMR_CHECK(audit_rank_launch(S(s), sc, vkmr_audit::tree_word_base(count, height + 1u)));
    for (uint32_t l = 1; l <= height; ++l) {
        const uint64_t n_out = ceil_shift(count, l), base = vkmr_audit::tree_word_base(count, l);
        VKMR_CHECK(launch(tree_audit_emit_kernel, grid_of(n_out), block, S(s), n_out, l, sc.mask + base, sc.word_start + base, bad_levels_dev, bad_nodes_dev,
                          capacity, info_dev, l == height ? 1u : 0u));
    }
    return VKMR_OK;
}

// ---- combine --------------------------------------------------------------------

vkmr_status vkmr_hip_combine_async(int dev, vkmr_stream s, const vkmr_digest* roots_dev, uint32_t n, void* scratch_dev,
                                   vkmr_digest* root_dev)
{
    if (!roots_dev || !root_dev || n == 0) return refuse(__func__, "bad argument");
    return vkmr_hip_reduce_async(dev, s, roots_dev, n, vkmr_math::height(n), scratch_dev, root_dev);   // at least one level
}

void vkmr_hip_digest_hex(const vkmr_digest* d, char* hex)
{
    static const char digits[] = "0123456789abcdef";
    for (int i = 0; i < 8; ++i)
        for (int b = 0; b < 4; ++b) {
            const unsigned v = (d->data[i] >> (24 - 8 * b)) & 0xffu;
            hex[8 * i + 2 * b] = digits[v >> 4];
            hex[8 * i + 2 * b + 1] = digits[v & 15u];
        }
    hex[64] = 0;
}

}  // extern "C"

#include "comm_rccl.hpp"
