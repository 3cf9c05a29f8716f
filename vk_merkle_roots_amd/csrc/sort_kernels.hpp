// sort_kernels.hpp -- leaf entries sorted and deduplicated on the device (include/vkmr_hip.h: vkmr_hip_forest_sort_entries_async,
// vkmr_hip_tree_sort_entries_async, vkmr_hip_gather_digests_async; sizes and scratch layout: sort_plan.hpp).  No hash is
// computed here.
//
// A stable LSD radix sort of (flat key, q) pairs, then the last pair of every run of equal keys is kept:
//   *_sort_keys_kernel     one lane per entry: key = offsets[t] + index for a valid entry, `total` for every other; payload q;
//                          the markers and the out-of-range entries are counted
//   sort_histogram_kernel  one workgroup per tile: the 256 digit counts of the tile, written bin-major
//   sort_scan_kernel       one workgroup per bin: the exclusive prefix over the bin's G words in place, and the bin's sum
//   sort_scatter_kernel    one workgroup per tile: every pair to  prefix(digit) + hist[digit][tile] + rank in the tile
//   sort_flags_kernel      one lane per sorted key: the survivor flags as ballot words
//   (tree_kernels.hpp's three ranking kernels, one level: survivors before each ballot word, and their number)
//   *_sort_emit_kernel     one lane per sorted key: a survivor's (tree, index, q) written at its rank; the counters completed
// No kernel waits for another workgroup: the order between the phases is that of the launches.  Nothing depends on the order
// in which atomics arrive: the LDS atomics of the histogram and the atomics of the two counters of left-out entries only
// count, and a pair's destination follows from the counts and its own place in the tile.
//
// A forest and one tree differ in how an entry becomes a key and how a key is reported: the two structs below, in
// entries.hpp's manner -- one body per kernel, and a __global__ kernel is its arguments as the struct and the call.
#pragma once

#include "sort_plan.hpp"

enum { SORT_VALID = 0, SORT_MARKER = 1, SORT_OUTSIDE = 2 };

// Entry q of a forest is (trees[q], indices[q]); the offsets are trusted as vkmr_hip_forest_find_async trusts them
// (non-decreasing, ending at or before `total`); a key at or past `total` is held to be outside all the same, so that no
// key has a bit the passes do not sort.
struct SortForest {
    const uint64_t* offsets; uint32_t ntrees; uint64_t total; const uint32_t* trees; uint32_t* trees_out;
    __device__ __forceinline__ uint32_t key(uint64_t q, const uint64_t* __restrict__ indices, uint64_t* out) const
    {
        const uint32_t t = trees[q];
        if (t == 0xFFFFFFFFu) return SORT_MARKER;
        if (t >= ntrees) return SORT_OUTSIDE;
        const uint64_t index = indices[q], o = offsets[t], c = offsets[t + 1u] - o;
        if (index >= c || index >= total - (o < total ? o : total)) return SORT_OUTSIDE;
        *out = o + index;
        return SORT_VALID;
    }
    // key < offsets[ntrees]: the tree is the upper bound of the key in offsets[0 .. ntrees], minus one (FindForest::found);
    // an empty tree has an empty range and is never named.
    __device__ __forceinline__ void emit(uint64_t rank, uint64_t key, uint64_t* __restrict__ indices_out) const
    {
        uint32_t a = 1u, b = ntrees;
        while (a < b) {
            const uint32_t mid = a + (b - a) / 2u;
            if (offsets[mid] > key) b = mid;
            else a = mid + 1u;
        }
        trees_out[rank] = a - 1u;
        indices_out[rank] = key - offsets[a - 1u];
    }
};

// One tree of `count` leaves at cell 0: the key is the index.
struct SortTree {
    uint64_t count;
    __device__ __forceinline__ uint32_t key(uint64_t q, const uint64_t* __restrict__ indices, uint64_t* out) const
    {
        const uint64_t index = indices[q];
        if (index == ~0ull) return SORT_MARKER;
        if (index >= count) return SORT_OUTSIDE;
        *out = index;
        return SORT_VALID;
    }
    __device__ __forceinline__ void emit(uint64_t rank, uint64_t key, uint64_t* __restrict__ indices_out) const { indices_out[rank] = key; }
};

// The entries a workgroup leaves out, counted: each wavefront adds the set bits of its two ballot words to two LDS words (an
// LDS atomic, for counting only), and the workgroup adds what is not zero to info[1] and info[2] -- one global atomic per
// workgroup and counter at the most; every wavefront adding to the same two words of memory was measured to cost more than the
// rest of the sort.  Every lane of the workgroup is here.
__device__ __forceinline__ void sort_count_left_out(unsigned long long* __restrict__ info, uint64_t markers, uint64_t outside)
{
    __shared__ uint32_t s_count[2];
    if (threadIdx.x < 2u) s_count[threadIdx.x] = 0u;
    __syncthreads();
    if ((threadIdx.x & 63u) == 0u) {
        if (markers) (void)atomicAdd(&s_count[0], (uint32_t)__popcll(markers));
        if (outside) (void)atomicAdd(&s_count[1], (uint32_t)__popcll(outside));
    }
    __syncthreads();
    if (threadIdx.x < 2u && s_count[threadIdx.x]) (void)atomicAdd(info + 1 + threadIdx.x, (unsigned long long)s_count[threadIdx.x]);
}

// One lane per entry.  info[1] and info[2] were zeroed before; `sentinel` is the launch's total (or count).
template <class Entries>
__device__ __forceinline__ void sort_keys(const Entries e, const uint64_t* __restrict__ indices, uint32_t k, uint64_t sentinel,
                                          uint64_t* __restrict__ key_out, uint32_t* __restrict__ val_out, unsigned long long* __restrict__ info)
{
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t key = sentinel;
    const uint32_t kind = q < k ? e.key(q, indices, &key) : (uint32_t)SORT_VALID;
    if (q < k) {
        key_out[q] = kind == SORT_VALID ? key : sentinel;
        val_out[q] = (uint32_t)q;
    }
    const uint64_t markers = __ballot(kind == SORT_MARKER), outside = __ballot(kind == SORT_OUTSIDE);
    sort_count_left_out(info, markers, outside);
}

__global__ __launch_bounds__(256) void forest_sort_keys_kernel(const uint64_t* __restrict__ offsets, uint32_t ntrees, uint64_t total,
                                                               const uint32_t* __restrict__ trees, const uint64_t* __restrict__ indices, uint32_t k,
                                                               uint64_t* __restrict__ key_out, uint32_t* __restrict__ val_out,
                                                               unsigned long long* __restrict__ info)
{
    sort_keys(SortForest{offsets, ntrees, total, trees, nullptr}, indices, k, total, key_out, val_out, info);
}

__global__ __launch_bounds__(256) void tree_sort_keys_kernel(uint64_t count, const uint64_t* __restrict__ indices, uint32_t k,
                                                             uint64_t* __restrict__ key_out, uint32_t* __restrict__ val_out,
                                                             unsigned long long* __restrict__ info)
{
    sort_keys(SortTree{count}, indices, k, count, key_out, val_out, info);
}

// Workgroup g counts the digits of tile g.  LDS atomics, for counting only; lane b then writes bin b's word.
__global__ __launch_bounds__(VKMR_SORT_THREADS) void sort_histogram_kernel(const uint64_t* __restrict__ keys, uint32_t k, uint32_t pass, uint64_t G,
                                                                           uint32_t* __restrict__ hist)
{
    __shared__ uint32_t s_bin[VKMR_SORT_BINS];
    s_bin[threadIdx.x] = 0u;
    __syncthreads();
    const uint64_t first = (uint64_t)blockIdx.x * vkmr_sort::tile_keys() + threadIdx.x;
#pragma unroll
    for (uint32_t r = 0; r < VKMR_SORT_KEYS_PER_LANE; ++r) {
        const uint64_t i = first + (uint64_t)r * VKMR_SORT_THREADS;
        if (i < k) (void)atomicAdd(&s_bin[vkmr_sort::digit(keys[i], pass)], 1u);
    }
    __syncthreads();
    hist[vkmr_sort::hist_word(threadIdx.x, blockIdx.x, G)] = s_bin[threadIdx.x];
}

// Workgroup b: hist[b][0 .. G) becomes its exclusive prefix, totals[b] its sum (at most k < 2^32).  G is a kernel argument:
// the trip count is the same in every lane.
__global__ __launch_bounds__(VKMR_SORT_THREADS) void sort_scan_kernel(uint32_t* __restrict__ hist, uint64_t G, uint32_t* __restrict__ totals)
{
    __shared__ uint32_t s_wave[VKMR_SORT_THREADS / 64];
    uint32_t* row = hist + vkmr_sort::hist_word(blockIdx.x, 0, G);
    uint32_t carry = 0u;
    for (uint64_t base = 0; base < G; base += VKMR_SORT_SCAN_SPAN) {
        const uint64_t g = base + threadIdx.x;
        const uint32_t v = g < G ? row[g] : 0u;
        uint32_t total;
        const uint32_t ex = vkmr_sizes::block_exclusive(v, s_wave, &total);
        if (g < G) row[g] = carry + ex;
        carry += total;
        __syncthreads();   // s_wave is reused by the next trip
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}

// Workgroup g scatters tile g.  s_base[d] is where the tile's next key with digit d goes: the keys with smaller digits
// (the prefix over totals, formed here), those with digit d in earlier tiles (the scanned histogram word), and those of
// this tile's earlier rounds.  A round is one key per lane, in key order: inside it a key's rank among the keys with its
// digit is the matching lanes below it in its wavefront (eight ballots give the lanes with the same digit) plus the matches
// in the wavefronts before (s_wave, written by the lowest matching lane of each wavefront: one writer per word).  So a key
// goes behind every earlier key with its digit: the pass is stable.
__global__ __launch_bounds__(VKMR_SORT_THREADS) void sort_scatter_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, uint32_t k,
                                                                         uint32_t pass, uint64_t G, const uint32_t* __restrict__ hist,
                                                                         const uint32_t* __restrict__ totals, uint64_t* __restrict__ keys_out,
                                                                         uint32_t* __restrict__ vals_out)
{
    constexpr uint32_t WAVES = VKMR_SORT_THREADS / 64;
    __shared__ uint32_t s_scan[WAVES];
    __shared__ uint32_t s_base[VKMR_SORT_BINS];
    __shared__ uint32_t s_wave[WAVES][VKMR_SORT_BINS];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t all;
    s_base[threadIdx.x] = vkmr_sizes::block_exclusive(totals[threadIdx.x], s_scan, &all) + hist[vkmr_sort::hist_word(threadIdx.x, blockIdx.x, G)];
    const uint64_t first = (uint64_t)blockIdx.x * vkmr_sort::tile_keys() + threadIdx.x;
    for (uint32_t r = 0; r < VKMR_SORT_KEYS_PER_LANE; ++r) {   // the same trips in every lane
#pragma unroll
        for (uint32_t w = 0; w < WAVES; ++w) s_wave[w][threadIdx.x] = 0u;
        const uint64_t i = first + (uint64_t)r * VKMR_SORT_THREADS;
        const bool in = i < k;
        const uint64_t key = in ? keys[i] : 0ull;
        const uint32_t val = in ? vals[i] : 0u;
        const uint32_t d = vkmr_sort::digit(key, pass);
        uint64_t same = __ballot(in);                  // the lanes of this wavefront that hold a key with digit d
#pragma unroll
        for (uint32_t b = 0; b < VKMR_SORT_RADIX_BITS; ++b) {
            const uint64_t set = __ballot((d >> b) & 1u);
            same &= ((d >> b) & 1u) ? set : ~set;
        }
        const uint32_t below = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
        __syncthreads();                               // s_wave is zero, s_base is this round's
        if (in && below == 0u) s_wave[wave][d] = (uint32_t)__popcll(same);
        __syncthreads();
        if (in) {
            uint32_t at = s_base[d] + below;
#pragma unroll
            for (uint32_t w = 0; w < WAVES; ++w) at += w < wave ? s_wave[w][d] : 0u;
            keys_out[at] = key;                        // at < k: the counts of all tiles and digits add up to k
            vals_out[at] = val;
        }
        __syncthreads();                               // every lane has read s_base and s_wave
        uint32_t round = 0u;
#pragma unroll
        for (uint32_t w = 0; w < WAVES; ++w) round += s_wave[w][threadIdx.x];
        s_base[threadIdx.x] += round;
        __syncthreads();                               // before s_wave is zeroed again
    }
}

// One lane per sorted key j: it survives when it is a valid key (below the sentinel) and the last of its run.
// mask[j >> 6] = the survivors among 64 keys.  Nothing is counted here: the ranking gives the number of survivors.
__global__ __launch_bounds__(256) void sort_flags_kernel(const uint64_t* __restrict__ keys, uint32_t k, uint64_t sentinel, uint64_t words,
                                                         uint64_t* __restrict__ mask)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t key = j < k ? keys[j] : sentinel;
    const bool last = key < sentinel && (j + 1 >= k || keys[j + 1] != key);
    const uint64_t m = __ballot(last);
    if ((threadIdx.x & 63u) == 0u && (j >> 6) < words) mask[j >> 6] = m;
}

// One lane per sorted key: a survivor's pair and the q it came from, at its rank among the survivors.  Lane 0 of the launch
// completes the counters: hdr[1] is the ranking's total, the survivors n; info[1] and info[2] are final since the keys kernel;
// every other entry is a valid one that a later equal pair displaced: info[3] = k - info[1] - info[2] - n.
template <class Entries>
__device__ __forceinline__ void sort_emit(const Entries e, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, uint32_t k,
                                          const uint64_t* __restrict__ mask, const uint64_t* __restrict__ word_start, const uint64_t* __restrict__ hdr,
                                          uint64_t* __restrict__ indices_out, uint32_t* __restrict__ order_out, uint64_t* __restrict__ info)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j == 0) {
        const uint64_t n = hdr[1];
        info[0] = n;
        info[3] = (uint64_t)k - info[1] - info[2] - n;
    }
    if (j >= k) return;
    const uint64_t m = mask[j >> 6], bit = 1ull << (j & 63ull);
    if (!(m & bit)) return;
    const uint64_t rank = word_start[j >> 6] + (uint64_t)__popcll(m & (bit - 1ull));   // < survivors <= k
    e.emit(rank, keys[j], indices_out);
    order_out[rank] = vals[j];
}

__global__ __launch_bounds__(256) void forest_sort_emit_kernel(const uint64_t* __restrict__ offsets, uint32_t ntrees, const uint64_t* __restrict__ keys,
                                                               const uint32_t* __restrict__ vals, uint32_t k, const uint64_t* __restrict__ mask,
                                                               const uint64_t* __restrict__ word_start, const uint64_t* __restrict__ hdr,
                                                               uint32_t* __restrict__ trees_out, uint64_t* __restrict__ indices_out,
                                                               uint32_t* __restrict__ order_out, uint64_t* __restrict__ info)
{
    sort_emit(SortForest{offsets, ntrees, 0ull, nullptr, trees_out}, keys, vals, k, mask, word_start, hdr, indices_out, order_out, info);
}

__global__ __launch_bounds__(256) void tree_sort_emit_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, uint32_t k,
                                                             const uint64_t* __restrict__ mask, const uint64_t* __restrict__ word_start,
                                                             const uint64_t* __restrict__ hdr, uint64_t* __restrict__ indices_out,
                                                             uint32_t* __restrict__ order_out, uint64_t* __restrict__ info)
{
    sort_emit(SortTree{0ull}, keys, vals, k, mask, word_start, hdr, indices_out, order_out, info);
}

// dst[j] = src[order[j]], one lane per cell: two 16-byte loads and two 16-byte stores.
__global__ __launch_bounds__(256) void gather_digests_kernel(const Node* __restrict__ src, const uint32_t* __restrict__ order, uint32_t n,
                                                             Node* __restrict__ dst)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    vkmr_dev::store_node(dst + j, vkmr_dev::load_node(src + order[j]));
}
