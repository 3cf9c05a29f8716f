// sort_plan.hpp -- the sizes of a device sort of leaf entries (include/vkmr_hip.h: vkmr_hip_forest_sort_entries_async,
// vkmr_hip_tree_sort_entries_async): the passes, the tiles, where a histogram word lies, the scan's span and the scratch
// layout.  Plain integer arithmetic, no HIP types: shared by the kernels (sort_kernels.hpp), the C ABI (vkmr_hip.hip) and the
// tests, which read the constants below from this text; tests/c/sort_plan_test.cpp replays the passes through these functions.
//
// The sort is a stable LSD radix sort of (key, q) pairs, 8 bits per pass.  The key of a valid entry is its flat position
// offsets[t] + index < total, that of every other entry the sentinel `total`; bit_length(total) bits are sorted, so at most 8
// passes (total <= 2^58).  A pass is three launches:
//   histogram  workgroup g counts the digits of tile g (keys [g * TILE, (g + 1) * TILE)) and writes word hist_word(bin, g, G)
//   scan       the exclusive prefix over the 256 * G words in word order, i.e. bin-major: workgroup b scans the G words of
//              bin b in place, VKMR_SORT_SCAN_SPAN words per trip, and leaves the bin's sum in totals[b]; the prefix over
//              the 256 sums is formed again by every scatter workgroup (256 lanes, one block scan)
//   scatter    key i of tile g with digit d goes to cell  prefix(d) + hist[d][g] + (keys of the tile before i with digit d)
// which is stable inside a tile and across tiles.  Pass p reads buffer p & 1 and writes the other.
//
// Scratch, in bytes from its start (16-byte aligned), every part rounded up to 16 bytes:
//   key[0], key[1]   8 k each   the ping-pong keys
//   val[0], val[1]   4 k each   the ping-pong payloads (q)
//   hist             4 * 256 * G, G = groups(k)
//   totals           4 * 256
//   mask             8 * W, W = ceil(k / 64): the ballot words of the survivor flags over the sorted keys
//   word_start       8 * W: survivors before each word
//   block            8 * ceil(W / 256): the sums / starts of blocks of 256 words
//   hdr              8 * 4: the ranking kernels' header (status, count, count of level 0)
#pragma once
#include <stddef.h>
#include <stdint.h>

#define VKMR_SORT_RADIX_BITS 8u        // bits per pass
#define VKMR_SORT_BINS 256u            // 2^VKMR_SORT_RADIX_BITS: one bin per lane of a workgroup
#define VKMR_SORT_THREADS 256u         // lanes of a histogram / scan / scatter workgroup
#define VKMR_SORT_KEYS_PER_LANE 4u     // keys a lane takes from its tile, one per round
#define VKMR_SORT_SCAN_SPAN 256u       // histogram words a scan workgroup takes per trip: one per lane
#define VKMR_SORT_RANK_BLOCK_WORDS 256u   // ballot words per block of the survivors' ranking (tree_plan.hpp: VKMR_MP_BLOCK_WORDS)

namespace vkmr_sort {

constexpr uint64_t MAX_TOTAL = 1ull << 58;

// Keys of one tile.
constexpr uint32_t tile_keys() { return VKMR_SORT_THREADS * VKMR_SORT_KEYS_PER_LANE; }

inline uint32_t bit_length(uint64_t v)
{
    uint32_t n = 0;
    while (v) { ++n; v >>= 1; }
    return n;
}

// Passes that sort every key <= total: ceil(bit_length(total) / 8); none for total == 0 (every key is the sentinel 0).
inline uint32_t passes(uint64_t total) { return (bit_length(total) + VKMR_SORT_RADIX_BITS - 1u) / VKMR_SORT_RADIX_BITS; }

// The digit pass p sorts by.  (constexpr: the kernels call these three as well)
constexpr uint32_t digit(uint64_t key, uint32_t p) { return (uint32_t)(key >> (VKMR_SORT_RADIX_BITS * p)) & (VKMR_SORT_BINS - 1u); }

// G: tiles, and workgroups of the histogram and the scatter.
inline uint64_t groups(uint32_t k) { return ((uint64_t)k + tile_keys() - 1u) / tile_keys(); }

// The tile of key i.
constexpr uint64_t tile_of(uint64_t i) { return i / tile_keys(); }

// Where the count of (bin, group) lies among the 256 * G histogram words: bin-major, so that the exclusive prefix in word
// order puts every smaller digit first and, inside a digit, every earlier tile first.
constexpr uint64_t hist_word(uint32_t bin, uint64_t group, uint64_t G) { return (uint64_t)bin * G + group; }
constexpr uint64_t hist_words(uint64_t G) { return (uint64_t)VKMR_SORT_BINS * G; }

// Trips of one scan workgroup over its bin's G words.
inline uint64_t scan_trips(uint64_t G) { return (G + VKMR_SORT_SCAN_SPAN - 1u) / VKMR_SORT_SCAN_SPAN; }

// The buffer (0 or 1) pass p reads; it writes the other.  result_buffer: where the sorted pairs lie after the last pass.
inline uint32_t pass_input(uint32_t p) { return p & 1u; }
inline uint32_t result_buffer(uint64_t total) { return passes(total) & 1u; }

struct Layout {
    uint64_t G, words, blocks;
    size_t key[2], val[2], hist, totals, mask, word_start, block, hdr, bytes;
};

inline size_t up16(size_t n) { return (n + 15u) & ~(size_t)15u; }

inline Layout layout(uint32_t k)
{
    Layout L;
    L.G = groups(k);
    L.words = ((uint64_t)k + 63u) / 64u;
    L.blocks = (L.words + VKMR_SORT_RANK_BLOCK_WORDS - 1u) / VKMR_SORT_RANK_BLOCK_WORDS;
    size_t at = 0;
    L.key[0] = at;      at += up16((size_t)k * 8u);
    L.key[1] = at;      at += up16((size_t)k * 8u);
    L.val[0] = at;      at += up16((size_t)k * 4u);
    L.val[1] = at;      at += up16((size_t)k * 4u);
    L.hist = at;        at += up16((size_t)hist_words(L.G) * 4u);
    L.totals = at;      at += up16((size_t)VKMR_SORT_BINS * 4u);
    L.mask = at;        at += up16((size_t)L.words * 8u);
    L.word_start = at;  at += up16((size_t)L.words * 8u);
    L.block = at;       at += up16((size_t)L.blocks * 8u);
    L.hdr = at;         at += 32u;
    L.bytes = at;
    return L;
}

// The layout depends on k alone today; `total` is part of the sizing call so that narrower keys for small totals can be
// laid out later without another entry point.
inline size_t scratch_bytes(uint64_t total, uint32_t k)
{
    (void)total;
    return k ? layout(k).bytes : 0u;
}

}  // namespace vkmr_sort
