// leafsort_plan.hpp -- the leaves of a forest sorted on the device, tree by tree, in digest order (include/vkmr_hip.h:
// vkmr_hip_forest_sort_leaves_async, vkmr_hip_tree_sort_leaves_async): the sort key, the passes, the elements, what a tie is and
// the scratch layout.  Plain integer arithmetic, no HIP types: shared by the kernels (leafsort_kernels.hpp), the C ABI
// (vkmr_hip.hip), the CPU twins (host/host_api.cpp) and the replay in tests/c/leafsort_plan_test.cpp; the tests read the
// constants below from this text.
//
// THE ORDER is absence_plan.hpp's: word 0 first, every word unsigned.  Equal digests keep their input order (a stable sort).
//
// THE KEY.  One global radix sort (sort_plan.hpp's engine, 8 bits a pass) of 64-bit keys with the tree on top, so that the
// segments stay where they are:
//   bits_T = bit_length(ntrees - 1)                               0 for one tree
//   P      = min(64 - bits_T, 2 * bit_length(max_count) + 8)      8 <= P <= 64
//   key    = (tree << P) | (prefix64 >> (64 - P)),  prefix64 = word0 << 32 | word1
//   passes = ceil((bits_T + P) / 8)                               at most 8
// key(a) < key(b) implies (tree, digest) a < b; equal keys say nothing, and the ties are placed by all 256 bits afterwards.  A
// narrower prefix drops passes where trees are small: 2^15 trees of 2 048 leaves sort in 6 passes, not 8.  Among hashed leaves
// two leaves of one tree tie with probability 2^-P, so about n / (512 * max_count) leaves tie: a derivation, not a measurement
// (info[2] is there to judge it).
//
// THE ELEMENTS.  Element i of the sort is cell offsets[0] + i for i < n = offsets[ntrees] - offsets[0]; elements n <= i < total
// carry the all-ones SENTINEL; the grids are sized by `total`.  The sentinel can equal a real key (the last tree of 2^bits_T, a
// prefix of all ones).  Nothing goes wrong: the sentinels come behind every leaf in INPUT order and the sort is stable, so the
// sorted positions [0, n) hold the leaves whatever their keys.  That is why the elements are numbered from offsets[0] and not by
// flat cell: a leaf at a cell behind a sentinel would lose this order.
//
// TIES.  Sorted position j < n ties when its key equals that of position j - 1 or of j + 1 < n.  m, their number, is counted
// first; above VKMR_LEAFSORT_MAX_TIES the call refuses (status bit 2) and writes nothing.  Otherwise a position that does not tie
// has dest = j, and a tied one looks at its run [a, b) of equal keys: dest = a + the members that are `less` in all 256 bits, or
// equal and earlier in the run (earlier in the run is earlier in the input: the sort was stable) -- walking back from j and on
// from j + 1, dest = j - (earlier members that are greater) + (later members that are less).  A run is no longer than m, so the
// walk is bounded by MAX_TIES^2 compares for whatever input; that bound is the point of the limit.
//
// Scratch, in bytes from its start (16-byte aligned), every part a multiple of 16 bytes:
//   sort     sort_plan.hpp's layout for k = total (the ping-pong keys and positions, the histograms)
//   dest     4 * total: where sorted position j goes
//   hdr      8 * VKMR_LEAFSORT_HEADER_WORDS: [0] status bits 0 and 1, [1] m, [2] leaves equal to an earlier one, [3] status bit 2
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "merkle_math.hpp"
#include "sort_plan.hpp"

#define VKMR_LEAFSORT_MAX_TIES 16384u            // 2^14: see DESIGN 3.30 for the measured pair that settles it
#define VKMR_LEAFSORT_HEADER_WORDS 4u
// info_dev[0] of vkmr_hip_forest_sort_leaves_async
#define VKMR_LEAFSORT_BAD_OFFSETS 1ull           // offsets decrease somewhere, or end behind `total`
#define VKMR_LEAFSORT_ABOVE_MAX_COUNT 2ull       // a tree of more than max_count leaves
#define VKMR_LEAFSORT_TOO_MANY_TIES 4ull         // m > VKMR_LEAFSORT_MAX_TIES

namespace vkmr_leafsort {

constexpr uint64_t MAX_TOTAL = 1ull << 32;       // total < 2^32: positions are uint32, as k is in sort_plan.hpp
constexpr uint64_t SENTINEL = ~0ull;

// bits_T and P of a call.
struct Shape {
    uint32_t bits_T, P;
};

inline Shape shape(uint32_t ntrees, uint64_t max_count)
{
    Shape s;
    s.bits_T = ntrees ? vkmr_sort::bit_length((uint64_t)ntrees - 1u) : 0u;     // <= 32
    const uint32_t wide = 2u * vkmr_sort::bit_length(max_count) + 8u;          // <= 136
    s.P = wide < 64u - s.bits_T ? wide : 64u - s.bits_T;
    return s;
}

inline uint32_t passes(const Shape& s) { return (s.bits_T + s.P + VKMR_SORT_RADIX_BITS - 1u) / VKMR_SORT_RADIX_BITS; }

// The key of a leaf of tree `tree` whose digest begins with the words w0, w1.  8 <= P <= 64: P == 64 is one tree and the whole
// prefix, and shifts by nothing; tree < 2^(64 - P).
VKMR_MATH_FN uint64_t key(uint32_t tree, uint32_t w0, uint32_t w1, uint32_t P)
{
    const uint64_t prefix = ((uint64_t)w0 << 32) | (uint64_t)w1;
    return P >= 64u ? prefix : (((uint64_t)tree << P) | (prefix >> (64u - P)));
}

// Where the sorted pairs lie after the last pass (sort_plan.hpp: pass p reads buffer p & 1).
inline uint32_t result_buffer(const Shape& s) { return passes(s) & 1u; }

struct Layout {
    vkmr_sort::Layout sort;
    size_t dest, hdr, bytes;
};

inline Layout layout(uint64_t total)   // total < MAX_TOTAL
{
    Layout L;
    L.sort = vkmr_sort::layout((uint32_t)total);
    size_t at = L.sort.bytes;          // every part of it is a multiple of 16 bytes
    L.dest = at;    at += vkmr_sort::up16((size_t)total * 4u);
    L.hdr = at;     at += vkmr_sort::up16((size_t)VKMR_LEAFSORT_HEADER_WORDS * 8u);
    L.bytes = at;
    return L;
}

inline size_t scratch_bytes(uint64_t total) { return (total == 0ull || total >= MAX_TOTAL) ? 0u : layout(total).bytes; }

}  // namespace vkmr_leafsort
