// abi_plan_test.cpp -- CPU-side replay of the integer rules the C ABI (vkmr_hip.hip) takes from the plan headers: the
// multiproof scratch layout and the stored tree's levels (csrc/tree_plan.hpp), the chunks and the scratch of a run of slices
// (csrc/reduce_plan.hpp), the map kernel's mode and tile (csrc/map_plan.hpp).  Every expectation is worked out here on its
// own, not through the header under test.  Built and run by tests/test_abi_plans.py (no GPU).
//
//   abi_plan_test layout    per (k, height): `k height bytes` after the checks; the test compares bytes with the library's
//   abi_plan_test slices    every chunk of every (capacity, nslices, count_last) fits vkmr_plan::slices_scratch_cells
//   abi_plan_test levels    level offsets and cell counts of stored trees against sums of ceil(count / 2^j)
//   abi_plan_test map DATA_WORDS COUNT    the mode ladder, the tiles, and `bench <mode> <tile> <avg_words>` for the given shape
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "map_plan.hpp"
#include "reduce_plan.hpp"
#include "tree_plan.hpp"

#define CHECK(cond, ...)                    \
    do {                                    \
        if (!(cond)) {                      \
            printf("FAIL: " __VA_ARGS__);   \
            printf("\n");                   \
            exit(1);                        \
        }                                   \
    } while (0)

typedef unsigned long long ull;

static const uint32_t KS[] = {1, 63, 64, 65, 16383, 16384, 16385};

static int layout()
{
    const uint32_t heights[] = {1, 2, 26, 58, 63};
    for (uint32_t k : KS)
        for (uint32_t h : heights) {
            const vkmr_tree::MultiproofLayout L = vkmr_tree::multiproof_layout(k, h);
            const uint64_t words = ((uint64_t)k + 63) / 64, blocks = (words + 255) / 256;   // 64 entries a word, 256 words a block
            CHECK(L.words == words && L.blocks == blocks, "words / blocks of k=%u", k);
            // cell, mask, word_start, block, hdr, end, back to back: each part starts where the one before it ends
            const size_t start[] = {L.cell, L.mask, L.word_start, L.block, L.hdr, L.end, L.bytes};
            const size_t size[] = {(size_t)k * 32, (size_t)(words * h) * 8, (size_t)(words * h) * 8, (size_t)(blocks * h) * 8, (size_t)(2 + 64) * 8, (size_t)k * 4};
            CHECK(L.cell == 0, "the cells do not come first (k=%u h=%u)", k, h);
            for (int p = 0; p < 6; ++p)
                CHECK(start[p + 1] == start[p] + size[p], "part %d overlaps the next or leaves a gap (k=%u h=%u)", p, k, h);
            CHECK(L.mask % 8 == 0 && L.word_start % 8 == 0 && L.block % 8 == 0 && L.hdr % 8 == 0, "a 64-bit part off the 8-byte grid (k=%u h=%u)", k, h);
            CHECK(L.end % 4 == 0, "end off the 4-byte grid (k=%u h=%u)", k, h);
            printf("%u %u %llu\n", k, h, (ull)L.bytes);
        }
    printf("ok: layout\n");
    return 0;
}

static int slices()
{
    const uint64_t capacities[] = {1, 2, 127, 128, 129, 255, 256, 257, 4096, 16383, 16384, 16385, (1ull << 18) + 1, (1ull << 19) - 1, 1ull << 19, (1ull << 19) + 1, 1ull << 26};
    const uint32_t runs[] = {1, 2, 3, 15, 16, 17, 2047, 2048, 4096, 32767, 32768, 32769, 65536, 65537, 98305};
    ull chunks_seen = 0;
    for (uint64_t capacity : capacities)
        for (uint32_t nslices : runs) {
            const uint64_t budget = vkmr_plan::slices_scratch_cells(capacity, nslices);
            const vkmr_plan::SliceChunks ch = vkmr_plan::slice_chunks(nslices);
            uint64_t covered = 0;
            for (uint32_t c = 0; c < ch.count(); ++c) {
                const uint32_t n = ch.size(c);
                CHECK(n >= 1 && n <= 32768u, "a chunk of %u slices", n);
                CHECK(ch.first(c) == covered, "chunk %u does not start where the one before ended", c);
                CHECK(c + 1 == ch.count() || n == 32768u, "a short chunk that is not the last");
                covered += n;
                // the launches of a chunk follow a full slice's schedule; a run of one slice follows its only slice's, of any length
                const uint64_t lasts[] = {capacity, capacity - capacity / 3, (capacity + 1) / 2, 129 < capacity ? 129 : capacity, 1};
                for (uint64_t count_last : lasts) {
                    const uint64_t n_full = nslices == 1 ? count_last : capacity;
                    CHECK(vkmr_plan::cells_written(n_full, n) * n <= budget, "capacity %llu, %u slices: a chunk of %u writes %llu cells, the scratch has %llu",
                          (ull)capacity, nslices, n, (ull)(vkmr_plan::cells_written(n_full, n) * n), (ull)budget);
                }
                ++chunks_seen;
            }
            CHECK(covered == nslices, "the chunks of %u slices cover %llu", nslices, (ull)covered);
        }
    CHECK(vkmr_plan::slice_chunks(98305).count() == 4 && vkmr_plan::slice_chunks(98305).size(3) == 1, "98305 slices: three full chunks and one slice");
    printf("ok: slices, %llu chunks\n", chunks_seen);
    return 0;
}

// ceil(count / 2^j) by division, j <= 63
static uint64_t ceil_div_pow2(uint64_t count, uint32_t j) { return (count >> j) + ((count & ((1ull << j) - 1)) ? 1 : 0); }

static int levels()
{
    uint64_t counts[200];
    int n = 0;
    for (uint64_t c : {1ull, 2ull, 3ull, 127ull, 128ull, 129ull}) counts[n++] = c;
    for (int e = 3; e <= 62; e += (e < 20 ? 1 : 7))
        for (int d = -1; d <= 1; ++d) counts[n++] = (1ull << e) + d;
    counts[n++] = 1ull << 58;
    counts[n++] = (1ull << 63) - 1;
    counts[n++] = 1ull << 63;
    for (int i = 0; i < n; ++i) {
        const uint64_t count = counts[i];
        uint32_t height = 0;
        while (height < 63 && ceil_div_pow2(count, height) > 1) ++height;
        for (uint32_t h : {height, height + 1 > 63 ? 63u : height + 1}) {   // the tree's own height, and one level above the root
            uint64_t off[VKMR_TREE_MAX_LEVELS];
            memset(off, 0xEE, sizeof off);
            const uint64_t cells = vkmr_tree::levels(count, h, off);
            uint64_t sum = 0;
            CHECK(off[0] == 0, "off[0] of count %llu", (ull)count);
            for (uint32_t l = 1; l <= h; ++l) {
                CHECK(off[l] == sum, "off[%u] of count %llu is %llu, the levels below have %llu cells", l, (ull)count, (ull)off[l], (ull)sum);
                sum += ceil_div_pow2(count, l);
            }
            CHECK(cells == sum && vkmr_tree::cells(count, h) == sum, "count %llu, height %u: %llu cells, the levels sum to %llu", (ull)count, h, (ull)cells, (ull)sum);
        }
        CHECK(vkmr_plan::height_ok(count, height) && (height == 0 || !vkmr_plan::height_ok(count, height - 1)), "height_ok at count %llu", (ull)count);
    }
    CHECK(!vkmr_plan::height_ok(0, 0) && !vkmr_plan::height_ok(1, 64) && vkmr_plan::height_ok(1, 63) && vkmr_plan::height_ok(1, 0), "height_ok at the edges");
    // multiproof_max_nodes: at most one node per pair of every level, and never more than k a level
    for (uint64_t count : {1ull, 2ull, 129ull, 1ull << 20, (1ull << 58) + 1})
        for (uint32_t k : KS) {
            uint32_t height = 0;
            while (ceil_div_pow2(count, height) > 1) ++height;
            uint64_t sum = 0;
            for (uint32_t l = 0; l < height; ++l) sum += ceil_div_pow2(count, l + 1) < k ? ceil_div_pow2(count, l + 1) : k;
            CHECK(vkmr_tree::multiproof_max_nodes(count, height, k) == sum, "multiproof_max_nodes(%llu, %u, %u)", (ull)count, height, k);
        }
    printf("ok: levels, %d counts\n", n);
    return 0;
}

static const char* mode_name(vkmr_map::Mode m)
{
    switch (m) {
        case vkmr_map::STAGED: return "STAGED";
        case vkmr_map::DIRECT512: return "DIRECT512";
        case vkmr_map::DIRECT256: return "DIRECT256";
        case vkmr_map::LONG512: return "LONG512";
        case vkmr_map::LONG256: return "LONG256";
    }
    return "?";
}

static int map(uint64_t bench_words, uint32_t bench_count)
{
    using namespace vkmr_map;
    // the smallest count whose per-lane tile reaches 1024: (count / 1024) & ~63 >= 1024, found here by walking, not by formula
    uint32_t big = 0;
    for (uint32_t c = 1; c < (1u << 24); ++c) {
        const uint32_t t = direct_tile(c);
        CHECK(t % 64 == 0 && t >= 256 && t <= 2048, "direct_tile(%u) = %u", c, t);
        if (!big && t >= 1024) big = c;
        CHECK(!big || t >= 1024, "direct_tile falls below 1024 again at %u", c);
    }
    CHECK(big == 1024u * 1024u, "direct_tile reaches 1024 at %u", big);
    const uint32_t counts[] = {1, 2, 255, 256, 257, 4096, 65535, 65536, big - 1, big, big + 1, 1u << 21, (1u << 21) - 1, 1u << 26, 0xFFFFFFFFu};
    for (uint32_t count : counts) {
        const bool wide = count >= big;
        for (uint64_t avg : {1ull, 2ull, 17ull, 31ull, 32ull, 33ull, 127ull, 128ull, 129ull, 1024ull}) {
            // the average is ceil(data_words / count): its first and last data_words, and one below the first
            const uint64_t lo = (avg - 1) * count + 1, hi = avg * count;
            for (uint64_t words : {lo - 1, lo, hi}) {
                const uint64_t a = words == lo - 1 ? avg - 1 : avg;
                const Plan p = plan(words, count);
                const Mode want = a >= 128 ? (wide ? LONG512 : LONG256) : a >= 32 ? (wide ? DIRECT512 : DIRECT256) : STAGED;
                CHECK(avg_words(words, count) == a, "avg_words(%llu, %u)", (ull)words, count);
                CHECK(p.mode == want, "count %u, %llu words (%llu on average): %s, not %s", count, (ull)words, (ull)a, mode_name(p.mode), mode_name(want));
                CHECK(p.tile % 64 == 0 && p.tile >= 256 && p.tile <= (p.mode == STAGED ? 1024u : 2048u), "count %u, %llu words: tile %u", count, (ull)words, p.tile);
                CHECK(p.mode == STAGED || p.tile == direct_tile(count), "a per-lane mode with another tile than direct_tile's");
                CHECK((uint64_t)tiles_of(count, p.tile) * p.tile >= count && (uint64_t)(tiles_of(count, p.tile) - 1) * p.tile < count, "tiles_of(%u, %u)", count, p.tile);
            }
        }
    }
    // staged tiles under the experiments' fit_pct as well: still whole groups of 64 inside [max_tile / 4, max_tile]
    for (uint32_t count : counts)
        for (uint64_t avg : {1ull, 8ull, 17ull, 31ull})
            for (int fit : {0, 50, 75, 100}) {
                const uint32_t t = staged_tile(avg * count, count, 1024, 17664, fit);
                CHECK(t % 64 == 0 && t >= 256 && t <= 1024, "staged_tile(count %u, avg %llu, fit %d) = %u", count, (ull)avg, fit, t);
            }
    const Plan b = plan(bench_words, bench_count);
    printf("bench %s %u %llu\n", mode_name(b.mode), b.tile, (ull)avg_words(bench_words, bench_count));
    printf("ok: map\n");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 2 && strcmp(argv[1], "layout") == 0) return layout();
    if (argc == 2 && strcmp(argv[1], "slices") == 0) return slices();
    if (argc == 2 && strcmp(argv[1], "levels") == 0) return levels();
    if (argc == 4 && strcmp(argv[1], "map") == 0) return map(strtoull(argv[2], nullptr, 10), (uint32_t)strtoull(argv[3], nullptr, 10));
    fprintf(stderr, "usage: %s layout | slices | levels | map DATA_WORDS COUNT\n", argv[0]);
    return 2;
}
