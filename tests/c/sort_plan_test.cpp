// sort_plan_test.cpp -- csrc/sort_plan.hpp replayed on the CPU: the radix passes of the entry sort, through the plan's own
// functions for tile -> group, (bin, group) -> word, the scan's order and trips, and destination = base + rank in the tile.
// A stand-alone program (tests/test_sort_entries_abi.py compiles it, plain and with -fsanitize=address,undefined):
//   sort_plan_test [cases.txt]     one case per line: total k key_0 .. key_{k-1}; then random inputs of its own
// For every input: every pass is a stable permutation, every destination is hit once, every histogram word lies inside the
// part of the scratch the plan gives it, the parts of the scratch do not overlap, and after the last pass the keys are sorted
// with equal keys in call order.  Prints "FAIL ..." and returns 1 otherwise.
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "sort_plan.hpp"

namespace {

int g_fail = 0;

#define CHECK(cond, ...)                       \
    do {                                       \
        if (!(cond)) {                         \
            if (g_fail++ < 20) {               \
                std::printf("FAIL %s: ", #cond); \
                std::printf(__VA_ARGS__);      \
                std::printf("\n");             \
            }                                  \
            return false;                      \
        }                                      \
    } while (0)

struct Part { const char* name; size_t at, bytes; };

// The parts of the layout, each with the bytes the kernels use of it.
std::vector<Part> parts_of(const vkmr_sort::Layout& L, uint32_t k)
{
    return {{"key0", L.key[0], (size_t)k * 8}, {"key1", L.key[1], (size_t)k * 8}, {"val0", L.val[0], (size_t)k * 4}, {"val1", L.val[1], (size_t)k * 4},
            {"hist", L.hist, (size_t)vkmr_sort::hist_words(L.G) * 4}, {"totals", L.totals, (size_t)VKMR_SORT_BINS * 4}, {"mask", L.mask, (size_t)L.words * 8},
            {"word_start", L.word_start, (size_t)L.words * 8}, {"block", L.block, (size_t)L.blocks * 8}, {"hdr", L.hdr, 32}};
}

bool check_layout(uint32_t k, uint64_t total)
{
    const vkmr_sort::Layout L = vkmr_sort::layout(k);
    const std::vector<Part> parts = parts_of(L, k);
    CHECK(vkmr_sort::scratch_bytes(total, k) == L.bytes && L.bytes % 16 == 0, "k %u", k);
    CHECK(L.G == vkmr_sort::groups(k) && L.G * vkmr_sort::tile_keys() >= k && (L.G - 1) * vkmr_sort::tile_keys() < k, "k %u G %" PRIu64, k, L.G);
    CHECK(L.words * 64 >= k && L.blocks * VKMR_SORT_RANK_BLOCK_WORDS >= L.words, "k %u", k);
    for (size_t a = 0; a < parts.size(); ++a) {
        CHECK(parts[a].at % 16 == 0 && parts[a].at + parts[a].bytes <= L.bytes, "k %u part %s", k, parts[a].name);
        for (size_t b = a + 1; b < parts.size(); ++b)
            CHECK(parts[a].at + parts[a].bytes <= parts[b].at || parts[b].at + parts[b].bytes <= parts[a].at, "k %u parts %s and %s overlap", k,
                  parts[a].name, parts[b].name);
    }
    return true;
}

// One case: the passes of passes(total) over (keys, q).
bool replay(uint64_t total, const std::vector<uint64_t>& input)
{
    const uint32_t k = (uint32_t)input.size();
    CHECK(k > 0 && total <= vkmr_sort::MAX_TOTAL, "k %u", k);
    if (!check_layout(k, total)) return false;
    const vkmr_sort::Layout L = vkmr_sort::layout(k);
    const uint32_t passes = vkmr_sort::passes(total);
    CHECK(passes <= 8 && (passes == 8 || (total >> (8 * passes)) == 0) && (passes == 0 || (total >> (8 * (passes - 1))) != 0), "total %" PRIu64, total);
    for (uint64_t key : input) CHECK(key <= total, "key %" PRIu64 " above the sentinel %" PRIu64, key, total);

    std::vector<uint64_t> key[2] = {input, std::vector<uint64_t>(k)};
    std::vector<uint32_t> val[2] = {std::vector<uint32_t>(k), std::vector<uint32_t>(k)};
    for (uint32_t q = 0; q < k; ++q) val[0][q] = q;
    const uint64_t G = L.G, words = vkmr_sort::hist_words(G);
    const uint32_t tile = vkmr_sort::tile_keys();

    for (uint32_t p = 0; p < passes; ++p) {
        const uint32_t in = vkmr_sort::pass_input(p), out = in ^ 1u;
        CHECK(in <= 1 && (p == 0 ? in == 0 : in != vkmr_sort::pass_input(p - 1)), "pass %u reads buffer %u", p, in);
        // histogram: tile g counts its digits into word (bin, g)
        std::vector<uint32_t> hist(words, 0u);
        std::vector<uint8_t> written(words, 0);
        for (uint64_t g = 0; g < G; ++g)
            for (uint32_t b = 0; b < VKMR_SORT_BINS; ++b) {
                const uint64_t w = vkmr_sort::hist_word(b, g, G);
                CHECK(w < words && L.hist + 4 * (w + 1) <= L.totals, "word (%u, %" PRIu64 ") = %" PRIu64 " outside the histogram", b, g, w);
                CHECK(!written[w], "word %" PRIu64 " belongs to two (bin, group) pairs", w);
                written[w] = 1;
            }
        for (uint64_t i = 0; i < k; ++i) {
            const uint64_t g = vkmr_sort::tile_of(i);
            CHECK(g < G && g * tile <= i && i < (g + 1) * tile, "key %" PRIu64 " in tile %" PRIu64, i, g);
            ++hist[vkmr_sort::hist_word(vkmr_sort::digit(key[in][i], p), g, G)];
        }
        // scan: one bin per workgroup, its G words in trips of the span, in place; the bin's sum in totals
        std::vector<uint32_t> totals(VKMR_SORT_BINS);
        for (uint32_t b = 0; b < VKMR_SORT_BINS; ++b) {
            uint32_t carry = 0;
            const uint64_t trips = vkmr_sort::scan_trips(G);
            CHECK(trips * VKMR_SORT_SCAN_SPAN >= G && (trips - 1) * VKMR_SORT_SCAN_SPAN < G, "G %" PRIu64 " trips %" PRIu64, G, trips);
            for (uint64_t t = 0; t < trips; ++t)
                for (uint64_t lane = 0; lane < VKMR_SORT_SCAN_SPAN; ++lane) {
                    const uint64_t g = t * VKMR_SORT_SCAN_SPAN + lane;
                    if (g >= G) continue;
                    uint32_t& w = hist[vkmr_sort::hist_word(b, g, G)];
                    const uint32_t v = w;
                    w = carry;
                    carry += v;
                }
            totals[b] = carry;
        }
        // the exclusive prefix in word order is the prefix over the bins' sums plus the word inside its bin
        std::vector<uint32_t> prefix(VKMR_SORT_BINS);
        uint32_t sum = 0;
        for (uint32_t b = 0; b < VKMR_SORT_BINS; ++b) {
            prefix[b] = sum;
            sum += totals[b];
        }
        CHECK(sum == k, "pass %u counts %u keys of %u", p, sum, k);
        // scatter: destination = base + rank in the tile
        std::vector<uint8_t> hit(k, 0);
        std::vector<uint32_t> rank(VKMR_SORT_BINS);
        for (uint64_t g = 0; g < G; ++g) {
            std::fill(rank.begin(), rank.end(), 0u);
            for (uint64_t i = g * tile; i < std::min<uint64_t>(k, (g + 1) * tile); ++i) {
                const uint32_t d = vkmr_sort::digit(key[in][i], p);
                const uint64_t at = (uint64_t)prefix[d] + hist[vkmr_sort::hist_word(d, g, G)] + rank[d]++;
                CHECK(at < k, "pass %u key %" PRIu64 " goes to %" PRIu64 " of %u", p, i, at, k);
                CHECK(!hit[at], "pass %u destination %" PRIu64 " hit twice", p, at);
                hit[at] = 1;
                key[out][at] = key[in][i];
                val[out][at] = val[in][i];
            }
        }
        // a stable permutation: the digits rise, and inside a digit the keys keep the order they had
        std::vector<uint32_t> where(k);   // payload q -> its place before the pass
        for (uint32_t i = 0; i < k; ++i) where[val[in][i]] = i;
        for (uint32_t j = 0; j < k; ++j) {
            CHECK(hit[j], "pass %u destination %u never hit", p, j);
            CHECK(key[out][j] == input[val[out][j]], "pass %u: key and payload parted at %u", p, j);
            if (j == 0) continue;
            const uint32_t d0 = vkmr_sort::digit(key[out][j - 1], p), d1 = vkmr_sort::digit(key[out][j], p);
            CHECK(d0 <= d1, "pass %u digits fall at %u", p, j);
            CHECK(d0 < d1 || where[val[out][j - 1]] < where[val[out][j]], "pass %u not stable at %u", p, j);
        }
    }
    const uint32_t at = vkmr_sort::result_buffer(total);
    CHECK(at == (passes & 1u), "result buffer %u after %u passes", at, passes);
    for (uint32_t j = 1; j < k; ++j) {
        CHECK(key[at][j - 1] <= key[at][j], "keys fall at %u", j);
        CHECK(key[at][j - 1] < key[at][j] || val[at][j - 1] < val[at][j], "equal keys out of call order at %u", j);
    }
    return true;
}

}  // namespace

int main(int argc, char** argv)
{
    size_t from_tables = 0;
    if (argc > 1) {
        std::ifstream f(argv[1]);
        std::string line;
        while (std::getline(f, line)) {
            if (line.empty()) continue;
            std::istringstream in(line);
            uint64_t total = 0, k = 0;
            in >> total >> k;
            std::vector<uint64_t> keys(k);
            for (uint64_t& x : keys) in >> x;
            if (!in) {
                std::printf("FAIL: case %zu cannot be read\n", from_tables);
                return 1;
            }
            if (!replay(total, keys)) std::printf("FAIL: case %zu of the tables (total %" PRIu64 ", k %" PRIu64 ")\n", from_tables, total, k);
            ++from_tables;
        }
    }
    std::mt19937_64 rng(20240611);
    size_t random = 0;
    const uint32_t tile = vkmr_sort::tile_keys();
    const uint64_t totals[] = {0, 1, 2, 255, 256, 257, 65535, 65536, 1ull << 24, (1ull << 32) - 1, 1ull << 32, (1ull << 40) + 12345, 1ull << 56, 1ull << 58};
    const uint32_t ks[] = {1, 2, 63, 65, 255, 257, tile - 1, tile, tile + 1, 3 * tile + 17};
    for (uint64_t total : totals)
        for (uint32_t k : ks)
            for (int narrow = 0; narrow < 2; ++narrow) {
                std::vector<uint64_t> keys(k);
                // all of [0, total], or a few distinct keys (long runs of equal keys across tiles), the sentinel among them
                const uint64_t span = narrow ? std::min<uint64_t>(total, 5) : total;
                for (uint64_t& x : keys) x = (rng() % 8 == 0) ? total : (span == ~0ull ? rng() : total - rng() % (span + 1));
                if (!replay(total, keys)) std::printf("FAIL: random case total %" PRIu64 " k %u narrow %d\n", total, k, narrow);
                ++random;
            }
    for (uint32_t k : {0u, 1u, 1000u, 1u << 20, 0xFFFFFFFFu})   // the layout alone, up to the largest batch
        if (k && !check_layout(k, 1ull << 58)) std::printf("FAIL: layout of k %u\n", k);
    if (vkmr_sort::scratch_bytes(100, 0) != 0) {
        std::printf("FAIL: scratch for no entry\n");
        ++g_fail;
    }
    if (g_fail) {
        std::printf("FAIL: %d checks\n", g_fail);
        return 1;
    }
    std::printf("ok: %zu cases from the tables, %zu random\n", from_tables, random);
    return 0;
}
