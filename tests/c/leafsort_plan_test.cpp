// leafsort_plan_test.cpp -- csrc/leafsort_plan.hpp replayed on the CPU.  A stand-alone program (tests/test_leafsort_abi.py
// compiles it with -fsanitize=address,undefined):
//   1. the key: over ntrees in {1, 2, 255, 256, 257, 2^32 - 1} and max_count in {1, 2, 2 048, 2^26, 2^31}, for crafted and random
//      (tree, digest) pairs, key(a) < key(b) implies (tree, digest) a < b; bits_T + P <= 64; the pass count
//   2. the passes: small forests laid at an offset with slack behind (the sentinel case among them: the last tree of two, a
//      prefix of all ones, keys equal to the sentinel) sorted by the radix passes with values through sort_plan.hpp's functions,
//      the ties placed by the plan's rule, against std::stable_sort under absence_plan.hpp's less
//   3. the scratch layout: the parts in order, aligned, none overlapping
// Prints "FAIL ..." and returns 1 otherwise.
#include <algorithm>
#include <array>
#include <cinttypes>
#include <cstdio>
#include <random>
#include <vector>

#include "absence_plan.hpp"
#include "leafsort_plan.hpp"

namespace {

int g_fail = 0;

#define CHECK(cond, ...)                         \
    do {                                         \
        if (!(cond)) {                           \
            if (g_fail++ < 20) {                 \
                std::printf("FAIL %s: ", #cond); \
                std::printf(__VA_ARGS__);        \
                std::printf("\n");               \
            }                                    \
            return false;                        \
        }                                        \
    } while (0)

typedef std::array<uint32_t, 8> Digest;

struct Leaf {
    uint32_t tree;
    Digest d;
};

bool leaf_less(const Leaf& a, const Leaf& b) { return a.tree != b.tree ? a.tree < b.tree : vkmr_absence::less(a.d.data(), b.d.data()); }

// ---- 1. the key ----------------------------------------------------------------------------------------------------------------

bool check_shape(uint32_t ntrees, uint64_t max_count, std::mt19937_64& rng, size_t* pairs)
{
    const vkmr_leafsort::Shape s = vkmr_leafsort::shape(ntrees, max_count);
    const uint32_t passes = vkmr_leafsort::passes(s);
    CHECK(s.bits_T == vkmr_sort::bit_length((uint64_t)ntrees - 1u) && s.bits_T <= 32u, "ntrees %u bits_T %u", ntrees, s.bits_T);
    CHECK(s.P >= 8u && s.bits_T + s.P <= 64u, "ntrees %u max_count %" PRIu64 " P %u", ntrees, max_count, s.P);
    CHECK(s.P == std::min<uint32_t>(64u - s.bits_T, 2u * vkmr_sort::bit_length(max_count) + 8u), "ntrees %u max_count %" PRIu64 " P %u", ntrees, max_count, s.P);
    CHECK(passes >= 1u && passes <= 8u && 8u * passes >= s.bits_T + s.P && 8u * (passes - 1u) < s.bits_T + s.P, "passes %u for %u bits", passes, s.bits_T + s.P);
    CHECK(vkmr_leafsort::result_buffer(s) == (passes & 1u), "result buffer after %u passes", passes);
    // the leaves: the corners of every word, neighbours across every bit of the prefix, and random ones, in the corner trees
    std::vector<uint32_t> trees = {0u, ntrees - 1u, ntrees / 2u, (uint32_t)(rng() % ntrees), (uint32_t)(rng() % ntrees)};
    std::vector<Digest> digests;
    for (uint32_t w0 : {0u, 1u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu})
        for (uint32_t w1 : {0u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu})
            for (uint32_t w7 : {0u, 0xFFFFFFFFu}) digests.push_back(Digest{w0, w1, w7, 5u, 5u, 5u, 5u, w7});
    for (int j = 0; j < 24; ++j) {
        Digest d;
        for (uint32_t& w : d) w = (uint32_t)rng();
        digests.push_back(d);
        Digest e = d;                      // the same but for one bit of the first 64, and the same but for word 2
        if (j < 16) e[j & 1] ^= 1u << (rng() % 32);
        else e[2] ^= 1u;
        digests.push_back(e);
    }
    std::vector<Leaf> leaves;
    for (uint32_t t : trees)
        for (const Digest& d : digests) leaves.push_back(Leaf{t, d});
    for (const Leaf& a : leaves) {
        const uint64_t ka = vkmr_leafsort::key(a.tree, a.d[0], a.d[1], s.P);
        CHECK(s.bits_T + s.P == 64u || (ka >> (s.bits_T + s.P)) == 0ull, "a key of %u bits has more", s.bits_T + s.P);
        CHECK(s.P == 64u || (ka >> s.P) == a.tree, "the tree %u is not on top of the key", a.tree);
        for (const Leaf& b : leaves) {
            const uint64_t kb = vkmr_leafsort::key(b.tree, b.d[0], b.d[1], s.P);
            CHECK(!(ka < kb) || leaf_less(a, b), "ntrees %u max_count %" PRIu64 ": the keys rise where the leaves do not", ntrees, max_count);
            CHECK(a.tree == b.tree || ka != kb, "leaves of trees %u and %u share a key", a.tree, b.tree);
            ++*pairs;
        }
    }
    return true;
}

// ---- 2. the passes ------------------------------------------------------------------------------------------------------------

// The radix passes over (key, element) pairs with values, through sort_plan.hpp's functions as the kernels use them.
bool radix(std::vector<uint64_t>& keys, std::vector<uint32_t>& vals, uint32_t passes)
{
    const uint32_t k = (uint32_t)keys.size();
    const uint64_t G = vkmr_sort::groups(k);
    const uint32_t tile = vkmr_sort::tile_keys();
    for (uint32_t p = 0; p < passes; ++p) {
        std::vector<uint32_t> hist(vkmr_sort::hist_words(G), 0u), totals(VKMR_SORT_BINS), prefix(VKMR_SORT_BINS), rank(VKMR_SORT_BINS);
        for (uint64_t i = 0; i < k; ++i) ++hist[vkmr_sort::hist_word(vkmr_sort::digit(keys[i], p), vkmr_sort::tile_of(i), G)];
        for (uint32_t b = 0; b < VKMR_SORT_BINS; ++b) {
            uint32_t carry = 0;
            for (uint64_t g = 0; g < G; ++g) {
                uint32_t& w = hist[vkmr_sort::hist_word(b, g, G)];
                const uint32_t v = w;
                w = carry;
                carry += v;
            }
            totals[b] = carry;
        }
        uint32_t sum = 0;
        for (uint32_t b = 0; b < VKMR_SORT_BINS; ++b) {
            prefix[b] = sum;
            sum += totals[b];
        }
        CHECK(sum == k, "pass %u counts %u keys of %u", p, sum, k);
        std::vector<uint64_t> keys_out(k);
        std::vector<uint32_t> vals_out(k);
        for (uint64_t g = 0; g < G; ++g) {
            std::fill(rank.begin(), rank.end(), 0u);
            for (uint64_t i = g * tile; i < std::min<uint64_t>(k, (g + 1) * tile); ++i) {
                const uint32_t d = vkmr_sort::digit(keys[i], p);
                const uint64_t at = (uint64_t)prefix[d] + hist[vkmr_sort::hist_word(d, g, G)] + rank[d]++;
                CHECK(at < k, "pass %u key %" PRIu64 " goes to %" PRIu64 " of %u", p, i, at, k);
                keys_out[at] = keys[i];
                vals_out[at] = vals[i];
            }
        }
        keys.swap(keys_out);
        vals.swap(vals_out);
    }
    return true;
}

// One forest: `counts` trees laid at cell `first` of `total` = first + n + slack cells, sorted by the plan's steps.
bool replay(const char* what, const std::vector<std::vector<Digest>>& trees, uint64_t first, uint64_t slack, uint64_t max_count, uint64_t want_sentinel_keys)
{
    const uint32_t ntrees = (uint32_t)trees.size();
    std::vector<uint64_t> offsets(ntrees + 1u, first);
    for (uint32_t t = 0; t < ntrees; ++t) offsets[t + 1u] = offsets[t] + trees[t].size();
    const uint64_t n = offsets[ntrees] - first, total = first + n + slack;
    std::vector<Digest> in(total, Digest{0xDEADBEEFu, 1u, 2u, 3u, 4u, 5u, 6u, 7u});
    for (uint32_t t = 0; t < ntrees; ++t) std::copy(trees[t].begin(), trees[t].end(), in.begin() + (ptrdiff_t)offsets[t]);
    const vkmr_leafsort::Shape s = vkmr_leafsort::shape(ntrees, max_count);
    // the elements: i < n is cell offsets[0] + i, the sentinel behind
    std::vector<uint64_t> keys(total, vkmr_leafsort::SENTINEL);
    std::vector<uint32_t> vals(total);
    uint64_t sentinel_keys = 0;
    for (uint64_t i = 0; i < total; ++i) {
        vals[i] = (uint32_t)i;
        if (i >= n) continue;
        const uint64_t cell = first + i;
        uint32_t t = 0;
        while (offsets[t + 1u] <= cell) ++t;
        keys[i] = vkmr_leafsort::key(t, in[cell][0], in[cell][1], s.P);
        sentinel_keys += keys[i] == vkmr_leafsort::SENTINEL;
    }
    CHECK(sentinel_keys == want_sentinel_keys, "%s: %" PRIu64 " leaves carry the sentinel's key", what, sentinel_keys);
    if (!radix(keys, vals, vkmr_leafsort::passes(s))) return false;
    for (uint64_t j = 0; j < total; ++j) CHECK((vals[j] < n) == (j < n), "%s: position %" PRIu64 " holds element %u of %" PRIu64 " leaves", what, j, vals[j], n);
    for (uint64_t j = 1; j < n; ++j) CHECK(keys[j - 1] < keys[j] || (keys[j - 1] == keys[j] && vals[j - 1] < vals[j]), "%s: not a stable sort at %" PRIu64, what, j);
    // the ties and the place
    std::vector<uint32_t> dest(n);
    uint64_t m = 0, repeats = 0, compares = 0;
    for (uint64_t j = 0; j < n; ++j) {
        const bool tied = (j > 0 && keys[j - 1] == keys[j]) || (j + 1 < n && keys[j + 1] == keys[j]);
        m += tied;
        uint32_t d = (uint32_t)j;
        bool repeat = false;
        const Digest& me = in[first + vals[j]];
        for (uint64_t r = j; tied && r > 0 && keys[r - 1] == keys[j]; --r, ++compares) {
            const Digest& other = in[first + vals[r - 1]];
            if (vkmr_absence::less(me.data(), other.data())) --d;
            else if (vkmr_absence::equal(me.data(), other.data())) repeat = true;
        }
        for (uint64_t r = j + 1; tied && r < n && keys[r] == keys[j]; ++r, ++compares)
            if (vkmr_absence::less(in[first + vals[r]].data(), me.data())) ++d;
        dest[j] = d;
        repeats += repeat;
    }
    CHECK(compares <= m * m, "%s: %" PRIu64 " compares for %" PRIu64 " ties", what, compares, m);
    // the emit, against std::stable_sort per tree
    std::vector<Digest> out(total, Digest{0xA5A5A5A5u, 0u, 0u, 0u, 0u, 0u, 0u, 0u});
    std::vector<uint32_t> order(total, 0xA5A5A5A5u);
    std::vector<uint8_t> hit(total, 0);
    for (uint64_t j = 0; j < n; ++j) {
        const uint64_t to = first + dest[j];
        CHECK(dest[j] < n && !hit[to], "%s: destination %u of position %" PRIu64, what, dest[j], j);
        hit[to] = 1;
        out[to] = in[first + vals[j]];
        order[to] = (uint32_t)(first + vals[j]);
    }
    uint64_t want_repeats = 0;
    for (uint32_t t = 0; t < ntrees; ++t) {
        std::vector<uint32_t> want(trees[t].size());
        for (size_t i = 0; i < want.size(); ++i) want[i] = (uint32_t)(offsets[t] + i);
        std::stable_sort(want.begin(), want.end(), [&](uint32_t x, uint32_t y) { return vkmr_absence::less(in[x].data(), in[y].data()); });
        for (size_t i = 0; i < want.size(); ++i) {
            CHECK(order[offsets[t] + i] == want[i] && out[offsets[t] + i] == in[want[i]], "%s: tree %u leaf %zu", what, t, i);
            want_repeats += i > 0 && in[want[i]] == in[want[i - 1]];
        }
    }
    CHECK(repeats == want_repeats, "%s: %" PRIu64 " repeats counted, %" PRIu64 " there", what, repeats, want_repeats);
    for (uint64_t c = 0; c < total; ++c) CHECK(hit[c] == (c >= first && c < first + n), "%s: cell %" PRIu64, what, c);
    return true;
}

std::vector<Digest> random_tree(std::mt19937_64& rng, size_t c, int narrow)
{
    std::vector<Digest> tree(c);
    for (Digest& d : tree) {
        for (uint32_t& w : d) w = (uint32_t)rng();
        if (narrow >= 1) d[0] = 0x80000000u - (uint32_t)(rng() % 2), d[1] = 0xFFFFFFFFu + (uint32_t)(rng() % 2);   // four prefixes, across the sign bit
        if (narrow >= 2) d[2] = d[3] = d[4] = d[5] = d[6] = 9u, d[7] = (uint32_t)(rng() % 4);                             // and equal digests
    }
    return tree;
}

// ---- 3. the layout ------------------------------------------------------------------------------------------------------------

bool check_layout(uint64_t total)
{
    const vkmr_leafsort::Layout L = vkmr_leafsort::layout(total);
    const vkmr_sort::Layout S = vkmr_sort::layout((uint32_t)total);
    CHECK(vkmr_leafsort::scratch_bytes(total) == L.bytes && L.bytes % 16 == 0, "total %" PRIu64, total);
    CHECK(L.sort.bytes == S.bytes && L.sort.key[1] == S.key[1] && L.sort.hist == S.hist && L.sort.G == S.G, "total %" PRIu64 ": not sort_plan's layout", total);
    const size_t at[] = {L.sort.key[0], L.sort.key[1], L.sort.val[0], L.sort.val[1], L.sort.hist, L.sort.totals, L.sort.mask, L.sort.word_start, L.sort.block,
                         L.sort.hdr, L.dest, L.hdr, L.bytes};
    const size_t bytes[] = {(size_t)total * 8, (size_t)total * 8, (size_t)total * 4, (size_t)total * 4, (size_t)vkmr_sort::hist_words(S.G) * 4,
                            (size_t)VKMR_SORT_BINS * 4, (size_t)S.words * 8, (size_t)S.words * 8, (size_t)S.blocks * 8, 32, (size_t)total * 4,
                            (size_t)VKMR_LEAFSORT_HEADER_WORDS * 8};
    for (size_t a = 0; a + 1 < sizeof at / sizeof at[0]; ++a)
        CHECK(at[a] % 16 == 0 && at[a] + bytes[a] <= at[a + 1], "total %" PRIu64 ": part %zu at %zu of %zu bytes, the next at %zu", total, a, at[a], bytes[a], at[a + 1]);
    return true;
}

}  // namespace

int main()
{
    std::mt19937_64 rng(20261021);
    size_t pairs = 0, forests = 0;
    for (uint32_t ntrees : {1u, 2u, 255u, 256u, 257u, 0xFFFFFFFFu})
        for (uint64_t max_count : {1ull, 2ull, 2048ull, 1ull << 26, 1ull << 31})
            if (!check_shape(ntrees, max_count, rng, &pairs)) std::printf("FAIL: ntrees %u max_count %" PRIu64 "\n", ntrees, max_count);
    {   // the figures of the header's text
        const vkmr_leafsort::Shape s = vkmr_leafsort::shape(1u << 15, 2048);
        if (s.bits_T != 15u || s.P != 32u || vkmr_leafsort::passes(s) != 6u || vkmr_leafsort::passes(vkmr_leafsort::shape(1u, 1ull << 26)) != 8u ||
            vkmr_leafsort::shape(1u, 1ull << 26).P != 62u || vkmr_leafsort::shape(1u, 1ull << 28).P != 64u) {
            std::printf("FAIL: 2^15 trees of 2 048 leaves do not sort in 6 passes of 32 + 15 bits\n");
            ++g_fail;
        }
        if (vkmr_leafsort::key(0u, 0x12345678u, 0x9ABCDEF0u, 64u) != 0x123456789ABCDEF0ull || vkmr_leafsort::key(3u, 0xFFFFFFFFu, 0u, 8u) != 0x3FFull) {
            std::printf("FAIL: the key at P == 64 or P == 8\n");
            ++g_fail;
        }
    }
    const size_t counts[] = {1, 2, 3, 0, 4, 5, 7, 8, 9, 0, 63, 64, 65, 130, 1023, 1024, 1025, 2500};
    for (int narrow = 0; narrow < 3; ++narrow)
        for (uint64_t first : {0ull, 37ull}) {
            std::vector<std::vector<Digest>> trees;
            for (size_t c : counts) trees.push_back(random_tree(rng, narrow == 2 ? std::min<size_t>(c, 130) : c, narrow));
            for (uint64_t max_count : {2500ull, 2500000ull})
                forests += replay("the small forest", trees, first, first ? 100 : 0, max_count, 0);
        }
    {   // the sentinel case: the last tree of two, max_count so large that P = 63, a prefix of all ones
        std::vector<std::vector<Digest>> trees = {random_tree(rng, 5, 0), random_tree(rng, 6, 0)};
        trees[1][1] = trees[1][4] = Digest{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
        trees[1][2] = Digest{0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u, 0u, 0u, 0u, 0u};
        trees[1][3] = Digest{0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
        forests += replay("the sentinel case", trees, 3, 50, 1ull << 40, 3);
        forests += replay("the sentinel case, more than a tile of slack", trees, 0, 1500, 1ull << 40, 3);
        std::vector<std::vector<Digest>> one = {trees[1]};
        forests += replay("the sentinel case of one tree", one, 2, 9, 1ull << 28, 3);
    }
    for (uint64_t total : {1ull, 2ull, 1000ull, 1024ull, 1025ull, 1ull << 20, (1ull << 26) + 3, (1ull << 32) - 1})
        if (!check_layout(total)) std::printf("FAIL: layout of total %" PRIu64 "\n", total);
    if (vkmr_leafsort::scratch_bytes(0) != 0 || vkmr_leafsort::scratch_bytes(1ull << 32) != 0) {
        std::printf("FAIL: scratch for no cell, or for more than positions can name\n");
        ++g_fail;
    }
    if (g_fail) {
        std::printf("FAIL: %d checks\n", g_fail);
        return 1;
    }
    std::printf("ok: %zu pairs of leaves, %zu forests\n", pairs, forests);
    return 0;
}
