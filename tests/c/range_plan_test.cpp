// range_plan_test.cpp -- csrc/range_plan.hpp replayed on the CPU, a program of its own (tests/test_range_abi.py builds it with
// AddressSanitizer and UBSan): the steps of the check's kernels with (level, node) identities in place of hashes, in arrays of exactly
// the sizes the plan bounds.
//   1. every run 0 <= a <= b < c of every c <= 40: the fold arrives at (H, 0) and reads exactly the row cells the rule names
//   2. random batches, Q up to 300 and runs of 0 to 300 leaves: the searches name the right query, no two queries share a cell of a
//      level's buffer, every node of every level is written once
//   3. the prefix over m as the three gather kernels form it, in 64 bits: 4 097 runs of 2^20 leaves carry 2^32 + 2^20
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <vector>

#include "range_plan.hpp"

static int failures = 0;
#define CHECK(cond, ...)                 \
    do {                                 \
        if (!(cond)) {                   \
            printf("FAIL: " __VA_ARGS__); \
            printf("\n");                \
            if (++failures > 20) exit(1); \
        }                                \
    } while (0)

struct Id {
    int level = -1;          // -1: never written
    uint64_t node = 0;
    uint32_t q = 0;
};

struct Query { uint64_t a, m, c; uint32_t h; };

// The check's level launches over one batch, as vkmr_hip_verify_forest_range_async enqueues them; `reads[q]` collects (row, level).
static void replay(const std::vector<Query>& qs, uint32_t stride, std::vector<std::vector<std::pair<uint32_t, uint32_t>>>* reads)
{
    const uint64_t Q = qs.size();
    std::vector<uint64_t> starts(Q + 1, 0);
    for (uint64_t q = 0; q < Q; ++q) starts[q + 1] = starts[q] + qs[q].m;
    const uint64_t N = starts[Q];
    std::vector<Id> leaves(N);
    for (uint64_t q = 0; q < Q; ++q)
        for (uint64_t j = 0; j < qs[q].m; ++j) leaves[starts[q] + j] = Id{0, qs[q].a + j, (uint32_t)q};
    for (uint64_t j = 0; j < N; ++j) {            // the leaves kernels' search
        const uint64_t q = vkmr_range::query_of_leaf(j, Q, [&](uint64_t i) { return starts[i]; });
        CHECK(starts[q] <= j && j < starts[q + 1], "leaf %llu is given to query %llu", (unsigned long long)j, (unsigned long long)q);
    }
    std::vector<Id> odd(vkmr_range::level_cells(N, Q, 1)), even(vkmr_range::level_cells(N, Q, 2)), tops(Q);
    const vkmr_range::Layout L = vkmr_range::layout(N, Q);
    CHECK(L.even - L.odd == 32 * odd.size() && L.bytes - L.even == 32 * even.size() && L.odd - L.tops == 32 * Q && L.tops - L.ok >= 4 * Q &&
              L.ok - L.sums >= 8 * L.groups && L.groups * VKMR_RANGE_THREADS >= Q + 1,
          "the scratch layout");
    for (uint32_t l = 0; l < stride; ++l) {
        const std::vector<Id>& in = (l & 1u) ? odd : even;
        std::vector<Id>& out = (l & 1u) ? even : odd;
        const uint64_t cells = vkmr_range::level_cells(N, Q, l + 1);
        CHECK(cells <= out.size(), "level %u has more cells than its buffer", l + 1);
        for (auto& id : out) id.level = -1;       // what an earlier level left there is dead
        uint64_t written = 0, want = 0;
        for (uint64_t q = 0; q < Q; ++q)
            if (qs[q].m && l + 1 < qs[q].h) want += vkmr_range::nodes(qs[q].a, qs[q].m, l + 1);
        for (uint64_t i = 0; i < cells; ++i) {
            const uint64_t q = vkmr_range::query_of_cell(i, l + 1, N, Q, [&](uint64_t k) { return starts[k]; });
            CHECK(q < Q, "cell %llu of level %u: query %llu", (unsigned long long)i, l + 1, (unsigned long long)q);
            // the search is right: no later query starts at or before i, and q does
            if (q + 1 < Q) CHECK(vkmr_range::level_cell(starts[q + 1], q + 1, l + 1, 0) > i, "cell %llu of level %u belongs behind query %llu", (unsigned long long)i, l + 1, (unsigned long long)q);
            const Query& z = qs[q];
            if (z.m == 0 || l >= z.h) continue;
            const uint64_t base = vkmr_range::level_cell(starts[q], q, l + 1, 0);
            const uint64_t j = i - base;
            if (i < base || j >= vkmr_range::nodes(z.a, z.m, l + 1)) continue;
            const vkmr_range::Step s = vkmr_range::step(z.a, z.m, z.c, l, j);
            CHECK(s.active, "an idle parent inside nodes()");
            const uint64_t al = z.a >> l, bl = (z.a + z.m - 1) >> l, p = (al >> 1) + j, n = vkmr_range::level_count(z.c, l);
            auto child = [&](uint32_t src, uint64_t k) {
                if (src == vkmr_range::FROM_LEFT) {
                    CHECK(vkmr_range::left_cell(z.a, l, z.h), "the left row is read at level %u where the rule names no cell", l);
                    if (reads) (*reads)[q].push_back({1u, l});
                    return Id{(int)l, al - 1, (uint32_t)q};
                }
                if (src == vkmr_range::FROM_RIGHT) {
                    CHECK(vkmr_range::right_cell(z.a + z.m - 1, z.c, l, z.h), "the right row is read at level %u where the rule names no cell", l);
                    if (reads) (*reads)[q].push_back({2u, l});
                    return Id{(int)l, bl + 1, (uint32_t)q};
                }
                CHECK(k < vkmr_range::nodes(z.a, z.m, l), "child %llu is outside the run's level %u", (unsigned long long)k, l);
                return l == 0 ? leaves.at(starts[q] + k) : in.at(vkmr_range::level_cell(starts[q], q, l, k));
            };
            const Id x = child(s.lsrc, s.lk), y = child(s.rsrc, s.rk);
            CHECK(x.level == (int)l && x.q == q && x.node == 2 * p, "parent %llu of level %u: left child (%d, %llu) of query %u", (unsigned long long)p, l + 1,
                  x.level, (unsigned long long)x.node, x.q);
            const uint64_t right = 2 * p + 1 < n ? 2 * p + 1 : 2 * p;
            CHECK(y.level == (int)l && y.q == q && y.node == right, "parent %llu of level %u: right child (%d, %llu)", (unsigned long long)p, l + 1, y.level,
                  (unsigned long long)y.node);
            Id& dst = l + 1 == z.h ? tops.at(q) : out.at(i);
            CHECK(dst.level == -1, "cell %llu of level %u is written twice", (unsigned long long)i, l + 1);
            dst = Id{(int)l + 1, p, (uint32_t)q};
            if (l + 1 < z.h) ++written;
        }
        CHECK(written == want, "level %u: %llu nodes written, %llu wanted", l + 1, (unsigned long long)written, (unsigned long long)want);
    }
    for (uint64_t q = 0; q < Q; ++q)
        if (qs[q].m) CHECK(tops[q].level == (int)qs[q].h && tops[q].node == 0 && tops[q].q == q, "query %llu arrives at (%d, %llu)", (unsigned long long)q, tops[q].level, (unsigned long long)tops[q].node);
}

// The three kernels of the prefix over m: per-workgroup sums, one workgroup's exclusive prefix over them, the places.
static uint64_t prefix(std::vector<uint64_t>& v)        // v[0 .. Q] holds m (v[Q] = 0) and becomes leaf_starts
{
    const uint64_t n = v.size(), groups = (n + VKMR_RANGE_THREADS - 1) / VKMR_RANGE_THREADS;
    std::vector<uint64_t> sums(groups, 0);
    for (uint64_t i = 0; i < n; ++i) sums[i / VKMR_RANGE_THREADS] += v[i];
    uint64_t carry = 0;
    for (uint64_t g = 0; g < groups; ++g) {
        const uint64_t s = sums[g];
        sums[g] = carry;
        carry += s;
    }
    for (uint64_t g = 0; g < groups; ++g) {
        uint64_t before = sums[g];
        for (uint64_t i = g * VKMR_RANGE_THREADS; i < n && i < (g + 1) * VKMR_RANGE_THREADS; ++i) {
            const uint64_t m = v[i];
            v[i] = before;
            before += m;
        }
    }
    return carry;
}

int main()
{
    // 1. every run of every small tree, alone in its batch, and all of one tree's runs in one batch
    uint64_t runs = 0;
    for (uint64_t c = 1; c <= 40; ++c) {
        const uint32_t h = vkmr_absence::height(c);
        std::vector<Query> all;
        for (uint64_t a = 0; a < c; ++a)
            for (uint64_t b = a; b < c; ++b) {
                all.push_back(Query{a, b - a + 1, c, h});
                ++runs;
            }
        std::vector<std::vector<std::pair<uint32_t, uint32_t>>> reads(all.size());
        replay(all, h + (uint32_t)(c % 3), &reads);
        for (size_t q = 0; q < all.size(); ++q) {
            const uint64_t a = all[q].a, b = a + all[q].m - 1;
            size_t want = 0;
            for (uint32_t l = 0; l < h; ++l) want += (vkmr_range::left_cell(a, l, h) ? 1 : 0) + (vkmr_range::right_cell(b, c, l, h) ? 1 : 0);
            CHECK(reads[q].size() == want, "c %llu run [%llu, %llu]: %zu row cells read, the rule names %zu", (unsigned long long)c, (unsigned long long)a,
                  (unsigned long long)b, reads[q].size(), want);
            for (uint32_t l = h; l < 64; ++l) CHECK(!vkmr_range::left_cell(a, l, h) && !vkmr_range::right_cell(b, c, l, h), "a cell at or above H");
        }
        std::vector<Query> one(1);
        for (const Query& z : all) {
            one[0] = z;
            replay(one, h, nullptr);
        }
    }
    printf("ok: %llu runs\n", (unsigned long long)runs);

    // 2. random batches
    std::mt19937_64 rng(7021);
    for (int round = 0; round < 60; ++round) {
        const uint64_t Q = 1 + rng() % 300;
        std::vector<Query> qs;
        uint32_t stride = 1;
        for (uint64_t q = 0; q < Q; ++q) {
            const uint64_t kind = rng() % 8;
            const uint64_t c = kind == 0 ? 0 : kind == 1 ? 1 + rng() % 4 : 1 + rng() % (round % 2 ? 5000 : 400);
            uint64_t m = c == 0 || kind == 2 ? 0 : 1 + rng() % 300;
            if (m > c) m = c;
            const uint64_t a = m ? rng() % (c - m + 1) : 0;
            const uint32_t h = vkmr_absence::height(c);
            if (h > stride) stride = h;
            qs.push_back(Query{a, m, c, h});
        }
        replay(qs, stride, nullptr);
    }
    printf("ok: 60 batches\n");

    // 3. the prefix in 64 bits
    std::vector<uint64_t> m(4097 + 1, 1ull << 20);
    m[4097] = 0;
    const uint64_t total = prefix(m);
    CHECK(total == (1ull << 32) + (1ull << 20) && m[4097] == total && m[0] == 0 && m[4096] == (1ull << 32) && m[257] == 257ull << 20, "the prefix: total %llu",
          (unsigned long long)total);
    CHECK(vkmr_range::layout(0, 4097).groups == 17, "groups");
    if (!failures) printf("ok: prefix %llu + %llu\n", (unsigned long long)(1ull << 32), (unsigned long long)(total - (1ull << 32)));

    // the refusals and the fences, on words
    const uint32_t z[8] = {0}, o[8] = {~0u, ~0u, ~0u, ~0u, ~0u, ~0u, ~0u, ~0u}, five[8] = {5}, six[8] = {6}, seven[8] = {7};
    CHECK(!vkmr_range::refused(0, 1, 3, 3, 5, 1, 3, z, o) && vkmr_range::refused(1, 1, 3, 3, 5, 1, 3, z, o) && vkmr_range::refused(0, 1, 2, 3, 5, 1, 3, z, o) &&
              vkmr_range::refused(0, 1, 3, 2, 5, 1, 3, z, o) && vkmr_range::refused(0, 1, 3, 3, 5, 3, 3, z, o) && vkmr_range::refused(0, 1, 3, 3, 5, 1, 3, o, z) &&
              vkmr_range::refused(0, 1, 3, 3, 5, 1, 0, z, o) && !vkmr_range::refused(0, 1, 0, 3, 0, 0, 0, z, o) &&
              vkmr_range::refused(0, 1, 3, 3, 5, vkmr_range::NONE, 0, z, o) && vkmr_range::refused(0, 1, 59, 63, (1ull << 58) + 1, 0, 1, z, o),
          "refused()");
    vkmr_range::Fences f = vkmr_range::fences(1, 3, 9, six, six, five, six, six, seven);        // leaves 5 | 6 | 7 for [6, 6]
    CHECK(f.ok && f.below && f.above, "fences: both");
    f = vkmr_range::fences(1, 2, 9, six, six, five, six, five, six);                            // 5 | 6 with no leaf behind, mid-tree
    CHECK(!f.ok, "fences: the right one is missing");
    f = vkmr_range::fences(7, 2, 9, six, six, five, six, five, six);                            // the same at the tree's end
    CHECK(f.ok && f.below && !f.above, "fences: the tree's end");
    f = vkmr_range::fences(1, 3, 9, seven, seven, five, six, six, seven);                       // two leaves below lo
    CHECK(!f.ok, "fences: the canonical shape");
    if (failures) return 1;
    printf("ok\n");
    return 0;
}
