// forest_store_plan_test.cpp -- CPU-side sweep over the layout of a STORED forest (csrc/forest_plan.hpp: stored_level_base,
// stored_cells): for a forest given by its tree sizes, walks every level vkmr_hip_reduce_forest_tree_async keeps and checks
// that the cells level l of tree t occupies lie inside level l's buffer, that no two trees' cells overlap, that no two
// levels' buffers overlap, and that the last cell used is below stored_cells.  The buffer sizes are summed here on their own,
// not through the header.  Built and run by tests/test_forest_proofs_abi.py (no GPU).
//
//   forest_store_plan_test FILE          one forest per line: `first_offset slack max_count c_0 c_1 ...` (max_count 0: the
//                                        largest c_t, at least 1; total = first_offset + sum c_t + slack).  Prints, per line,
//                                        `levels cells_summed_here highest_cell_used_plus_one`
//   forest_store_plan_test --random N    N random forests (nonzero first offsets, slack, empty trees, loose max_count)
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "forest_plan.hpp"

using namespace vkmr_forest;

static void die(const char* what, uint32_t l, uint32_t t)
{
    printf("FAIL: %s at level %u, tree %u\n", what, l, t);
    exit(1);
}

// Returns the highest cell of the stored forest that holds a node, plus one; *levels and *summed: the levels kept and the
// cells of their buffers, added up here.
static uint64_t replay(uint64_t first, uint64_t slack, uint64_t max_count, const std::vector<uint64_t>& c, uint32_t* levels, uint64_t* summed)
{
    const uint32_t ntrees = (uint32_t)c.size();
    std::vector<uint64_t> off(ntrees + 1);
    off[0] = first;
    uint64_t largest = 0;
    for (uint32_t t = 0; t < ntrees; ++t) {
        off[t + 1] = off[t] + c[t];
        if (c[t] > largest) largest = c[t];
    }
    const uint64_t total = off[ntrees] + slack;
    if (max_count == 0) max_count = largest ? largest : 1;
    if (largest > max_count) die("a tree above max_count in the test's own input", 0, 0);
    const uint32_t L = launches(total, max_count);
    uint64_t base = 0, high = 0;                       // base: where level l's buffer starts, by this test's own sum
    for (uint32_t l = 1; l <= L; ++l) {
        const uint64_t cells = (total >> l) + ntrees;  // the header states this expression; level_cells is not called here
        if (stored_level_base(total, ntrees, l) != base) die("stored_level_base is not the sum of the levels below", l, 0);
        uint64_t prev_end = 0;
        for (uint32_t t = 0; t < ntrees; ++t) {
            if (c[t] != 0 && height(c[t]) > L) die("a tree does not finish within the levels", l, t);
            const uint64_t p = pos(off[t], t, l);
            // every tree owns at least its first cell at every level, as in the roots-only plan
            const uint64_t n = level_count(c[t], l) ? level_count(c[t], l) : 1;
            if (t > 0 && p < prev_end) die("two trees overlap", l, t);
            if (p + n > cells) die("a tree passes its level's buffer", l, t);
            prev_end = p + n;
            if (c[t] != 0 && l < height(c[t])) {       // kept in the forest: a tree's last level goes to the roots
                const uint64_t end = base + p + level_count(c[t], l);
                if (end > high) high = end;
            }
        }
        base += cells;                                 // the next level starts behind this one: the buffers do not overlap
    }
    if (stored_cells(total, ntrees, L) != base) die("stored_cells is not the sum of the levels", L, 0);
    if (high > base) die("a node lies behind stored_cells", L, 0);
    *levels = L;
    *summed = base;
    return high;
}

int main(int argc, char** argv)
{
    if (argc == 3 && strcmp(argv[1], "--random") == 0) {
        uint64_t x = 2685821657736338717ull;
        auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
        const int n = atoi(argv[2]);
        unsigned long long trees = 0;
        for (int i = 0; i < n; ++i) {
            const uint32_t ntrees = 1 + (uint32_t)(rnd() % 300);
            const uint64_t span = 1ull << (rnd() % 15);          // sizes up to 2^14 - 1: levels 0..14
            std::vector<uint64_t> c(ntrees);
            uint64_t largest = 1;
            for (auto& v : c) {
                v = (rnd() % 5 == 0) ? 0 : rnd() % span;
                if (rnd() % 7 == 0) v = 1ull << (rnd() % 15);    // exact powers of two, and 1
                if (v > largest) largest = v;
            }
            const uint64_t first = (rnd() % 2 == 0) ? 1 + rnd() % 1000 : 0, slack = (rnd() % 2 == 0) ? 1 + rnd() % 1000 : 0;
            const uint64_t max_count = (i % 3 == 0) ? 0 : (i % 3 == 1) ? largest + rnd() % 5000 : ~0ull;
            uint32_t L;
            uint64_t summed;
            replay(first, slack, max_count, c, &L, &summed);
            trees += ntrees;
        }
        printf("ok: %d random forests, %llu trees\n", n, trees);
        return 0;
    }
    if (argc != 2) {
        fprintf(stderr, "usage: %s FILE | --random N\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    std::string line;
    int ch, lines = 0;
    auto flush = [&]() {
        if (line.empty()) return;
        std::vector<uint64_t> v;
        char* p = &line[0];
        for (;;) {
            char* e;
            const unsigned long long x = strtoull(p, &e, 10);
            if (e == p) break;
            v.push_back(x);
            p = e;
        }
        if (v.size() < 4) { printf("FAIL: short line\n"); exit(1); }
        std::vector<uint64_t> c(v.begin() + 3, v.end());
        uint32_t L;
        uint64_t summed;
        const uint64_t high = replay(v[0], v[1], v[2], c, &L, &summed);
        printf("%u %llu %llu\n", L, (unsigned long long)summed, (unsigned long long)high);
        line.clear();
        ++lines;
    };
    while ((ch = fgetc(f)) != EOF) {
        if (ch == '\n') flush();
        else line.push_back((char)ch);
    }
    flush();
    fclose(f);
    printf("ok: %d forests\n", lines);
    return 0;
}
