// forest_plan_test.cpp -- CPU-side sweep over the forest layout (csrc/forest_plan.hpp): for a forest given by its tree sizes,
// replays every launch vkmr_hip_reduce_forest_async would issue and checks, level by level, that no two trees' cells overlap,
// that no tree passes the level's cell count (the lanes of that launch), that what goes to scratch stays inside
// scratch_cells(total, ntrees), and that the last launch is level max(1, ceil(log2 max_count)).  Built and run by
// tests/test_forest_abi.py (no GPU).
//
//   forest_plan_test FILE          one forest per line: `first_offset slack max_count c_0 c_1 ...` (max_count 0: the largest
//                                  c_t, at least 1; total = first_offset + sum c_t + slack).  Prints, per line,
//                                  `launches scratch_cells_written scratch_cells_budget`
//   forest_plan_test --random N    N random forests (tree sizes 0 .. a few thousand, empty trees included, loose max_count)
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "forest_plan.hpp"

using namespace vkmr_forest;

static uint32_t ceil_log2(uint64_t n)
{
    uint32_t h = 0;
    while (h < 64 && ((n - 1) >> h) != 0) ++h;
    return n <= 1 ? 0 : h;
}

static void die(const char* what, uint32_t l, uint32_t t)
{
    printf("FAIL: %s at level %u, tree %u\n", what, l, t);
    exit(1);
}

// Returns the scratch cells written (the highest cell + 1); *nlaunch: the launches.
static uint64_t replay(uint64_t first, uint64_t slack, uint64_t max_count, const std::vector<uint64_t>& c, uint32_t* nlaunch)
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
    const uint64_t m = max_count < total ? max_count : total;
    if (L != (ceil_log2(m) > 1 ? ceil_log2(m) : 1)) die("the last launch is not level max(1, ceil(log2 max_count))", L, 0);
    const uint64_t budget = scratch_cells(total, ntrees);
    uint64_t high = 0;
    for (uint32_t t = 0; t < ntrees; ++t) {
        if (c[t] == 0) continue;
        const uint32_t h = height(c[t]);
        if (h != (ceil_log2(c[t]) > 1 ? ceil_log2(c[t]) : 1)) die("height", 0, t);
        if (h > L) die("a tree does not finish within the launches", h, t);
        if (level_count(c[t], h) != 1 || (h > 1 && level_count(c[t], h - 1) < 2)) die("level_count does not end in one node at the height", h, t);
    }
    for (uint32_t l = 1; l <= L; ++l) {
        const uint64_t cells = level_cells(total, ntrees, l);
        uint64_t prev_end = 0;
        for (uint32_t t = 0; t < ntrees; ++t) {
            const uint64_t p = pos(off[t], t, l);
            // every tree owns at least its first cell at every level (the empty tree's root is written from it at level 1)
            const uint64_t n = level_count(c[t], l) ? level_count(c[t], l) : 1;
            if (t > 0 && p < prev_end) die("two trees overlap", l, t);
            if (t > 0 && p <= pos(off[t - 1], t - 1, l)) die("pos is not strictly increasing", l, t);
            if (p + n > cells) die("a tree passes the level's cells", l, t);
            prev_end = p + n;
            if (c[t] != 0 && l < height(c[t])) {       // written to scratch: the last level of a tree goes to the roots
                const uint64_t end = level_base(total, ntrees, l) + p + n;
                if (end > budget) die("a scratch write passes the budget", l, t);
                if (end > high) high = end;
            }
        }
        // the two buffers do not overlap: level l is read while level l + 1 is written
        if (l + 1 <= L && (l & 1u) && cells > level_base(total, ntrees, l + 1)) die("buffer A runs into buffer B", l, 0);
        if (l >= 3 && cells > level_cells(total, ntrees, l - 2)) die("a level is larger than the one two below", l, 0);
    }
    *nlaunch = L;
    if (budget < high) die("budget", 0, 0);
    return high;
}

int main(int argc, char** argv)
{
    if (argc == 3 && strcmp(argv[1], "--random") == 0) {
        uint64_t x = 88172645463325252ull;
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
            const uint64_t first = (rnd() % 3 == 0) ? rnd() % 1000 : 0, slack = (rnd() % 3 == 0) ? rnd() % 1000 : 0;
            const uint64_t max_count = (i % 3 == 0) ? 0 : (i % 3 == 1) ? largest + rnd() % 5000 : ~0ull;
            uint32_t L;
            replay(first, slack, max_count, c, &L);
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
        const uint64_t high = replay(v[0], v[1], v[2], c, &L);
        printf("%u %llu %llu\n", L, (unsigned long long)high, (unsigned long long)scratch_cells(v[0] + v[1] + [&] { uint64_t s = 0; for (auto k : c) s += k; return s; }(), (uint32_t)c.size()));
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
