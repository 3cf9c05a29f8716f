// forest_update_plan_test.cpp -- CPU replay of the level loop of vkmr_hip_forest_update_async with the functions the kernel
// itself runs (csrc/forest_plan.hpp: update_step, update_same_node).  For a forest given by its tree sizes and a sorted set of
// (tree, index) entries it walks the launches l = 1 .. H, applies the run-head rule as forest_update_level_kernel does, and checks
//   - that within a launch no two heads write the same cell,
//   - that the cells written over all launches are exactly the ancestors of the updated leaves, found here by brute force from
//     the counts alone (halving loops, no call into the header) and placed with stored_level_base and pos,
//   - that every touched tree's root is written exactly once, at its own level h_t, and no other root is written,
//   - that every cell read is one of the tree's own cells of level l - 1,
//   - that a level buffer is only written below a tree's last level, so level H's buffer gets nothing a build does not write.
// Built and run by tests/test_forest_update_abi.py (no GPU).
//
//   forest_update_plan_test FILE    one case per line: `first_offset slack max_count ntrees c_0 .. k t_0 i_0 t_1 i_1 ..` (max_count 0:
//                                   the largest c_t, at least 1; total = first_offset + sum c_t + slack; the entries strictly
//                                   increasing and in range).  Prints, per line, `H level_cells_written roots_written node_hashes`
#include <algorithm>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "forest_plan.hpp"

using namespace vkmr_forest;

static void die(const char* what, uint32_t l, uint32_t t, uint64_t i)
{
    printf("FAIL: %s at level %u, tree %u, index %llu\n", what, l, t, (unsigned long long)i);
    exit(1);
}

// Nodes per level of a tree of c >= 1 leaves, by halving: n[0] = c, ..., n[h] = 1, h >= 1.
static std::vector<uint64_t> halvings(uint64_t c)
{
    std::vector<uint64_t> n{c};
    do n.push_back((n.back() + 1) / 2);
    while (n.back() > 1);
    return n;
}

typedef std::pair<uint32_t, uint64_t> Cell;   // (level, cell of the stored forest), or (0, tree) for a root

static void replay(uint64_t first, uint64_t slack, uint64_t max_count, const std::vector<uint64_t>& c, const std::vector<uint32_t>& et,
                   const std::vector<uint64_t>& ei)
{
    const uint32_t ntrees = (uint32_t)c.size();
    const size_t k = et.size();
    std::vector<uint64_t> off(ntrees + 1);
    off[0] = first;
    uint64_t largest = 0;
    for (uint32_t t = 0; t < ntrees; ++t) {
        off[t + 1] = off[t] + c[t];
        largest = std::max(largest, c[t]);
    }
    const uint64_t total = off[ntrees] + slack;
    if (max_count == 0) max_count = largest ? largest : 1;
    if (largest > max_count) die("a tree above max_count in the test's own input", 0, 0, 0);
    const uint32_t H = launches(total, max_count);
    std::vector<uint64_t> base(H + 2, 0);              // where level l's buffer starts, summed here
    for (uint32_t l = 1; l <= H; ++l) base[l + 1] = base[l] + (total >> l) + ntrees;

    std::vector<std::vector<uint64_t>> levels_of(ntrees);
    for (uint32_t t = 0; t < ntrees; ++t)
        if (c[t]) levels_of[t] = halvings(c[t]);

    // what must be written: every ancestor of every entry, by brute force
    std::vector<Cell> want;
    for (size_t q = 0; q < k; ++q) {
        const uint32_t t = et[q];
        if (t >= ntrees || ei[q] >= c[t]) die("an entry outside the forest in the test's own input", 0, t, ei[q]);
        if (q > 0 && !(et[q - 1] < t || (et[q - 1] == t && ei[q - 1] < ei[q]))) die("entries not strictly increasing in the test's own input", 0, t, ei[q]);
        const std::vector<uint64_t>& n = levels_of[t];
        const uint32_t h = (uint32_t)n.size() - 1;
        if (h > H) die("a tree does not finish within the levels", h, t, ei[q]);
        for (uint32_t l = 1; l < h; ++l) want.push_back(Cell(l, base[l] + (off[t] >> l) + t + (ei[q] >> l)));
        want.push_back(Cell(0, t));
    }
    std::sort(want.begin(), want.end());
    want.erase(std::unique(want.begin(), want.end()), want.end());

    std::vector<Cell> got;
    uint64_t hashes = 0;
    for (uint32_t l = 1; l <= H; ++l) {
        std::vector<Cell> launch;
        for (size_t q = 0; q < k; ++q) {
            const uint32_t t = et[q];
            const uint64_t i = ei[q];
            if (q > 0 && update_same_node(et[q - 1], ei[q - 1], t, i, l)) continue;   // not the head of its run
            const UpdateStep s = update_step(off[t], c[t], t, i, l);
            if (!s.active) continue;
            const std::vector<uint64_t>& n = levels_of[t];
            const uint32_t h = (uint32_t)n.size() - 1;
            if (l > h) die("a tree takes part above its root", l, t, i);
            // the two cells hash_parent reads: 2p and right_child(p, n_in), inside the tree's own level l - 1
            const uint64_t own_first = (l == 1) ? off[t] : (off[t] >> (l - 1)) + t, own_n = n[l - 1];
            if (s.n_in != own_n) die("n_in is not the level's node count", l, t, i);
            const uint64_t a = s.in_first + 2 * s.p, b = s.in_first + vkmr_math::right_child(s.p, s.n_in);
            if (a < own_first || a >= own_first + own_n || b < own_first || b >= own_first + own_n) die("a read outside the tree's own cells", l, t, i);
            if (l == 1 ? a >= total : a >= (total >> (l - 1)) + ntrees) die("a read outside the level's buffer", l, t, i);
            if (s.root != (l == h)) die("the root is not at the tree's own level", l, t, i);
            if (s.root) {
                launch.push_back(Cell(0, t));
            } else {                                   // l < h: never level H's buffer beyond what a build writes (h <= H)
                if (s.out >= (total >> l) + ntrees) die("a write outside the level's buffer", l, t, i);
                if (s.out != (off[t] >> l) + t + (i >> l) || (i >> l) >= n[l]) die("a write outside the tree's own cells", l, t, i);
                launch.push_back(Cell(l, base[l] + s.out));
            }
            ++hashes;
        }
        std::sort(launch.begin(), launch.end());
        if (std::adjacent_find(launch.begin(), launch.end()) != launch.end()) die("two heads of one launch write the same cell", l, 0, 0);
        got.insert(got.end(), launch.begin(), launch.end());
    }
    std::sort(got.begin(), got.end());
    if (std::adjacent_find(got.begin(), got.end()) != got.end()) die("a cell or a root is written in two launches", 0, 0, 0);
    if (got != want) die("the cells written are not the ancestors of the updated leaves", 0, 0, 0);
    uint64_t roots = 0;
    for (const Cell& x : got) roots += x.first == 0;
    printf("%u %llu %llu %llu\n", H, (unsigned long long)(got.size() - roots), (unsigned long long)roots, (unsigned long long)hashes);
}

int main(int argc, char** argv)
{
    if (argc != 2) {
        fprintf(stderr, "usage: %s FILE\n", argv[0]);
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
        if (v.size() < 5 || v.size() < 4 + v[3] + 1 || v.size() != 4 + v[3] + 1 + 2 * v[4 + v[3]]) { printf("FAIL: malformed line %d\n", lines + 1); exit(1); }
        const size_t ntrees = (size_t)v[3], k = (size_t)v[4 + ntrees];
        std::vector<uint64_t> c(v.begin() + 4, v.begin() + 4 + ntrees), ei(k);
        std::vector<uint32_t> et(k);
        for (size_t q = 0; q < k; ++q) {
            et[q] = (uint32_t)v[5 + ntrees + 2 * q];
            ei[q] = v[6 + ntrees + 2 * q];
        }
        replay(v[0], v[1], v[2], c, et, ei);
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
