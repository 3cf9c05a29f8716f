// forest_append_plan_test.cpp -- CPU replay of the level launches of vkmr_hip_forest_append_async with the range rule the ABI and
// the kernel share (csrc/forest_plan.hpp: append_first_cell, append_end_cell).  A forest is given by its tree sizes and a split
// point s: trees 0 .. s - 1 are resident, trees s .. ntrees - 1 are appended in one call.  For every launch l = 1 .. H the replay
// walks the wavefronts from the range's first cell as forest_append_level_kernel does -- the tree of a cell is the last of
// trees 0 .. s + m - 1 that begins at or before it, then forest_level's own tests -- and checks
//   - that the range stays inside the level's buffer (level_cells) and holds no cell of a node of a resident tree,
//   - that the cells and roots written over all launches are exactly the nodes of the new trees, found here by brute force from
//     the counts alone (halving loops), each written once; a new tree without a leaf gets its root once, at level 1,
//   - that every cell read is one of the tree's own cells of level l - 1,
//   - that no lane in front of the first new tree or behind the last one writes.
// Built and run by tests/test_forest_append_abi.py (no GPU).
//
//   forest_append_plan_test FILE   one case per line: `first_offset slack max_count split c_0 c_1 ..` (max_count 0: the largest
//                                  c_t, at least 1; total = first_offset + sum c_t + slack; split < ntrees).  Prints, per line,
//                                  `H level_cells_written roots_written lanes_launched`
#include <algorithm>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "forest_plan.hpp"

using namespace vkmr_forest;

static void die(const char* what, uint32_t l, uint32_t t, uint64_t p)
{
    printf("FAIL: %s at level %u, tree %u, cell %llu\n", what, l, t, (unsigned long long)p);
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

typedef std::pair<uint32_t, uint64_t> Cell;   // (level, cell of that level's buffer), or (0, tree) for a root

static void replay(uint64_t first, uint64_t slack, uint64_t max_count, uint32_t split, const std::vector<uint64_t>& c)
{
    const uint32_t ntrees = (uint32_t)c.size();
    if (split >= ntrees) die("no tree to append in the test's own input", 0, split, 0);
    std::vector<uint64_t> off(ntrees + 1);
    off[0] = first;
    uint64_t largest = 0;
    for (uint32_t t = 0; t < ntrees; ++t) {
        off[t + 1] = off[t] + c[t];
        largest = std::max(largest, c[t]);
    }
    const uint64_t total = off[ntrees] + slack, used = off[split], n_leaves = off[ntrees] - used;
    const uint32_t end_tree = ntrees;              // first_tree + m
    if (max_count == 0) max_count = largest ? largest : 1;
    if (largest > max_count) die("a tree above max_count in the test's own input", 0, 0, 0);
    const uint32_t H = launches(total, max_count);

    std::vector<std::vector<uint64_t>> levels_of(ntrees);
    for (uint32_t t = 0; t < ntrees; ++t)
        if (c[t]) levels_of[t] = halvings(c[t]);

    // what must be written: every node above the leaves of every new tree, by brute force
    std::vector<Cell> want;
    for (uint32_t t = split; t < ntrees; ++t) {
        want.push_back(Cell(0, t));
        if (!c[t]) continue;
        const std::vector<uint64_t>& n = levels_of[t];
        const uint32_t h = (uint32_t)n.size() - 1;
        if (h > H) die("a tree does not finish within the levels", h, t, 0);
        for (uint32_t l = 1; l < h; ++l)
            for (uint64_t j = 0; j < n[l]; ++j) want.push_back(Cell(l, (off[t] >> l) + t + j));
    }
    std::sort(want.begin(), want.end());

    std::vector<Cell> got;
    uint64_t lanes = 0;
    for (uint32_t l = 1; l <= H; ++l) {
        const uint64_t base = append_first_cell(used, split, l), end = append_end_cell(used + n_leaves, end_tree, l);
        if (base != (used >> l) + split || end != ((used + n_leaves) >> l) + end_tree) die("the range is not pos_l of its two ends", l, split, base);
        if (end <= base) die("an empty range", l, split, base);
        if (end > level_cells(total, ntrees, l)) die("the range passes the level's cells", l, split, end);
        for (uint32_t t = 0; t < split; ++t) {     // the resident trees end in front of the range
            const uint64_t n = c[t] ? levels_of[t].size() > l ? levels_of[t][l] : 1 : 1;
            if ((off[t] >> l) + t + n > base) die("the range holds a cell of a resident tree", l, t, base);
        }
        for (uint64_t p0 = base; p0 < end; p0 += 64) {   // the wavefronts of the launch: p0 >= end returns
            for (uint32_t lane = 0; lane < 64; ++lane, ++lanes) {
                const uint64_t p = p0 + lane;
                uint32_t t = 0, top = end_tree - 1;   // forest_find_tree over trees 0 .. end_tree - 1: the last that begins at or before p
                while (t < top) {
                    const uint32_t mid = t + (top - t + 1) / 2;
                    if (pos(off[mid], mid, l) <= p) t = mid;
                    else top = mid - 1;
                }
                const uint64_t o = off[t], ct = off[t + 1] - o, at = pos(o, t, l);
                if (p < at) continue;
                if (t < split) die("a lane of the range holds a resident tree", l, t, p);
                const uint64_t j = p - at;
                if (ct == 0) {
                    if (l == 1 && j == 0) got.push_back(Cell(0, t));
                    continue;
                }
                const uint64_t n_in = level_count(ct, l - 1), n_out = level_count(ct, l);
                if ((l > 1 && n_in == 1) || j >= n_out) continue;
                if (p >= end) die("a lane behind the range holds a node", l, t, p);
                const std::vector<uint64_t>& n = levels_of[t];
                if (l >= n.size() || n_in != n[l - 1] || n_out != n[l]) die("level_count is not the level's node count", l, t, p);
                const uint64_t own_first = pos(o, t, l - 1), a = own_first + 2 * j, b = own_first + vkmr_math::right_child(j, n_in);
                if (a >= own_first + n_in || b < own_first || b >= own_first + n_in) die("a read outside the tree's own cells", l, t, p);
                if (l == 1 ? b >= used + n_leaves || a < used : b >= level_cells(total, ntrees, l - 1)) die("a read outside the level below", l, t, p);
                got.push_back(n_out == 1 ? Cell(0, t) : Cell(l, p));
            }
        }
    }
    std::sort(got.begin(), got.end());
    if (std::adjacent_find(got.begin(), got.end()) != got.end()) die("a cell or a root is written twice", 0, 0, 0);
    if (got != want) die("the cells written are not the nodes of the new trees", 0, 0, 0);
    uint64_t roots = 0;
    for (const Cell& x : got) roots += x.first == 0;
    printf("%u %llu %llu %llu\n", H, (unsigned long long)(got.size() - roots), (unsigned long long)roots, (unsigned long long)lanes);
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
        if (v.size() < 5) { printf("FAIL: malformed line %d\n", lines + 1); exit(1); }
        replay(v[0], v[1], v[2], (uint32_t)v[3], std::vector<uint64_t>(v.begin() + 4, v.end()));
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
