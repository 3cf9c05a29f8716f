// forest_copy_plan_test.cpp -- CPU replay of vkmr_hip_forest_copy_trees_async and vkmr_hip_forest_drop_front_async with the rules
// the ABI and the kernels share (csrc/forest_plan.hpp: copy_step, copy_find_tree, append_first_cell, append_end_cell,
// drop_front_offset).  The replay keeps VALUES: a leaf is a number, a node is mix(left, right), and every buffer starts as a
// guard value, so that a cell nobody may write takes part in the comparison.
//
// copy: a source forest is built by brute force (halving loops; a tree's last level goes to its root alone, as the build
// does).  The destination holds `first_tree` resident trees that end at cell `used`, then room.  The launches l = 0 .. H_d are
// walked wavefront by wavefront from append's range as forest_copy_level_kernel does -- the tree of a cell among trees 0 ..
// first_tree + m - 1 of the NEW destination offsets, then copy_step -- and the replay checks
//   - that every cell read is a cell the source's build stored (or a leaf of the source tree), never a guard,
//   - that no cell, leaf or root is written twice, none outside the level's buffer, none of a resident tree,
//   - that afterwards EVERY cell of the destination -- leaves, level buffers, roots -- equals a brute-force build over the
//     destination offsets into the same guard-filled buffers: what a build writes is there, what it does not write is guard.
// drop: for every k the offsets after drop_front_offset keep pos_l strictly increasing at every level, inside the level's
// cells, and a build over them writes exactly the cells of trees >= k it wrote before (and the zero roots of the dropped trees).
// Built and run by tests/test_forest_repack_abi.py (no GPU).
//
//   forest_copy_plan_test FILE          one case per line: `src_first src_slack src_max first_tree used dst_slack dst_max behind
//                                       nsel sel_0 .. c_0 c_1 ..` (a max of 0: the largest count concerned, at least 1).
//                                       Prints, per line, `H_s H_d leaves_written cells_written roots_written lanes_launched`
//   forest_copy_plan_test --drop FILE   one case per line: `first slack max_count c_0 c_1 ..`; prints `H ntrees` per line
#include <algorithm>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "forest_plan.hpp"

using namespace vkmr_forest;

static const uint64_t GUARD = 0xC3C3C3C3C3C3C3C3ull;

static void die(const char* what, uint32_t l, uint32_t t, uint64_t p)
{
    printf("FAIL: %s at level %u, tree %u, cell %llu\n", what, l, t, (unsigned long long)p);
    exit(1);
}

static uint64_t mix(uint64_t a, uint64_t b)
{
    uint64_t x = a * 0x9E3779B97F4A7C15ull + (b ^ (b >> 29)) * 0xBF58476D1CE4E5B9ull + 0x94D049BB133111EBull;
    x ^= x >> 31;
    x = x * 0xD6E8FEB86659FD93ull + 1;
    return x == GUARD ? 1 : x;
}

// A stored forest as it lies in memory: the leaves, one buffer per level 1 .. H of level_cells cells, the roots.
struct Stored {
    uint64_t total;
    uint32_t ntrees, H;
    std::vector<uint64_t> leaves, roots;
    std::vector<std::vector<uint64_t>> level;   // [0] unused

    Stored(uint64_t total_, uint32_t ntrees_, uint64_t max_count) : total(total_), ntrees(ntrees_), H(launches(total_, max_count))
    {
        leaves.assign(total, GUARD);
        roots.assign(ntrees, GUARD);
        level.resize(H + 1);
        for (uint32_t l = 1; l <= H; ++l) level[l].assign(level_cells(total, ntrees, l), GUARD);
    }
    bool operator==(const Stored& o) const { return leaves == o.leaves && roots == o.roots && level == o.level; }
};

// What a build over trees [lo, hi) of `off` writes into s, tree by tree from the counts alone: levels 1 .. h - 1 to their cells,
// level h to the root, the zero root of an empty tree.  The leaves are s.leaves.
static void build(Stored& s, const std::vector<uint64_t>& off, uint32_t lo, uint32_t hi)
{
    for (uint32_t t = lo; t < hi; ++t) {
        const uint64_t c = off[t + 1] - off[t];
        if (!c) {
            s.roots[t] = 0;
            continue;
        }
        std::vector<uint64_t> cur(s.leaves.begin() + off[t], s.leaves.begin() + off[t + 1]);
        for (uint32_t l = 1;; ++l) {
            std::vector<uint64_t> next;
            for (uint64_t j = 0; 2 * j < cur.size(); ++j) next.push_back(mix(cur[2 * j], cur[std::min<uint64_t>(2 * j + 1, cur.size() - 1)]));
            if (next.size() == 1) {
                s.roots[t] = next[0];
                break;
            }
            if (l > s.H) die("a tree does not finish within the levels", l, t, 0);
            for (uint64_t j = 0; j < next.size(); ++j) {
                const uint64_t p = (off[t] >> l) + t + j;
                if (p >= s.level[l].size()) die("the build itself leaves the level's cells", l, t, p);
                s.level[l][p] = next[j];
            }
            cur.swap(next);
        }
    }
}

static std::vector<uint64_t> offsets_from(uint64_t first, const std::vector<uint64_t>& c)
{
    std::vector<uint64_t> off(c.size() + 1);
    off[0] = first;
    for (size_t t = 0; t < c.size(); ++t) off[t + 1] = off[t] + c[t];
    return off;
}

static void replay_copy(const std::vector<uint64_t>& v)
{
    const uint64_t src_first = v[0], src_slack = v[1], first_tree64 = v[3], used = v[4], dst_slack = v[5], behind = v[7], m64 = v[8];
    uint64_t src_max = v[2], dst_max = v[6];
    if (v.size() < 9 + m64 + 1) die("malformed case", 0, 0, 0);
    const uint32_t first_tree = (uint32_t)first_tree64, m = (uint32_t)m64;
    const std::vector<uint64_t> sel(v.begin() + 9, v.begin() + 9 + m), c(v.begin() + 9 + m, v.end());
    const uint32_t src_ntrees = (uint32_t)c.size();
    uint64_t largest = 1, chosen_largest = 1;
    for (uint64_t x : c) largest = std::max(largest, x);
    for (uint64_t t : sel) {
        if (t >= src_ntrees) die("a selection outside the source in the test's own input", 0, (uint32_t)t, 0);
        chosen_largest = std::max(chosen_largest, c[t]);
    }

    // the source: built by brute force
    const std::vector<uint64_t> src_off = offsets_from(src_first, c);
    if (src_max == 0) src_max = largest;
    Stored src(src_off[src_ntrees] + src_slack, src_ntrees, src_max);
    for (uint64_t i = 0; i < src.total; ++i) src.leaves[i] = mix(i, 7);
    build(src, src_off, 0, src_ntrees);

    // the destination before: first_tree resident trees that end at `used` (tree 0 holds them all; with no resident tree the
    // forest begins at offset `used`), then m + behind empty trees; after: the chosen counts
    std::vector<uint64_t> dst_c;
    for (uint32_t t = 0; t < first_tree; ++t) dst_c.push_back(t == 0 ? used : 0);
    std::vector<uint64_t> before_c = dst_c;
    uint64_t n_leaves = 0;
    for (uint64_t t : sel) dst_c.push_back(c[t]), n_leaves += c[t];
    for (uint64_t i = 0; i < behind; ++i) dst_c.push_back(0);
    before_c.resize(dst_c.size(), 0);
    const uint32_t dst_ntrees = (uint32_t)dst_c.size(), end_tree = first_tree + m;
    const uint64_t dst_first = first_tree ? 0 : used;
    const std::vector<uint64_t> off_before = offsets_from(dst_first, before_c), off = offsets_from(dst_first, dst_c);
    if (dst_max == 0) dst_max = std::max(chosen_largest, used ? used : 1);
    if (chosen_largest > dst_max || (first_tree && used > dst_max)) die("a tree above max_count in the test's own input", 0, 0, 0);
    const uint64_t dst_total = used + n_leaves + dst_slack;
    Stored dst(dst_total, dst_ntrees, dst_max), want(dst_total, dst_ntrees, dst_max), resident(dst_total, dst_ntrees, dst_max);
    if (first_tree)
        for (uint64_t i = 0; i < used; ++i) dst.leaves[i] = want.leaves[i] = resident.leaves[i] = mix(i, 13);
    build(dst, off_before, 0, dst_ntrees);
    build(resident, off_before, 0, first_tree);
    uint64_t at = used;
    for (uint64_t t : sel)
        for (uint64_t i = 0; i < c[t]; ++i) want.leaves[at++] = src.leaves[src_off[t] + i];
    build(want, off, 0, dst_ntrees);
    const uint32_t H = dst.H;

    // the launches
    Stored written(dst_total, dst_ntrees, dst_max);          // GUARD: not written; 1: written
    uint64_t lanes = 0, n_leaf = 0, n_cell = 0, n_root = 0;
    for (uint32_t l = 0; l <= H; ++l) {
        const uint64_t base = append_first_cell(used, first_tree, l), end = append_end_cell(used + n_leaves, end_tree, l);
        if (end < base) die("a range that ends in front of its first cell", l, first_tree, base);
        if (end > (l ? level_cells(dst_total, dst_ntrees, l) : dst_total)) die("the range passes the level's cells", l, first_tree, end);
        for (uint64_t p0 = base; p0 < end; p0 += 64) {
            for (uint32_t lane = 0; lane < 64; ++lane, ++lanes) {
                const uint64_t p = p0 + lane;
                const uint32_t u = copy_find_tree(off.data(), end_tree, l, p);
                const uint64_t o_d = off[u], cnt = off[u + 1] - o_d, first = pos(o_d, u, l);
                if (p < first) continue;
                if (u < first_tree) die("a lane of the range holds a resident tree", l, u, p);
                const uint32_t ts = (uint32_t)sel[u - first_tree];
                const CopyStep s = copy_step(o_d, u, cnt, src_off[ts], ts, l, p - first);
                uint64_t *cell = nullptr, *mark = nullptr, value = 0;
                switch (s.kind) {
                case COPY_NOTHING: continue;
                case COPY_ZERO_ROOT: cell = &dst.roots[u], mark = &written.roots[u], ++n_root; break;
                case COPY_ROOT: cell = &dst.roots[u], mark = &written.roots[u], value = src.roots[ts], ++n_root; break;
                case COPY_LEAF:
                    if (l != 0 || s.src < src_off[ts] || s.src >= src_off[ts + 1]) die("a leaf read outside the source tree", l, ts, s.src);
                    if (s.dst != p || s.dst < used || s.dst >= used + n_leaves) die("a leaf written outside the new leaves", l, u, s.dst);
                    cell = &dst.leaves[s.dst], mark = &written.leaves[s.dst], value = src.leaves[s.src], ++n_leaf;
                    break;
                case COPY_CELL:
                    if (l == 0 || l > src.H || s.src >= src.level[l].size()) die("a cell read outside the source's level", l, ts, s.src);
                    if (s.dst != p || p >= end || s.dst >= dst.level[l].size()) die("a cell written outside the range", l, u, s.dst);
                    cell = &dst.level[l][s.dst], mark = &written.level[l][s.dst], value = src.level[l][s.src], ++n_cell;
                    break;
                }
                if (value == GUARD) die("a read of a cell the source's build never stored", l, ts, s.src);
                if (*mark != GUARD) die("a cell or a root is written twice", l, u, p);
                *mark = 1;
                *cell = value;
            }
        }
    }
    if (!(dst == want)) die("the destination is not what a build over its offsets writes", 0, 0, 0);
    // what was written is exactly what the build writes for the new trees: nothing of a resident tree, no root behind them
    for (uint32_t t = 0; t < dst_ntrees; ++t)
        if ((written.roots[t] != GUARD) != (t >= first_tree && t < end_tree)) die("the roots written are not the new trees'", 0, t, 0);
    for (uint32_t l = 1; l <= H; ++l)
        for (uint64_t p = 0; p < dst.level[l].size(); ++p)
            if ((written.level[l][p] != GUARD) != (want.level[l][p] != GUARD && resident.level[l][p] == GUARD))
                die("the cells written are not the new trees' nodes", l, 0, p);
    if (n_leaf != n_leaves) die("the leaves written are not the new leaves", 0, 0, n_leaf);
    printf("%u %u %llu %llu %llu %llu\n", src.H, H, (unsigned long long)n_leaf, (unsigned long long)n_cell, (unsigned long long)n_root, (unsigned long long)lanes);
}

static void replay_drop(const std::vector<uint64_t>& v)
{
    const uint64_t first = v[0], slack = v[1];
    uint64_t max_count = v[2];
    const std::vector<uint64_t> c(v.begin() + 3, v.end());
    const uint32_t ntrees = (uint32_t)c.size();
    uint64_t largest = 1;
    for (uint64_t x : c) largest = std::max(largest, x);
    if (max_count == 0) max_count = largest;
    const std::vector<uint64_t> off = offsets_from(first, c);
    const uint64_t total = off[ntrees] + slack;
    Stored leaves_only(total, ntrees, max_count);
    for (uint64_t i = 0; i < total; ++i) leaves_only.leaves[i] = mix(i, 7);
    const uint32_t H = leaves_only.H;
    for (uint32_t k = 0; k <= ntrees; ++k) {
        std::vector<uint64_t> now(ntrees + 1);
        for (uint32_t t = 0; t <= ntrees; ++t) now[t] = drop_front_offset(off[t], off[k], t, k);
        for (uint32_t l = 1; l <= H; ++l) {
            for (uint32_t t = 0; t + 1 < ntrees; ++t)
                if (pos(now[t + 1], t + 1, l) <= pos(now[t], t, l)) die("pos_l does not increase after the drop", l, t, k);
            const uint64_t n_last = level_count(now[ntrees] - now[ntrees - 1], l);
            if (pos(now[ntrees - 1], ntrees - 1, l) + (n_last ? n_last : 1) > level_cells(total, ntrees, l)) die("the last tree passes the level's cells", l, ntrees - 1, k);
        }
        for (uint32_t t = k; t <= ntrees; ++t)
            if (now[t] != off[t]) die("a tree that stays has moved", 0, t, k);
        Stored got = leaves_only, want = leaves_only;
        build(got, now, 0, ntrees);                          // a fresh build over the offsets after the drop
        build(want, off, k, ntrees);                         // the cells of trees >= k as the build wrote them before
        for (uint32_t t = 0; t < k; ++t) want.roots[t] = 0;
        if (!(got == want)) die("a build over the offsets after the drop does not write the kept trees' cells alone", 0, k, 0);
    }
    printf("%u %u\n", H, ntrees);
}

int main(int argc, char** argv)
{
    const bool drop = argc == 3 && !strcmp(argv[1], "--drop");
    if (argc != 2 && !drop) {
        fprintf(stderr, "usage: %s [--drop] FILE\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[argc - 1], "r");
    if (!f) { perror(argv[argc - 1]); return 2; }
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
        if (v.size() < (drop ? 4u : 10u)) { printf("FAIL: malformed line %d\n", lines + 1); exit(1); }
        if (drop) replay_drop(v);
        else replay_copy(v);
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
