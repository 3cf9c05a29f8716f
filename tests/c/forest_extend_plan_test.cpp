// forest_extend_plan_test.cpp -- CPU replay of the level launches of vkmr_hip_forest_extend_async and vkmr_hip_forest_shrink_async
// with the range rule the ABI and the kernel share (csrc/forest_plan.hpp: extend_first_cell, extend_end_cell).  A case is a forest
// of small trees in front, the open tree t going from c to c2 leaves at offset o, and empty trees behind.  The replay keeps VALUES:
// a leaf is a number, a node is mix(left, right), a cell that nobody has stored is absent.  It builds the old forest by brute force
// (halving loops; a tree's last level goes to its root alone, as the build does), gives the new leaves new values, then walks the
// wavefronts of every launch l = 1 .. H from the range's first cell as forest_extend_level_kernel does -- the search among trees
// 0 .. t over the NEW offsets, then forest_level's own tests -- and checks
//   - that the nodes written at level l are exactly [first_l, cnt(c2, l)) of tree t, first_l restated here from the counts alone,
//     and the root; each once; a tree shrunk to no leaf gets its zero root once, at level 1,
//   - that no cell of another tree, no reserved cell and no root of another tree is written,
//   - that every cell read is a leaf in use, a cell a lower launch of this call wrote, or a cell the build had stored,
//   - that afterwards every cell and root a fresh build over the new counts writes holds the fresh build's value,
//   - that level l launches at most (|c2 - c| >> l) + 2 + 63 lanes.
// Built and run by tests/test_forest_extend_abi.py (no GPU).
//
//   forest_extend_plan_test [--plain] FILE   one case per line: `first_offset slack max_count behind c c2 front_0 front_1 ..`
//                                  (max_count 0: the largest count, at least 1; t = the number of front counts; total =
//                                  first_offset + sum front + max(c, c2) + slack).  Prints, per line, `H cells_written
//                                  roots_written lanes_launched`.  --plain replays with first_l = min(c, c2) >> l, the rule
//                                  without the lone-node clause: it must fail.
#include <algorithm>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "forest_plan.hpp"

using namespace vkmr_forest;

static bool plain = false;

static void die(const char* what, uint32_t l, uint64_t c, uint64_t c2, uint64_t p)
{
    printf("FAIL: %s at level %u, %llu -> %llu leaves, cell %llu\n", what, l, (unsigned long long)c, (unsigned long long)c2, (unsigned long long)p);
    exit(1);
}

static uint64_t mix(uint64_t a, uint64_t b)
{
    uint64_t x = a * 0x9E3779B97F4A7C15ull + (b ^ (b >> 29)) * 0xBF58476D1CE4E5B9ull + 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x * 0xD6E8FEB86659FD93ull + 1;
}

typedef std::pair<uint32_t, uint64_t> Cell;   // (level >= 1, cell of that level's buffer), or (0, tree) for a root
typedef std::map<Cell, uint64_t> Store;

// Nodes per level of a tree of c >= 1 leaves, by halving: n[0] = c, ..., n[h] = 1, h >= 1.
static std::vector<uint64_t> halvings(uint64_t c)
{
    std::vector<uint64_t> n{c};
    do n.push_back((n.back() + 1) / 2);
    while (n.back() > 1);
    return n;
}

// What a build over `counts` writes, tree by tree from the counts alone: levels 1 .. h - 1 to their cells, level h to the root,
// the zero root of an empty tree.
static Store fresh(const std::vector<uint64_t>& off, const std::vector<uint64_t>& leaves)
{
    Store s;
    for (uint32_t t = 0; t + 1 < off.size(); ++t) {
        const uint64_t c = off[t + 1] - off[t];
        if (!c) {
            s[Cell(0, t)] = 0;
            continue;
        }
        std::vector<uint64_t> cur(leaves.begin() + off[t], leaves.begin() + off[t + 1]);
        for (uint32_t l = 1;; ++l) {
            std::vector<uint64_t> next;
            for (uint64_t j = 0; 2 * j < cur.size(); ++j) next.push_back(mix(cur[2 * j], cur[std::min<uint64_t>(2 * j + 1, cur.size() - 1)]));
            if (next.size() == 1) {
                s[Cell(0, t)] = next[0];
                break;
            }
            for (uint64_t j = 0; j < next.size(); ++j) s[Cell(l, (off[t] >> l) + t + j)] = next[j];
            cur.swap(next);
        }
    }
    return s;
}

static void replay(uint64_t first, uint64_t slack, uint64_t max_count, uint32_t behind, uint64_t c, uint64_t c2, const std::vector<uint64_t>& front)
{
    const uint32_t t = (uint32_t)front.size(), ntrees = t + 1 + behind;
    std::vector<uint64_t> off(ntrees + 1), off2(ntrees + 1);
    off[0] = off2[0] = first;
    uint64_t largest = std::max(c, c2);
    for (uint32_t i = 0; i < t; ++i) {
        off[i + 1] = off2[i + 1] = off[i] + front[i];
        largest = std::max(largest, front[i]);
    }
    const uint64_t o = off[t];
    for (uint32_t i = t + 1; i <= ntrees; ++i) off[i] = o + c, off2[i] = o + c2;
    const uint64_t total = o + std::max(c, c2) + slack;
    if (max_count == 0) max_count = largest ? largest : 1;
    if (largest > max_count) die("a tree above max_count in the test's own input", 0, c, c2, 0);
    const uint32_t H = launches(total, max_count);

    std::vector<uint64_t> leaves(total);
    for (uint64_t i = 0; i < total; ++i) leaves[i] = mix(i, 7);
    Store store = fresh(off, leaves);                        // the forest as the build left it
    for (uint64_t i = o + c; i < o + c2; ++i) leaves[i] = mix(i, 11);   // the new leaves (none when shrinking)
    const Store want = fresh(off2, leaves);

    const std::vector<uint64_t> n_old = c ? halvings(c) : std::vector<uint64_t>(), n_new = c2 ? halvings(c2) : std::vector<uint64_t>();
    // nodes of level l by halving; above a tree's root, and for no leaf, the rule's cnt(): 1, or 0 for an empty tree
    auto cnt = [](const std::vector<uint64_t>& n, uint32_t l) -> uint64_t { return n.empty() ? 0 : l < n.size() ? n[l] : 1; };
    if (n_new.size() > H + 1) die("the tree does not finish within the levels", H, c, c2, 0);

    uint64_t lanes = 0, cells_written = 0, roots_written = 0;
    for (uint32_t l = 1; l <= H; ++l) {
        // the rule, restated from the halvings: which nodes the launch must write
        uint64_t want_first = 0, want_end = 0;
        bool want_root = false;
        if (c2 == 0) want_root = l == 1;
        else if (l == 1 || cnt(n_new, l - 1) > 1) {
            want_end = cnt(n_new, l);
            want_first = (cnt(n_old, l) <= 1 || want_end <= 1) ? 0 : (std::min(c, c2) >> l);
            want_root = want_end == 1;
        }
        uint64_t base = extend_first_cell(o, t, c, c2, l);
        const uint64_t end = extend_end_cell(o, t, c2, l), at = pos(o, t, l);
        if (plain) base = std::min(at + (std::min(c, c2) >> l), end);
        if (end < base || base < at) die("the range is not one of the open tree's", l, c, c2, base);
        if (end > level_cells(total, ntrees, l)) die("the range passes the level's cells", l, c, c2, end);
        const uint64_t change = c2 > c ? c2 - c : c - c2;
        std::vector<uint64_t> got;
        bool got_root = false;
        uint64_t level_lanes = 0;
        for (uint64_t p0 = base; p0 < end; p0 += 64) {       // the wavefronts of the launch: p0 >= end returns
            for (uint32_t lane = 0; lane < 64; ++lane, ++level_lanes) {
                const uint64_t p = p0 + lane;
                uint32_t tt = 0, top = t;                    // forest_find_tree over trees 0 .. t: the last that begins at or before p
                while (tt < top) {
                    const uint32_t mid = tt + (top - tt + 1) / 2;
                    if (pos(off2[mid], mid, l) <= p) tt = mid;
                    else top = mid - 1;
                }
                if (tt != t) die("a lane of the range holds an earlier tree", l, c, c2, p);
                const uint64_t ct = off2[tt + 1] - off2[tt], tree_at = pos(off2[tt], tt, l);
                if (p < tree_at) continue;
                const uint64_t j = p - tree_at;
                if (ct == 0) {
                    if (l == 1 && j == 0) {
                        if (got_root) die("the root is written twice", l, c, c2, p);
                        got_root = true;
                        store[Cell(0, t)] = 0;
                    }
                    continue;
                }
                const uint64_t n_in = level_count(ct, l - 1), n_out = level_count(ct, l);
                if ((l > 1 && n_in == 1) || j >= n_out) continue;
                if (p >= end) die("a lane behind the range holds a node", l, c, c2, p);
                const uint64_t in_first = pos(off2[tt], tt, l - 1), a = in_first + 2 * j, b = in_first + vkmr_math::right_child(j, n_in);
                uint64_t va, vb;
                if (l == 1) {
                    if (a < o || b >= o + c2) die("a read outside the tree's leaves", l, c, c2, p);
                    va = leaves[a], vb = leaves[b];
                } else {
                    const Store::const_iterator ia = store.find(Cell(l - 1, a)), ib = store.find(Cell(l - 1, b));
                    if (ia == store.end() || ib == store.end()) die("a read of a cell that nobody has stored", l, c, c2, ia == store.end() ? a : b);
                    va = ia->second, vb = ib->second;
                }
                if (n_out == 1) {
                    if (got_root) die("the root is written twice", l, c, c2, p);
                    got_root = true;
                    store[Cell(0, t)] = mix(va, vb);
                } else {
                    if (p < at || p >= at + n_out) die("a write outside the open tree's cells", l, c, c2, p);
                    got.push_back(j);
                    store[Cell(l, p)] = mix(va, vb);
                }
            }
        }
        std::vector<uint64_t> nodes;
        for (uint64_t j = want_first; j < (want_root ? 0 : want_end); ++j) nodes.push_back(j);
        if (!plain && (got != nodes || got_root != want_root)) die("the nodes written are not [first_l, cnt(c2, l)) and the root", l, c, c2, base);
        if (level_lanes > (change >> l) + 2 + 63) die("more lanes than the edge needs", l, c, c2, level_lanes);
        lanes += level_lanes, cells_written += got.size(), roots_written += got_root;
    }
    for (const Store::value_type& x : want) {                // every cell and root a fresh build writes holds its value
        const Store::const_iterator it = store.find(x.first);
        if (it == store.end() || it->second != x.second) die(x.first.first ? "a cell is not the fresh build's" : "a root is not the fresh build's", x.first.first, c, c2, x.first.second);
    }
    printf("%u %llu %llu %llu\n", H, (unsigned long long)cells_written, (unsigned long long)roots_written, (unsigned long long)lanes);
}

int main(int argc, char** argv)
{
    if (argc == 3 && !strcmp(argv[1], "--plain")) plain = true, ++argv, --argc;
    if (argc != 2) {
        fprintf(stderr, "usage: forest_extend_plan_test [--plain] FILE\n");
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
        if (v.size() < 6) { printf("FAIL: malformed line %d\n", lines + 1); exit(1); }
        replay(v[0], v[1], v[2], (uint32_t)v[3], v[4], v[5], std::vector<uint64_t>(v.begin() + 6, v.end()));
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
