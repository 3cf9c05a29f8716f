// frontier_plan_test.cpp -- CPU replay of vkmr_hip_frontier_extend_async's launches with the rules the ABI, the kernels and the CPU
// twins share (csrc/frontier_plan.hpp).  A case is a batch of T trees, tree q going from c_q to c_q + n_q leaves.  The replay keeps
// VALUES: a leaf is a number, a node is mix(left, right).  Per tree it builds the old tree and the new tree by brute force (halving
// loops), takes the old frontier from the old tree, then walks the lanes of every launch l = 1 .. launches(stride) as
// frontier_level_kernel does -- the wavefront's search and the lane's search over the offsets, then frontier_plan.hpp's step() --
// and the commit, and checks
//   - that the search finds the last tree whose first cell is at or before the lane's cell,
//   - that every cell is written once, inside the level's cells, and that no two trees' cells overlap,
//   - that every read is a new leaf of the lane's own tree, a cell the launch before wrote for that tree, or the one named old
//     peak: cell l - 1 of the frontier, the left child of the tree's first node, only where bit l - 1 of the old count is set,
//   - that tree q forms at most (n_q >> l) + 2 nodes at level l, and every one of [c >> l, ceil(c2 / 2^l)),
//   - that a launch has at most sum((n_q >> l) + 2) + 63 lanes, one per cell (the cells are sum(n_q >> l) + 2 T and at most
//     T - 1 more, the carries of adding the shifted offsets: T <= 32 here),
//   - that the roots, written once each, and the committed frontiers (zero cells included) are the brute-force tree's, and
//     that the root walk over the new frontier gives the same root,
//   - that no cell past scratch_cells() is touched.
// Built and run by tests/test_frontier_abi.py (no GPU).
//
//   frontier_plan_test FILE   one batch per line: `stride c_0 n_0 c_1 n_1 ..`.  Prints, per line,
//                             `launches cells_touched hashes lanes` (cells_touched: one past the last scratch cell written).
#include <algorithm>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "frontier_plan.hpp"

using namespace vkmr_frontier;

static int batch_no = 0;

static void die(const char* what, uint32_t l, uint32_t q, uint64_t c, uint64_t n, uint64_t p)
{
    printf("FAIL: %s in batch %d at level %u, tree %u (%llu + %llu leaves), cell %llu\n", what, batch_no, l, q, (unsigned long long)c,
           (unsigned long long)n, (unsigned long long)p);
    exit(1);
}

static uint64_t mix(uint64_t a, uint64_t b)
{
    uint64_t x = a * 0x9E3779B97F4A7C15ull + (b ^ (b >> 29)) * 0xBF58476D1CE4E5B9ull + 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x * 0xD6E8FEB86659FD93ull + 1;   // never 0: 0 is the cell of a clear bit and the root of no leaf
}

// Every level of the tree over `leaves` by halving, the last node paired with itself: levels[0] the leaves, the last the root.
static std::vector<std::vector<uint64_t>> brute(const std::vector<uint64_t>& leaves)
{
    std::vector<std::vector<uint64_t>> lv{leaves};
    if (leaves.empty()) return lv;
    do {
        const std::vector<uint64_t>& cur = lv.back();
        std::vector<uint64_t> next;
        for (uint64_t j = 0; 2 * j < cur.size(); ++j) next.push_back(mix(cur[2 * j], cur[std::min<uint64_t>(2 * j + 1, cur.size() - 1)]));
        lv.push_back(next);
    } while (lv.back().size() > 1);
    return lv;
}

// The frontier of a brute-force tree: 64 cells, 0 for a clear bit.
static std::vector<uint64_t> frontier_of(const std::vector<std::vector<uint64_t>>& lv)
{
    std::vector<uint64_t> peaks(64, 0);
    const uint64_t c = lv[0].size();
    for (uint32_t l = 0; l < 64; ++l)
        if (has_peak(c, l)) peaks[l] = lv[l][(c >> l) - 1];
    return peaks;
}

// The root walk of frontier_plan.hpp's head, with mix.
static uint64_t walk(uint64_t c, const std::vector<uint64_t>& peaks)
{
    if (c == 0) return 0;
    bool have = false;
    uint64_t carry = 0;
    const uint32_t H = height(c);
    for (uint32_t l = 0; l < H; ++l) {
        if (has_peak(c, l)) carry = mix(peaks[l], have ? carry : peaks[l]), have = true;
        else if (have) carry = mix(carry, carry);
    }
    return have ? carry : peaks[H];
}

// frontier_find_tree, with the offsets as the kernel reads them.
static uint32_t find_tree(const std::vector<uint64_t>& off, uint32_t T, uint32_t l, uint64_t p0, uint32_t lane)
{
    uint32_t t0 = 0, top = T - 1;
    while (t0 < top) {
        const uint32_t mid = t0 + (top - t0 + 1) / 2;
        if (first_cell(off[mid], mid, l) <= p0) t0 = mid;
        else top = mid - 1;
    }
    uint32_t t = t0;
    if (t0 + 1 < T && first_cell(off[t0 + 1], t0 + 1, l) <= p0 + 63) {
        const uint64_t p = p0 + lane;
        top = (T - 1 - t0 < lane) ? T - 1 : t0 + lane;
        while (t < top) {
            const uint32_t mid = t + (top - t + 1) / 2;
            if (first_cell(off[mid], mid, l) <= p) t = mid;
            else top = mid - 1;
        }
    }
    return t;
}

static void replay(uint32_t stride, const std::vector<uint64_t>& cs, const std::vector<uint64_t>& ns)
{
    const uint32_t T = (uint32_t)cs.size();
    std::vector<uint64_t> off(T + 1, 0);
    uint64_t max_new = 0;
    for (uint32_t q = 0; q < T; ++q) off[q + 1] = off[q] + ns[q], max_new = std::max(max_new, ns[q]);
    const uint64_t total_new = off[T];
    for (uint32_t q = 0; q < T; ++q)
        if (refusal(cs[q], off[q], off[q + 1], q, T, total_new, max_new, stride)) die("the test's own batch is refused", 0, q, cs[q], ns[q], 0);

    // the values: old leaves, new leaves, the old frontier and what the new tree must give
    std::vector<uint64_t> new_leaves(total_new);
    std::vector<std::vector<uint64_t>> old_peaks(T), want_peaks(T);
    std::vector<uint64_t> want_root(T);
    for (uint32_t q = 0; q < T; ++q) {
        std::vector<uint64_t> leaves(cs[q]);
        for (uint64_t i = 0; i < cs[q]; ++i) leaves[i] = mix(((uint64_t)q << 40) + i, 7);
        old_peaks[q] = frontier_of(brute(leaves));
        for (uint64_t i = 0; i < ns[q]; ++i) {
            new_leaves[off[q] + i] = mix(((uint64_t)q << 40) + cs[q] + i, 11);
            leaves.push_back(new_leaves[off[q] + i]);
        }
        const std::vector<std::vector<uint64_t>> lv = brute(leaves);
        want_peaks[q] = frontier_of(lv);
        want_root[q] = leaves.empty() ? 0 : lv.back()[0];
        if (walk(leaves.size(), want_peaks[q]) != want_root[q]) die("the root walk over the new frontier is not the tree's root", 0, q, cs[q], ns[q], 0);
        if (walk(cs[q], old_peaks[q]) != (cs[q] ? brute(std::vector<uint64_t>(leaves.begin(), leaves.begin() + cs[q])).back()[0] : 0))
            die("the root walk over the old frontier is not the old tree's root", 0, q, cs[q], ns[q], 0);
    }

    const uint64_t budget = scratch_cells(total_new, T), stage0 = staging_base(total_new, T);
    std::vector<uint64_t> value(budget, 0);
    std::vector<uint32_t> wrote(budget, 0), owner(budget, 0);      // the launch that wrote the cell (0: nobody), and for which tree
    std::vector<uint64_t> roots(T, 0);
    std::vector<uint32_t> roots_written(T, 0);
    uint64_t touched = 0, hashes = 0, lanes = 0;
    const uint32_t H = launches(stride);
    for (uint32_t l = 1; l <= H; ++l) {
        const uint64_t cells = level_cells(total_new, T, l), in_base = level_base(total_new, T, l - 1), out_base = level_base(total_new, T, l);
        uint64_t need = 0;
        for (uint32_t q = 0; q < T; ++q) need += (ns[q] >> l) + 2;
        if (cells > need + 63) die("more lanes than sum((n >> l) + 2) + 63", l, 0, 0, 0, cells);
        if (cells > need + (T - 1)) die("more cells than the shifted offsets' carries explain", l, 0, 0, 0, cells);
        lanes += cells;
        std::vector<uint64_t> formed(T, 0);
        for (uint64_t p0 = 0; p0 < cells; p0 += 64) {          // a wavefront at or behind `cells` returns
            for (uint32_t lane = 0; lane < 64; ++lane) {
                const uint64_t p = p0 + lane;
                const uint32_t q = find_tree(off, T, l, p0, lane);
                uint32_t brute_q = 0;
                for (uint32_t t = 0; t < T; ++t)
                    if (first_cell(off[t], t, l) <= p) brute_q = t;
                if (q != brute_q) die("the search finds another tree", l, q, cs[q], ns[q], p);
                const uint64_t o = off[q], c = cs[q], n = ns[q], c2 = c + n;
                const uint64_t j = first_node(c, l) + (p - first_cell(o, q, l));
                const Step s = step(o, q, c, c2, l, j);
                if (!s.active) continue;
                if (p >= cells) die("a lane behind the level's cells holds a node", l, q, c, n, p);
                if (q + 1 < T && p >= first_cell(off[q + 1], q + 1, l)) die("a node in the next tree's cells", l, q, c, n, p);
                if (j < (c >> l) || j >= level_count(c2, l) || l > height(c2)) die("a node outside [c >> l, cnt(c2, l))", l, q, c, n, p);
                uint64_t a, b;
                if (s.left_is_peak) {
                    if (!has_peak(c, l - 1) || 2 * j + 1 != (c >> (l - 1)) || j != (c >> l)) die("an old value read that is not the named peak", l, q, c, n, p);
                    if (l - 1 >= stride) die("a peak read past the frontier's cells", l, q, c, n, p);
                    a = old_peaks[q][l - 1];
                } else if (l == 1) {
                    if (s.in_left < o || s.in_left >= o + n) die("a read outside the tree's new leaves", l, q, c, n, s.in_left);
                    a = new_leaves[s.in_left];
                } else {
                    const uint64_t at = in_base + s.in_left;
                    if (s.in_left >= level_cells(total_new, T, l - 1) || wrote[at] != l - 1 || owner[at] != q) die("a read of a cell the launch before did not write for this tree", l, q, c, n, s.in_left);
                    a = value[at];
                }
                if (s.right_is_left) b = a;
                else if (l == 1) {
                    if (s.in_right < o || s.in_right >= o + n) die("a read outside the tree's new leaves", l, q, c, n, s.in_right);
                    b = new_leaves[s.in_right];
                } else {
                    const uint64_t at = in_base + s.in_right;
                    if (s.in_right >= level_cells(total_new, T, l - 1) || wrote[at] != l - 1 || owner[at] != q) die("a read of a cell the launch before did not write for this tree", l, q, c, n, s.in_right);
                    b = value[at];
                }
                const uint64_t x = mix(a, b);
                ++hashes, ++formed[q];
                if (s.root != (l == height(c2))) die("the root is not node 0 of level H(c2)", l, q, c, n, p);
                if (s.root) {
                    if (roots_written[q]++) die("a root written twice", l, q, c, n, p);
                    roots[q] = x;
                } else {
                    const uint64_t at = out_base + p;
                    if (at >= stage0) die("a write past the level buffer", l, q, c, n, p);
                    if (wrote[at] == l) die("a cell written twice in one launch", l, q, c, n, p);
                    value[at] = x, wrote[at] = l, owner[at] = q;
                    touched = std::max(touched, at + 1);
                }
                if (s.peak) {
                    const uint64_t at = stage0 + (uint64_t)q * VKMR_FRONTIER_MAX_STRIDE + l;
                    if (at >= budget || wrote[at]) die("a staged peak written twice or past the scratch", l, q, c, n, at);
                    value[at] = x, wrote[at] = l;
                    touched = std::max(touched, at + 1);
                }
            }
        }
        for (uint32_t q = 0; q < T; ++q) {
            const uint64_t c2 = cs[q] + ns[q], want = l <= height(c2) && c2 ? level_count(c2, l) - (cs[q] >> l) : 0;
            if (formed[q] != want) die("the nodes formed are not all of [c >> l, cnt(c2, l))", l, q, cs[q], ns[q], formed[q]);
            if (formed[q] > (ns[q] >> l) + 2) die("more nodes than (n >> l) + 2", l, q, cs[q], ns[q], formed[q]);
        }
    }
    // the commit
    for (uint32_t q = 0; q < T; ++q) {
        const uint64_t c = cs[q], c2 = c + ns[q];
        for (uint32_t l = 0; l < stride; ++l) {
            uint64_t x = 0;
            if (has_peak(c2, l)) {
                const PeakSource from = peak_source(c, c2, l);
                if (from == PEAK_OLD) {
                    if (!has_peak(c, l)) die("the cell of a clear bit read as an old peak", l, q, c, ns[q], 0);
                    x = old_peaks[q][l];
                } else if (from == PEAK_LAST_LEAF) {
                    if (ns[q] == 0) die("the last new leaf of a tree that took none", l, q, c, ns[q], 0);
                    x = new_leaves[off[q + 1] - 1];
                } else {
                    const uint64_t at = stage0 + (uint64_t)q * VKMR_FRONTIER_MAX_STRIDE + l;
                    if (!wrote[at]) die("a staged peak nobody wrote", l, q, c, ns[q], at);
                    x = value[at];
                }
            }
            if (x != want_peaks[q][l]) die("a committed peak is not the tree's", l, q, c, ns[q], 0);
        }
        for (uint32_t l = stride; l < 64; ++l)
            if (want_peaks[q][l]) die("a peak past the frontier's cells", l, q, c, ns[q], 0);
        uint64_t root;
        if (c2 == 0 || root_is_old_peak(c, c2)) {
            if (roots_written[q]) die("a root formed that the commit writes", 0, q, c, ns[q], 0);
            root = c2 == 0 ? 0 : old_peaks[q][height(c)];
        } else {
            if (roots_written[q] != 1) die("a root no launch formed", 0, q, c, ns[q], 0);
            root = roots[q];
        }
        if (root != want_root[q]) die("a root is not the tree's", 0, q, c, ns[q], 0);
    }
    if (touched > budget) die("a cell past the scratch", 0, 0, 0, 0, touched);
    printf("%u %llu %llu %llu\n", H, (unsigned long long)touched, (unsigned long long)hashes, (unsigned long long)lanes);
}

int main(int argc, char** argv)
{
    if (argc != 2) {
        fprintf(stderr, "usage: frontier_plan_test FILE\n");
        return 2;
    }
    FILE* f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    std::string line;
    int ch;
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
        if (v.size() < 3 || v.size() % 2 == 0) { printf("FAIL: malformed line %d\n", batch_no + 1); exit(1); }
        std::vector<uint64_t> cs, ns;
        for (size_t i = 1; i + 1 < v.size(); i += 2) cs.push_back(v[i]), ns.push_back(v[i + 1]);
        replay((uint32_t)v[0], cs, ns);
        line.clear();
        ++batch_no;
    };
    while ((ch = fgetc(f)) != EOF) {
        if (ch == '\n') flush();
        else line.push_back((char)ch);
    }
    flush();
    fclose(f);
    printf("ok: %d batches\n", batch_no);
    return 0;
}
