// diff_plan_test.cpp -- CPU replay of vkmr_hip_forest_diff_async and vkmr_hip_tree_diff_async with the functions the kernels
// and the driver themselves run (csrc/diff_plan.hpp: forest_step, tree_step, level_at, the frontier bounds, the grouping of
// step 0, the scratch layout).  For a forest given by its tree sizes and a set of changed leaves it builds both forests' levels
// in the real layout -- a 64-bit mixing function stands in for SHA-256d, and every cell that is no node is poisoned, differently
// on the two sides -- runs the descent, and checks
//   - that the result is the model's: the changed leaves, found here by comparing the two level-0 windows cell by cell,
//   - that the frontier is strictly increasing by (tree, node) after every step and never shrinks,
//   - that no poisoned cell is read (every read goes through a map of the cells the build wrote),
//   - that every scratch part is 16-byte aligned, in bounds and disjoint, and that every index a step uses lies in its part,
//   - that the nodes whose children were compared are exactly the distinct ancestors (t, l, i >> l), 1 <= l <= h_t,
//   - that an overflow is reported at the first step whose frontier exceeds `capacity`, with that frontier's size.
// The same cells as ONE tree (count = the leaves, at its own height and one above) go through the tree's form.
// Built and run by tests/test_diff_abi.py (no GPU), plain and with -fsanitize=address,undefined.
//
//   diff_plan_test FILE   one case per line: `first_offset slack max_count capacity ntrees c_0 .. k t_0 i_0 t_1 i_1 ..` (max_count 0:
//                         the largest c_t, at least 1; total = first_offset + sum c_t + slack; the entries strictly increasing
//                         and in range).  Prints, per line, `status n roots compared H`, then `ok: N forests`.
#include <algorithm>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <utility>
#include <vector>

#include "diff_plan.hpp"

using namespace vkmr_diff;

static void die(const char* what, uint64_t a = 0, uint64_t b = 0, uint64_t c = 0)
{
    printf("FAIL: %s (%llu, %llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b, (unsigned long long)c);
    exit(1);
}

static uint64_t mix(uint64_t a, uint64_t b)
{
    uint64_t x = a * 0x9E3779B97F4A7C15ull ^ (b + 0xD1B54A32D192ED03ull) * 0xBF58476D1CE4E5B9ull;
    x ^= x >> 31;
    x *= 0x94D049BB133111EBull;
    return x ^ (x >> 29);
}

// A buffer of cells of which only the ones the build wrote may be read.
struct Cells {
    std::vector<uint64_t> v;
    std::vector<char> node;
    Cells(uint64_t n, uint64_t poison) : v(n, poison), node(n, 0) {}
    void put(uint64_t at, uint64_t x)
    {
        if (at >= v.size()) die("the test's own build writes outside a buffer", at, v.size());
        v[at] = x;
        node[at] = 1;
    }
    uint64_t get(uint64_t at) const
    {
        if (at >= v.size()) die("a read outside a buffer", at, v.size());
        if (!node[at]) die("a poisoned cell is read", at);
        return v[at];
    }
};

typedef std::pair<uint32_t, uint64_t> Entry;   // (tree, node)

struct Info {
    uint64_t status, n, roots, compared;
};

// The scratch parts a step may index, from the layout: checked once per case, then every index against its part's size.
struct Parts {
    Layout L;
    uint64_t block_words;
    explicit Parts(uint32_t capacity) : L(layout(capacity))
    {
        const size_t at[] = {L.node[0], L.node[1], L.tree[0], L.tree[1], L.mask, L.word_start, L.block, L.hdr, L.bytes};
        const size_t need[] = {8ull * capacity, 8ull * capacity, 4ull * capacity, 4ull * capacity, 8 * (size_t)L.words, 8 * (size_t)L.words,
                               8 * (size_t)std::max<uint64_t>(L.blocks, VKMR_DIFF_ROOT_GROUPS), 8ull * VKMR_DIFF_HEADER_WORDS};
        if (at[0] != 0) die("the scratch does not start at 0");
        for (int i = 0; i < 8; ++i) {
            if (at[i] % 16) die("a scratch part is not 16-byte aligned", i, at[i]);
            if (at[i] + need[i] > at[i + 1]) die("a scratch part overlaps the next or ends past the scratch", i, at[i], at[i + 1]);
        }
        if (L.bytes != scratch_bytes(capacity) || L.bytes % 16) die("scratch_bytes is not the layout's end");
        if (L.words * VKMR_DIFF_WORD_ENTRIES < capacity) die("fewer mask bits than entries");
        block_words = (at[7] - at[6]) / 8;
    }
    void step(uint64_t bound, uint32_t capacity) const
    {
        const uint64_t words = mask_words(bound);
        if (bound == 0 || bound > capacity) die("a step's bound is 0 or above capacity", bound, capacity);
        if (words > L.words || rank_blocks(words) > block_words) die("a step's mask words or blocks leave their part", words, L.words);
        if (words * VKMR_DIFF_WORD_ENTRIES < bound) die("a step's mask words do not cover its lanes", words, bound);
    }
};

static void check_frontier(const std::vector<Entry>& next, size_t before, uint32_t step)
{
    for (size_t j = 1; j < next.size(); ++j)
        if (!(next[j - 1] < next[j])) die("the frontier is not strictly increasing", step, j);
    if (next.size() < before) die("the frontier shrank", step, before, next.size());
}

// The model's frontier sizes from the changed leaves alone: after step s the entries of a tree of height h stand at level_at(h, s + 1).
static Info expect(const std::vector<uint32_t>& heights, uint32_t H, const std::vector<Entry>& changed, uint32_t capacity)
{
    // `changed` is sorted by (tree, index), so equal (tree, index >> shift) keys are neighbours: distinct keys by one pass
    auto distinct = [&](auto shift_of, auto takes_part) {
        uint64_t count = 0;
        bool have = false;
        Entry prev(0, 0);
        for (const Entry& e : changed) {
            if (!takes_part(heights[e.first])) continue;
            const Entry key(e.first, e.second >> shift_of(heights[e.first]));
            if (!have || key != prev) ++count;
            prev = key;
            have = true;
        }
        return count;
    };
    const uint64_t trees = distinct([](uint32_t) { return 63u; }, [](uint32_t) { return true; });       // an index is below 2^58
    for (uint32_t s = 0; s <= H; ++s) {
        const uint64_t at = distinct([s](uint32_t h) { return h > s ? h - s : 0u; }, [](uint32_t) { return true; });
        if (at > capacity) return {4, at, trees, 0};
    }
    uint64_t ancestors = 0;
    for (uint32_t l = 1; l <= 63; ++l) ancestors += distinct([l](uint32_t) { return l; }, [l](uint32_t h) { return h >= l; });
    return {0, changed.size(), trees, ancestors};
}

static void same(const Info& got, const Info& want, const char* what)
{
    if (got.status != want.status || got.n != want.n || got.roots != want.roots) die(what, got.status, got.n, got.roots);
    if (want.status == 0 && got.compared != want.compared) die("the nodes compared are not the distinct ancestors", got.compared, want.compared);
}

// ---- the forest -------------------------------------------------------------------------------------------------------------

struct Forest {
    Cells leaves, levels, roots;
    Forest(uint64_t total, uint64_t stored, uint32_t ntrees, uint64_t poison) : leaves(total, poison), levels(stored, poison + 1), roots(ntrees, poison + 2) {}
};

static void build(Forest& f, const std::vector<uint64_t>& off, uint64_t total, uint32_t H)
{
    const uint32_t ntrees = (uint32_t)off.size() - 1;
    for (uint32_t t = 0; t < ntrees; ++t) {
        const uint64_t o = off[t], c = off[t + 1] - o;
        if (c == 0) {
            f.roots.put(t, 0);
            continue;
        }
        for (uint32_t l = 1; l <= H; ++l) {
            const uint64_t n_in = vkmr_forest::level_count(c, l - 1), n = vkmr_forest::level_count(c, l);
            if (l > 1 && n_in < 2) break;
            const Cells& in = l == 1 ? f.leaves : f.levels;
            const uint64_t in_first = forest_child_base(total, ntrees, l) + vkmr_forest::pos(o, t, l - 1);
            for (uint64_t p = 0; p < n; ++p) {
                const uint64_t x = mix(in.get(in_first + 2 * p), in.get(in_first + vkmr_math::right_child(p, n_in)));
                if (n == 1) f.roots.put(t, x);
                else f.levels.put(vkmr_forest::stored_level_base(total, ntrees, l) + vkmr_forest::pos(o, t, l) + p, x);
            }
        }
    }
}

static Info forest_diff(const Forest& A, const Forest& B, const std::vector<uint64_t>& off, uint64_t total, uint32_t H, uint32_t capacity,
                        std::vector<Entry>& answer)
{
    const uint32_t ntrees = (uint32_t)off.size() - 1;
    const Parts parts(capacity);
    Info info = {0, 0, 0, 0};
    // step 0, as the workgroups take the trees
    const uint32_t groups = root_groups(ntrees);
    const uint64_t span = root_span(ntrees);
    if (groups == 0 || groups > VKMR_DIFF_ROOT_GROUPS || groups > parts.block_words || span % VKMR_DIFF_THREADS || (uint64_t)groups * span < ntrees)
        die("step 0's groups do not cover the trees", groups, span, ntrees);
    std::vector<Entry> frontier;
    for (uint32_t g = 0; g < groups; ++g)
        for (uint64_t t = g * span; t < std::min<uint64_t>((g + 1) * span, ntrees); ++t)
            if (off[t + 1] > off[t] && A.roots.get(t) != B.roots.get(t)) frontier.push_back(Entry((uint32_t)t, 0));
    check_frontier(frontier, 0, 0);
    info.n = info.roots = frontier.size();
    if (frontier.size() > capacity) info.status = 4;
    const uint32_t steps = (capacity == 0 || total == 0) ? 0 : H;
    for (uint32_t step = 1; step <= steps && info.status == 0; ++step) {
        const uint64_t bound = forest_frontier_bound(total, ntrees, capacity, step);
        parts.step(bound, capacity);
        if (frontier.size() > bound) die("the frontier is above the host's bound", step, frontier.size(), bound);
        std::vector<Entry> next;
        for (const Entry& e : frontier) {
            const uint32_t t = e.first;
            const uint64_t o = off[t], c = off[t + 1] - o, p = e.second;
            const uint32_t l = level_at(vkmr_math::height(c), step);
            if (l == 0) {
                next.push_back(e);
                continue;
            }
            ++info.compared;
            if (p >= vkmr_forest::level_count(c, l)) die("an entry is no node of its level", step, t, p);
            const Step s = forest_step(o, c, t, p, l);
            const uint64_t at = forest_child_base(total, ntrees, l) + s.left;
            const Cells &a = l == 1 ? A.leaves : A.levels, &b = l == 1 ? B.leaves : B.levels;
            if (a.get(at) != b.get(at)) next.push_back(Entry(t, 2 * p));
            if (s.has_right && a.get(at + 1) != b.get(at + 1)) next.push_back(Entry(t, 2 * p + 1));
        }
        check_frontier(next, frontier.size(), step);
        frontier.swap(next);
        info.n = frontier.size();
        if (frontier.size() > capacity) info.status = 4;
    }
    answer = frontier;
    return info;
}

// ---- one tree over the same cells ---------------------------------------------------------------------------------------------

struct Tree {
    Cells leaves, levels;
    Tree(uint64_t count, uint64_t cells, uint64_t poison) : leaves(count, poison), levels(cells, poison + 1) {}
};

static void build(Tree& tr, uint64_t count, uint32_t height, const uint64_t* lvl)
{
    for (uint32_t l = 1; l <= height; ++l) {
        const uint64_t n_in = vkmr_math::ceil_shift(count, l - 1), n = vkmr_math::ceil_shift(count, l);
        const Cells& in = l == 1 ? tr.leaves : tr.levels;
        for (uint64_t p = 0; p < n; ++p)
            tr.levels.put(lvl[l] + p, mix(in.get(tree_child_base(lvl, l) + 2 * p), in.get(tree_child_base(lvl, l) + vkmr_math::right_child(p, n_in))));
    }
}

static Info tree_diff(const Tree& A, const Tree& B, uint64_t count, uint32_t height, const uint64_t* lvl, uint32_t capacity, std::vector<Entry>& answer)
{
    const Parts parts(capacity);
    Info info = {0, 0, 0, 0};
    std::vector<Entry> frontier;
    const bool differs = height ? A.levels.get(lvl[height]) != B.levels.get(lvl[height]) : A.leaves.get(0) != B.leaves.get(0);
    if (differs) frontier.push_back(Entry(0, 0));
    info.n = info.roots = frontier.size();
    if (frontier.size() > capacity) info.status = 4;
    const uint32_t steps = capacity == 0 ? 0 : height;
    for (uint32_t step = 1; step <= steps && info.status == 0; ++step) {
        const uint32_t l = level_at(height, step);
        const uint64_t bound = tree_frontier_bound(count, height, capacity, step);
        parts.step(bound, capacity);
        if (l == 0) die("a tree's step below level 1", step);
        if (frontier.size() > bound) die("the tree's frontier is above the host's bound", step, frontier.size(), bound);
        std::vector<Entry> next;
        for (const Entry& e : frontier) {
            const uint64_t p = e.second;
            ++info.compared;
            if (p >= vkmr_math::ceil_shift(count, l)) die("an entry is no node of the tree's level", step, l, p);
            const Step s = tree_step(count, tree_child_base(lvl, l), p, l);
            const Cells &a = l == 1 ? A.leaves : A.levels, &b = l == 1 ? B.leaves : B.levels;
            if (a.get(s.left) != b.get(s.left)) next.push_back(Entry(0, 2 * p));
            if (s.has_right && a.get(s.left + 1) != b.get(s.left + 1)) next.push_back(Entry(0, 2 * p + 1));
        }
        check_frontier(next, frontier.size(), step);
        frontier.swap(next);
        info.n = frontier.size();
        if (frontier.size() > capacity) info.status = 4;
    }
    answer = frontier;
    return info;
}

// ---- one case -----------------------------------------------------------------------------------------------------------------

static void replay(uint64_t first, uint64_t slack, uint64_t max_count, uint32_t capacity, const std::vector<uint64_t>& c, const std::vector<Entry>& entries)
{
    const uint32_t ntrees = (uint32_t)c.size();
    std::vector<uint64_t> off(ntrees + 1);
    std::vector<uint32_t> heights(ntrees);
    off[0] = first;
    uint64_t largest = 0;
    for (uint32_t t = 0; t < ntrees; ++t) {
        off[t + 1] = off[t] + c[t];
        largest = std::max(largest, c[t]);
        heights[t] = 0;
        for (uint64_t n = c[t]; n > 1 || heights[t] == 0; n = (n + 1) / 2) ++heights[t];   // by halving, no call into the headers
    }
    const uint64_t leaves = off[ntrees] - first, total = off[ntrees] + slack;
    if (max_count == 0) max_count = largest ? largest : 1;
    if (largest > max_count) die("a tree above max_count in the test's own input");
    const uint32_t H = vkmr_forest::launches(total, max_count);
    const uint64_t stored = vkmr_forest::stored_cells(total, ntrees, H);

    Forest A(total, stored, ntrees, 0xA5A5A5A500000000ull), B(total, stored, ntrees, 0x5A5A5A5A00000000ull);
    for (uint64_t at = first; at < off[ntrees]; ++at) {
        A.leaves.put(at, mix(at, 1));
        B.leaves.put(at, mix(at, 1));
    }
    for (const Entry& e : entries) {
        if (e.first >= ntrees || e.second >= c[e.first]) die("an entry of the test's own input is out of range", e.first, e.second);
        B.leaves.put(off[e.first] + e.second, mix(off[e.first] + e.second, 2));
    }
    build(A, off, total, H);
    build(B, off, total, H);
    // the model: the two windows cell by cell
    std::vector<Entry> changed;
    for (uint32_t t = 0; t < ntrees; ++t)
        for (uint64_t i = 0; i < c[t]; ++i)
            if (A.leaves.v[off[t] + i] != B.leaves.v[off[t] + i]) changed.push_back(Entry(t, i));
    if (changed != entries) die("the mixing function lost a change");

    std::vector<Entry> answer;
    const Info got = forest_diff(A, B, off, total, H, capacity, answer);
    const Info want = expect(heights, H, changed, capacity);
    same(got, want, "the forest's status, n or differing roots are not the model's");
    if (got.status == 0 && answer != changed) die("the forest's answer is not the changed leaves", answer.size(), changed.size());
    printf("%llu %llu %llu %llu %u\n", (unsigned long long)got.status, (unsigned long long)got.n, (unsigned long long)got.roots,
           (unsigned long long)got.compared, H);

    // the same leaves as one tree, at its own height (0 for one leaf) and one level above
    if (leaves == 0) return;
    std::vector<Entry> flat;
    for (const Entry& e : changed) flat.push_back(Entry(0, off[e.first] - first + e.second));
    const uint32_t own = leaves == 1 ? 0 : vkmr_math::height(leaves);
    for (uint32_t height = own; height <= own + 1; ++height) {
        uint64_t lvl[VKMR_TREE_MAX_LEVELS];
        const uint64_t cells = vkmr_tree::levels(leaves, height, lvl);
        Tree TA(leaves, cells, 0xC3C3C3C300000000ull), TB(leaves, cells, 0x3C3C3C3C00000000ull);
        for (uint64_t i = 0; i < leaves; ++i) {
            TA.leaves.put(i, A.leaves.v[first + i]);
            TB.leaves.put(i, B.leaves.v[first + i]);
        }
        build(TA, leaves, height, lvl);
        build(TB, leaves, height, lvl);
        const Info tgot = tree_diff(TA, TB, leaves, height, lvl, capacity, answer);
        const Info twant = expect(std::vector<uint32_t>(1, height), height, flat, capacity);
        same(tgot, twant, "the tree's status, n or differing root are not the model's");
        if (tgot.status == 0 && answer != flat) die("the tree's answer is not the changed leaves", answer.size(), flat.size());
    }
}

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    unsigned long long first, slack, max_count, capacity, ntrees, k, x, y;
    size_t cases = 0;
    while (fscanf(f, "%llu %llu %llu %llu %llu", &first, &slack, &max_count, &capacity, &ntrees) == 5) {
        std::vector<uint64_t> c;
        for (unsigned long long t = 0; t < ntrees; ++t) {
            if (fscanf(f, "%llu", &x) != 1) return 2;
            c.push_back(x);
        }
        if (fscanf(f, "%llu", &k) != 1) return 2;
        std::vector<Entry> entries;
        for (unsigned long long q = 0; q < k; ++q) {
            if (fscanf(f, "%llu %llu", &x, &y) != 2) return 2;
            entries.push_back(Entry((uint32_t)x, y));
        }
        replay(first, slack, max_count, (uint32_t)capacity, c, entries);
        ++cases;
    }
    fclose(f);
    printf("ok: %zu forests\n", cases);
    return 0;
}
