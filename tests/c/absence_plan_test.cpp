// absence_plan_test.cpp -- csrc/absence_plan.hpp replayed on the CPU with a toy hash, for every tree of 1..130 leaves and every
// index 0..c: ctz as `top`, which cells of the two rows the check reads (the rows are heap arrays of exactly H(c) cells, so a
// read outside them is AddressSanitizer's to report), that the compact fold reaches the root a level-by-level build gives, that
// it agrees with two plain folds, the hash count, the verdicts present / absent / not proven, the order and the lower bound's loop.
// A program of its own: `absence_plan_test` prints "ok: <cases> cases" and returns 0, or says FAIL and returns 1.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <set>
#include <utility>
#include <vector>

#include "absence_plan.hpp"

namespace {

struct Cell { uint32_t w[8]; };

int failures = 0;
#define EXPECT(cond, ...)                      \
    do {                                       \
        if (!(cond)) {                         \
            if (failures++ < 20) {             \
                printf("FAIL %s: ", #cond);    \
                printf(__VA_ARGS__);           \
                printf("\n");                  \
            }                                  \
        }                                      \
    } while (0)

uint64_t pair_calls = 0;

// Not a hash anyone should use: it only has to tell (a, b) from (b, a) and from every other pair the sweep forms.
void toy_pair(const uint32_t* a, const uint32_t* b, uint32_t* out)
{
    ++pair_calls;
    uint64_t s = 0x9E3779B97F4A7C15ull;
    for (int w = 0; w < 8; ++w) s = (s ^ a[w]) * 0x100000001B3ull + 0x632BE59Bull;
    for (int w = 0; w < 8; ++w) s = (s ^ b[w]) * 0x100000001B3ull + 0x85EBCA6Bull;
    for (int w = 0; w < 8; ++w) {
        s ^= s >> 29;
        s *= 0xBF58476D1CE4E5B9ull;
        out[w] = (uint32_t)(s >> 32);
    }
}

// Leaf j of the sweep's trees: word 0 = 2j + 1, so that the digest with word 0 = 2i stands between leaves i - 1 and i.
Cell leaf_of(uint64_t j)
{
    Cell x;
    x.w[0] = (uint32_t)(2 * j + 1);
    for (int w = 1; w < 8; ++w) x.w[w] = 0x01010101u * (uint32_t)w + (uint32_t)j;
    return x;
}

Cell gap_of(uint64_t i)
{
    Cell x = leaf_of(i);
    x.w[0] = (uint32_t)(2 * i);
    return x;
}

bool same(const Cell& a, const Cell& b) { return memcmp(a.w, b.w, 32) == 0; }

// levels[l], 0 <= l <= H: the duplicate-last tree, built level by level.
std::vector<std::vector<Cell>> build(uint64_t c)
{
    std::vector<std::vector<Cell>> levels(1);
    for (uint64_t j = 0; j < c; ++j) levels[0].push_back(leaf_of(j));
    for (uint32_t l = 0; l < vkmr_absence::height(c); ++l) {
        const std::vector<Cell>& in = levels[l];
        std::vector<Cell> out((in.size() + 1) / 2);
        for (size_t j = 0; j < out.size(); ++j) toy_pair(in[2 * j].w, in[vkmr_math::right_child(j, in.size())].w, out[j].w);
        levels.push_back(out);
    }
    return levels;
}

// The plain inclusion proof of leaf i, and its fold; `at`, where given, receives the node the fold stands on at every level.
std::vector<Cell> plain_proof(const std::vector<std::vector<Cell>>& levels, uint64_t i, uint32_t H)
{
    std::vector<Cell> row(H);
    for (uint32_t l = 0; l < H; ++l) row[l] = levels[l][vkmr_math::sibling(i >> l, levels[l].size())];
    return row;
}

Cell plain_fold(Cell cur, uint64_t i, const std::vector<Cell>& row, std::vector<Cell>* at = nullptr)
{
    for (uint32_t l = 0; l < row.size(); ++l) {
        if (at) at->push_back(cur);
        Cell next;
        if ((i >> l) & 1ull) toy_pair(row[l].w, cur.w, next.w);
        else toy_pair(cur.w, row[l].w, next.w);
        cur = next;
    }
    if (at) at->push_back(cur);
    return cur;
}

struct Reads {
    std::set<std::pair<uint32_t, uint32_t>>* seen;
    void operator()(uint32_t row, uint32_t l) const { seen->insert({row, l}); }
};

uint32_t check(const Cell& x, uint64_t i, const Cell& pred, const Cell& succ, const Cell* main_row, const Cell* low_row, uint32_t h, const Cell& root, uint64_t c,
               std::set<std::pair<uint32_t, uint32_t>>* seen = nullptr, uint32_t t = 0, uint32_t ntrees = 1)
{
    std::set<std::pair<uint32_t, uint32_t>> mine;
    return vkmr_absence::verdict(x.w, t, ntrees, i, pred.w, succ.w, main_row ? main_row->w : nullptr, low_row ? low_row->w : nullptr, h, h, root.w, c, toy_pair,
                                 Reads{seen ? seen : &mine});
}

void order_and_bound()
{
    Cell a = {}, b = {};
    a.w[0] = 0x7FFFFFFFu;
    b.w[0] = 0x80000000u;
    for (int w = 1; w < 8; ++w) a.w[w] = 0xFFFFFFFFu;
    EXPECT(vkmr_absence::less(a.w, b.w) && !vkmr_absence::less(b.w, a.w), "word 0 is unsigned");
    Cell lo7 = leaf_of(3), hi7 = leaf_of(3);
    hi7.w[7] += 1;
    EXPECT(vkmr_absence::less(lo7.w, hi7.w) && !vkmr_absence::less(hi7.w, lo7.w) && !vkmr_absence::equal(lo7.w, hi7.w), "word 7 decides last");
    Cell first = leaf_of(3), second = leaf_of(3);
    first.w[1] = 1; first.w[7] = 0xFFFFFFFFu;
    second.w[1] = 2; second.w[7] = 0;
    EXPECT(vkmr_absence::less(first.w, second.w), "an earlier word outweighs a later one");
    EXPECT(!vkmr_absence::less(lo7.w, lo7.w) && vkmr_absence::equal(lo7.w, lo7.w), "a digest is not below itself");
    EXPECT(vkmr_absence::height(0) == 0 && vkmr_absence::height(1) == 1 && vkmr_absence::height(2) == 1 && vkmr_absence::height(3) == 2 &&
               vkmr_absence::height(130) == 8, "H");
    for (uint64_t c = 0; c <= 130; ++c) {
        std::vector<Cell> leaves;
        for (uint64_t j = 0; j < c; ++j) leaves.push_back(leaf_of(j));
        for (uint64_t i = 0; i <= c; ++i) {
            const Cell g = gap_of(i);
            const uint64_t at = vkmr_absence::lower_bound(c, [&](uint64_t mid) { return vkmr_absence::less(leaves[mid].w, g.w); });
            EXPECT(at == i, "lower bound of gap %llu in %llu leaves is %llu", (unsigned long long)i, (unsigned long long)c, (unsigned long long)at);
            if (i < c) {
                const uint64_t on = vkmr_absence::lower_bound(c, [&](uint64_t mid) { return vkmr_absence::less(leaves[mid].w, leaves[i].w); });
                EXPECT(on == i, "lower bound of leaf %llu in %llu leaves is %llu", (unsigned long long)i, (unsigned long long)c, (unsigned long long)on);
            }
        }
    }
}

}  // namespace

int main()
{
    order_and_bound();
    uint64_t cases = 0;
    const Cell zero = {};
    Cell garbage;
    for (int w = 0; w < 8; ++w) garbage.w[w] = 0xDEAD0000u + (uint32_t)w;
    for (uint64_t c = 1; c <= 130; ++c) {
        const std::vector<std::vector<Cell>> levels = build(c);
        const uint32_t H = vkmr_absence::height(c);
        const Cell root = levels[H][0];
        EXPECT(levels[H].size() == 1, "c %llu: level H has one node", (unsigned long long)c);
        for (uint64_t i = 0; i <= c; ++i, ++cases) {
            const bool two = i > 0 && i < c;
            uint32_t top = 0;
            if (i > 0) while (!((i >> top) & 1ull)) ++top;
            if (i > 0) EXPECT(vkmr_absence::top(i) == top, "top(%llu)", (unsigned long long)i);
            EXPECT(vkmr_absence::two_sided(i, c) == two, "two_sided");
            if (two) EXPECT(top < H, "c %llu i %llu: top %u is below H %u", (unsigned long long)c, (unsigned long long)i, top, H);
            const uint64_t a = vkmr_absence::anchor(i, c);
            EXPECT(a == (i < c ? i : c - 1), "anchor");
            const Cell pred = i > 0 ? levels[0][i - 1] : zero, succ = i < c ? levels[0][i] : zero, x = gap_of(i);
            // the rows, exactly H cells each on the heap; the low row garbage wherever the plan says no cell lies
            std::vector<Cell> main_row = plain_proof(levels, a, H), low_row(H, garbage);
            for (uint32_t l = 0; l < H; ++l) {
                EXPECT(vkmr_absence::low_cell(i, c, l) == (two && l < top), "low_cell");
                if (two && l < top) {
                    const uint64_t p = (i - 1) >> l;
                    EXPECT((p & 1ull) && (p ^ 1ull) < levels[l].size(), "c %llu i %llu l %u: a left sibling that exists", (unsigned long long)c, (unsigned long long)i, l);
                    low_row[l] = levels[l][p ^ 1ull];
                }
            }
            std::set<std::pair<uint32_t, uint32_t>> seen, want;
            for (uint32_t l = 0; l < H; ++l) want.insert({0u, l});
            for (uint32_t l = 0; two && l < top; ++l) want.insert({1u, l});
            const uint64_t before = pair_calls;
            const uint32_t v = check(x, i, pred, succ, main_row.data(), low_row.data(), H, root, c, &seen);
            EXPECT(v == VKMR_ABSENCE_ABSENT, "c %llu i %llu: verdict %u", (unsigned long long)c, (unsigned long long)i, v);
            EXPECT(pair_calls - before == vkmr_absence::hashes(i, c) && vkmr_absence::hashes(i, c) == H + (two ? top : 0u), "c %llu i %llu: %llu hashes",
                   (unsigned long long)c, (unsigned long long)i, (unsigned long long)(pair_calls - before));
            EXPECT(seen == want, "c %llu i %llu: the cells read", (unsigned long long)c, (unsigned long long)i);
            // two plain folds: both reach the root, and the predecessor's stands on main[top] at level top
            std::vector<Cell> at;
            EXPECT(same(plain_fold(i < c ? succ : pred, a, main_row), root), "c %llu i %llu: the anchor's plain fold", (unsigned long long)c, (unsigned long long)i);
            if (two) {
                EXPECT(same(plain_fold(pred, i - 1, plain_proof(levels, i - 1, H), &at), root), "the predecessor's plain fold");
                EXPECT(same(at[top], main_row[top]), "c %llu i %llu: the paths meet at main[top]", (unsigned long long)c, (unsigned long long)i);
                for (uint32_t l = 0; l < top; ++l) EXPECT(same(plain_proof(levels, i - 1, H)[l], low_row[l]), "the low row is the plain proof below top");
            }
            // present: the leaf itself as the query; pred and the low row are not looked at
            if (i < c) {
                std::vector<Cell> junk(H, garbage);
                seen.clear();
                EXPECT(check(succ, i, garbage, succ, main_row.data(), junk.data(), H, root, c, &seen) == VKMR_ABSENCE_PRESENT, "c %llu i %llu: present",
                       (unsigned long long)c, (unsigned long long)i);
                for (const auto& r : seen) EXPECT(r.first == 0u, "a present proof reads the main row alone");
            }
            // not proven: the neighbours swapped, the query on or outside its neighbours, a wrong count / height / tree / root
            if (two) EXPECT(check(x, i, succ, pred, main_row.data(), low_row.data(), H, root, c) == VKMR_ABSENCE_NOT_PROVEN, "pred and succ swapped");
            if (i > 0) EXPECT(check(pred, i, pred, succ, main_row.data(), low_row.data(), H, root, c) == VKMR_ABSENCE_NOT_PROVEN, "x == pred");
            if (i < c) EXPECT(check(gap_of(i + 1), i, pred, succ, main_row.data(), low_row.data(), H, root, c) == VKMR_ABSENCE_NOT_PROVEN, "x above succ");
            EXPECT(check(x, c + 1, pred, succ, main_row.data(), low_row.data(), H, root, c) == VKMR_ABSENCE_NOT_PROVEN, "index above the count");
            EXPECT(check(x, i, pred, succ, main_row.data(), low_row.data(), H + 1, root, c) == VKMR_ABSENCE_NOT_PROVEN, "a wrong height");
            EXPECT(check(x, i, pred, succ, main_row.data(), low_row.data(), H, root, c, nullptr, 1, 1) == VKMR_ABSENCE_NOT_PROVEN, "a tree outside the forest");
            EXPECT(check(x, i, pred, succ, main_row.data(), low_row.data(), H, garbage, c) == VKMR_ABSENCE_NOT_PROVEN, "another root");
            if (i == c && vkmr_absence::height(c + 1) == H)
                EXPECT(check(x, i, pred, succ, main_row.data(), low_row.data(), H, root, c + 1) == VKMR_ABSENCE_NOT_PROVEN, "above the last leaf under a count one larger");
            for (uint32_t l = 0; two && l < top; ++l) {
                std::vector<Cell> bent = low_row;
                bent[l].w[l & 7u] ^= 1u;
                EXPECT(check(x, i, pred, succ, main_row.data(), bent.data(), H, root, c) == VKMR_ABSENCE_NOT_PROVEN, "a low cell below top flipped");
            }
        }
    }
    // no leaf: absent under the zero root alone, with no row at all
    EXPECT(check(gap_of(0), 0, zero, zero, nullptr, nullptr, 0, zero, 0) == VKMR_ABSENCE_ABSENT, "an empty tree under the zero root");
    EXPECT(check(gap_of(0), 0, zero, zero, nullptr, nullptr, 0, garbage, 0) == VKMR_ABSENCE_NOT_PROVEN, "an empty tree under another root");
    EXPECT(check(gap_of(0), 1, zero, zero, nullptr, nullptr, 0, zero, 0) == VKMR_ABSENCE_NOT_PROVEN, "an index into an empty tree");
    if (failures) {
        printf("FAIL: %d check(s)\n", failures);
        return 1;
    }
    printf("ok: %llu cases\n", (unsigned long long)cases);
    return 0;
}
