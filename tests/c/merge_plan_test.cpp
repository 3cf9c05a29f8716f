// merge_plan_test.cpp -- csrc/merge_plan.hpp replayed on the CPU.  A stand-alone program (tests/test_merge_abi.py compiles it with
// -fsanitize=address,undefined):
//   1. the placement: forests A (strictly increasing trees) and B (non-decreasing trees) laid at an offset with slack behind go
//      through the kernels' steps with values -- the lower bound by absence_plan.hpp's loop, the counts and marks at the slots,
//      the flags, pos0, the two-level exclusive prefix in rows of VKMR_MERGE_SCAN_ROW words, then every leaf to a_dest / b_dest
//      and every tree to tree_start -- for all three ops, against std::set_union, std::set_difference and std::set_intersection
//      over the trees after std::unique of B's; every output cell written exactly once and none at or behind n_out; the three
//      n_out identities.  The shapes: B empty, below A, above A (the shared slot of the next tree), equal to A, larger than A,
//      into an empty tree, both empty, runs of 1, 2, 64, 65 and 257 leaves of B at slot 0, in the middle and behind the last leaf,
//      a repeat across a tree boundary of B, the all-zero and the all-ones digest, a forest whose words cross a row of the scan,
//      and random trees of 0 to 300 leaves a side from a 9-bit alphabet in word 7
//   2. the scratch layout: the parts in order, aligned, none overlapping, the scan region whole rows that hold every word
// Prints "FAIL ..." and returns 1 otherwise.
#include <algorithm>
#include <array>
#include <cinttypes>
#include <cstdio>
#include <random>
#include <vector>

#include "absence_plan.hpp"
#include "merge_plan.hpp"

namespace {

int g_fail = 0;

#define CHECK(cond, ...)                         \
    do {                                         \
        if (!(cond)) {                           \
            if (g_fail++ < 20) {                 \
                std::printf("FAIL %s: ", #cond); \
                std::printf(__VA_ARGS__);        \
                std::printf("\n");               \
            }                                    \
            return false;                        \
        }                                        \
    } while (0)

typedef std::array<uint32_t, 8> Digest;
typedef std::vector<Digest> Tree;

bool digest_less(const Digest& a, const Digest& b) { return vkmr_absence::less(a.data(), b.data()); }

Digest small(uint32_t w7) { return Digest{7u, 7u, 7u, 7u, 7u, 7u, 7u, w7}; }

// A forest laid at cell `first` of a buffer with `slack` cells behind.
struct Laid {
    std::vector<Digest> cells;
    std::vector<uint64_t> offsets;
    uint64_t total() const { return cells.size(); }
    uint64_t lo() const { return offsets.front(); }
    uint64_t n() const { return offsets.back() - offsets.front(); }
};

Laid lay(const std::vector<Tree>& trees, uint64_t first, uint64_t slack)
{
    Laid L;
    L.cells.assign(first, small(0xDEADu));
    L.offsets.push_back(first);
    for (const Tree& t : trees) {
        L.cells.insert(L.cells.end(), t.begin(), t.end());
        L.offsets.push_back(L.cells.size());
    }
    L.cells.insert(L.cells.end(), slack, small(0xBEEFu));
    return L;
}

// The kernels' steps with values, and the result against the standard algorithms.
bool replay(const std::vector<Tree>& ta, const std::vector<Tree>& tb, uint64_t first_a, uint64_t slack_a, uint64_t first_b, uint64_t slack_b, uint32_t op,
            size_t* leaves)
{
    const Laid A = lay(ta, first_a, slack_a), B = lay(tb, first_b, slack_b);
    const uint32_t ntrees = (uint32_t)ta.size();
    const uint64_t a_total = A.total(), b_total = B.total(), nA = A.n(), nB = B.n();
    CHECK(vkmr_merge::fits(a_total, b_total), "fits");
    const vkmr_merge::Layout L = vkmr_merge::layout(a_total, b_total);
    std::vector<uint32_t> scan((size_t)L.rows * VKMR_MERGE_SCAN_ROW, 0u), tot((size_t)L.rows, 0u), pos0((size_t)b_total, 0x12345678u);
    uint64_t matches = 0, repeats = 0;
    // the mark kernel: a lane per element of B
    for (uint32_t t = 0; t < ntrees; ++t) {
        const uint64_t o = A.offsets[t], c = A.offsets[t + 1] - o;
        for (uint64_t cell = B.offsets[t]; cell < B.offsets[t + 1]; ++cell) {
            const uint64_t j = cell - B.lo();
            const Digest& me = B.cells[cell];
            const bool repeat = cell > B.offsets[t] && vkmr_absence::equal(me.data(), B.cells[cell - 1].data());
            const uint64_t lb = vkmr_absence::lower_bound(c, [&](uint64_t mid) { return vkmr_absence::less(A.cells[o + mid].data(), me.data()); });
            const bool match = lb < c && vkmr_absence::equal(A.cells[o + lb].data(), me.data());
            const uint64_t slot = o - A.lo() + lb;
            CHECK(slot < L.S && L.S + j < L.words - 1u, "slot %" PRIu64 " of %" PRIu64, slot, L.S);
            if (vkmr_merge::kept(op, repeat, match)) {
                scan[slot] += 1u;
                scan[L.S + j] = 1u;
                pos0[j] = (uint32_t)slot;
            } else {
                pos0[j] = VKMR_MERGE_NONE;
            }
            if (vkmr_merge::marks(op, repeat, match)) {
                CHECK(scan[slot] == 0u, "slot %" PRIu64 " marked twice", slot);
                scan[slot] = 1u;
            }
            matches += match && !repeat;
            repeats += repeat;
        }
    }
    // the scan: every row in place, the row sums, their prefix
    for (uint64_t r = 0; r < L.rows; ++r) {
        uint32_t carry = 0u;
        for (uint32_t g = 0; g < VKMR_MERGE_SCAN_ROW; ++g) {
            uint32_t& w = scan[(size_t)r * VKMR_MERGE_SCAN_ROW + g];
            const uint32_t v = w;
            w = carry;
            carry += v;
        }
        tot[r] = carry;
    }
    uint32_t carry = 0u;
    for (uint64_t r = 0; r < L.rows; ++r) {
        const uint32_t v = tot[r];
        tot[r] = carry;
        carry += v;
    }
    auto E = [&](uint64_t x) { return vkmr_merge::prefix(scan.data(), tot.data(), x); };
    const uint32_t e_S = E(L.S);
    const uint64_t n_out = vkmr_merge::n_out(op, nA, e_S);
    CHECK(n_out == vkmr_merge::n_out_of_counts(op, nA, nB, matches, repeats), "op %u: n_out %" PRIu64 " from the scan, nA %" PRIu64 " nB %" PRIu64 " matches %" PRIu64
          " repeats %" PRIu64, op, n_out, nA, nB, matches, repeats);
    // the emit kernel: every leaf to its closed-form cell
    const uint64_t capacity = nA + nB + 3u;
    std::vector<Digest> out((size_t)capacity, small(0xA5A5u));
    std::vector<uint32_t> written((size_t)capacity, 0u);
    for (uint64_t i = 0; i < nA; ++i) {
        uint64_t dest;
        if (!vkmr_merge::a_dest(op, i, E(i), E(i + 1u), &dest)) continue;
        CHECK(dest < n_out, "op %u: leaf %" PRIu64 " of A goes to %" PRIu64 " of %" PRIu64, op, i, dest, n_out);
        out[dest] = A.cells[A.lo() + i];
        ++written[dest];
    }
    for (uint64_t j = 0; op == VKMR_MERGE_UNION && j < nB; ++j) {
        if (pos0[j] == VKMR_MERGE_NONE) continue;
        const uint64_t dest = vkmr_merge::b_dest(pos0[j], E(L.S + j) - e_S);
        CHECK(dest < n_out, "leaf %" PRIu64 " of B goes to %" PRIu64 " of %" PRIu64, j, dest, n_out);
        out[dest] = B.cells[B.lo() + j];
        ++written[dest];
    }
    for (uint64_t k = 0; k < capacity; ++k) CHECK(written[k] == (k < n_out ? 1u : 0u), "op %u: cell %" PRIu64 " written %u times, n_out %" PRIu64, op, k, written[k], n_out);
    // against the standard algorithms, tree by tree from tree_start
    uint64_t at = 0;
    for (uint32_t t = 0; t <= ntrees; ++t) {
        const uint64_t base_a = A.offsets[t] - A.lo(), base_b = B.offsets[t] - B.lo();
        const uint64_t start = vkmr_merge::tree_start(op, base_a, E(base_a), E(L.S + base_b) - e_S);
        CHECK(start == at, "op %u: tree %u starts at %" PRIu64 ", the trees in front hold %" PRIu64, op, t, start, at);
        if (t == ntrees) break;
        Tree b = tb[t], want;
        b.erase(std::unique(b.begin(), b.end()), b.end());
        if (op == VKMR_MERGE_UNION) std::set_union(ta[t].begin(), ta[t].end(), b.begin(), b.end(), std::back_inserter(want), digest_less);
        else if (op == VKMR_MERGE_DIFFERENCE) std::set_difference(ta[t].begin(), ta[t].end(), b.begin(), b.end(), std::back_inserter(want), digest_less);
        else std::set_intersection(ta[t].begin(), ta[t].end(), b.begin(), b.end(), std::back_inserter(want), digest_less);
        for (size_t k = 0; k < want.size(); ++k) CHECK(at + k < n_out && out[at + k] == want[k], "op %u: tree %u leaf %zu", op, t, k);
        at += want.size();
    }
    CHECK(at == n_out, "op %u: %" PRIu64 " leaves, n_out %" PRIu64, op, at, n_out);
    *leaves += nA + nB;
    return true;
}

bool replay_all_ops(const std::vector<Tree>& ta, const std::vector<Tree>& tb, uint64_t first_a, uint64_t slack_a, uint64_t first_b, uint64_t slack_b, size_t* leaves)
{
    for (uint32_t op = 0; op < 3u; ++op)
        if (!replay(ta, tb, first_a, slack_a, first_b, slack_b, op, leaves)) return false;
    return true;
}

Tree range(uint32_t from, uint32_t n, uint32_t step = 1u)
{
    Tree t;
    for (uint32_t i = 0; i < n; ++i) t.push_back(small(from + i * step));
    return t;
}

Tree sorted(Tree t)
{
    std::sort(t.begin(), t.end(), digest_less);
    return t;
}

Tree join(std::initializer_list<Tree> parts)
{
    Tree t;
    for (const Tree& p : parts) t.insert(t.end(), p.begin(), p.end());
    return sorted(t);
}

// ---- 2. the scratch layout -------------------------------------------------------------------------------------------------------

bool check_layout(uint64_t a_total, uint64_t b_total)
{
    if (!vkmr_merge::fits(a_total, b_total)) {
        CHECK(vkmr_merge::scratch_bytes(a_total, b_total) == 0u, "a size that does not fit has no scratch");
        return true;
    }
    const vkmr_merge::Layout L = vkmr_merge::layout(a_total, b_total);
    CHECK(L.S == a_total + 1u && L.words == a_total + b_total + 2u, "S and words");
    CHECK(L.rows * VKMR_MERGE_SCAN_ROW >= L.words && (L.rows - 1u) * VKMR_MERGE_SCAN_ROW < L.words, "%" PRIu64 " rows for %" PRIu64 " words", L.rows, L.words);
    CHECK(L.scan == 0u && L.tot == 4u * L.rows * VKMR_MERGE_SCAN_ROW && L.grand >= L.tot + 4u * L.rows && L.pos0 == L.grand + 16u, "scan, tot, grand");
    CHECK(L.hdr >= L.pos0 + 4u * b_total && L.bytes == L.hdr + 8u * VKMR_MERGE_HEADER_WORDS, "pos0, hdr");
    for (size_t part : {L.scan, L.tot, L.grand, L.pos0, L.hdr, L.bytes}) CHECK(part % 16u == 0u, "a part off the 16-byte grid");
    CHECK(vkmr_merge::scratch_bytes(a_total, b_total) == L.bytes, "scratch_bytes");
    return true;
}

}  // namespace

int main()
{
    size_t leaves = 0, forests = 0;
    const Digest zero = Digest{0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u}, ones = Digest{~0u, ~0u, ~0u, ~0u, ~0u, ~0u, ~0u, ~0u};
    const Digest half_below = Digest{0x7FFFFFFFu, ~0u, ~0u, ~0u, ~0u, ~0u, ~0u, ~0u}, half = Digest{0x80000000u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    // the case shapes: A's leaves at w7 = 1000, 2000, ... so that runs fit between them
    {
        const Tree a10 = range(1000u, 10u, 1000u);
        std::vector<Tree> ta, tb;
        auto add = [&](const Tree& a, const Tree& b) { ta.push_back(a); tb.push_back(b); };
        add(a10, {});                                                         // B empty
        add(a10, range(1u, 5u));                                              // below A's first leaf
        add(a10, range(20000u, 5u));                                          // above A's last: the slot of the next tree's first element
        add(a10, a10);                                                        // equal, leaf for leaf
        add(range(1000u, 3u, 1000u), range(500u, 40u, 100u));                 // larger than A
        add({}, join({range(5u, 4u), {a10[0]}}));                             // into an empty tree; its last digest ...
        add(a10, join({{a10[0]}, range(1001u, 3u)}));                         // ... opens the next tree of B: no repeat across the boundary
        add({}, {});                                                          // both empty
        for (uint32_t run : {1u, 2u, 64u, 65u, 257u}) {
            add(a10, range(10u, run));                                        // at slot 0
            add(a10, range(5001u, run));                                      // in the middle
            add(a10, range(10001u, run));                                     // behind the last leaf
            add(a10, join({range(10u, run), range(5001u, run), range(10001u, run), {a10[4], a10[4], a10[9]}, Tree(40, small(7777u))}));
        }
        add({zero, half_below, half, ones}, {zero, zero, half_below, half_below, half, ones, ones});
        add({half_below, half}, {zero, ones});
        add({}, {});
        for (auto place : {std::array<uint64_t, 4>{0u, 0u, 0u, 0u}, std::array<uint64_t, 4>{37u, 100u, 11u, 7u}}) {
            if (!replay_all_ops(ta, tb, place[0], place[1], place[2], place[3], &leaves)) return 1;
            ++forests;
        }
        // one tree, one leaf against one leaf
        if (!replay_all_ops(std::vector<Tree>{a10}, std::vector<Tree>{join({a10, range(1u, 300u, 7u)})}, 0u, 0u, 0u, 0u, &leaves)) return 1;
        if (!replay_all_ops(std::vector<Tree>{Tree{a10[0]}}, std::vector<Tree>{Tree{a10[0]}}, 0u, 0u, 0u, 0u, &leaves)) return 1;
        if (!replay_all_ops(std::vector<Tree>{Tree{a10[0]}}, std::vector<Tree>{Tree{a10[1]}}, 0u, 0u, 3u, 1u, &leaves)) return 1;
        forests += 3;
    }
    // matches and non-matches alternating over more than one row of the scan: 3 trees of 4 000 leaves, B every other leaf and a
    // digest above every third
    {
        std::vector<Tree> ta, tb;
        for (uint32_t t = 0; t < 3u; ++t) {
            ta.push_back(range(10u, 4000u, 10u));
            tb.push_back(join({range(10u, 2000u, 20u), range(11u, 1333u, 30u)}));
        }
        if (!replay_all_ops(ta, tb, 5u, 9u, 8195u, 0u, &leaves)) return 1;
        ++forests;
    }
    // random trees of 0 to 300 leaves a side from a 9-bit alphabet in word 7
    std::mt19937_64 rng(20261021u);
    for (int f = 0; f < 40; ++f) {
        const uint32_t ntrees = 1u + (uint32_t)(rng() % 12u);
        std::vector<Tree> ta, tb;
        for (uint32_t t = 0; t < ntrees; ++t) {
            Tree a, b;
            for (uint64_t i = rng() % 301u; i > 0; --i) a.push_back(small((uint32_t)(rng() % 512u)));
            for (uint64_t i = rng() % 301u; i > 0; --i) b.push_back(small((uint32_t)(rng() % 512u)));
            a = sorted(a);
            a.erase(std::unique(a.begin(), a.end()), a.end());
            ta.push_back(a);
            tb.push_back(sorted(b));
        }
        if (!replay_all_ops(ta, tb, rng() % 50u, rng() % 50u, rng() % 50u, rng() % 50u, &leaves)) return 1;
        ++forests;
    }
    for (uint64_t a : {0ull, 1ull, 100ull, 8190ull, 8191ull, 8192ull, 5933ull, 1ull << 26, (1ull << 32) - 3ull, 1ull << 32, 1ull << 40})
        for (uint64_t b : {0ull, 1ull, 2ull, 8192ull, 1ull << 16, 1ull << 24, (1ull << 32) - 1ull})
            if (!check_layout(a, b)) return 1;
    if (g_fail) return 1;
    std::printf("ok: %zu leaves merged three ways, %zu forests\n", leaves, forests);
    return 0;
}
