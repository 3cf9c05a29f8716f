// merkleblock_plan_test.cpp -- csrc/merkleblock_plan.hpp replayed with values, a program of its own (built with
// -fsanitize=address,undefined by tests/merkleblock_cases.py).  Per case it places every flag and every hash the way the
// kernels do -- a prefix sum of the groups over the sorted entries, then one step per (entry, level) -- into arrays sized by
// the three bounds, and compares them with a recursive walk of the rule written here on its own: every flag, every hash's
// (level, node), each written exactly once, nothing outside the bounds.
//
// Input, one case a line:  max_count ntrees c_0 .. c_{ntrees-1} k t_0 i_0 .. t_{k-1} i_{k-1}      (entries sorted, in range)
// Output, one line a case: blocks flags hashes flag_bytes;  then "ok: N cases".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <set>
#include <sstream>
#include <string>
#include <utility>
#include <vector>

#include "merkleblock_plan.hpp"

namespace {

struct Cell { uint32_t t, l; uint64_t p; bool operator==(const Cell& o) const { return t == o.t && l == o.l && p == o.p; } };

int fails = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            if (fails++ < 20) {                            \
                std::printf("FAIL %s: ", #cond);           \
                std::printf(__VA_ARGS__);                  \
                std::printf("\n");                         \
            }                                              \
        }                                                  \
    } while (0)

// The rule itself, recursively.
struct Walk {
    uint64_t c;
    std::vector<std::set<uint64_t>> A;
    std::vector<int> flags;
    std::vector<std::pair<uint32_t, uint64_t>> cells;
    void visit(uint32_t l, uint64_t p)
    {
        const bool f = A[l].count(p) != 0;
        flags.push_back(f ? 1 : 0);
        if (l == 0 || !f) {
            cells.push_back({l, p});
            return;
        }
        visit(l - 1, 2 * p);
        if (2 * p + 1 < vkmr_forest::level_count(c, l - 1)) visit(l - 1, 2 * p + 1);
    }
};

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    std::string line;
    size_t cases = 0;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        uint64_t max_count;
        uint32_t ntrees, k;
        ss >> max_count >> ntrees;
        std::vector<uint64_t> counts(ntrees);
        uint64_t total = 0;
        for (auto& c : counts) { ss >> c; total += c; }
        ss >> k;
        std::vector<uint32_t> trees(k);
        std::vector<uint64_t> idx(k);
        for (uint32_t q = 0; q < k; ++q) ss >> trees[q] >> idx[q];
        if (!ss) return 3;
        const uint32_t stride = vkmr_forest::launches(total, max_count);
        const uint64_t cap_h = vkmr_mb::max_hashes(total, ntrees, max_count, k), cap_b = vkmr_mb::max_flag_bytes(total, ntrees, max_count, k);
        const vkmr_mb::Layout L = vkmr_mb::layout(k, stride);
        CHECK(cap_b <= L.words * 4 && cap_h <= (uint64_t)k * (stride + 1ull), "case %zu: the scratch bound is below the call's", cases);

        // the groups and their prefix sums, entry by entry; a tree's tail goes with its last entry
        std::vector<uint64_t> flag_at(k), hash_at(k), bit_start, hash_start;
        std::vector<uint32_t> block_of(k);
        uint64_t F = 0, Hs = 0;
        for (uint32_t q = 0; q < k; ++q) {
            const bool has_prev = q > 0 && trees[q - 1] == trees[q], has_next = q + 1 < k && trees[q + 1] == trees[q];
            const uint64_t c = counts[trees[q]];
            const uint32_t h = vkmr_mb::height(c);
            CHECK(h <= stride, "case %zu: height %u above the stride %u", cases, h, stride);
            const vkmr_mb::Group g = vkmr_mb::group(has_prev, has_prev ? idx[q - 1] : 0, idx[q], h);
            if (!has_prev) { bit_start.push_back(F); hash_start.push_back(Hs); }
            block_of[q] = (uint32_t)bit_start.size() - 1;
            flag_at[q] = F;
            hash_at[q] = Hs;
            const uint32_t tail = has_next ? 0u : vkmr_mb::tail(idx[q], c, h);
            F += g.flags + tail;
            Hs += g.hashes + tail;
        }
        bit_start.push_back(F);
        hash_start.push_back(Hs);
        const size_t B = bit_start.size() - 1;
        std::vector<uint64_t> byte_start(B + 1, 0);
        for (size_t b = 0; b < B; ++b) byte_start[b + 1] = byte_start[b] + (bit_start[b + 1] - bit_start[b] + 7) / 8;
        CHECK(Hs <= cap_h, "case %zu: %llu hashes above the bound %llu", cases, (unsigned long long)Hs, (unsigned long long)cap_h);
        CHECK(byte_start[B] <= cap_b, "case %zu: %llu flag bytes above the bound %llu", cases, (unsigned long long)byte_start[B], (unsigned long long)cap_b);

        // the emit, one step per (entry, level): arrays of exactly the bounds' sizes, so that the sanitizer sees any step outside
        std::vector<int> bits(cap_b * 8, 0), bit_writes(cap_b * 8, 0);
        std::vector<Cell> out(cap_h, Cell{~0u, 0, 0});
        std::vector<int> writes(cap_h, 0);
        auto put_hash = [&](uint64_t at, uint32_t t, uint32_t l, uint64_t p) {
            CHECK(at < Hs, "case %zu: hash %llu of %llu", cases, (unsigned long long)at, (unsigned long long)Hs);
            if (at < cap_h) { out[at] = Cell{t, l, p}; ++writes[at]; }
        };
        for (uint32_t q = 0; q < k && fails == 0; ++q) {
            const bool has_prev = q > 0 && trees[q - 1] == trees[q], has_next = q + 1 < k && trees[q + 1] == trees[q];
            const uint32_t t = trees[q], b = block_of[q];
            const uint64_t c = counts[t], a = has_prev ? idx[q - 1] : 0, i = idx[q];
            const uint32_t h = vkmr_mb::height(c);
            const vkmr_mb::Group g = vkmr_mb::group(has_prev, a, i, h);
            const uint64_t bit0 = 8 * byte_start[b] + (flag_at[q] - bit_start[b]);
            auto set_flag = [&](uint64_t rel, int v) {
                const uint64_t at = bit0 + rel;
                CHECK(at < 8 * byte_start[b + 1], "case %zu: a flag of block %u outside its bytes", cases, b);
                if (at < bits.size()) { bits[at] = v; ++bit_writes[at]; }
            };
            for (uint32_t l = 0; l <= h; ++l) {
                if (has_prev && vkmr_mb::climbs(a, l, g.top)) {
                    set_flag(vkmr_mb::climb_place(a, l), 0);
                    put_hash(hash_at[q] + vkmr_mb::climb_place(a, l), t, l, (a >> l) + 1);
                }
                if (l <= g.top) set_flag(vkmr_mb::path_flag(g, i, l), 1);
                if (vkmr_mb::descends(g, i, l)) {
                    set_flag(vkmr_mb::left_flag(g, i, l), 0);
                    put_hash(hash_at[q] + vkmr_mb::left_hash(g, i, l), t, l, (i >> l) - 1);
                }
                if (l == 0) put_hash(hash_at[q] + vkmr_mb::leaf_hash(g), t, 0, i);
                if (!has_next && vkmr_mb::climbs(i, l, vkmr_mb::edge_level(i, c, h))) {
                    set_flag(g.flags + vkmr_mb::climb_place(i, l), 0);
                    put_hash(hash_at[q] + g.hashes + vkmr_mb::climb_place(i, l), t, l, (i >> l) + 1);
                }
            }
        }

        // against the recursion
        uint64_t flags_total = 0;
        for (size_t b = 0, q = 0; b < B && fails == 0; ++b) {
            Walk w;
            const uint32_t t = trees[q];
            w.c = counts[t];
            const uint32_t h = vkmr_mb::height(w.c);
            w.A.assign(h + 1, {});
            for (; q < k && trees[q] == t; ++q) w.A[0].insert(idx[q]);
            for (uint32_t l = 0; l < h; ++l)
                for (uint64_t p : w.A[l]) w.A[l + 1].insert(p >> 1);
            w.visit(h, 0);
            flags_total += w.flags.size();
            CHECK(w.flags.size() == bit_start[b + 1] - bit_start[b], "case %zu tree %u: %zu flags, the plan has %llu", cases, t, w.flags.size(),
                  (unsigned long long)(bit_start[b + 1] - bit_start[b]));
            CHECK(w.cells.size() == hash_start[b + 1] - hash_start[b], "case %zu tree %u: %zu hashes, the plan has %llu", cases, t, w.cells.size(),
                  (unsigned long long)(hash_start[b + 1] - hash_start[b]));
            if (fails) break;
            // flags <= 2 * hashes + h and flags <= k_t * h + hashes: what the byte bound rests on
            CHECK(w.flags.size() <= 2 * w.cells.size() + h && w.flags.size() <= w.A[0].size() * h + w.cells.size(), "case %zu tree %u: the flag bounds", cases, t);
            for (size_t f = 0; f < w.flags.size(); ++f) {
                const uint64_t at = 8 * byte_start[b] + f;
                CHECK(bit_writes[at] == 1 && bits[at] == w.flags[f], "case %zu tree %u flag %zu: written %d times as %d, the walk has %d", cases, t, f,
                      bit_writes[at], bits[at], w.flags[f]);
            }
            for (uint64_t at = 8 * byte_start[b] + w.flags.size(); at < 8 * byte_start[b + 1]; ++at)
                CHECK(bit_writes[at] == 0, "case %zu tree %u: a padding bit written", cases, t);
            for (size_t j = 0; j < w.cells.size(); ++j) {
                const uint64_t at = hash_start[b] + j;
                CHECK(writes[at] == 1 && out[at] == (Cell{t, w.cells[j].first, w.cells[j].second}),
                      "case %zu tree %u hash %zu: written %d times as (%u, %u, %llu), the walk has (%u, %llu)", cases, t, j, writes[at], out[at].t, out[at].l,
                      (unsigned long long)out[at].p, w.cells[j].first, (unsigned long long)w.cells[j].second);
                CHECK(w.cells[j].second < vkmr_forest::level_count(w.c, w.cells[j].first) && w.cells[j].first < h, "case %zu tree %u: a hash of no stored node",
                      cases, t);
            }
        }
        std::printf("%zu %llu %llu %llu\n", B, (unsigned long long)flags_total, (unsigned long long)Hs, (unsigned long long)byte_start[B]);
        ++cases;
        if (fails) break;
    }
    if (fails) return 1;
    std::printf("ok: %zu cases\n", cases);
    return 0;
}
