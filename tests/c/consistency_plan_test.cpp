// consistency_plan_test.cpp -- CPU replay of vkmr_hip_forest_consistency_async's gather and vkmr_hip_verify_consistency_async's
// walk with the rules the ABI, the kernels and the CPU twins share (csrc/consistency_plan.hpp, and frontier_plan.hpp's
// node_source / node_cell), with values.  A case is a forest (first offset, counts) and queries (tree, old count c).  The replay
// keeps the forest as the build stores it -- the leaves, one buffer per level with tree t's nodes from cell (o_t >> l) + t, a
// level of a single node in the roots alone -- under a 64-bit mix in place of SHA-256d, every cell nobody writes poisoned, and
// checks for every query what consistency_gather_kernel's lane (query, l) does:
//   - the source and the cell of every peak and every right neighbour lie inside the level they name: the node below the
//     level's count, the cell inside the level's buffer and inside the tree's own cells (no cell of another tree, no padding,
//     no poison), the roots only for a level of one node;
// and what consistency_fold_kernel's lane does with the gathered rows alone, step by step through step():
//   - it reads only cells the gather wrote, and every cell the gather wrote (the read set is the written set);
//   - the old root it forms is the root of the tree built from the first c leaves, the new root that of the tree as it is;
//   - it hashes at most H(c) + H(c2) times.
//
//   consistency_plan_test FILE   one case per line: `first stride ntrees c_0 .. nq t_0 c_0 t_1 c_1 ..`.  Prints, per line,
//                                `cells read, node hashes, status` (status != 0: refused, nothing replayed), then "ok: N cases".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <sstream>
#include <string>
#include <fstream>
#include <vector>

#include "consistency_plan.hpp"

namespace {

const uint64_t POISON = 0xDEADDEADDEADDEADull;
int failures = 0;
#define CHECK(cond, ...)                                             \
    do {                                                             \
        if (!(cond)) {                                               \
            if (failures++ < 20) { printf("FAIL %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } \
        }                                                            \
    } while (0)

uint64_t mix(uint64_t a, uint64_t b)
{
    uint64_t x = a * 0x9E3779B97F4A7C15ull + (b ^ 0xC2B2AE3D27D4EB4Full) * 0xFF51AFD7ED558CCDull + 0x165667B19E3779F9ull;
    x ^= x >> 29;
    x *= 0xBF58476D1CE4E5B9ull;
    return x ^ (x >> 32);
}

// The root of the tree built from leaves[0 .. c), c >= 1.
uint64_t built_root(const uint64_t* leaves, uint64_t c)
{
    std::vector<uint64_t> cur(leaves, leaves + c);
    do {
        const uint64_t n = cur.size();
        std::vector<uint64_t> up((n + 1) / 2);
        for (uint64_t j = 0; j < up.size(); ++j) up[j] = mix(cur[2 * j], cur[vkmr_math::right_child(j, n)]);
        cur.swap(up);
    } while (cur.size() > 1);
    return cur[0];
}

struct Forest {
    uint64_t total;
    uint32_t ntrees, H;
    std::vector<uint64_t> offsets, leaves, roots;
    std::vector<std::vector<uint64_t>> level;   // level[l], l >= 1: (total >> l) + ntrees cells

    Forest(uint64_t first, const std::vector<uint64_t>& counts) : ntrees((uint32_t)counts.size())
    {
        offsets.push_back(first);
        uint64_t most = 1;
        for (uint64_t c : counts) {
            offsets.push_back(offsets.back() + c);
            if (c > most) most = c;
        }
        total = offsets.back();
        H = vkmr_math::height(most);
        leaves.assign(total, POISON);
        roots.assign(ntrees, POISON);
        level.assign(H + 1, std::vector<uint64_t>());
        for (uint32_t l = 1; l <= H; ++l) level[l].assign((total >> l) + ntrees, POISON);
        for (uint32_t t = 0; t < ntrees; ++t) {
            const uint64_t o = offsets[t], c = counts[t];
            if (c == 0) {
                roots[t] = 0;
                continue;
            }
            for (uint64_t i = 0; i < c; ++i) leaves[o + i] = mix(o + i, 0x1234u + t);
            std::vector<uint64_t> cur(leaves.begin() + o, leaves.begin() + o + c);
            for (uint32_t l = 1; l <= vkmr_math::height(c); ++l) {
                const uint64_t n = cur.size();
                std::vector<uint64_t> up((n + 1) / 2);
                for (uint64_t j = 0; j < up.size(); ++j) up[j] = mix(cur[2 * j], cur[vkmr_math::right_child(j, n)]);
                if (up.size() == 1) {
                    CHECK(l == vkmr_math::height(c), "the last level of tree %u", t);
                    roots[t] = up[0];
                } else {
                    for (uint64_t j = 0; j < up.size(); ++j) {
                        const uint64_t cell = (o >> l) + t + j;
                        CHECK(cell < level[l].size() && level[l][cell] == POISON, "the build's cell %llu of level %u", (unsigned long long)cell, l);
                        level[l][cell] = up[j];
                    }
                }
                cur.swap(up);
            }
        }
    }

    // Node `node` of level l of tree t, read as consistency_gather_kernel reads it; every bound checked on the way.
    uint64_t read(uint32_t t, uint32_t l, uint64_t node, uint64_t c2)
    {
        const uint64_t o = offsets[t];
        CHECK(node < vkmr_frontier::level_count(c2, l), "node %llu of level %u of a tree of %llu", (unsigned long long)node, l, (unsigned long long)c2);
        const vkmr_frontier::GatherSource from = vkmr_frontier::node_source(c2, l);
        const uint64_t cell = vkmr_frontier::node_cell(o, t, l, node);
        if (from == vkmr_frontier::GATHER_LEAF) {
            CHECK(l == 0 && cell >= o && cell < offsets[t + 1], "leaf cell %llu of tree %u", (unsigned long long)cell, t);
            return cell < total ? leaves[cell] : POISON;
        }
        if (from == vkmr_frontier::GATHER_ROOT) {
            CHECK(l >= 1 && l == vkmr_math::height(c2) && node == 0, "the roots for level %u of a tree of %llu", l, (unsigned long long)c2);
            return roots[t];
        }
        CHECK(from == vkmr_frontier::GATHER_LEVEL && l >= 1 && l <= H && l < vkmr_math::height(c2), "level %u of a tree of %llu", l, (unsigned long long)c2);
        if (l > H) return POISON;
        const uint64_t lo = (o >> l) + t, next = t + 1 < ntrees ? (offsets[t + 1] >> l) + t + 1 : level[l].size();
        CHECK(cell >= lo && cell < lo + vkmr_frontier::level_count(c2, l) && cell < next && cell < level[l].size(), "cell %llu of level %u, tree %u",
              (unsigned long long)cell, l, t);
        return cell < level[l].size() ? level[l][cell] : POISON;
    }
};

void replay(const std::string& line)
{
    std::istringstream in(line);
    uint64_t first, n;
    uint32_t stride, ntrees, nq;
    in >> first >> stride >> ntrees;
    std::vector<uint64_t> counts;
    for (uint32_t t = 0; t < ntrees; ++t) {
        in >> n;
        counts.push_back(n);
    }
    in >> nq;
    std::vector<uint32_t> trees(nq);
    std::vector<uint64_t> old(nq);
    for (uint32_t q = 0; q < nq; ++q) in >> trees[q] >> old[q];
    if (!in) {
        CHECK(false, "a line that does not parse");
        return;
    }
    Forest f(first, counts);
    uint32_t status = 0;
    for (uint32_t q = 0; q < nq; ++q) status |= vkmr_consistency::refusal(trees[q], ntrees, f.offsets.data(), old[q], stride);
    uint64_t cells = 0, hashes = 0;
    for (uint32_t q = 0; q < nq && status == 0; ++q) {
        const uint32_t t = trees[q];
        const uint64_t c = old[q], c2 = counts[t];
        CHECK(vkmr_consistency::checkable(c, c2, stride), "a query the check let through");
        if (c == 0) continue;
        // the gather: what lane (q, l) writes; `wrote` bit l of row r
        std::vector<uint64_t> peaks(stride, 0), rights(stride, 0);
        uint64_t wrote[2] = {0, 0}, seen[2] = {0, 0};
        for (uint32_t l = 0; l < stride; ++l) {
            if (vkmr_consistency::has_peak(c, l)) {
                peaks[l] = f.read(t, l, vkmr_consistency::peak_node(c, l), c2);
                wrote[0] |= 1ull << l;
            }
            if (vkmr_consistency::has_right(c, c2, l)) {
                CHECK(vkmr_frontier::node_source(c2, l) != vkmr_frontier::GATHER_ROOT, "a right neighbour in the roots");
                rights[l] = f.read(t, l, vkmr_consistency::right_node(c, l), c2);
                wrote[1] |= 1ull << l;
            }
        }
        for (uint32_t l = 0; l < stride; ++l) CHECK(peaks[l] != POISON && rights[l] != POISON, "query %u cell %u is a cell nobody wrote", q, l);
        // the fold: consistency_fold_kernel's loop on the rows alone
        const uint32_t H1 = vkmr_consistency::height(c), steps = vkmr_consistency::steps(c, c2);
        uint64_t acc = 0, mine = 0;
        bool have = false;
        for (uint32_t i = 0;; ++i) {
            if (i == H1) {
                if (!have) {
                    CHECK(vkmr_consistency::low_level(c) == H1 && H1 < stride, "no hash below the old root of %llu", (unsigned long long)c);
                    acc = peaks[H1];
                    seen[0] |= 1ull << H1;
                }
                CHECK(acc == built_root(f.leaves.data() + f.offsets[t], c), "the old root of query %u (%llu of %llu)", q, (unsigned long long)c, (unsigned long long)c2);
                if (have) acc = peaks[vkmr_consistency::low_level(c)];
                seen[0] |= 1ull << vkmr_consistency::low_level(c);
                have = true;
            }
            if (i == steps) break;
            const vkmr_consistency::Step s = vkmr_consistency::step(c, c2, i, have);
            if (!s.hash) continue;
            CHECK(s.l < stride && !(s.peak && s.right), "step %u of query %u", i, q);
            if (s.peak) seen[0] |= 1ull << s.l;
            if (s.right) seen[1] |= 1ull << s.l;
            const uint64_t x = s.peak ? peaks[s.l] : s.right ? rights[s.l] : acc;
            const uint64_t a = s.peak ? x : acc;
            const uint64_t b = s.right ? x : (have ? acc : a);
            acc = mix(a, b);
            have = true;
            ++mine;
        }
        CHECK(acc == f.roots[t], "the new root of query %u (%llu of %llu)", q, (unsigned long long)c, (unsigned long long)c2);
        CHECK(seen[0] == wrote[0] && seen[1] == wrote[1], "query %u (%llu of %llu) reads %llx %llx, the gather wrote %llx %llx", q, (unsigned long long)c,
              (unsigned long long)c2, (unsigned long long)seen[0], (unsigned long long)seen[1], (unsigned long long)wrote[0], (unsigned long long)wrote[1]);
        CHECK(mine <= (uint64_t)H1 + vkmr_consistency::height(c2), "%llu hashes for %llu of %llu", (unsigned long long)mine, (unsigned long long)c, (unsigned long long)c2);
        hashes += mine;
        cells += (uint64_t)__builtin_popcountll(wrote[0]) + (uint64_t)__builtin_popcountll(wrote[1]);
    }
    printf("%llu %llu %u\n", (unsigned long long)cells, (unsigned long long)hashes, status);
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 2) {
        fprintf(stderr, "usage: consistency_plan_test FILE\n");
        return 2;
    }
    std::ifstream file(argv[1]);
    if (!file) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    std::string line;
    unsigned long n = 0;
    while (std::getline(file, line)) {
        if (line.empty()) continue;
        replay(line);
        ++n;
    }
    if (failures) {
        printf("FAIL: %d checks\n", failures);
        return 1;
    }
    printf("ok: %lu cases\n", n);
    return 0;
}
