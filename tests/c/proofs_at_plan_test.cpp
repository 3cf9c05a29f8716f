// proofs_at_plan_test.cpp -- CPU replay of vkmr_hip_forest_proofs_at_async's edge launch and gather with the rules the ABI, the
// kernels and the CPU twin share (csrc/proofs_at_plan.hpp, and frontier_plan.hpp's node_source / node_cell), with values.  A case
// is a forest (first offset, counts) and epochs (tree, old count c).  The replay keeps the forest as the build stores it -- the
// leaves, one buffer per level with tree t's nodes from cell (o_t >> l) + t, a level of a single node in the roots alone --
// under a 64-bit mix in place of SHA-256d, every cell nobody writes poisoned, and checks for every epoch what
// proofs_at_edge_kernel's lane does, level by level through edge_step():
//   - the source and the cell of every peak it loads lie inside the level they name (the node below the level's count, the cell
//     inside the tree's own cells: no cell of another tree, no padding, no poison), the roots only for a level of one node;
//   - the cells of the edge row that take a carry are exactly the levels has_edge() names, every other cell takes a zero, no
//     store goes behind the row, and the old root is stored exactly once;
//   - the old root is the root of the tree built from the first c leaves, and the hashes are hashes(c) <= H(c);
// and, for EVERY leaf i < c, what proofs_at_gather_kernel's lanes (query, l) do:
//   - a cell from the stored forest passes the same bounds; a cell from the edge row is one the edge lane wrote a carry to;
//   - cell l is the sibling the tree built from the first c leaves has for leaf i at level l, and the height is its height.
//
//   proofs_at_plan_test FILE   one case per line: `first stride ntrees c_0 .. nE t_0 c_0 t_1 c_1 ..`.  Prints, per line,
//                              `edge cells, node hashes, proofs, status` (status != 0: refused, nothing replayed), then "ok: N cases".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "proofs_at_plan.hpp"

namespace {

const uint64_t POISON = 0xDEADDEADDEADDEADull;
int failures = 0;
#define CHECK(cond, ...)                                             \
    do {                                                             \
        if (!(cond)) {                                               \
            if (failures++ < 20) { printf("FAIL %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } \
        }                                                            \
    } while (0)
typedef unsigned long long ull;

uint64_t mix(uint64_t a, uint64_t b)
{
    uint64_t x = a * 0x9E3779B97F4A7C15ull + (b ^ 0xC2B2AE3D27D4EB4Full) * 0xFF51AFD7ED558CCDull + 0x165667B19E3779F9ull;
    x ^= x >> 29;
    x *= 0xBF58476D1CE4E5B9ull;
    return x ^ (x >> 32);
}

// Levels 0 .. H(c) of the tree built from leaves[0 .. c), c >= 1.
std::vector<std::vector<uint64_t>> built_levels(const uint64_t* leaves, uint64_t c)
{
    std::vector<std::vector<uint64_t>> levels(1, std::vector<uint64_t>(leaves, leaves + c));
    do {
        const std::vector<uint64_t>& cur = levels.back();
        const uint64_t n = cur.size();
        std::vector<uint64_t> up((n + 1) / 2);
        for (uint64_t j = 0; j < up.size(); ++j) up[j] = mix(cur[2 * j], cur[vkmr_math::right_child(j, n)]);
        levels.push_back(std::move(up));
    } while (levels.back().size() > 1);
    return levels;
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
            for (uint64_t i = 0; i < c; ++i) leaves[o + i] = mix(o + i, 0x4321u + t);
            const std::vector<std::vector<uint64_t>> built = built_levels(leaves.data() + o, c);
            CHECK(built.size() == vkmr_math::height(c) + 1u, "the levels of tree %u", t);
            for (uint32_t l = 1; l < built.size(); ++l) {
                if (built[l].size() == 1) {
                    roots[t] = built[l][0];
                    continue;
                }
                for (uint64_t j = 0; j < built[l].size(); ++j) {
                    const uint64_t cell = (o >> l) + t + j;
                    CHECK(cell < level[l].size() && level[l][cell] == POISON, "the build's cell %llu of level %u", (ull)cell, l);
                    level[l][cell] = built[l][j];
                }
            }
        }
    }

    // Node `node` of level l of tree t, read as proofs_at_node names it; every bound checked on the way.
    uint64_t read(uint32_t t, uint32_t l, uint64_t node, uint64_t c2)
    {
        const uint64_t o = offsets[t];
        CHECK(node < vkmr_frontier::level_count(c2, l), "node %llu of level %u of a tree of %llu", (ull)node, l, (ull)c2);
        const vkmr_frontier::GatherSource from = vkmr_frontier::node_source(c2, l);
        const uint64_t cell = vkmr_frontier::node_cell(o, t, l, node);
        if (from == vkmr_frontier::GATHER_LEAF) {
            CHECK(l == 0 && cell >= o && cell < offsets[t + 1], "leaf cell %llu of tree %u", (ull)cell, t);
            return cell < total ? leaves[cell] : POISON;
        }
        if (from == vkmr_frontier::GATHER_ROOT) {
            CHECK(l >= 1 && l == vkmr_math::height(c2) && node == 0, "the roots for level %u of a tree of %llu", l, (ull)c2);
            return roots[t];
        }
        CHECK(from == vkmr_frontier::GATHER_LEVEL && l >= 1 && l <= H && l < vkmr_math::height(c2), "level %u of a tree of %llu", l, (ull)c2);
        if (l > H) return POISON;
        const uint64_t lo = (o >> l) + t, next = t + 1 < ntrees ? (offsets[t + 1] >> l) + t + 1 : level[l].size();
        CHECK(cell >= lo && cell < lo + vkmr_frontier::level_count(c2, l) && cell < next && cell < level[l].size(), "cell %llu of level %u, tree %u", (ull)cell,
              l, t);
        return cell < level[l].size() ? level[l][cell] : POISON;
    }
};

void replay(const std::string& line)
{
    std::istringstream in(line);
    uint64_t first, n;
    uint32_t stride, ntrees, nE;
    in >> first >> stride >> ntrees;
    std::vector<uint64_t> counts;
    for (uint32_t t = 0; t < ntrees; ++t) {
        in >> n;
        counts.push_back(n);
    }
    in >> nE;
    std::vector<uint32_t> trees(nE);
    std::vector<uint64_t> old(nE);
    for (uint32_t e = 0; e < nE; ++e) in >> trees[e] >> old[e];
    if (!in || stride == 0 || stride > 63) {
        CHECK(false, "a line that does not parse");
        return;
    }
    Forest f(first, counts);
    uint32_t status = 0;
    for (uint32_t e = 0; e < nE; ++e) status |= vkmr_proofs_at::refusal(trees[e], ntrees, f.offsets.data(), old[e], stride);
    uint64_t cells = 0, hashes = 0, proofs = 0;
    for (uint32_t e = 0; e < nE && status == 0; ++e) {
        const uint32_t t = trees[e];
        const uint64_t c = old[e], c2 = counts[t];
        CHECK(c <= c2 && vkmr_proofs_at::bit_length(c2) <= stride, "an epoch the check let through");
        // the edge lane: proofs_at_edge_kernel's loop.  row[l] starts as poison: every cell must be written
        std::vector<uint64_t> row(stride, POISON);
        uint64_t root = POISON, carry = 0, wrote = 0, mine = 0;
        uint32_t root_stores = 0;
        bool have = false;
        row[0] = 0;
        if (vkmr_proofs_at::levels(c) != 0 && vkmr_proofs_at::levels(c) < stride) row[vkmr_proofs_at::levels(c)] = 0;   // the row has no cell for the root
        if (c == 0) {
            root = 0;
            ++root_stores;
        }
        for (uint32_t l = 0; l < stride; ++l) {
            const vkmr_proofs_at::EdgeStep s = vkmr_proofs_at::edge_step(c, l, have);
            CHECK(!(s.stored && s.hash) && (!s.stored || s.to_root) && (!s.to_root || l + 1u == vkmr_proofs_at::levels(c)), "step %u of %llu", l, (ull)c);
            if (!s.hash) {
                uint64_t x = 0;
                if (s.stored) {
                    CHECK(vkmr_proofs_at::root_is_stored(c) && c == (1ull << (l + 1u)), "a stored root for %llu", (ull)c);
                    x = f.read(t, l + 1u, 0, c2);
                }
                if (s.to_root) {                  // the kernel takes this root behind its loop
                    root = x;
                    ++root_stores;
                } else if (l + 1u < stride) {
                    CHECK(row[l + 1u] == POISON, "cell %u written twice", l + 1u);
                    row[l + 1u] = 0;
                }
                continue;
            }
            CHECK(l < vkmr_proofs_at::height(c) && l >= vkmr_proofs_at::low_level(c) && s.twice == (l == vkmr_proofs_at::low_level(c)) &&
                      s.peak == vkmr_proofs_at::has_peak(c, l), "the operands of level %u of %llu", l, (ull)c);
            CHECK(!s.peak || vkmr_frontier::node_source(c2, l) != vkmr_frontier::GATHER_ROOT, "a peak below H(c) in the roots: level %u of %llu", l, (ull)c);
            const uint64_t a = s.peak ? f.read(t, l, vkmr_proofs_at::peak_node(c, l), c2) : carry;
            const uint64_t b = s.twice ? a : carry;
            carry = mix(a, b);
            have = true;
            ++mine;
            if (s.to_root) {
                root = carry;
                ++root_stores;
            } else {
                CHECK(l + 1u < stride && row[l + 1u] == POISON, "a carry behind the row, or cell %u written twice", l + 1u);
                if (l + 1u < stride) row[l + 1u] = carry;
                wrote |= 1ull << (l + 1u);
            }
        }
        uint64_t named = 0;
        for (uint32_t l = 0; l < 64u; ++l)
            if (vkmr_proofs_at::has_edge(c, l)) named |= 1ull << l;
        CHECK(wrote == named, "epoch %u (%llu of %llu): carries in %llx, the plan names %llx", e, (ull)c, (ull)c2, (ull)wrote, (ull)named);
        for (uint32_t l = 0; l < stride; ++l) {
            CHECK(row[l] != POISON, "epoch %u cell %u is a cell nobody wrote", e, l);
            CHECK(((wrote >> l) & 1ull) || row[l] == 0, "epoch %u cell %u is neither a carry nor zero", e, l);
        }
        CHECK(root_stores == 1, "%u stores to the old root of epoch %u", root_stores, e);
        CHECK(mine == vkmr_proofs_at::hashes(c) && mine <= vkmr_proofs_at::levels(c), "%llu hashes for %llu", (ull)mine, (ull)c);
        hashes += mine;
        cells += (uint64_t)__builtin_popcountll(wrote);
        if (c == 0) {
            CHECK(root == 0, "the root of a tree not yet begun");
            continue;
        }
        const std::vector<std::vector<uint64_t>> was = built_levels(f.leaves.data() + f.offsets[t], c);
        const uint32_t H1 = vkmr_proofs_at::height(c);
        CHECK(was.size() == H1 + 1u && root == was[H1][0], "the old root of epoch %u (%llu of %llu)", e, (ull)c, (ull)c2);
        // the gather: every leaf of the old tree
        for (uint64_t i = 0; i < c; ++i) {
            for (uint32_t l = 0; l < stride; ++l) {
                const vkmr_proofs_at::CellSource from = vkmr_proofs_at::cell_source(c, l, i);
                if (l >= H1) {
                    CHECK(from == vkmr_proofs_at::CELL_ZERO, "a cell above the height");
                    continue;
                }
                const uint64_t s = vkmr_proofs_at::sibling(c, l, i);
                CHECK(s < was[l].size() && s == vkmr_math::sibling(i >> l, was[l].size()), "the sibling of leaf %llu at level %u", (ull)i, l);
                uint64_t x = POISON;
                if (from == vkmr_proofs_at::CELL_STORED) {
                    CHECK(vkmr_proofs_at::complete(c, l, s) && vkmr_frontier::node_source(c2, l) != vkmr_frontier::GATHER_ROOT, "a stored cell");
                    x = f.read(t, l, s, c2);
                } else {
                    CHECK(from == vkmr_proofs_at::CELL_EDGE && ((wrote >> l) & 1ull) && s + 1u == was[l].size(), "an edge cell at level %u of %llu", l, (ull)c);
                    x = row[l];
                }
                CHECK(s < was[l].size() && x == was[l][s], "cell %u of leaf %llu as of %llu of %llu", l, (ull)i, (ull)c, (ull)c2);
            }
            ++proofs;
        }
        CHECK(vkmr_proofs_at::cell_source(c, 0, c) == vkmr_proofs_at::CELL_ZERO, "an index at the count");
    }
    printf("%llu %llu %llu %u\n", (ull)cells, (ull)hashes, (ull)proofs, status);
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 2) {
        fprintf(stderr, "usage: proofs_at_plan_test FILE\n");
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
