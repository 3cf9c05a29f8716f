// audit_plan_test.cpp -- csrc/audit_plan.hpp replayed on the CPU: the scratch layout of an audit and every launch's writes into
// it, for the shapes a file names.  Stand-alone (g++ -I vk_merkle_roots_amd/csrc), no HIP; tests/test_audit_abi.py builds and
// runs it and compares the printed numbers with its own arithmetic.
//
// Input: one shape per line, "F total ntrees max_count capacity" (a forest) or "T count height capacity" (one tree).
// Output: one line per shape, "bytes words_used words_bound launches", then "ok: N shapes"; "FAIL ..." and exit 1 on the first
// part out of order, off the 16-byte grid or written past its end.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "audit_plan.hpp"

static int fail(const char* what, long line)
{
    printf("FAIL line %ld: %s\n", line, what);
    return 1;
}

struct Span { size_t lo, hi; };   // bytes [lo, hi) of the scratch

int main(int argc, char** argv)
{
    if (argc != 2) return fail("usage: audit_plan_test FILE", 0);
    FILE* f = fopen(argv[1], "r");
    if (!f) return fail("cannot open the input", 0);
    char kind;
    long shapes = 0;
    while (fscanf(f, " %c", &kind) == 1) {
        ++shapes;
        unsigned long long total, a, b = 0, cap;
        if (kind == 'F') {
            if (fscanf(f, "%llu %llu %llu %llu", &total, &a, &b, &cap) != 4) return fail("bad forest line", shapes);
        } else if (kind == 'T') {
            if (fscanf(f, "%llu %llu %llu", &total, &a, &cap) != 3) return fail("bad tree line", shapes);
        } else {
            return fail("unknown kind", shapes);
        }
        const bool forest = kind == 'F';
        const uint32_t ntrees = forest ? (uint32_t)a : 1u, capacity = (uint32_t)cap;
        const uint32_t levels = forest ? vkmr_forest::launches(total, b) : (uint32_t)a;
        if (levels > VKMR_AUDIT_MAX_LEVELS) return fail("more levels than the scratch is sized for", shapes);
        const vkmr_audit::Layout L = vkmr_audit::layout(total, ntrees, capacity);
        // the parts: in order, on the 16-byte grid, ending at the reported size
        const size_t starts[5] = {L.mask, L.word_start, L.block, L.hdr, L.bytes};
        if (starts[0] != 0) return fail("the first part does not start the scratch", shapes);
        for (int i = 0; i < 5; ++i)
            if (starts[i] % 16u || (i && starts[i] < starts[i - 1])) return fail("parts out of order or off the 16-byte grid", shapes);
        if (L.bytes != vkmr_audit::scratch_bytes(total, ntrees, capacity)) return fail("scratch_bytes is not the layout's end", shapes);
        if (capacity == 0 && L.bytes != 0) return fail("capacity 0 needs no scratch", shapes);
        // monotone in the shape, constant in a capacity above 0
        if (vkmr_audit::scratch_bytes(total + 1, ntrees, capacity) < L.bytes || vkmr_audit::scratch_bytes(total, ntrees + 1u, capacity) < L.bytes ||
            vkmr_audit::scratch_bytes(total, ntrees, capacity + 1u) < L.bytes)
            return fail("scratch_bytes is not monotone", shapes);
        uint64_t used = 0;
        unsigned launches = 0;
        if (capacity > 0) {
            // the level launches: level l's wavefronts write words [base(l), base(l) + words_of(cells_l)) of the mask part
            std::vector<Span> written;
            for (uint32_t l = 1; l <= levels; ++l) {
                const uint64_t cells = forest ? vkmr_audit::forest_level_cells(total, ntrees, l) : vkmr_audit::tree_level_cells(total, l);
                const uint64_t base = forest ? vkmr_audit::forest_word_base(total, ntrees, l) : vkmr_audit::tree_word_base(total, l);
                if (base != used) return fail("a level's ballot words do not follow those of the level below", shapes);
                // the last wavefront of the grid that passes p0 < cells writes word (cells - 1) / 64
                const uint64_t last = cells ? (cells - 1) / 64 : 0, words = vkmr_audit::words_of(cells);
                if (cells && last + 1 != words) return fail("a wavefront has no ballot word", shapes);
                written.push_back({L.mask + (size_t)base * 8u, L.mask + (size_t)(base + words) * 8u});
                used += words;
                ++launches;
            }
            const uint64_t end = forest ? vkmr_audit::forest_word_base(total, ntrees, levels + 1u) : vkmr_audit::tree_word_base(total, levels + 1u);
            if (end != used || used > L.words) return fail("the call uses more ballot words than the scratch holds", shapes);
            for (const Span& s : written)
                if (s.hi > L.word_start) return fail("a level launch writes past the mask part", shapes);
            // the ranking: block sums and starts over rank_blocks(used) blocks, word starts over `used` words, the header
            const uint64_t blocks = vkmr_audit::rank_blocks(used);
            if (blocks > L.blocks) return fail("more ranking blocks than the scratch holds", shapes);
            if (L.word_start + (size_t)used * 8u > L.block) return fail("the word starts run into the blocks", shapes);
            if (L.block + (size_t)blocks * 8u > L.hdr) return fail("the blocks run into the header", shapes);
            if (L.hdr + (size_t)VKMR_AUDIT_HEADER_WORDS * 8u > L.bytes) return fail("the header runs past the scratch", shapes);
            if (2u + 1u > VKMR_AUDIT_HEADER_WORDS) return fail("the ranking's header of one level does not fit", shapes);
            launches += 3u + levels;   // the ranking, one emit per level
        } else {
            launches = levels;
        }
        // the nodes a tree holds, two ways
        if (!forest && vkmr_audit::tree_nodes(total, levels) != vkmr_tree::cells(total, levels)) return fail("tree_nodes", shapes);
        printf("%zu %llu %llu %u\n", L.bytes, (unsigned long long)used, (unsigned long long)L.words, launches);
    }
    fclose(f);
    // the nodes of one forest tree against a plain loop, every count up to 5000
    for (uint64_t c = 0; c <= 5000; ++c) {
        uint64_t n = c == 0 ? 1 : 0, m = c;
        while (c) {
            m = (m + 1) / 2;
            n += m;
            if (m == 1) break;
        }
        if (vkmr_audit::forest_tree_nodes(c) != n) return fail("forest_tree_nodes", (long)c);
    }
    printf("ok: %ld shapes\n", shapes);
    return 0;
}
