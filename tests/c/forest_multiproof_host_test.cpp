// forest_multiproof_host_test.cpp -- stand-alone driver of vkmr_host_cpu_forest_multiproof and
// vkmr_host_cpu_verify_forest_multiproof (csrc/host/host_api.cpp), meant to be compiled TOGETHER with host_api.cpp and
// cpu_sha256d.cpp under -fsanitize=address,undefined (tests/test_forest_multiproof_abi.py does): every buffer below has
// exactly the size the contract names, so a read or write past one is a sanitizer report.
//
// Input file, one case per line:  stride ntrees c_0 .. c_{ntrees-1} k t_0 i_0 .. t_{k-1} i_{k-1}
// The leaves are a fixed pattern.  Per case: the gather with a node buffer of M - 1 cells (refused with bit 2, M and the
// counts valid), again with exactly M cells, the verifier on the result (accepts), on a changed leaf, on one node fewer and
// on a swapped pair of entries (rejects).  Output, one line per case:  M m_0 .. m_{stride-1}   then "ok: N cases".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "vkmr_host.h"

static int fail(size_t line, const char* what)
{
    printf("FAIL line %zu: %s\n", line, what);
    return 1;
}

int main(int argc, char** argv)
{
    if (argc != 2) return fail(0, "usage: forest_multiproof_host_test CASES");
    std::ifstream in(argv[1]);
    if (!in) return fail(0, "cannot open the case file");
    std::string text;
    size_t cases = 0;
    std::vector<std::string> answers;
    while (std::getline(in, text)) {
        ++cases;
        std::istringstream ls(text);
        uint32_t stride, ntrees, k;
        if (!(ls >> stride >> ntrees)) return fail(cases, "header");
        std::vector<uint64_t> offsets(ntrees + 1, 0);
        for (uint32_t t = 0; t < ntrees; ++t) {
            uint64_t c;
            if (!(ls >> c)) return fail(cases, "counts");
            offsets[t + 1] = offsets[t] + c;
        }
        if (!(ls >> k) || k == 0) return fail(cases, "k");
        std::vector<uint32_t> trees(k);
        std::vector<uint64_t> indices(k);
        for (uint32_t q = 0; q < k; ++q)
            if (!(ls >> trees[q] >> indices[q])) return fail(cases, "entries");
        const uint64_t total = offsets[ntrees];
        std::vector<vkmr_digest> leaves(total);
        uint32_t x = 2463534242u + (uint32_t)cases;
        for (uint64_t i = 0; i < total; ++i)
            for (int w = 0; w < 8; ++w) {
                x ^= x << 13; x ^= x >> 17; x ^= x << 5;
                leaves[i].data[w] = x;
            }
        std::vector<vkmr_digest> roots(ntrees);
        if (vkmr_host_cpu_forest_roots(leaves.data(), offsets.data(), ntrees, roots.data()) != 0) return fail(cases, "roots");

        std::vector<uint32_t> heights(k);
        std::vector<uint64_t> info(2 + stride);
        // no room at all: bit 2 (or M == 0), M and the counts valid
        int rc = vkmr_host_cpu_forest_multiproof(leaves.data(), offsets.data(), ntrees, trees.data(), indices.data(), k, stride, nullptr, 0,
                                                 heights.data(), info.data());
        const uint64_t M = info[1];
        if (rc != (M > 0 ? 4 : 0)) return fail(cases, "a node buffer of no cell");
        if (M > 0) {
            std::vector<vkmr_digest> tight(M - 1);
            rc = vkmr_host_cpu_forest_multiproof(leaves.data(), offsets.data(), ntrees, trees.data(), indices.data(), k, stride, tight.data(), M - 1,
                                                 heights.data(), info.data());
            if (rc != 4 || info[0] != 4 || info[1] != M) return fail(cases, "a node buffer of M - 1 cells");
        }
        std::vector<vkmr_digest> nodes(M);
        rc = vkmr_host_cpu_forest_multiproof(leaves.data(), offsets.data(), ntrees, trees.data(), indices.data(), k, stride, nodes.data(), M,
                                             heights.data(), info.data());
        if (rc != 0 || info[0] != 0 || info[1] != M) return fail(cases, "a node buffer of M cells");
        uint64_t sum = 0;
        for (uint32_t l = 0; l < stride; ++l) sum += info[2 + l];
        if (sum != M) return fail(cases, "the level counts do not add up to M");

        std::vector<vkmr_digest> proved(k);
        for (uint32_t q = 0; q < k; ++q) proved[q] = leaves[offsets[trees[q]] + indices[q]];
        auto verdict = [&](const std::vector<vkmr_digest>& lv, const std::vector<uint32_t>& tr, const std::vector<uint64_t>& ix, uint64_t m) {
            return vkmr_host_cpu_verify_forest_multiproof(lv.data(), tr.data(), ix.data(), heights.data(), k, stride, m ? nodes.data() : nullptr, m,
                                                          roots.data(), ntrees);
        };
        if (verdict(proved, trees, indices, M) != 1) return fail(cases, "the proof is not accepted");
        std::vector<vkmr_digest> changed(proved);
        changed[k / 2].data[3] ^= 0x10u;
        if (verdict(changed, trees, indices, M) != 0) return fail(cases, "a changed leaf is accepted");
        if (M > 0 && verdict(proved, trees, indices, M - 1) != 0) return fail(cases, "a proof of one node fewer is accepted");
        if (k >= 2) {
            std::vector<uint32_t> st(trees);
            std::vector<uint64_t> si(indices);
            std::swap(st[0], st[1]);
            std::swap(si[0], si[1]);
            if (verdict(proved, st, si, M) != 0) return fail(cases, "swapped entries are accepted");
        }
        // a bad entry: only the status is written
        std::vector<uint64_t> bad(indices);
        bad[k - 1] = offsets[trees[k - 1] + 1] - offsets[trees[k - 1]];
        std::vector<uint64_t> info2(2 + stride, 0x5a5a5a5a5a5a5a5aull);
        rc = vkmr_host_cpu_forest_multiproof(leaves.data(), offsets.data(), ntrees, trees.data(), bad.data(), k, stride, nodes.data(), M, heights.data(),
                                             info2.data());
        if (rc != 1 || info2[0] != 1 || info2[1] != 0x5a5a5a5a5a5a5a5aull) return fail(cases, "an index equal to its tree's count");

        std::ostringstream os;
        os << M;
        for (uint32_t l = 0; l < stride; ++l) os << ' ' << info[2 + l];
        answers.push_back(os.str());
    }
    for (const std::string& a : answers) printf("%s\n", a.c_str());
    printf("ok: %zu cases\n", cases);
    return 0;
}
