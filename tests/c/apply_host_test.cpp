// apply_host_test.cpp -- stand-alone driver of vkmr_host_cpu_apply_forest_multiproof and vkmr_host_cpu_apply_multiproof
// (csrc/host/host_api.cpp), meant to be compiled TOGETHER with host_api.cpp and cpu_sha256d.cpp under
// -fsanitize=address,undefined (tests/test_apply_abi.py does): every buffer below has exactly the size the contract names,
// so a read or write past one is a sanitizer report.
//
// Input file, one case per line:  stride ntrees c_0 .. c_{ntrees-1} k t_0 i_0 .. t_{k-1} i_{k-1}
// The old and the new leaves are fixed patterns.  Per case: the forest's multiproof gathered, the witness applied (accepted;
// the named trees' new roots equal those of the forest rebuilt over the updated leaves, the cells of the others keep their
// pattern), applied in place, applied with a changed old leaf, one node fewer and a count of 0 (refused, nothing written),
// and the first trees of the case applied one by one through the single tree's call.
// Output, one line per case:  M named   then "ok: N cases".
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

static bool same(const vkmr_digest& a, const vkmr_digest& b) { return memcmp(a.data, b.data, 32) == 0; }

int main(int argc, char** argv)
{
    if (argc != 2) return fail(0, "usage: apply_host_test CASES");
    std::ifstream in(argv[1]);
    if (!in) return fail(0, "cannot open the case file");
    std::string text;
    size_t cases = 0;
    std::vector<std::string> answers;
    vkmr_digest canary;
    memset(canary.data, 0xC3, 32);
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
        std::vector<uint64_t> indices(k), counts(k);
        for (uint32_t q = 0; q < k; ++q) {
            if (!(ls >> trees[q] >> indices[q])) return fail(cases, "entries");
            counts[q] = offsets[trees[q] + 1] - offsets[trees[q]];
        }
        const uint64_t total = offsets[ntrees];
        std::vector<vkmr_digest> leaves(total), fresh(k);
        uint32_t x = 2463534242u + (uint32_t)cases;
        auto next = [&]() { x ^= x << 13; x ^= x >> 17; x ^= x << 5; return x; };
        for (uint64_t i = 0; i < total; ++i)
            for (int w = 0; w < 8; ++w) leaves[i].data[w] = next();
        for (uint32_t q = 0; q < k; ++q)
            for (int w = 0; w < 8; ++w) fresh[q].data[w] = next();
        std::vector<vkmr_digest> roots(ntrees);
        if (vkmr_host_cpu_forest_roots(leaves.data(), offsets.data(), ntrees, roots.data()) != 0) return fail(cases, "roots");

        std::vector<uint32_t> heights(k);
        std::vector<uint64_t> info(2 + stride);
        int rc = vkmr_host_cpu_forest_multiproof(leaves.data(), offsets.data(), ntrees, trees.data(), indices.data(), k, stride, nullptr, 0, heights.data(),
                                                 info.data());
        const uint64_t M = info[1];
        if (rc != (M > 0 ? 4 : 0)) return fail(cases, "the node count");
        std::vector<vkmr_digest> nodes(M);
        rc = vkmr_host_cpu_forest_multiproof(leaves.data(), offsets.data(), ntrees, trees.data(), indices.data(), k, stride, nodes.data(), M,
                                             heights.data(), info.data());
        if (rc != 0) return fail(cases, "the gather");

        std::vector<vkmr_digest> proved(k), after(leaves);
        for (uint32_t q = 0; q < k; ++q) {
            proved[q] = leaves[offsets[trees[q]] + indices[q]];
            after[offsets[trees[q]] + indices[q]] = fresh[q];
        }
        std::vector<vkmr_digest> want(ntrees);
        if (vkmr_host_cpu_forest_roots(after.data(), offsets.data(), ntrees, want.data()) != 0) return fail(cases, "roots of the updated forest");
        std::vector<bool> named(ntrees, false);
        for (uint32_t q = 0; q < k; ++q) named[trees[q]] = true;

        auto apply = [&](const std::vector<vkmr_digest>& old, const std::vector<uint64_t>& cs, uint64_t m, std::vector<vkmr_digest>& out) {
            return vkmr_host_cpu_apply_forest_multiproof(old.data(), fresh.data(), trees.data(), indices.data(), cs.data(), k, stride,
                                                         m ? nodes.data() : nullptr, m, roots.data(), ntrees, out.data());
        };
        std::vector<vkmr_digest> out(ntrees, canary);
        if (apply(proved, counts, M, out) != 1) return fail(cases, "the witness is not accepted");
        uint32_t n_named = 0;
        for (uint32_t t = 0; t < ntrees; ++t) {
            if (named[t] ? !same(out[t], want[t]) : !same(out[t], canary)) return fail(cases, named[t] ? "a new root differs from the rebuild's" : "an unnamed cell was written");
            n_named += named[t] ? 1 : 0;
        }
        // in place: the roots themselves advance
        std::vector<vkmr_digest> inplace(roots);
        if (vkmr_host_cpu_apply_forest_multiproof(proved.data(), fresh.data(), trees.data(), indices.data(), counts.data(), k, stride,
                                                  M ? nodes.data() : nullptr, M, inplace.data(), ntrees, inplace.data()) != 1)
            return fail(cases, "in place: not accepted");
        for (uint32_t t = 0; t < ntrees; ++t)
            if (!same(inplace[t], named[t] ? want[t] : roots[t])) return fail(cases, "in place: other roots than out of place");
        // refusals write nothing
        auto untouched = [&](const std::vector<vkmr_digest>& o) {
            for (const vkmr_digest& d : o)
                if (!same(d, canary)) return false;
            return true;
        };
        std::vector<vkmr_digest> changed(proved), clean(ntrees, canary);
        changed[k / 2].data[3] ^= 0x10u;
        if (apply(changed, counts, M, clean) != 0 || !untouched(clean)) return fail(cases, "a changed old leaf");
        if (M > 0 && (apply(proved, counts, M - 1, clean) != 0 || !untouched(clean))) return fail(cases, "one node fewer");
        std::vector<uint64_t> none(counts);
        none[k - 1] = 0;
        if (apply(proved, none, M, clean) != 0 || !untouched(clean)) return fail(cases, "a count of 0");

        // the first trees one by one: a forest of one tree gathers the single tree's multiproof
        uint32_t done = 0;
        for (uint32_t a = 0; a < k && done < 20; ++done) {
            uint32_t b = a + 1;
            while (b < k && trees[b] == trees[a]) ++b;
            const uint32_t t = trees[a], n = b - a, h = heights[a];
            const uint64_t one[2] = {0, counts[a]};
            std::vector<uint32_t> zero(n, 0), hs(n);
            std::vector<uint64_t> inf(2 + h);
            rc = vkmr_host_cpu_forest_multiproof(leaves.data() + offsets[t], one, 1, zero.data(), indices.data() + a, n, h, nullptr, 0, hs.data(), inf.data());
            const uint64_t m = inf[1];
            std::vector<vkmr_digest> mine(m);
            rc = vkmr_host_cpu_forest_multiproof(leaves.data() + offsets[t], one, 1, zero.data(), indices.data() + a, n, h, mine.data(), m, hs.data(),
                                                 inf.data());
            if (rc != 0) return fail(cases, "one tree's gather");
            vkmr_digest root = canary;
            if (vkmr_host_cpu_apply_multiproof(proved.data() + a, fresh.data() + a, indices.data() + a, n, counts[a], h, m ? mine.data() : nullptr, m,
                                               &roots[t], &root) != 1 || !same(root, want[t]))
                return fail(cases, "one tree's apply");
            root = canary;
            if (vkmr_host_cpu_apply_multiproof(changed.data() + a, fresh.data() + a, indices.data() + a, n, counts[a], h, m ? mine.data() : nullptr, m,
                                               &want[t], &root) != 0 || !same(root, canary))
                return fail(cases, "one tree's apply against the wrong root");
            a = b;
        }

        std::ostringstream os;
        os << M << ' ' << n_named;
        answers.push_back(os.str());
    }
    for (const std::string& a : answers) printf("%s\n", a.c_str());
    printf("ok: %zu cases\n", cases);
    return 0;
}
