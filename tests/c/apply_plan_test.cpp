// apply_plan_test.cpp -- CPU-side replay of the scratch layout of the apply calls (vkmr_hip_apply_multiproof_async and its
// forest twin) as csrc/tree_plan.hpp lays it out.  Every expectation is worked out here on its own, not through the header
// under test.  Built and run by tests/test_apply_abi.py (no GPU).
//
//   apply_plan_test    per (k, levels): `k levels bytes` after the checks; the test compares bytes with the library's
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "tree_plan.hpp"

#define CHECK(cond, ...)                    \
    do {                                    \
        if (!(cond)) {                      \
            printf("FAIL: " __VA_ARGS__);   \
            printf("\n");                   \
            exit(1);                        \
        }                                   \
    } while (0)

typedef unsigned long long ull;

int main()
{
    const uint32_t ks[] = {1, 63, 64, 65, 16384, 16385};
    const uint32_t levels[] = {1, 2, 11, 26, 58, 63};
    int n = 0;
    for (uint32_t k : ks)
        for (uint32_t h : levels) {
            const vkmr_tree::ApplyLayout A = vkmr_tree::apply_layout(k, h);
            const vkmr_tree::MultiproofLayout L = vkmr_tree::multiproof_layout(k, h);
            // the verifier's layout whole, at the front: side 0 is the verifier's fold to the letter
            CHECK(A.mp.cell == L.cell && A.mp.mask == L.mask && A.mp.word_start == L.word_start && A.mp.block == L.block && A.mp.hdr == L.hdr &&
                      A.mp.end == L.end && A.mp.bytes == L.bytes && A.mp.words == L.words && A.mp.blocks == L.blocks,
                  "the verifier's layout is not kept (k=%u levels=%u)", k, h);
            const uint64_t words = ((uint64_t)k + 63) / 64, blocks = (words + 255) / 256;
            const size_t verifier = (size_t)k * 32 + (size_t)(words * h) * 16 + (size_t)(blocks * h) * 8 + (size_t)(2 + 64) * 8 + (size_t)k * 4;
            CHECK(L.bytes == verifier, "the verifier's scratch is %llu bytes, not %llu (k=%u levels=%u)", (ull)L.bytes, (ull)verifier, k, h);
            // behind it: k cells, k end words, k heights, each starting on 16 bytes at the first such place behind the part before
            const size_t start[] = {A.cell1, A.end1, A.heights, A.bytes};
            const size_t size[] = {(size_t)k * 32, (size_t)k * 4, (size_t)k * 4};
            size_t at = verifier;
            for (int p = 0; p < 3; ++p) {
                const size_t want = (at + 15) / 16 * 16;
                CHECK(start[p] == want, "part %d starts at %llu, not %llu (k=%u levels=%u)", p, (ull)start[p], (ull)want, k, h);
                CHECK(start[p] % 16 == 0, "part %d off the 16-byte grid", p);
                at = start[p] + size[p];
            }
            CHECK(A.bytes == (at + 15) / 16 * 16 && A.bytes >= at, "the total does not hold the last part (k=%u levels=%u)", k, h);
            printf("%u %u %llu\n", k, h, (ull)A.bytes);
            ++n;
        }
    printf("ok: %d layouts\n", n);
    return 0;
}
