// merkle_math.hpp -- the integer rules of a duplicate-last Merkle tree, each stated once, no HIP types: read by the kernels, the
// C ABI, the CPU backend (host/) and, through reduce_plan.hpp (vkmr_plan::) and forest_plan.hpp (vkmr_forest::), the tests/c sweeps.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define VKMR_MATH_FN __host__ __device__ __forceinline__
#else
#define VKMR_MATH_FN inline
#endif

namespace vkmr_math {
// Nodes of level l of a tree over n leaves: ceil(n / 2^l), and 0 for n == 0.  l <= 63 and n <= 2^63, so that the sum does
// not wrap (a count is a number of 32-byte cells in memory).  The spelling the bulk reduction's instructions were tuned with.
VKMR_MATH_FN uint64_t ceil_shift(uint64_t n, unsigned l) { return (n + ((1ull << l) - 1ull)) >> l; }
// Levels of the tree over c >= 1 leaves: max(1, ceil(log2 c)) -- a lone leaf is hashed with itself once (CpuSha256D::Root's do-while).
VKMR_MATH_FN uint32_t height(uint64_t c) { return c <= 2 ? 1u : 64u - (uint32_t)__builtin_clzll(c - 1); }
// The duplicate-last rule from below: the right child of parent j in a level of n cells (2 j < n), the left one again at the edge.
VKMR_MATH_FN uint64_t right_child(uint64_t j, uint64_t n) { return (2 * j + 1 < n) ? 2 * j + 1 : 2 * j; }
// The same rule from a path: the cell a proof takes beside node p of a level of n cells (p < n), p itself at the edge.
VKMR_MATH_FN uint64_t sibling(uint64_t p, uint64_t n) { return ((p ^ 1ull) < n) ? (p ^ 1ull) : p; }
}  // namespace vkmr_math
