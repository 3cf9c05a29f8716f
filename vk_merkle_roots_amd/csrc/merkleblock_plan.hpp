// merkleblock_plan.hpp -- partial Merkle trees in BIP37 order (the `merkleblock` message, Bitcoin Core's CPartialMerkleTree):
// where every flag and every hash of a tree's walk goes, found without walking.  Plain integer arithmetic, no HIP types:
// shared by the kernels (merkleblock_kernels.hpp), the C ABI (vkmr_hip.hip), the CPU twin (host/host_api.cpp) and the replay
// in tests/c/merkleblock_plan_test.cpp.
//
// THE RULE.  A tree of c >= 1 leaves has h = max(1, ceil(log2 c)) levels above its leaves (the project's height: a lone leaf is
// hashed with itself) and w(l) = ceil(c / 2^l) nodes at level l.  A_0 is the set of matched leaves, A_{l+1} = unique(A_l >> 1).
// visit(h, 0) starts the walk; visit(l, p) appends the flag f = (p in A_l); if l == 0 or !f it appends the hash of stored node
// (l, p); otherwise visit(l - 1, 2p), then visit(l - 1, 2p + 1) only if 2p + 1 < w(l - 1).  Flag number i is bit i & 7 of byte
// i >> 3, padding bits 0.  For c >= 2 this is byte for byte what Bitcoin Core's TraverseAndBuild writes.  THE LONE LEAF: for
// c == 1 the rule gives two flags (1, 1) and one hash, and the root the receiver forms is hash_pair(leaf, leaf); Bitcoin has
// one flag and the txid as the root.  It is not special-cased: this engine's root of such a tree is not Bitcoin's anyway.
//
// POSITIONS WITHOUT A WALK: the closed form, entry by entry.  With the matched leaves sorted, what the walk appends between
// the flag of one matched leaf a (exclusive) and the flag of the next one b (inclusive) depends on a, b and c alone.  Let
// top = bit_length(a ^ b) - 1, the level at which the paths of a and b are the two children of one node.  The walk
//   climbs    from a: at every level l < top where bit l of a is 0 the right sibling (l, (a >> l) + 1) follows -- flag 0 and its
//             hash.  It exists: it lies in front of b.  That is zeros(a, top) nodes, l ascending;
//   descends  to b: the path node of level top (flag 1), then for l = top - 1 .. 0 the left sibling (l, (b >> l) - 1) where bit
//             l of b is 1 (flag 0 and its hash) and the path node of level l (flag 1); the leaf's hash behind its flag.
// The first matched leaf of a tree has no climb and descends from the root: top = h.  Behind the last matched leaf b the walk
// climbs to the root: the right sibling at every level l < h where bit l of b is 0 and (b >> l) + 1 < w(l), which is
// l < bit_length(b ^ (c - 1)) -- from that level on b's path is the tree's right edge, where BIP37 carries nothing (the
// project's multiproof carries the node itself there).  So an entry's group is
//     flags  = up + (top + 1) + ones(b, top)        hashes = up + ones(b, top) + 1        up = zeros(a, top), 0 for the first
// and a tree's tail zeros(b, min(h, bit_length(b ^ (c - 1)))) flags and as many hashes.  An exclusive prefix sum of the groups
// over the sorted entries (the tail added to a tree's last entry) places every group; inside a group every position is a
// population count (below).  Seen from a node, its place is the number of visited nodes in front of it in the walk's order: its
// ancestors plus, level by level, the visited nodes to its left.  That count IS the prefix of the groups in front of its entry
// plus its place in its own group, so the sums over levels are taken once per entry here, not once per node.  The alternative,
// "sizes up, offsets down" -- the flags and hashes of every visited subtree summed level by level, one launch per level, then
// the offsets handed down again, one launch per level, with both sums kept per (level, run of entries) in scratch -- was not
// taken: this form needs no launch per level and no per-level scratch.
// Checked against the recursive walk for every subset of every c <= 11, every single leaf and adjacent pair up to c = 130
// and random forests (tests/test_merkleblock_abi.py through tests/c/merkleblock_plan_test.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "forest_plan.hpp"

#define VKMR_MB_FN VKMR_MATH_FN
#define VKMR_MB_THREADS 256   // entries (or blocks) per workgroup of the prefix sums: vkmr_sizes::block_exclusive's workgroup

namespace vkmr_mb {

using vkmr_math::height;

VKMR_MB_FN uint32_t bit_length(uint64_t x) { return x == 0 ? 0u : 64u - (uint32_t)__builtin_clzll(x); }
// Set bits of x below bit m (m <= 64).
VKMR_MB_FN uint32_t ones_below(uint64_t x, uint32_t m) { return m == 0 ? 0u : (uint32_t)__builtin_popcountll(m >= 64 ? x : x & ((1ull << m) - 1ull)); }
VKMR_MB_FN uint32_t zeros_below(uint64_t x, uint32_t m) { return m - ones_below(x, m); }

// The levels below which leaf b of a tree of c leaves (height h) still has right siblings to climb past: above, its path is the
// tree's right edge.
VKMR_MB_FN uint32_t edge_level(uint64_t b, uint64_t c, uint32_t h)
{
    const uint32_t e = bit_length(b ^ (c - 1ull));
    return e < h ? e : h;
}

// What the walk appends for one entry: matched leaf b of a tree of height h, behind matched leaf a of the same tree (has_prev)
// or as the tree's first.
struct Group {
    uint32_t top;      // the level of the group's first path flag: where the path of b leaves the path of a; h for the first
    uint32_t up;       // right siblings on the climb from a: flag 0 and a hash each, in front of everything else
    uint32_t ones;     // left siblings on the way down to b
    uint32_t flags, hashes;
};

VKMR_MB_FN Group group(bool has_prev, uint64_t a, uint64_t b, uint32_t h)
{
    Group g;
    g.top = has_prev ? bit_length(a ^ b) - 1u : h;
    g.up = has_prev ? zeros_below(a, g.top) : 0u;
    g.ones = ones_below(b, g.top);
    g.flags = g.up + g.top + 1u + g.ones;
    g.hashes = g.up + g.ones + 1u;
    return g;
}

// Flags (= hashes) behind a tree's last matched leaf b.
VKMR_MB_FN uint32_t tail(uint64_t b, uint64_t c, uint32_t h) { return zeros_below(b, edge_level(b, c, h)); }

// Places inside a group, counted from its first flag / first hash.
// The right sibling of leaf a's path at level l of a climb that ends below level `limit` (a group: its top; a tail: the edge
// level): there is one when l < limit and bit l of a is 0, and it is the climb's node number zeros(a, l), as flag and as hash.
VKMR_MB_FN bool climbs(uint64_t a, uint32_t l, uint32_t limit) { return l < limit && !((a >> l) & 1ull); }
VKMR_MB_FN uint32_t climb_place(uint64_t a, uint32_t l) { return zeros_below(a, l); }
// The flag of b's path node at level l <= top.
VKMR_MB_FN uint32_t path_flag(const Group& g, uint64_t b, uint32_t l) { return g.up + (g.top - l) + g.ones - ones_below(b, l); }
// The left sibling of b's path at level l < top, there when bit l of b is 1: its flag is the one in front of the path node's.
VKMR_MB_FN bool descends(const Group& g, uint64_t b, uint32_t l) { return l < g.top && ((b >> l) & 1ull); }
VKMR_MB_FN uint32_t left_flag(const Group& g, uint64_t b, uint32_t l) { return path_flag(g, b, l) - 1u; }
VKMR_MB_FN uint32_t left_hash(const Group& g, uint64_t b, uint32_t l) { return g.up + g.ones - ones_below(b, l + 1u); }
// The matched leaf's own hash: the group's last.
VKMR_MB_FN uint32_t leaf_hash(const Group& g) { return g.up + g.ones; }

// ---- sizes.  Bounds from the rule: every flag 0 carries a hash, every matched leaf carries one, so
//     hashes = k_t + (the tree's multiproof nodes) - (those at a duplicate-last edge) <= k_t + multiproof nodes;
// the visited nodes form a binary tree whose leaves are the hash carriers and whose one-child nodes lie on the right edge, at
// most h of them: flags <= 2 * hashes + h (and flags <= k_t * h + hashes: at most h path flags above each matched leaf).
inline uint64_t max_hashes(uint64_t total, uint32_t ntrees, uint64_t max_count, uint32_t k)
{
    return (uint64_t)k + vkmr_forest::multiproof_max_nodes(total, ntrees, max_count, k);
}

// Every block starts on a byte: ceil(flags_t / 8) summed over at most min(k, ntrees) blocks.
inline uint64_t max_flag_bytes(uint64_t total, uint32_t ntrees, uint64_t max_count, uint32_t k)
{
    const uint64_t blocks = k < ntrees ? k : ntrees;
    const uint64_t flags = 2ull * max_hashes(total, ntrees, max_count, k) + blocks * vkmr_forest::launches(total, max_count);
    return (flags + 7ull) / 8ull + blocks;
}

// The same bound from k and the stride alone, for the scratch: hashes <= k * (stride + 1), at most k blocks.
inline uint64_t scratch_flag_bytes(uint32_t k, uint32_t stride)
{
    const uint64_t flags = 2ull * (uint64_t)k * (stride + 1ull) + (uint64_t)k * stride;
    return (flags + 7ull) / 8ull + (uint64_t)k;
}

// Where the parts of a call's scratch lie, in bytes; every part starts on 16 bytes.
struct Layout {
    uint64_t groups;      // workgroups of the prefix sums over the entries (and over the blocks: no more blocks than entries)
    uint64_t words;       // 32-bit words the flags are ORed into before they go out byte-exact
    size_t flag_at, hash_at, block_of, sums, bit_start, byte_sums, flag_words, bytes;
};

inline size_t round_up_16(size_t bytes) { return (bytes + 15u) & ~(size_t)15u; }

inline Layout layout(uint32_t k, uint32_t stride)
{
    Layout L;
    L.groups = ((uint64_t)k + VKMR_MB_THREADS - 1) / VKMR_MB_THREADS;
    L.words = (scratch_flag_bytes(k, stride) + 3ull) / 4ull;
    size_t at = 0;
    L.flag_at = at;    at = round_up_16(at + (size_t)k * sizeof(uint64_t));            // flags in front of entry q's group, over all trees
    L.hash_at = at;    at = round_up_16(at + (size_t)k * sizeof(uint64_t));            // hashes in front of it
    L.block_of = at;   at = round_up_16(at + (size_t)k * sizeof(uint32_t));            // the block (named tree) of entry q
    L.sums = at;       at = round_up_16(at + (size_t)(3 * L.groups) * sizeof(uint64_t));   // per workgroup: flags, hashes, blocks
    L.bit_start = at;  at = round_up_16(at + ((size_t)k + 1) * sizeof(uint64_t));      // flags in front of block b, over all trees
    L.byte_sums = at;  at = round_up_16(at + (size_t)L.groups * sizeof(uint64_t));     // per workgroup of blocks: flag bytes
    L.flag_words = at; at = round_up_16(at + (size_t)L.words * sizeof(uint32_t));
    L.bytes = at;
    return L;
}

}  // namespace vkmr_mb
