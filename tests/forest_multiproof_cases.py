"""Multiproofs inside a forest restated with hashlib, and the entry sets, mutations and helpers tests/test_forest_multiproof_abi.py
(no GPU) and tests/test_gpu_forest_multiproof.py share: the definition that vkmr_hip_forest_multiproof_async,
vkmr_hip_verify_forest_multiproof_async and the two vkmr_host_cpu_*forest_multiproof functions are checked against
(include/vkmr_hip.h states the same contract in words).  A plain module: no fixtures, no GPU.

Forest: tree t is leaves[offsets[t] : offsets[t+1]], c_t of them, h_t = max(1, ceil(log2 c_t)); H = the forest's stride.
Entries: (tree, index) pairs, strictly increasing.  A_0(t) = tree t's indices, A_{l+1}(t) = unique(A_l(t) >> 1).  For
l = 0 .. H - 1, for t ascending over the named trees with l < h_t, for p in A_l(t) ascending: nothing when p ^ 1 is in A_l(t),
else ONE node, L_t[l][p ^ 1], or L_t[l][p] where p ^ 1 >= n_l.  The verifier needs no count, only the height of each tree."""
import numpy as np

import forest_cases as fc
import forest_proof_cases as fp
import multiproof_cases as mc
from merkle_model import cpu_levels, node, random_leaves, tree_height  # noqa: F401

ROOT = fc.ROOT
stride_of = fp.stride_of


def by_tree(trees, indices):
    """{tree: sorted unique indices} in ascending tree order."""
    out = {}
    for t, i in zip(trees, indices):
        out.setdefault(int(t), set()).add(int(i))
    return {t: sorted(out[t]) for t in sorted(out)}


def sorted_entries(pairs):
    """(trees uint32, indices uint64): the pairs sorted lexicographically, each once."""
    pairs = sorted(set((int(t), int(i)) for t, i in pairs))
    return np.array([t for t, _ in pairs], dtype=np.uint32), np.array([i for _, i in pairs], dtype=np.uint64)


def emitted_positions(counts, trees, indices, stride):
    """([(l, tree, cell)] of the multiproof's nodes in order, the per-level counts [stride]).  No hashing."""
    cur = by_tree(trees, indices)
    heights = {t: tree_height(counts[t]) for t in cur}
    out, level_counts = [], []
    for l in range(stride):
        m = 0
        for t in cur:
            if l >= heights[t]:
                continue
            n = -(-counts[t] >> l)
            have = set(cur[t])
            for p in cur[t]:
                if p ^ 1 in have:
                    continue
                out.append((l, t, p ^ 1 if p ^ 1 < n else p))
                m += 1
            cur[t] = sorted(set(p >> 1 for p in cur[t]))
        level_counts.append(m)
    return out, level_counts


def make(leaves, offsets, trees, indices, stride, cache=None):
    """(nodes [M, 8], heights [k] uint32, level counts [stride], roots {t: [8]} of the named trees) of sorted in-range entries.
    cache: a dict that keeps the levels of the trees between calls over the same leaves."""
    leaves = np.asarray(leaves, dtype=np.uint32).reshape(-1, 8)
    off = [int(x) for x in offsets]
    counts = [off[t + 1] - off[t] for t in range(len(off) - 1)]
    pos, level_counts = emitted_positions(counts, trees, indices, stride)
    cache = {} if cache is None else cache
    for t in set(int(t) for t in trees):
        if t not in cache:
            cache[t] = cpu_levels(leaves[off[t]: off[t + 1]])
    levels = {t: cache[t] for t in set(int(t) for t in trees)}
    nodes = np.zeros((len(pos), 8), dtype=np.uint32)
    for i, (l, t, c) in enumerate(pos):
        nodes[i] = levels[t][l][c]
    heights = np.array([len(levels[int(t)]) - 1 for t in trees], dtype=np.uint32)
    return nodes, heights, level_counts, {t: lv[-1][0] for t, lv in levels.items()}


def verify(leaves, trees, indices, heights, stride, nodes, roots):
    """The acceptance rule of vkmr_hip_verify_forest_multiproof_async.  roots: [ntrees, 8]."""
    trees, idx, heights = [int(t) for t in trees], [int(i) for i in indices], [int(h) for h in heights]
    k = len(idx)
    if k == 0 or len(leaves) != k or len(trees) != k or len(heights) != k or not 1 <= stride <= 63:
        return False
    pairs = list(zip(trees, idx))
    if any(b <= a for a, b in zip(pairs, pairs[1:])):
        return False
    for t, i, h in zip(trees, idx, heights):
        if t >= len(roots) or not 1 <= h <= stride or i >> h:
            return False
    height = {}
    for t, h in zip(trees, heights):
        if height.setdefault(t, h) != h:
            return False
    cur = {}
    for t, i, v in zip(trees, idx, leaves):
        cur.setdefault(t, {})[i] = np.asarray(v, dtype=np.uint32)
    # the indices and heights must imply exactly len(nodes) nodes: count before folding
    implied = sum(sum(mc.emitted_positions(1 << height[t], height[t], sorted(cur[t]))[1]) for t in cur)
    if implied != len(nodes):
        return False
    used = 0
    for l in range(stride):
        for t in sorted(cur):
            if l >= height[t]:
                continue
            nxt = {}
            for P in sorted(set(p >> 1 for p in cur[t])):
                kids = []
                for c in (2 * P, 2 * P + 1):
                    if c in cur[t]:
                        kids.append(cur[t][c])
                    else:
                        kids.append(np.asarray(nodes[used], dtype=np.uint32))
                        used += 1
                nxt[P] = node(kids[0], kids[1])
            cur[t] = nxt
    assert used == len(nodes)
    return all(list(cur[t]) == [0] and bool((cur[t][0] == np.asarray(roots[t], dtype=np.uint32)).all()) for t in cur)


def max_nodes(total, ntrees, max_count, k):
    """The closed form of vkmr_hip_forest_multiproof_max_nodes."""
    if total == 0 or ntrees == 0 or max_count == 0:
        return 0
    return sum(min(k, (total >> (l + 1)) + ntrees) for l in range(stride_of(total, max_count)))


def split(trees, indices, heights, nodes, stride):
    """{tree: (indices, height, nodes [M_t, 8], level counts [height])}: the level-major nodes regrouped per tree, from the
    indices and heights alone (a tree of height h behaves as one of 2^h leaves: the verifier's view)."""
    groups = by_tree(trees, indices)
    height = {int(t): int(h) for t, h in zip(trees, heights)}
    counts = {t: mc.emitted_positions(1 << height[t], height[t], groups[t])[1] for t in groups}
    parts = {t: [] for t in groups}
    at = 0
    for l in range(stride):
        for t in groups:
            if l < height[t]:
                parts[t].append(np.asarray(nodes[at: at + counts[t][l]], dtype=np.uint32).reshape(-1, 8))
                at += counts[t][l]
    assert at == len(nodes)
    return {t: (np.array(groups[t], dtype=np.uint64), height[t], np.concatenate(parts[t]).reshape(-1, 8), counts[t]) for t in groups}


def entry_sets(counts, rng):
    """{name: (trees, indices)} over the non-empty trees of `counts` (at least one): every leaf (the big tree of
    one_big_among_small sampled as forest_proof_cases.all_queries does), one leaf per tree, the first and last leaf of every
    tree, 7 random leaves per non-empty tree."""
    full = [t for t, c in enumerate(counts) if c]
    every = fp.all_queries(counts)
    return {
        "every leaf": sorted_entries(zip(every[0].tolist(), every[1].tolist())),
        "one per tree": sorted_entries((t, int(rng.integers(0, counts[t]))) for t in full),
        "first and last": sorted_entries((t, i) for t in full for i in (0, counts[t] - 1)),
        "7 random per tree": sorted_entries((t, int(i)) for t in full for i in rng.integers(0, counts[t], size=7)),
    }


MUTATIONS = ("node zeroed", "last node dropped", "node appended", "leaf changed", "entries swapped", "entry repeated", "index >= 2^h",
             "tree >= ntrees", "height 0", "height above stride", "one entry of a tree with another height", "a tree's height + 1",
             "a tree's height - 1", "touched root changed")
STILL_ACCEPTED = "untouched root changed"


def mutations(leaves, trees, indices, heights, stride, nodes, roots, rng):
    """[(name, leaves, trees, indices, heights, nodes, roots)]: every MUTATIONS entry the proof allows, each of which must be
    rejected, and STILL_ACCEPTED, which must not.  One that needs what the case lacks (a node of an empty proof, a second
    entry, a tree of two entries, room under the stride, a height above 1, an untouched tree) is left out."""
    leaves, nodes, roots = (np.array(a, dtype=np.uint32).reshape(-1, 8) for a in (leaves, nodes, roots))
    trees, idx, heights = np.array(trees, dtype=np.uint32), np.array(indices, dtype=np.uint64), np.array(heights, dtype=np.uint32)
    k, ntrees = idx.shape[0], roots.shape[0]
    out = []

    def add(name, leaves=leaves, trees=trees, idx=idx, heights=heights, nodes=nodes, roots=roots):
        out.append((name, leaves, trees, idx, heights, nodes, roots))

    if nodes.shape[0]:
        z = nodes.copy()
        z[int(rng.integers(0, nodes.shape[0]))] = 0
        add("node zeroed", nodes=z)
        add("last node dropped", nodes=nodes[:-1].copy())
    add("node appended", nodes=np.concatenate([nodes, random_leaves(rng, 1)]))
    c = leaves.copy()
    c[int(rng.integers(0, k)), 0] ^= np.uint32(1)
    add("leaf changed", leaves=c)
    if k >= 2:
        a = int(rng.integers(0, k - 1))
        st, si, sh = trees.copy(), idx.copy(), heights.copy()
        for arr in (st, si, sh):
            arr[a], arr[a + 1] = arr[a + 1], arr[a]
        add("entries swapped", trees=st, idx=si, heights=sh)
        r = int(rng.integers(1, k))
        rt, ri, rh = trees.copy(), idx.copy(), heights.copy()
        rt[r], ri[r], rh[r] = rt[r - 1], ri[r - 1], rh[r - 1]
        add("entry repeated", trees=rt, idx=ri, heights=rh)
    o = idx.copy()
    o[-1] = np.uint64((1 << int(heights[-1])) + int(o[-1]))
    add("index >= 2^h", idx=o)
    t2 = trees.copy()
    t2[-1] = ntrees
    add("tree >= ntrees", trees=t2)
    q = int(rng.integers(0, k))
    whole = trees == trees[q]
    h0 = heights.copy()
    h0[whole] = 0
    add("height 0", heights=h0)
    h1 = heights.copy()
    h1[whole] = stride + 1
    add("height above stride", heights=h1)
    multi = [int(t) for t in np.unique(trees) if int((trees == t).sum()) >= 2]
    if multi:
        t = multi[int(rng.integers(0, len(multi)))]
        first = int(np.flatnonzero(trees == t)[int(rng.integers(0, 2))])
        h2 = heights.copy()
        h2[first] = heights[first] + 1 if heights[first] < stride else heights[first] - 1
        if h2[first] >= 1:
            add("one entry of a tree with another height", heights=h2)
    low = np.flatnonzero(heights < stride)
    if low.shape[0]:
        h3 = heights.copy()
        h3[trees == trees[low[0]]] += 1
        add("a tree's height + 1", heights=h3)
    tall = np.flatnonzero(heights > 1)
    if tall.shape[0]:
        h4 = heights.copy()
        h4[trees == trees[tall[-1]]] -= 1
        add("a tree's height - 1", heights=h4)
    r2 = roots.copy()
    r2[int(trees[q]), 7] ^= np.uint32(0x80000000)
    add("touched root changed", roots=r2)
    untouched = sorted(set(range(ntrees)) - set(int(t) for t in trees))
    if untouched:
        r3 = roots.copy()
        r3[untouched[int(rng.integers(0, len(untouched)))]] ^= np.uint32(0xFFFFFFFF)
        add(STILL_ACCEPTED, roots=r3)
    return out


def host_make(leaves, offsets, trees, indices, stride, capacity=None):
    """(return code, nodes [M, 8], heights [k], info [2 + stride]) of vkmr_host_cpu_forest_multiproof.  Every output starts as a
    0xA5 pattern; the node buffer has `capacity` cells (max_nodes's bound with max_count = total when None) and is cut to
    info[1] only when the call returned 0."""
    import vk_merkle_roots_amd as vk
    leaves = np.ascontiguousarray(leaves, dtype=np.uint32).reshape(-1, 8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    trees = np.ascontiguousarray(trees, dtype=np.uint32)
    indices = np.ascontiguousarray(indices, dtype=np.uint64)
    k, ntrees = trees.shape[0], offsets.shape[0] - 1
    if capacity is None:
        capacity = sum(min(k, (leaves.shape[0] >> (l + 1)) + ntrees) for l in range(stride))
    nodes = np.full((max(capacity, 1), 8), 0xA5A5A5A5, dtype=np.uint32)
    heights = np.full(k, 0xA5A5A5A5, dtype=np.uint32)
    info = np.full(2 + stride, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    rc = vk.host_lib().vkmr_host_cpu_forest_multiproof(leaves.ctypes.data if leaves.size else None, offsets.ctypes.data, ntrees, trees.ctypes.data,
                                                       indices.ctypes.data, k, stride, nodes.ctypes.data, capacity, heights.ctypes.data,
                                                       info.ctypes.data)
    return rc, (nodes[: int(info[1])] if rc == 0 else nodes), heights, info


def host_verify(leaves, trees, indices, heights, stride, nodes, roots):
    """vkmr_host_cpu_verify_forest_multiproof on host arrays: bool."""
    import vk_merkle_roots_amd as vk
    leaves = np.ascontiguousarray(leaves, dtype=np.uint32).reshape(-1, 8)
    trees = np.ascontiguousarray(trees, dtype=np.uint32).reshape(-1)
    idx = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
    heights = np.ascontiguousarray(heights, dtype=np.uint32).reshape(-1)
    nodes = np.ascontiguousarray(nodes, dtype=np.uint32).reshape(-1, 8)
    roots = np.ascontiguousarray(roots, dtype=np.uint32).reshape(-1, 8)
    r = vk.host_lib().vkmr_host_cpu_verify_forest_multiproof(leaves.ctypes.data, trees.ctypes.data, idx.ctypes.data, heights.ctypes.data, idx.shape[0],
                                                             stride, nodes.ctypes.data if nodes.shape[0] else None, nodes.shape[0],
                                                             roots.ctypes.data, roots.shape[0])
    assert r in (0, 1)
    return r == 1


def leaves_at(leaves, offsets, trees, indices):
    """[k, 8]: the proved leaves of the entries."""
    leaves = np.asarray(leaves, dtype=np.uint32).reshape(-1, 8)
    off = np.asarray(offsets, dtype=np.uint64)
    return leaves[(off[np.asarray(trees, dtype=np.int64)] + np.asarray(indices, dtype=np.uint64)).astype(np.int64)]


def roots_array(roots_by_tree, ntrees):
    """[ntrees, 8]: the named trees' roots, the others a pattern nothing may read as a match."""
    out = np.full((ntrees, 8), 0x5C5C5C5C, dtype=np.uint32)
    for t, r in roots_by_tree.items():
        out[t] = r
    return out
