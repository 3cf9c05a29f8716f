"""Applying a multiproof restated with hashlib, on top of tests/forest_multiproof_cases.py and tests/multiproof_cases.py, and
the entry sets, leaf patterns and helpers tests/test_apply_abi.py (no GPU) and tests/test_gpu_apply.py share: the definition
that vkmr_hip_apply_multiproof_async, vkmr_hip_apply_forest_multiproof_async and the two vkmr_host_cpu_apply_* functions are
checked against (include/vkmr_hip.h states the same contract in words).  A plain module: no fixtures, no GPU.

A holder of the roots alone is given the old and the new leaves at the entries, the multiproof gathered before the update
and the count c_t of every named tree.  The old leaves are folded as the verifier folds them, against the old roots.  The new
leaves are folded beside them with ONE change: where a left child p of tree t's level l has no sibling among the entries and
p + 1 >= n_l(t) = ceil(c_t / 2^l), the proof's node -- the node's own OLD value -- is still consumed, but the new side's
right operand is the new side's own value of p."""
import numpy as np

import forest_cases as fc
import forest_multiproof_cases as fm
from merkle_model import cpu_levels, node, random_leaves, tree_height  # noqa: F401

NON_EMPTY = sorted(name for name, counts in fc.CASES.items() if sum(counts))
EDGE_KS = (1, 63, 64, 65, 16384, 16385)        # a ballot word and a prefix block of the ranking, and one to either side
LEAF_PATTERNS = ("random", "every leaf equal")


def case_leaves(name, pattern="random"):
    """The leaves of fc.CASES[name]: random digests, or every leaf one digest -- where a rule that compares values instead of
    using the count takes every left child for a duplicated one."""
    counts = fc.CASES[name]
    leaves = fc.random_leaves(sum(counts), seed=len(name) * 7919 + sum(counts))
    if pattern == "every leaf equal":
        leaves[:] = leaves[0]
    return leaves


def entry_sets(counts, rng):
    """fm.entry_sets and "left of the last pair": per non-empty tree the leaf (c - 1) & ~1.  For even c > 2 that leaf's path
    meets a duplicated node above level 0 while the leaf itself is not last."""
    sets = dict(fm.entry_sets(counts, rng))
    sets["left of the last pair"] = fm.sorted_entries((t, (c - 1) & ~1) for t, c in enumerate(counts) if c)
    return sets


def counts_of(counts, trees):
    """uint64 [k]: the count of each entry's tree."""
    return np.array([counts[int(t)] for t in trees], dtype=np.uint64)


def fold_both(old_leaves, new_leaves, indices, count, height, take):
    """(old root, new root) of one tree's entries; take() gives the next node of the proof."""
    old = {int(i): np.asarray(v, dtype=np.uint32) for i, v in zip(indices, old_leaves)}
    new = {int(i): np.asarray(v, dtype=np.uint32) for i, v in zip(indices, new_leaves)}
    for l in range(height):
        n = -(-count >> l)
        old_next, new_next = {}, {}
        for P in sorted(set(p >> 1 for p in old)):
            left, right = 2 * P, 2 * P + 1
            if left in old and right in old:
                old_next[P], new_next[P] = node(old[left], old[right]), node(new[left], new[right])
            elif left in old:
                given = take()
                old_next[P] = node(old[left], given)
                new_next[P] = node(new[left], new[left] if left + 1 >= n else given)     # the one change
            else:
                given = take()
                old_next[P], new_next[P] = node(given, old[right]), node(given, new[right])
        old, new = old_next, new_next
    assert list(old) == [0]
    return old[0], new[0]


def apply_forest(old_leaves, new_leaves, trees, indices, counts, stride, nodes, roots):
    """The rule of vkmr_hip_apply_forest_multiproof_async: the new roots [ntrees, 8], a copy of `roots` with the named trees
    advanced, or None when ok would be 0.  counts: one per entry."""
    trees, idx, cs = [int(t) for t in trees], [int(i) for i in indices], [int(c) for c in counts]
    k = len(idx)
    if k == 0 or len(old_leaves) != k or len(new_leaves) != k or len(trees) != k or len(cs) != k or not 1 <= stride <= 63:
        return None
    pairs = list(zip(trees, idx))
    if any(b <= a for a, b in zip(pairs, pairs[1:])):
        return None
    count = {}
    for t, i, c in zip(trees, idx, cs):
        if t >= len(roots) or c < 1 or i >= c or tree_height(c) > stride or count.setdefault(t, c) != c:
            return None
    by_tree = fm.by_tree(trees, idx)
    implied = sum(sum(fm.mc.emitted_positions(1 << tree_height(count[t]), tree_height(count[t]), by_tree[t])[1]) for t in by_tree)
    if implied != len(nodes):
        return None
    # level-major over the whole forest: every tree's nodes of level l lie before any node of level l + 1
    level_counts = fm.emitted_positions({t: 1 << tree_height(count[t]) for t in by_tree}, trees, idx, stride)[1]
    at = [sum(level_counts[:l]) for l in range(stride)]
    out = np.array(roots, dtype=np.uint32).reshape(-1, 8).copy()
    for t in by_tree:
        rows = [q for q in range(k) if trees[q] == t]
        h = tree_height(count[t])
        # one tree's fold reads its own nodes of each level in turn: hand them out level by level
        per_level = fm.mc.emitted_positions(1 << h, h, by_tree[t])[1]
        queue = []
        for l in range(h):
            queue += [np.asarray(nodes[at[l] + j], dtype=np.uint32) for j in range(per_level[l])]
            at[l] += per_level[l]
        it = iter(queue)
        old_root, new_root = fold_both([old_leaves[q] for q in rows], [new_leaves[q] for q in rows], [idx[q] for q in rows], count[t], h,
                                       lambda: next(it))
        if not (old_root == np.asarray(roots[t], dtype=np.uint32)).all():
            return None
        out[t] = new_root
    return out


def apply_tree(old_leaves, new_leaves, indices, count, height, nodes, root):
    """The rule of vkmr_hip_apply_multiproof_async: the new root [8], or None when ok would be 0."""
    idx = [int(i) for i in indices]
    k = len(idx)
    if k == 0 or len(old_leaves) != k or len(new_leaves) != k or not 1 <= height <= 63 or not 1 <= count <= (1 << height):
        return None
    if any(b <= a for a, b in zip(idx, idx[1:])) or idx[-1] >= count:
        return None
    if sum(fm.mc.emitted_positions(1 << height, height, idx)[1]) != len(nodes):
        return None
    it = iter([np.asarray(v, dtype=np.uint32) for v in nodes])
    old_root, new_root = fold_both(old_leaves, new_leaves, idx, count, height, lambda: next(it))
    return new_root if (old_root == np.asarray(root, dtype=np.uint32)).all() else None


def rebuilt_roots(leaves, counts, trees=None, height=None):
    """{t: root} of the trees (all non-empty ones when None) of a forest, by cpu_levels of its leaves as they are."""
    off = fc.offsets_of(counts)
    named = sorted(set(int(t) for t in trees)) if trees is not None else [t for t, c in enumerate(counts) if c]
    return {t: cpu_levels(leaves[int(off[t]): int(off[t + 1])], height)[-1][0] for t in named}


def updated(leaves, counts, trees, indices, new_leaves):
    """A copy of the forest's leaves with new_leaves at the entries."""
    out = np.array(leaves, dtype=np.uint32).reshape(-1, 8).copy()
    off = fc.offsets_of(counts)
    out[(off[np.asarray(trees, dtype=np.int64)] + np.asarray(indices, dtype=np.uint64)).astype(np.int64)] = new_leaves
    return out


def counts_for_heights(heights, trees, counts):
    """fm.mutations speaks in heights, the apply calls in counts: the per-entry counts that tell `heights` -- the count of the
    entry's tree where that is its height (a tree past the forest: any), else a count of exactly that height (0 for height 0)."""
    out = np.zeros(len(heights), dtype=np.uint64)
    for q, (h, t) in enumerate(zip(heights, trees)):
        c = counts[int(t)] if int(t) < len(counts) else 0
        if c and tree_height(c) == int(h):
            out[q] = c
        else:
            out[q] = 0 if int(h) == 0 else (1 << int(h)) if int(h) <= 63 else 2**64 - 1
            assert int(out[q]) == 0 or tree_height(int(out[q])) == int(h)
    return out


CANARY = np.uint32(0xC3C3C3C3)


def host_apply_forest(old_leaves, new_leaves, trees, indices, counts, stride, nodes, roots, in_place=False):
    """(1 or 0, new roots [ntrees, 8]) of vkmr_host_cpu_apply_forest_multiproof; the new roots start as CANARY (as a copy of
    the roots, and are the roots argument itself, with in_place)."""
    import vk_merkle_roots_amd as vk
    old = np.ascontiguousarray(old_leaves, dtype=np.uint32).reshape(-1, 8)
    new = np.ascontiguousarray(new_leaves, dtype=np.uint32).reshape(-1, 8)
    trees = np.ascontiguousarray(trees, dtype=np.uint32).reshape(-1)
    idx = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
    counts = np.ascontiguousarray(counts, dtype=np.uint64).reshape(-1)
    nodes = np.ascontiguousarray(nodes, dtype=np.uint32).reshape(-1, 8)
    roots = np.ascontiguousarray(roots, dtype=np.uint32).reshape(-1, 8).copy()
    out = roots if in_place else np.full(roots.shape, CANARY, dtype=np.uint32)
    r = vk.host_lib().vkmr_host_cpu_apply_forest_multiproof(old.ctypes.data, new.ctypes.data, trees.ctypes.data, idx.ctypes.data, counts.ctypes.data,
                                                            idx.shape[0], stride, nodes.ctypes.data if nodes.shape[0] else None, nodes.shape[0],
                                                            roots.ctypes.data, roots.shape[0], out.ctypes.data)
    assert r in (0, 1)
    return r, out


def host_apply_tree(old_leaves, new_leaves, indices, count, height, nodes, root):
    """(1 or 0, new root [8]) of vkmr_host_cpu_apply_multiproof; the new root starts as CANARY."""
    import vk_merkle_roots_amd as vk
    old = np.ascontiguousarray(old_leaves, dtype=np.uint32).reshape(-1, 8)
    new = np.ascontiguousarray(new_leaves, dtype=np.uint32).reshape(-1, 8)
    idx = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
    nodes = np.ascontiguousarray(nodes, dtype=np.uint32).reshape(-1, 8)
    root = np.ascontiguousarray(root, dtype=np.uint32).reshape(8)
    out = np.full(8, CANARY, dtype=np.uint32)
    r = vk.host_lib().vkmr_host_cpu_apply_multiproof(old.ctypes.data, new.ctypes.data, idx.ctypes.data, idx.shape[0], int(count), int(height),
                                                     nodes.ctypes.data if nodes.shape[0] else None, nodes.shape[0], root.ctypes.data, out.ctypes.data)
    assert r in (0, 1)
    return r, out


def scratch_bytes(k, levels):
    """The closed form of vkmr_hip_apply_multiproof_scratch_bytes: the verifier's scratch in whole 16-byte units, then k cells,
    k end words and k heights, each part starting on 16 bytes."""
    if k == 0 or levels > 63:
        return 0
    words = (k + 63) // 64
    blocks = (words + 255) // 256
    verifier = 32 * k + 16 * words * levels + 8 * blocks * levels + 8 * (2 + 64) + 4 * k
    up = lambda b: (b + 15) // 16 * 16      # noqa: E731
    return up(verifier) + 32 * k + up(4 * k) + up(4 * k)
