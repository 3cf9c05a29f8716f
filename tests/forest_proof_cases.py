"""Proofs inside a forest restated with hashlib, and the helpers tests/test_forest_proofs_abi.py (no GPU) and
tests/test_gpu_forest_proofs.py share: the definition that vkmr_hip_forest_proofs_async, vkmr_hip_verify_forest_proofs_async
and vkmr_host_cpu_forest_proofs are checked against (include/vkmr_hip.h states the same contract in words).  A plain module.

Forest: tree t is leaves[offsets[t] : offsets[t+1]], c_t of them, h_t = max(1, ceil(log2 c_t)).  Level l of a tree has
n_l = ceil(c_t / 2^l) nodes, node j of level l + 1 = SHA-256d(L[l][2j] || L[l][min(2j + 1, n_l - 1)]).  The proof of leaf i of
tree t is, for l < h_t, L_t[l][p ^ 1] with p = i >> l, or L_t[l][p] where p ^ 1 >= n_l; it is padded with zero cells to the
stride.  A tree >= ntrees or an index >= c_t has height 0 and only zero cells."""
import numpy as np

import forest_cases as fc
from merkle_model import build_plan_exe, cpu_levels, fold, forests_replay, host_fold, node, proof_path, random_counts, tree_height  # noqa: F401

ROOT = fc.ROOT


def stride_of(total, max_count):
    """H: the levels of a forest's build and the stride of its proofs."""
    return tree_height(max(1, min(int(max_count), int(total))))


def gather(leaves, offsets, trees, indices, stride):
    """(siblings [k, stride, 8], heights [k], roots {t: [8]} of the trees some valid query named)."""
    leaves = np.asarray(leaves, dtype=np.uint32).reshape(-1, 8)
    off = [int(x) for x in offsets]
    ntrees = len(off) - 1
    k = len(trees)
    sib = np.zeros((k, stride, 8), dtype=np.uint32)
    heights = np.zeros(k, dtype=np.uint32)
    cache, roots = {}, {}
    for q in range(k):
        t, i = int(trees[q]), int(indices[q])
        if t >= ntrees or i >= off[t + 1] - off[t]:
            continue
        if t not in cache:
            cache[t] = cpu_levels(leaves[off[t]: off[t + 1]])
            roots[t] = cache[t][-1][0]
        lv = cache[t]
        h = len(lv) - 1
        assert h <= stride
        heights[q] = h
        sib[q, :h] = proof_path(lv, i, h)
    return sib, heights, roots


def accepts(leaf, tree, index, siblings, height, stride, roots):
    """The acceptance rule of vkmr_hip_verify_forest_proofs_async for one proof."""
    height, tree, index = int(height), int(tree), int(index)
    if not 1 <= height <= stride or index >> height or tree >= len(roots):
        return False
    return bool((fold(leaf, index, siblings, height) == roots[tree]).all())


def host_cpu_proofs(leaves, offsets, trees, indices, stride):
    """(return code, siblings [k, stride, 8], heights [k]) of vkmr_host_cpu_forest_proofs; both outputs start as a 0xA5 pattern."""
    import vk_merkle_roots_amd as vk
    leaves = np.ascontiguousarray(leaves, dtype=np.uint32).reshape(-1, 8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    trees = np.ascontiguousarray(trees, dtype=np.uint32)
    indices = np.ascontiguousarray(indices, dtype=np.uint64)
    k = trees.shape[0]
    sib = np.full((k, stride, 8), 0xA5A5A5A5, dtype=np.uint32)
    heights = np.full(k, 0xA5A5A5A5, dtype=np.uint32)
    rc = vk.host_lib().vkmr_host_cpu_forest_proofs(leaves.ctypes.data if leaves.size else None, offsets.ctypes.data, offsets.shape[0] - 1,
                                                   trees.ctypes.data, indices.ctypes.data, k, stride, sib.ctypes.data, heights.ctypes.data)
    return rc, sib, heights


def all_queries(counts, sample_above=5000, seed=1):
    """(trees [k] uint32, indices [k] uint64): every leaf of every tree; of a tree above `sample_above` leaves (the big tree
    of one_big_among_small) both ends, the cells around every power of two and 200 random leaves."""
    rng = np.random.default_rng(seed)
    trees, indices = [], []
    for t, c in enumerate(counts):
        if c <= sample_above:
            idx = range(c)
        else:
            edges = {0, 1, c - 2, c - 1} | {x for b in range(1, c.bit_length()) for x in ((1 << b) - 1, 1 << b) if x < c}
            idx = sorted(edges | {int(x) for x in rng.integers(0, c, size=200)})
        trees += [t] * len(idx)
        indices += list(idx)
    return np.array(trees, dtype=np.uint32), np.array(indices, dtype=np.uint64)


def random_queries(rng, counts, k):
    """k random (tree, index) pairs that name a leaf; the forest has at least one."""
    c = np.asarray(counts, dtype=np.int64)
    full = np.nonzero(c > 0)[0]
    trees = full[rng.integers(0, full.shape[0], size=k)]
    indices = (rng.random(k) * c[trees]).astype(np.int64)
    return trees.astype(np.uint32), np.minimum(indices, c[trees] - 1).astype(np.uint64)


def stored_cells(total, ntrees, max_count):
    """The closed form of vkmr_hip_forest_tree_bytes / 32."""
    if ntrees == 0 or max_count == 0:
        return 0
    return sum((total >> l) + ntrees for l in range(1, stride_of(total, max_count) + 1))


def build_store_plan_exe(directory):
    """tests/c/forest_store_plan_test.cpp compiled into `directory`; its path."""
    return build_plan_exe(directory, "forest_store_plan_test")


def store_plan_replay(exe, directory, forests):
    """For each (first_offset, slack, max_count, counts): (levels, cells the test summed on its own, highest cell used + 1);
    the C test has checked the level bounds and the overlaps on the way."""
    return forests_replay(exe, directory, forests, "stored_forests.txt")
