"""Proofs inside a forest restated with hashlib, and the helpers tests/test_forest_proofs_abi.py (no GPU) and
tests/test_gpu_forest_proofs.py share: the definition that vkmr_hip_forest_proofs_async, vkmr_hip_verify_forest_proofs_async
and vkmr_host_cpu_forest_proofs are checked against (include/vkmr_hip.h states the same contract in words).  A plain module.

Forest: tree t is leaves[offsets[t] : offsets[t+1]], c_t of them, h_t = max(1, ceil(log2 c_t)).  Level l of a tree has
n_l = ceil(c_t / 2^l) nodes, node j of level l + 1 = SHA-256d(L[l][2j] || L[l][min(2j + 1, n_l - 1)]).  The proof of leaf i of
tree t is, for l < h_t, L_t[l][p ^ 1] with p = i >> l, or L_t[l][p] where p ^ 1 >= n_l; it is padded with zero cells to the
stride.  A tree >= ntrees or an index >= c_t has height 0 and only zero cells."""
import hashlib
import os
import subprocess

import numpy as np

import forest_cases as fc

ROOT = fc.ROOT


def node(l, r):
    """SHA-256d(l || r) of word-valued digests."""
    b = np.concatenate([l, r]).astype(">u4").tobytes()
    return np.frombuffer(hashlib.sha256(hashlib.sha256(b).digest()).digest(), dtype=">u4").astype(np.uint32)


def tree_height(count):
    return max(1, int(count - 1).bit_length())


def stride_of(total, max_count):
    """H: the levels of a forest's build and the stride of its proofs."""
    return tree_height(max(1, min(int(max_count), int(total))))


def cpu_levels(leaves):
    """Levels 0 .. h of the tree over `leaves` ([c, 8] uint32, c >= 1); the last one is the root."""
    levels = [np.asarray(leaves, dtype=np.uint32).reshape(-1, 8)]
    for _ in range(tree_height(levels[0].shape[0])):
        cur = levels[-1]
        n = cur.shape[0]
        levels.append(np.stack([node(cur[2 * p], cur[min(2 * p + 1, n - 1)]) for p in range((n + 1) // 2)]))
    assert levels[-1].shape[0] == 1
    return levels


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
        for l in range(h):
            p = i >> l
            sib[q, l] = lv[l][p ^ 1] if (p ^ 1) < lv[l].shape[0] else lv[l][p]
    return sib, heights, roots


def fold(leaf, index, siblings, height):
    """The root a proof claims: bit l of the index set puts the sibling on the left."""
    cur = np.asarray(leaf, dtype=np.uint32)
    for l in range(int(height)):
        cur = node(siblings[l], cur) if (int(index) >> l) & 1 else node(cur, siblings[l])
    return cur


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


def host_fold(leaf, index, siblings, height):
    """vkmr_host_cpu_fold_proof."""
    import vk_merkle_roots_amd as vk
    leaf = np.ascontiguousarray(leaf, dtype=np.uint32)
    siblings = np.ascontiguousarray(siblings, dtype=np.uint32)
    out = np.zeros(8, dtype=np.uint32)
    vk.host_lib().vkmr_host_cpu_fold_proof(leaf.ctypes.data, int(index), siblings.ctypes.data, int(height), out.ctypes.data)
    return out


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


def random_counts(rng, budget):
    """Tree sizes of one random forest of at most `budget` leaves: a mix of shapes, empty trees included (the generator of
    tests/test_gpu_forest.py)."""
    ntrees = int(rng.integers(1, 33))
    kind = int(rng.integers(0, 4))
    if kind == 0:
        counts = rng.integers(0, 20, size=ntrees)
    elif kind == 1:
        counts = rng.integers(1, 5000, size=ntrees)
    elif kind == 2:
        counts = (1 << rng.integers(0, 15, size=ntrees)) + rng.integers(-1, 2, size=ntrees)
    else:
        counts = rng.integers(1, 200, size=ntrees)
        counts[int(rng.integers(0, ntrees))] = int(rng.integers(1, budget // 2))
    counts = [int(c) for c in counts]
    while sum(counts) > budget:
        counts.pop()
    return counts


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
    exe = os.path.join(str(directory), "forest_store_plan_test")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "vk_merkle_roots_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "forest_store_plan_test.cpp"), "-o", exe])
    return exe


def store_plan_replay(exe, directory, forests):
    """For each (first_offset, slack, max_count, counts): (levels, cells the test summed on its own, highest cell used + 1);
    the C test has checked the level bounds and the overlaps on the way."""
    path = os.path.join(str(directory), "stored_forests.txt")
    with open(path, "w") as f:
        for first, slack, max_count, counts in forests:
            f.write(" ".join(str(int(x)) for x in [first, slack, max_count] + list(counts)) + "\n")
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = r.stdout.decode()
    assert r.returncode == 0 and "FAIL" not in text and f"ok: {len(forests)} forests" in text, text[-2000:]
    return [tuple(int(x) for x in line.split()) for line in text.splitlines()[: len(forests)]]
