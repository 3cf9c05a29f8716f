"""Leaf updates of a stored forest (vkmr_hip_forest_update_async, MerkleForest.update): the entry sets, the brute-force count of
what an update must rehash and the raw-API build between guard patterns that tests/test_forest_update_abi.py (no GPU) and
tests/test_gpu_forest_update.py share.  A plain module: no fixtures, no GPU.

An entry is a (tree, index) pair: leaf `index` of tree `tree`.  An update over sorted unique entries rewrites exactly the
ancestors of the named leaves: node index >> l of tree t's level l for 1 <= l <= h_t, level h_t being the root."""
import os
import subprocess

import numpy as np

import forest_cases as fc
import forest_proof_cases as fp
from merkle_model import build_plan_exe, tree_height

GUARD = 0xC3C3C3C3


def sorted_entries(pairs):
    """(trees uint32, indices uint64) of the distinct (tree, index) pairs, in lexicographic order."""
    pairs = sorted(set((int(t), int(i)) for t, i in pairs))
    return np.array([t for t, _ in pairs], dtype=np.uint32), np.array([i for _, i in pairs], dtype=np.uint64)


def first_and_last(counts):
    return sorted_entries([(t, i) for t, c in enumerate(counts) if c for i in (0, c - 1)])


def one_pair(counts):
    """Both children of one level-1 node: the last full pair of the largest tree (of its only leaf when it has one)."""
    t = int(np.argmax(counts))
    c = counts[t]
    return sorted_entries([(t, 0)] if c == 1 else [(t, (c - 2) & ~1), (t, ((c - 2) & ~1) + 1)])


def random_third(counts, rng):
    every = [(t, i) for t, c in enumerate(counts) for i in range(c)]
    pick = rng.choice(len(every), size=max(1, len(every) // 3), replace=False)
    return sorted_entries([every[int(j)] for j in pick])


def every_leaf(counts):
    return sorted_entries([(t, i) for t, c in enumerate(counts) for i in range(c)])


def update_sets(counts, rng):
    """name -> (trees, indices): the entry sets every case is updated with; the forest has at least one leaf."""
    return {"first_and_last": first_and_last(counts), "one_pair": one_pair(counts), "random_third": random_third(counts, rng),
            "every_leaf": every_leaf(counts)}


def cells_of(counts, trees, indices, first=0):
    """Where entries land in the leaves buffer."""
    off = fc.offsets_of(counts).astype(np.int64) + first
    return off[np.asarray(trees, dtype=np.int64)] + np.asarray(indices, dtype=np.int64)


def rewritten(counts, trees, indices):
    """(cells of level buffers, roots, node hashes) an update over the entries writes, from the counts alone."""
    nodes = set()
    for t, i in zip(trees, indices):
        t, i = int(t), int(i)
        for l in range(1, tree_height(counts[t]) + 1):
            nodes.add((t, l, i >> l))
    roots = len({t for t, _, _ in nodes})
    return len(nodes) - roots, roots, len(nodes)


def plan_replay(exe, directory, cases):
    """One line per (first_offset, slack, max_count, counts, trees, indices) replayed by tests/c/forest_update_plan_test.cpp: per
    case (H, level cells written, roots written, node hashes); the C test has checked overlap, bounds and ancestry on the way."""
    path = os.path.join(str(directory), "forest_updates.txt")
    with open(path, "w") as f:
        for first, slack, max_count, counts, trees, indices in cases:
            words = [first, slack, max_count, len(counts)] + list(counts) + [len(trees)]
            for t, i in zip(trees, indices):
                words += [t, i]
            f.write(" ".join(str(int(x)) for x in words) + "\n")
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    text = r.stdout.decode()
    assert r.returncode == 0 and "FAIL" not in text and f"ok: {len(cases)} forests" in text, text[-2000:]
    return [tuple(int(x) for x in line.split()) for line in text.splitlines()[: len(cases)]]


def build_update_plan_exe(directory):
    return build_plan_exe(directory, "forest_update_plan_test")


class RawForest:
    """A stored forest built through the raw API into buffers PREFILLED with a guard pattern, so that the cells nobody writes
    (padding, level H, slack) take part in a byte-for-byte comparison.  `leaves` fills the whole leaves buffer: `first` cells in
    front of tree 0 and the slack behind the last tree included, total = its rows."""

    def __init__(self, gpu, leaves, counts, max_count, first=0):
        import vk_merkle_roots_amd as vk
        self.gpu, self.counts, self.ntrees, self.total, self.max_count = gpu, list(counts), len(counts), int(leaves.shape[0]), int(max_count)
        self.H = fp.stride_of(self.total, max_count)
        self.forest_bytes = gpu.forest_tree_bytes(self.total, self.ntrees, max_count)
        assert self.forest_bytes == 32 * fp.stored_cells(self.total, self.ntrees, max_count)
        self.d_leaves = gpu.upload(np.ascontiguousarray(leaves, dtype=np.uint32))
        self.d_off = gpu.upload(fc.offsets_of(counts) + np.uint64(first))
        self.d_forest = gpu.upload(np.full(self.forest_bytes // 4, GUARD, dtype=np.uint32))
        self.d_roots = gpu.upload(np.full(8 * self.ntrees, GUARD, dtype=np.uint32))
        self.d_status = gpu.upload(np.full(1, 0xDEADBEEF, dtype=np.uint32))
        gpu.reduce_forest_tree_async(self.d_leaves, self.total, self.d_off, self.ntrees, max_count, self.d_forest, self.d_roots, self.d_status)
        assert int(gpu.download(self.d_status, 4)[0]) == 0
        self.handle = vk.MerkleForest(gpu, self.d_leaves, self.total, counts, self.d_off, max_count, self.d_forest, self.d_roots)

    def update(self, trees, indices, new):
        """The raw update of sorted entries; the status word, prefilled with 0xDEADBEEF."""
        gpu = self.gpu
        bufs = [gpu.upload(np.ascontiguousarray(trees, dtype=np.uint32)), gpu.upload(np.ascontiguousarray(indices, dtype=np.uint64)),
                gpu.upload(np.ascontiguousarray(new, dtype=np.uint32)), gpu.upload(np.full(1, 0xDEADBEEF, dtype=np.uint32))]
        self.handle.update_async(bufs[0], bufs[1], bufs[2], len(trees), bufs[3])
        status = int(gpu.download(bufs[3], 4)[0])
        for b in bufs:
            b.free()
        return status

    def state(self):
        """(leaves, forest buffer, roots) as they lie in device memory, every cell."""
        gpu = self.gpu
        return (gpu.download(self.d_leaves, 32 * self.total), gpu.download(self.d_forest, self.forest_bytes),
                gpu.download(self.d_roots, 32 * self.ntrees))

    def free(self):
        for b in (self.d_leaves, self.d_off, self.d_forest, self.d_roots, self.d_status):
            b.free()


def same_state(got, want):
    return all(a.shape == b.shape and (a == b).all() for a, b in zip(got, want))
