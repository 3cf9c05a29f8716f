"""The diff of two stored forests or trees of one shape (vkmr_hip_forest_diff_async, vkmr_hip_tree_diff_async, MerkleForest.diff,
MerkleTree.diff): the model, the forests, the change sets and the raw-API build that tests/test_diff_abi.py (no GPU) and
tests/test_gpu_diff.py share.  A plain module: no fixtures, no GPU.

The model is the rule on the leaves: numpy's any(a != b, axis=1) over the cells of the trees, turned into sorted (tree, index)
pairs.  The counters come from the counts alone: forest_update_cases.rewritten gives the trees touched and the distinct
ancestors (t, l, i >> l), 1 <= l <= h_t, which is what a descent that visits the changed paths and nothing else compares."""
import functools
import os
import re
import subprocess
import zlib

import numpy as np

import forest_cases as fc
import forest_update_cases as fu
from merkle_model import ROOT, build_plan_exe, random_leaves

OVERFLOW = 4                                   # status bit 2: more than `capacity` leaves differ

# name -> (first offset, slack behind the last tree, max_count or None for the largest count, counts)
FORESTS = {name: (0, 0, None, counts) for name, counts in fc.CASES.items()}
FORESTS.update({
    "window": (5, 7, None, [9, 0, 33, 1, 64, 100]),                 # cells in front of tree 0 and behind the last tree are no leaves
    "max_count_below_total": (0, 0, 200, [40, 3, 70, 129]),         # H = 8 above every tree's own height: every tree's leaves are carried
    "tiny_trees": (0, 0, None, [1, 2, 3, 5]),
    "empty_both_ends": (0, 0, None, [0, 0, 6, 11, 0]),
    "side_by_side": (0, 0, None, [7, 150, 20]),                     # the mask word's edge: 32 entries
    "twenty_thousand": (0, 0, None, [3, 20000, 5]),                 # the ranking's second block: 8192 entries
})
SIDE_BY_SIDE = (31, 32, 33, 63, 64, 65)
BLOCK_EDGE = (8191, 8192, 8193)
COMMON_SETS = ("none", "one_leaf", "first_and_last", "one_pair", "random_third", "every_leaf", "odd_last", "siblings_swapped", "one_whole_tree")


def seed_of(*what):
    return zlib.crc32(repr(what).encode())


def shape_of(name):
    """(first, slack, max_count, counts, total) of a forest of the table."""
    first, slack, max_count, counts = FORESTS[name]
    if max_count is None:
        max_count = max(max(counts), 1)
    return first, slack, max_count, list(counts), first + sum(counts) + slack


def entries_of(name, change):
    """(trees uint32, indices uint64), sorted, of the leaves the change set names in the forest -- or None when the forest has
    no such leaves (no leaf at all, no odd tree, no tree of two leaves)."""
    counts = shape_of(name)[3]
    rng = np.random.default_rng(seed_of("entries", name, change))
    if change == "none":
        return fu.sorted_entries([])
    if sum(counts) == 0:
        return None
    if change == "one_leaf":
        every = fu.every_leaf(counts)
        j = int(rng.integers(0, every[0].shape[0]))
        return every[0][j: j + 1], every[1][j: j + 1]
    if change in ("first_and_last", "one_pair", "random_third", "every_leaf"):
        return fu.update_sets(counts, rng)[change]
    if change == "odd_last":                   # the path through the duplicated nodes: leaf 4 of 5 must come out alone
        pairs = [(t, c - 1) for t, c in enumerate(counts) if c % 2]
        return fu.sorted_entries(pairs) if pairs else None
    if change == "siblings_swapped":           # leaves 2j and 2j + 1 of the largest tree trade places
        t = int(np.argmax(counts))
        if counts[t] < 2:
            return None
        j = int(rng.integers(0, counts[t] // 2))
        return fu.sorted_entries([(t, 2 * j), (t, 2 * j + 1)])
    if change == "one_whole_tree":             # every leaf of one tree and none of its neighbours'
        live = [t for t, c in enumerate(counts) if c]
        t = live[len(live) // 2]
        return fu.sorted_entries([(t, i) for i in range(counts[t])])
    m = re.fullmatch(r"run_of_(\d+)", change)  # that many leaves side by side in the largest tree, from leaf 1 on
    t = int(np.argmax(counts))
    return fu.sorted_entries([(t, 1 + i) for i in range(int(m.group(1)))])


def sets_of(name):
    extra = {"side_by_side": SIDE_BY_SIDE, "twenty_thousand": BLOCK_EDGE}.get(name, ())
    names = [c for c in COMMON_SETS if entries_of(name, c) is not None]
    return names + [f"run_of_{n}" for n in extra]


PAIRS = [(name, change) for name in sorted(FORESTS) for change in sets_of(name)]
SMALL_PAIRS = [(name, change) for name, change in PAIRS if shape_of(name)[4] <= 6000]


def model(a, b, offsets):
    """(trees uint32, indices uint64): the leaves of the trees at `offsets` in which the cell arrays a and b differ."""
    offsets = np.asarray(offsets, dtype=np.int64)
    if offsets.shape[0] < 2:
        return np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint64)
    lo, hi = int(offsets[0]), int(offsets[-1])
    flat = np.nonzero(np.any(a[lo:hi] != b[lo:hi], axis=1))[0] + lo
    trees = np.searchsorted(offsets, flat, side="right") - 1          # the last tree that starts at or before the cell: never an empty one
    return trees.astype(np.uint32), (flat - offsets[trees]).astype(np.uint64)


def counters(counts, trees, indices):
    """info_dev of a completed call: (0, n, trees whose roots differ, nodes whose children were compared)."""
    _, roots, nodes = fu.rewritten(counts, trees, indices)
    return 0, int(len(trees)), roots, nodes


class Case:
    """Two leaves buffers a and b of one forest that differ in the leaves a change set names -- and in every cell outside
    the trees --, the model's answer and the counters."""

    def __init__(self, name, change):
        self.name, self.change = name, change
        self.first, self.slack, self.max_count, self.counts, self.total = shape_of(name)
        self.ntrees = len(self.counts)
        self.offsets = fc.offsets_of(self.counts) + np.uint64(self.first)
        rng = np.random.default_rng(seed_of("leaves", name, change))
        self.a = random_leaves(rng, self.total)
        self.b = self.a.copy()
        lo, hi = self.first, self.first + sum(self.counts)
        self.b[:lo] = random_leaves(rng, lo)
        self.b[hi:] = random_leaves(rng, self.total - hi)
        trees, indices = entries_of(name, change)
        cells = fu.cells_of(self.counts, trees, indices, self.first) if len(trees) else np.zeros(0, dtype=np.int64)
        if change == "siblings_swapped":
            self.b[cells] = self.a[cells[::-1]]
        else:                                  # one bit of one word, the word and the bit moving with the entry: all 32 bytes take part
            q = np.arange(cells.shape[0])
            self.b[cells, q % 8] ^= np.uint32(1) << ((5 * q) % 32).astype(np.uint32)
        self.trees, self.indices = model(self.a, self.b, self.offsets)
        assert (self.trees == trees).all() and (self.indices == indices).all()
        self.n = int(self.trees.shape[0])
        self.info = counters(self.counts, self.trees, self.indices)
        self.leaves_b = self.b[cells]
        self.flat = cells - self.first         # the same leaves as one tree over the window's cells

    def window(self, cells):
        return cells[self.first: self.first + sum(self.counts)]

    def plan_line(self, capacity):
        return (self.first, self.slack, self.max_count, capacity, self.counts, self.trees, self.indices)


@functools.lru_cache(maxsize=None)
def case(name, change):
    return Case(name, change)


def tree_counters(count, height, flat):
    """info_dev of a completed tree diff: the ancestors up to `height`, which may be above the count's own."""
    nodes = {(l, int(i) >> l) for i in flat for l in range(1, height + 1)}
    return 0, int(len(flat)), 1 if len(flat) else 0, len(nodes)


# ---- the plan header's text and its replay -------------------------------------------------------------------------------------

def plan_constants():
    text = open(os.path.join(ROOT, "vk_merkle_roots_amd", "csrc", "diff_plan.hpp")).read()
    return {k: int(v) for k, v in re.findall(r"#define (VKMR_DIFF_\w+) (\d+)u", text)}


def up16(n):
    return (n + 15) & ~15


def scratch_bytes(capacity):
    """The layout written out: two frontiers of 8 + 4 bytes an entry, two mask bits per entry and their starts, the block
    words (at least one per workgroup of step 0), the header."""
    c = plan_constants()
    words = -(-capacity // c["VKMR_DIFF_WORD_ENTRIES"])
    blocks = max(-(-words // c["VKMR_DIFF_RANK_BLOCK_WORDS"]), c["VKMR_DIFF_ROOT_GROUPS"])
    return 2 * up16(8 * capacity) + 2 * up16(4 * capacity) + 2 * up16(8 * words) + up16(8 * blocks) + up16(8 * c["VKMR_DIFF_HEADER_WORDS"])


def build_diff_plan_exe(directory, sanitize=False):
    if not sanitize:
        return build_plan_exe(directory, "diff_plan_test")
    exe = os.path.join(str(directory), "diff_plan_test_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "vk_merkle_roots_amd", "csrc"), os.path.join(ROOT, "tests", "c", "diff_plan_test.cpp"), "-o", exe])
    return exe


def plan_replay(exe, directory, lines, file_name="diffs.txt"):
    """One line per (first, slack, max_count, capacity, counts, trees, indices) replayed by tests/c/diff_plan_test.cpp: per
    case (status, n, roots, compared, H); the C test has checked the answer, the order, the reads and the scratch on the way."""
    path = os.path.join(str(directory), file_name)
    with open(path, "w") as f:
        for first, slack, max_count, capacity, counts, trees, indices in lines:
            words = [first, slack, max_count, capacity, len(counts)] + list(counts) + [len(trees)]
            for t, i in zip(trees, indices):
                words += [t, i]
            f.write(" ".join(str(int(x)) for x in words) + "\n")
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    text = r.stdout.decode()
    assert r.returncode == 0 and "FAIL" not in text and f"ok: {len(lines)} forests" in text, text[-2000:]
    return [tuple(int(x) for x in line.split()) for line in text.splitlines()[: len(lines)]]


# ---- the raw build on a device ---------------------------------------------------------------------------------------------------

class RawForest:
    """A stored forest built through the raw API into buffers PREFILLED with `pattern` (forest_update_cases.RawForest's
    manner, the pattern the caller's): the cells nobody writes hold it, so two forests of equal leaves differ there."""

    def __init__(self, gpu, leaves, counts, max_count, first, pattern):
        import vk_merkle_roots_amd as vk
        self.gpu, self.ntrees, self.total = gpu, len(counts), int(leaves.shape[0])
        self.forest_bytes = gpu.forest_tree_bytes(self.total, self.ntrees, max_count)
        self.d_leaves = gpu.upload(np.ascontiguousarray(leaves, dtype=np.uint32)) if self.total else None
        self.d_off = gpu.upload(fc.offsets_of(counts) + np.uint64(first))
        self.d_forest = gpu.upload(np.full(self.forest_bytes // 4, pattern, dtype=np.uint32))
        self.d_roots = gpu.upload(np.full(8 * self.ntrees, pattern, dtype=np.uint32))
        d_status = gpu.upload(np.full(1, 0xDEADBEEF, dtype=np.uint32))
        gpu.reduce_forest_tree_async(self.d_leaves, self.total, self.d_off, self.ntrees, max_count, self.d_forest, self.d_roots, d_status)
        assert int(gpu.download(d_status, 4)[0]) == 0
        d_status.free()
        self.handle = vk.MerkleForest(gpu, self.d_leaves, self.total, counts, self.d_off, max_count, self.d_forest, self.d_roots)

    def state(self):
        """(leaves, forest buffer, roots) as they lie in device memory, every cell."""
        gpu = self.gpu
        return (gpu.download(self.d_leaves, 32 * self.total) if self.total else np.zeros(0, dtype=np.uint32),
                gpu.download(self.d_forest, self.forest_bytes), gpu.download(self.d_roots, 32 * self.ntrees))

    def free(self):
        for b in (self.d_leaves, self.d_off, self.d_forest, self.d_roots):
            if b:
                b.free()
