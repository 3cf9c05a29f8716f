"""The open tree of a stored forest grown or shrunk by leaves (vkmr_hip_forest_extend_async, vkmr_hip_forest_shrink_async,
MerkleForest.extend / shrink): the (c -> c') tables, the CPU replay's driver and the raw-API forest between guard patterns that
tests/test_forest_extend_abi.py (no GPU) and tests/test_gpu_forest_extend.py share.  A plain module: no fixtures, no GPU.

A case is the trees in front, the open tree's count before and after, and the number of empty trees behind it."""
import os
import subprocess

import numpy as np

import forest_append_cases as fa
import forest_cases as fc
import forest_update_cases as fu
from merkle_model import build_plan_exe

GUARD, STATUS_FILL = fa.GUARD, fa.STATUS_FILL
MASK_FILL = 0x5A5A5A5A5A5A5A5A

# The smallest shapes that can go wrong, as extends; each is also run the other way round, as a shrink.
GROW = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3),                                          # from empty or one leaf
        (2, 3), (2, 5), (3, 4), (4, 5), (4, 8), (4, 9), (5, 6), (5, 7), (7, 8),          # two to nine leaves: the lone-node levels
        (63, 64), (63, 130), (64, 65), (127, 129), (128, 129),                           # around the wavefront edge
        (1024, 1025)]                                                                    # height 10 -> 11
TO_NOTHING = sorted({c for pair in GROW for c in pair if c})                             # c -> 0
PAIRS = GROW + [(b, a) for a, b in GROW if a] + [(c, 0) for c in TO_NOTHING]
FRONT = [1, 1, 3]                                                                        # the open tree is tree 3 at offset 5
THREE = [(2, 3), (63, 130), (4, 8), (3, 2), (130, 63), (8, 4)]                           # repeated in the two further settings


def build_extend_plan_exe(directory):
    return build_plan_exe(directory, "forest_extend_plan_test")


def run_replay(exe, directory, cases, plain=False):
    """One line per (first_offset, slack, max_count, behind, c, c2, front counts) through tests/c/forest_extend_plan_test.cpp:
    (return code, output)."""
    path = os.path.join(str(directory), "forest_extends.txt")
    with open(path, "w") as f:
        for first, slack, max_count, behind, c, c2, front in cases:
            f.write(" ".join(str(int(x)) for x in [first, slack, max_count, behind, c, c2] + list(front)) + "\n")
    r = subprocess.run([exe] + (["--plain"] if plain else []) + [path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    return r.returncode, r.stdout.decode()


def plan_replay(exe, directory, cases):
    """Per case (H, level cells written, roots written, lanes launched); the C test has checked the nodes written, the reads, the
    values against a fresh build and the lanes per level on the way."""
    rc, text = run_replay(exe, directory, cases)
    assert rc == 0 and "FAIL" not in text and f"ok: {len(cases)} forests" in text, text[-2000:]
    return [tuple(int(x) for x in line.split()) for line in text.splitlines()[: len(cases)]]


def dirty(c, c2, l):
    """(first node, end node) of the open tree's level l >= 1 that a call from c to c2 leaves must write to the level buffer or
    the root, from the counts alone: the rule of the issue, with Python's integers."""
    cnt = lambda x, k: 0 if x == 0 else ((x - 1) >> k) + 1
    if c2 == 0:
        return (0, 1) if l == 1 else (0, 0)
    if l > 1 and cnt(c2, l - 1) == 1:
        return 0, 0
    first = 0 if cnt(c, l) <= 1 or cnt(c2, l) <= 1 else min(c, c2) >> l
    return first, cnt(c2, l)


class Open:
    """A stored forest of trees `front`, the open tree of c leaves and `behind` empty trees, built through the raw API between
    guard patterns (fu.RawForest) over a leaves buffer of leaves.shape[0] cells, and driven through HipDevice.forest_extend_enqueue
    and forest_shrink_enqueue.  `leaves` is the whole buffer as it is when the tree is largest; the cells behind the leaves in
    use start as the guard pattern."""

    def __init__(self, gpu, leaves, front, c, behind, max_count):
        self.gpu, self.leaves, self.front, self.c, self.behind, self.max_count = gpu, np.asarray(leaves, dtype=np.uint32), list(front), c, behind, max_count
        self.tree, self.o, self.ntrees, self.total = len(front), sum(front), len(front) + 1 + behind, int(self.leaves.shape[0])
        self.raw = fu.RawForest(gpu, fa.guarded(self.leaves, self.used), self.counts_now(), max_count)
        self.d_mutated = gpu.upload(np.full(self.ntrees, MASK_FILL, dtype=np.uint64))

    def counts_now(self):
        return self.front + [self.c] + [0] * self.behind

    @property
    def used(self):
        return self.o + self.c

    def put_leaves(self, cell, leaves):
        """`leaves` copied into the leaves buffer from cell `cell` on, as a caller who maps into level 0 does; that address."""
        where = self.raw.d_leaves.at(32 * cell)
        if leaves.shape[0]:
            self.gpu._call("vkmr_hip_memcpy_h2d_async", where, leaves.ctypes.data, leaves.nbytes)
            self.gpu.sync()
        return where

    def extend_raw(self, tree, count, used, leaves, in_place=False, mutated=False):
        """One raw extend with exactly these arguments; the status word, prefilled with 0xDEADBEEF."""
        gpu, raw = self.gpu, self.raw
        leaves = np.ascontiguousarray(leaves, dtype=np.uint32).reshape(-1, 8)
        d_status = gpu.upload(np.full(1, STATUS_FILL, dtype=np.uint32))
        d_new = None if in_place else gpu.upload(leaves)
        where = self.put_leaves(used, leaves) if in_place else d_new
        gpu.forest_extend_enqueue(raw.d_leaves, raw.d_forest, self.total, raw.d_off, self.ntrees, self.max_count, tree, count, used, where,
                                  leaves.shape[0], raw.d_roots, self.d_mutated if mutated else None, d_status)
        status = int(gpu.download(d_status, 4)[0])
        for b in (d_status, d_new):
            if b:
                b.free()
        return status

    def shrink_raw(self, tree, count, used, r, mutated=False):
        gpu, raw = self.gpu, self.raw
        d_status = gpu.upload(np.full(1, STATUS_FILL, dtype=np.uint32))
        gpu.forest_shrink_enqueue(raw.d_leaves, raw.d_forest, self.total, raw.d_off, self.ntrees, self.max_count, tree, count, used, r, raw.d_roots,
                                  self.d_mutated if mutated else None, d_status)
        status = int(gpu.download(d_status, 4)[0])
        d_status.free()
        return status

    def go(self, c2, in_place=False, mutated=False):
        """The open tree taken from its count to c2 leaves, by the next leaves of the case or by dropping; the status word."""
        if c2 >= self.c:
            status = self.extend_raw(self.tree, self.c, self.used, self.leaves[self.used: self.o + c2], in_place=in_place, mutated=mutated)
        else:
            status = self.shrink_raw(self.tree, self.c, self.used, self.c - c2, mutated=mutated)
        if status == 0:
            self.c = c2
        return status

    def state(self):
        """(leaves, forest buffer, roots, offsets, masks) as they lie in device memory, every cell."""
        gpu = self.gpu
        return (*self.raw.state(), gpu.download(self.raw.d_off, 8 * (self.ntrees + 1), dtype=np.uint64),
                gpu.download(self.d_mutated, 8 * self.ntrees, dtype=np.uint64))

    def fresh_state(self):
        """(leaves, forest buffer, roots, offsets) of a fresh build, between the same guard patterns, over the counts as they are."""
        fresh = fu.RawForest(self.gpu, fa.guarded(self.leaves, self.used), self.counts_now(), self.max_count)
        state = (*fresh.state(), self.gpu.download(fresh.d_off, 8 * (self.ntrees + 1), dtype=np.uint64))
        fresh.free()
        return state

    def free(self):
        self.raw.free()
        self.d_mutated.free()


def assert_as_fresh(got, before, fresh, used, note):
    """The state after a call against a fresh build of the final counts: the leaves in use, the offsets, the roots and every cell
    of the forest buffer that the fresh build writes are the fresh build's; every other cell -- the guard pattern in the fresh
    build: free leaves, padding, the cells of dropped nodes -- is what it was before the call."""
    leaves, b_leaves, f_leaves = (x[0].reshape(-1, 8) for x in (got, before, fresh))
    assert (leaves[:used] == f_leaves[:used]).all(), (note, "leaves in use")
    assert (leaves[used:] == b_leaves[used:]).all(), (note, "free leaves")
    cells, b_cells, f_cells = (x[1].reshape(-1, 8) for x in (got, before, fresh))
    unwritten = (f_cells == GUARD).all(axis=1)
    want = np.where(unwritten[:, None], b_cells, f_cells)
    assert (cells == want).all(), (note, "forest", np.nonzero((cells != want).any(axis=1))[0][:8])
    for what, a, b in zip(("roots", "offsets"), got[2:4], fresh[2:4]):
        assert a.shape == b.shape and (a == b).all(), (note, what)
    if len(got) > 4 and len(before) > 4:
        assert (got[4] == before[4]).all(), (note, "masks")
