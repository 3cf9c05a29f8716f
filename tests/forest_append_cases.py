"""Stored forests that grow (vkmr_hip_forest_append_async, vkmr_hip_forest_truncate_async, MerkleForest.append): the split
points, the brute-force count of what an append must write and the raw-API growth between guard patterns that
tests/test_forest_append_abi.py (no GPU) and tests/test_gpu_forest_append.py share.  A plain module: no fixtures, no GPU.

A case is a list of tree sizes and a split point s: trees 0 .. s - 1 are resident in a forest built with room for the rest,
trees s .. are appended."""
import os
import subprocess

import numpy as np

import forest_cases as fc
import forest_update_cases as fu
from merkle_model import build_plan_exe, tree_height

GUARD = fu.GUARD
STATUS_FILL = 0xDEADBEEF


def split_points(ntrees):
    """The split points every case is grown from: nothing resident, one tree, half of them, all but the last."""
    return sorted({s for s in (0, 1, ntrees // 2, ntrees - 1) if 0 <= s < ntrees})


def written(counts, split):
    """(cells of level buffers, roots) an append of trees split.. writes, from the counts alone."""
    cells = 0
    for c in counts[split:]:
        for l in range(1, tree_height(c) if c else 0):
            cells += ((c - 1) >> l) + 1
    return cells, len(counts) - split


def plan_replay(exe, directory, cases):
    """One line per (first_offset, slack, max_count, split, counts) replayed by tests/c/forest_append_plan_test.cpp: per case
    (H, level cells written, roots written, lanes launched); the C test has checked coverage, overlap and bounds on the way."""
    path = os.path.join(str(directory), "forest_appends.txt")
    with open(path, "w") as f:
        for first, slack, max_count, split, counts in cases:
            f.write(" ".join(str(int(x)) for x in [first, slack, max_count, split] + list(counts)) + "\n")
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    text = r.stdout.decode()
    assert r.returncode == 0 and "FAIL" not in text and f"ok: {len(cases)} forests" in text, text[-2000:]
    return [tuple(int(x) for x in line.split()) for line in text.splitlines()[: len(cases)]]


def build_append_plan_exe(directory):
    return build_plan_exe(directory, "forest_append_plan_test")


def guarded(leaves, used_end):
    """The leaves buffer of a forest whose leaves end at cell used_end: `leaves` in front, the guard pattern behind."""
    out = np.array(leaves, dtype=np.uint32, copy=True)
    out[used_end:] = GUARD
    return out


class Growing:
    """A stored forest of CAPACITY len(counts) trees and leaves.shape[0] cells of which trees 0 .. split - 1 are resident, built
    through the raw API between guard patterns (fu.RawForest), and grown through HipDevice.forest_append_enqueue.  `leaves` is
    the whole leaves buffer as it will be when every tree is there: `first` cells in front of tree 0, the slack behind the
    last tree; the cells behind the resident leaves start as the guard pattern."""

    def __init__(self, gpu, leaves, counts, max_count, split, first=0):
        self.gpu, self.leaves, self.counts, self.max_count, self.first = gpu, np.asarray(leaves, dtype=np.uint32), list(counts), max_count, first
        self.ntrees, self.total = len(counts), int(self.leaves.shape[0])
        self.used_trees = split
        self.raw = fu.RawForest(gpu, guarded(self.leaves, self.used), self.counts_now(), max_count, first=first)
        self.d_mutated = gpu.upload(np.full(self.ntrees, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64))

    def counts_now(self):
        return self.counts[: self.used_trees] + [0] * (self.ntrees - self.used_trees)

    @property
    def used(self):
        return self.first + sum(self.counts[: self.used_trees])

    def append_raw(self, first_tree, used, leaves, new_offsets, m=None, in_place=False, mutated=False):
        """One raw append with exactly these arguments; the status word, prefilled with 0xDEADBEEF.  in_place: the leaves are
        copied to digests + used by the caller first and handed over as that address."""
        gpu, raw = self.gpu, self.raw
        leaves = np.ascontiguousarray(leaves, dtype=np.uint32).reshape(-1, 8)
        new_offsets = np.ascontiguousarray(new_offsets, dtype=np.uint64)
        m = new_offsets.shape[0] - 1 if m is None else m
        d_off, d_status = gpu.upload(new_offsets), gpu.upload(np.full(1, STATUS_FILL, dtype=np.uint32))
        d_new = None
        if in_place:
            where = self.put_leaves(used, leaves)
        else:
            d_new = gpu.upload(leaves) if leaves.shape[0] else None
            where = d_new
        gpu.forest_append_enqueue(raw.d_leaves, raw.d_forest, self.total, raw.d_off, self.ntrees, self.max_count, first_tree, used, where,
                                  leaves.shape[0], d_off, m, raw.d_roots, self.d_mutated if mutated else None, d_status)
        status = int(gpu.download(d_status, 4)[0])
        for b in (d_off, d_status, d_new):
            if b:
                b.free()
        return status

    def put_leaves(self, cell, leaves):
        """`leaves` copied into the leaves buffer from cell `cell` on, as a caller who maps into level 0 does; that address."""
        where = self.raw.d_leaves.at(32 * cell)
        if leaves.shape[0]:
            self.gpu._call("vkmr_hip_memcpy_h2d_async", where, leaves.ctypes.data, leaves.nbytes)
            self.gpu.sync()
        return where

    def append_next(self, m, in_place=False, mutated=False):
        """The next m trees of the case appended; the status word."""
        lo, hi = self.used_trees, self.used_trees + m
        used = self.used
        n = sum(self.counts[lo:hi])
        status = self.append_raw(lo, used, self.leaves[used: used + n], fc.offsets_of(self.counts[lo:hi]), in_place=in_place, mutated=mutated)
        if status == 0:
            self.used_trees = hi
        return status

    def truncate(self, keep_trees):
        self.gpu.forest_truncate_enqueue(self.raw.d_off, self.ntrees, keep_trees, self.raw.d_roots)
        self.gpu.sync()
        self.used_trees = keep_trees

    def state(self):
        """(leaves, forest buffer, roots, offsets, masks) as they lie in device memory, every cell."""
        gpu = self.gpu
        return (*self.raw.state(), gpu.download(self.raw.d_off, 8 * (self.ntrees + 1), dtype=np.uint64),
                gpu.download(self.d_mutated, 8 * self.ntrees, dtype=np.uint64))

    def fresh_state(self):
        """(leaves, forest buffer, roots, offsets) of a fresh build, between the same guard patterns, over the trees in use now."""
        fresh = fu.RawForest(self.gpu, guarded(self.leaves, self.used), self.counts_now(), self.max_count, first=self.first)
        state = (*fresh.state(), self.gpu.download(fresh.d_off, 8 * (self.ntrees + 1), dtype=np.uint64))
        fresh.free()
        return state

    def free(self):
        self.raw.free()
        self.d_mutated.free()


def assert_same(got, want, note):
    for what, a, b in zip(("leaves", "forest", "roots", "offsets"), got, want):
        assert a.shape == b.shape and (a == b).all(), (note, what, np.nonzero(a != b)[0][:8])
