"""Forests that slide (vkmr_hip_forest_drop_front_async, vkmr_hip_forest_copy_trees_async, MerkleForest.drop_front, append_from,
repacked): the selections, the placements and the raw-API copy between guard patterns that tests/test_forest_repack_abi.py (no
GPU) and tests/test_gpu_forest_repack.py share.  A plain module: no fixtures, no GPU.

A copy case is a source forest (a list of tree sizes), a selection of its trees and a placement in the destination: the first
free tree and the cell `used` where the destination's leaves in use end."""
import os
import subprocess

import numpy as np

import forest_append_cases as fa
import forest_cases as fc
import forest_update_cases as fu
from merkle_model import build_plan_exe, tree_height

GUARD, STATUS_FILL = fa.GUARD, fa.STATUS_FILL
MASK_FILL = 0x5A5A5A5A5A5A5A5A
USED = (0, 1, 5, 64)          # odd shifts: (o_s >> l) and (o_d >> l) part ways at every level
FIRST_TREES = (0, 3)
PLACEMENTS = [(first_tree, used) for first_tree in FIRST_TREES for used in USED]
SRC_FIRST, SRC_SLACK, DST_SLACK, BEHIND = 3, 2, 7, 2


def selections(ntrees):
    """name -> source trees: identity, reversed, a suffix, every other tree, a repeat."""
    last = ntrees - 1
    return {"identity": list(range(ntrees)), "reversed": list(range(ntrees))[::-1], "suffix": list(range(ntrees // 2, ntrees)),
            "every_other": list(range(0, ntrees, 2)), "repeat": [last, 0, last, ntrees // 2, 0]}


def drop_points(ntrees):
    return sorted({k for k in (0, 1, 2, ntrees // 2, ntrees - 1, ntrees) if 0 <= k <= ntrees})


def max_counts(counts, sel, used, first_tree, tight_dst):
    """(src_max_count, dst_max_count): the destination tight and the source loose, or the other way round, so that the
    destination has fewer levels than the source in one and more in the other."""
    chosen = max([counts[t] for t in sel] + [used if first_tree else 0, 1])
    return (2**63, chosen) if tight_dst else (max(1, max(counts)), 2**63)


def written(counts, sel):
    """(leaves, cells of level buffers, roots) a copy of trees `sel` writes, from the counts alone."""
    leaves = cells = 0
    for t in sel:
        c = counts[t]
        leaves += c
        for l in range(1, tree_height(c) if c else 0):
            cells += ((c - 1) >> l) + 1
    return leaves, cells, len(sel)


def build_copy_plan_exe(directory):
    return build_plan_exe(directory, "forest_copy_plan_test")


def _run(exe, path, n, drop):
    r = subprocess.run([exe] + (["--drop"] if drop else []) + [path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    text = r.stdout.decode()
    assert r.returncode == 0 and "FAIL" not in text and f"ok: {n} forests" in text, text[-2000:]
    return [tuple(int(x) for x in line.split()) for line in text.splitlines()[:n]]


def copy_replay(exe, directory, cases):
    """One line per (src_first, src_slack, src_max, first_tree, used, dst_slack, dst_max, behind, sel, counts) replayed by
    tests/c/forest_copy_plan_test.cpp: per case (H_s, H_d, leaves, level cells, roots written, lanes launched); the C test has
    compared every cell of the destination with a brute-force build on the way."""
    path = os.path.join(str(directory), "forest_copies.txt")
    with open(path, "w") as f:
        for *head, sel, counts in cases:
            f.write(" ".join(str(int(x)) for x in list(head) + [len(sel)] + list(sel) + list(counts)) + "\n")
    return _run(exe, path, len(cases), False)


def drop_replay(exe, directory, cases):
    """One line per (first, slack, max_count, counts): every k replayed; per case (H, ntrees)."""
    path = os.path.join(str(directory), "forest_drops.txt")
    with open(path, "w") as f:
        for first, slack, max_count, counts in cases:
            f.write(" ".join(str(int(x)) for x in [first, slack, max_count] + list(counts)) + "\n")
    return _run(exe, path, len(cases), True)


class Source:
    """A stored forest to copy from, built through the raw API (fu.RawForest) at offset SRC_FIRST with slack behind it, and its
    mutation masks in device memory."""

    def __init__(self, gpu, counts, max_count, seed, leaves=None):
        self.gpu, self.counts, self.max_count = gpu, list(counts), max_count
        n = sum(counts)
        self.leaves = fc.random_leaves(SRC_FIRST + n + SRC_SLACK, seed) if leaves is None else leaves
        self.raw = fu.RawForest(gpu, self.leaves, counts, max_count, first=SRC_FIRST)
        self.ntrees, self.total = self.raw.ntrees, self.raw.total
        self.d_mutated = gpu.alloc(8 * self.ntrees)
        gpu.forest_tree_mutated_async(self.raw.d_leaves, self.raw.d_forest, self.total, self.raw.d_off, self.ntrees, max_count, self.d_mutated)
        self.masks = gpu.download(self.d_mutated, 8 * self.ntrees, dtype=np.uint64)
        self.off = fc.offsets_of(counts).astype(np.int64) + SRC_FIRST

    def tree_leaves(self, t):
        return self.leaves[int(self.off[t]): int(self.off[t + 1])]

    def free(self):
        self.raw.free()
        self.d_mutated.free()


class Destination(fa.Growing):
    """A destination forest between guard patterns (fa.Growing): `first_tree` resident trees whose leaves end at cell `used`
    (tree 0 holds them all; with no resident tree the forest begins at offset `used`), then room for the trees `sel` of `src`
    and BEHIND more empty trees, DST_SLACK cells behind the last leaf."""

    def __init__(self, gpu, src, sel, first_tree, used, max_count, seed=77):
        self.src, self.sel, self.first_tree = src, list(sel), first_tree
        resident = [used if t == 0 else 0 for t in range(first_tree)]
        chosen = [src.counts[t] for t in sel]
        head = fc.random_leaves(used, seed)
        parts = [head] + [src.tree_leaves(t) for t in sel] + [fc.random_leaves(DST_SLACK, seed + 1)]
        super().__init__(gpu, np.concatenate(parts), resident + chosen + [0] * BEHIND, max_count, first_tree, first=0 if first_tree else used)

    def copy_raw(self, sel, first_tree, used, new_offsets, n_leaves=None, m=None, flagged=False, src_masks=True):
        """One raw copy with exactly these arguments; the status word, prefilled with 0xDEADBEEF."""
        gpu, raw, src = self.gpu, self.raw, self.src
        sel, new_offsets = np.ascontiguousarray(sel, dtype=np.uint32), np.ascontiguousarray(new_offsets, dtype=np.uint64)
        m = sel.shape[0] if m is None else m
        n_leaves = int(new_offsets[-1]) if n_leaves is None else n_leaves
        d_sel, d_off, d_status = gpu.upload(sel), gpu.upload(new_offsets), gpu.upload(np.full(1, STATUS_FILL, dtype=np.uint32))
        gpu.forest_copy_trees_enqueue(src.raw.d_leaves, src.raw.d_forest, src.total, src.raw.d_off, src.ntrees, src.max_count, src.raw.d_roots,
                                      src.d_mutated if flagged and src_masks else None, d_sel, m, n_leaves, d_off, raw.d_leaves, raw.d_forest,
                                      self.total, raw.d_off, self.ntrees, self.max_count, first_tree, used, raw.d_roots,
                                      self.d_mutated if flagged else None, d_status)
        status = int(gpu.download(d_status, 4)[0])
        for b in (d_sel, d_off, d_status):
            b.free()
        return status

    def copy_all(self, flagged=False, src_masks=True):
        """The case's own copy; the status word."""
        status = self.copy_raw(self.sel, self.first_tree, self.used, fc.offsets_of([self.src.counts[t] for t in self.sel]), flagged=flagged,
                               src_masks=src_masks)
        if status == 0:
            self.used_trees = self.first_tree + len(self.sel)
        return status


def assert_unchanged(after, before, note):
    for what, a, b in zip(("leaves", "forest", "roots", "offsets", "masks"), after, before):
        assert a.shape == b.shape and (a == b).all(), (note, what, np.nonzero(a != b)[0][:8])
