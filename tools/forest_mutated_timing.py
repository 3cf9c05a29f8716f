#!/usr/bin/env python3
"""What the mutation flag costs (vkmr_hip_reduce_forest_mutated_async beside vkmr_hip_reduce_forest_async, and the scan
vkmr_hip_forest_tree_mutated_async), timed with HIP events: medians of interleaved runs in one process after a warm-up of every
shape, stamped with the build id.  Prints one JSON line (and writes it to --out).  GPU box.
    python3 tools/forest_mutated_timing.py [--log2 26] [--runs 10] [--out profiles/forest_mutated_timing.json]

  W1 mixed   2^log2 leaves, tree sizes uniform in [1, 4095] (default_rng(42)), the last tree cut to fit: tools/forest_timing.py's W1
  W2 equal   2^(log2 - 11) trees of 2^11: its W2
  one tree   one tree of 2^log2 leaves
Each with random leaves, plain and flagged (target: flagged within 5 % of plain on W1 and W2); W2 and the one tree once more with
EVERY LEAF EQUAL -- every lane of every level hits, the case the ballot and the skip-if-set read are there for (a report, no
target).  The scan: the stored W1 built by the flagged twin, then scanned; GB/s over the cells it reads (every node below a root)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vk_merkle_roots_amd as vk  # noqa: E402
from vk_merkle_roots_amd.engine import forest_offsets  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log2", type=int, default=26)
ap.add_argument("--runs", type=int, default=10)
ap.add_argument("--out", default=None)
a = ap.parse_args()
dev = vk.HipDevice(0)
n = 1 << a.log2
rng = np.random.default_rng(7)
d_rand, d_same = dev.alloc(32 * n), dev.alloc(32 * n)
chunk = min(n, 1 << 22)
base = rng.integers(0, 2**32, size=(chunk, 8), dtype=np.uint32)
same = np.tile(base[:1], (chunk, 1))
for at in range(0, n, chunk):   # random digests, uploaded in pieces: one random piece, made different per piece; and one digest everywhere
    part = base ^ np.uint32(at // chunk * 2654435761 & 0xFFFFFFFF)
    for d, src in ((d_rand, part), (d_same, same)):
        vk.check(dev.lib.vkmr_hip_memcpy_h2d_async(dev.index, dev.stream, d.at(32 * at), src.ctypes.data, src.nbytes), "h2d")
        dev.sync()


def cut_to_fit(sizes, total):
    ends = np.cumsum(sizes)
    k = int(np.searchsorted(ends, total))
    counts = [int(c) for c in sizes[:k]]
    if sum(counts) < total:
        counts.append(total - sum(counts))
    return counts


def node_hashes(counts):
    """Hashes of a forest: every node of every level 1..h_t."""
    c = np.asarray(counts, dtype=np.int64)
    c = c[c > 0]
    total, level = 0, c.copy()
    h = np.maximum(1, np.frexp(c - 1)[1]).astype(np.int64)
    for l in range(1, int(h.max()) + 1):
        level = (level + 1) // 2
        total += int(level[h >= l].sum())
    return total


class Forest:
    """One shape: its offsets and, per form, buffers of its own (the forms are interleaved)."""

    def __init__(self, counts, max_count):
        self.counts, self.max_count = counts, max_count
        self.offsets, self.ntrees = forest_offsets(counts)
        self.d_off = dev.upload(self.offsets)
        self.d_scr = dev.alloc(dev.lib.vkmr_hip_forest_scratch_bytes(n, self.ntrees))
        self.d_roots, self.d_froots = dev.alloc(32 * self.ntrees), dev.alloc(32 * self.ntrees)
        self.d_mut, self.d_status = dev.alloc(8 * self.ntrees), dev.alloc(4)

    def plain(self, d_in):
        return lambda: dev.reduce_forest_async(d_in, n, self.d_off, self.ntrees, self.max_count, self.d_scr, self.d_roots, self.d_status)

    def flagged(self, d_in):
        return lambda: dev.reduce_forest_mutated_async(d_in, n, self.d_off, self.ntrees, self.max_count, self.d_scr, self.d_froots, self.d_mut,
                                                       self.d_status)

    def masks(self):
        assert int(dev.download(self.d_status, 4)[0]) == 0
        return dev.download(self.d_mut, 8 * self.ntrees, dtype=np.uint64)

    def roots_agree(self):
        return bool((dev.download(self.d_roots, 32 * self.ntrees) == dev.download(self.d_froots, 32 * self.ntrees)).all())


w1_counts = cut_to_fit(np.random.default_rng(42).integers(1, 4096, size=n // 1024 + 16), n)
w1 = Forest(w1_counts, 4095)
cap = min(n, 1 << 11)
w2 = Forest([cap] * (n // cap), cap)
one = Forest([n], n)
d_forest = dev.alloc(dev.forest_tree_bytes(n, w1.ntrees, 4095))
d_sroots, d_smut, d_scan = dev.alloc(32 * w1.ntrees), dev.alloc(8 * w1.ntrees), dev.alloc(8 * w1.ntrees)


def stored_build():
    dev.reduce_forest_tree_mutated_async(d_rand, n, w1.d_off, w1.ntrees, 4095, d_forest, d_sroots, d_smut, w1.d_status)


def scan():
    dev.forest_tree_mutated_async(d_rand, d_forest, n, w1.d_off, w1.ntrees, 4095, d_scan)


forms = [("plain_w1", w1.plain(d_rand)), ("flagged_w1", w1.flagged(d_rand)), ("plain_w2", w2.plain(d_rand)), ("flagged_w2", w2.flagged(d_rand)),
         ("plain_one_tree", one.plain(d_rand)), ("flagged_one_tree", one.flagged(d_rand)),
         ("plain_w2_all_equal", w2.plain(d_same)), ("flagged_w2_all_equal", w2.flagged(d_same)),
         ("plain_one_tree_all_equal", one.plain(d_same)), ("flagged_one_tree_all_equal", one.flagged(d_same)),
         ("stored_build_flagged_w1", stored_build), ("scan_w1", scan)]
checks = {}
# warm up until the clocks have settled, every shape at least twice; the masks of every form are checked here, where each form's
# buffers still hold its own result
for _ in range(5):
    w1.plain(d_rand)(); w1.flagged(d_rand)()
for _ in range(2):
    for _, fn in forms:
        fn()
dev.sync()
for shape, name in ((w1, "w1"), (w2, "w2"), (one, "one_tree")):
    shape.plain(d_rand)(); shape.flagged(d_rand)()
    checks[name + "_random_masks_zero"] = bool(not shape.masks().any())
    checks[name + "_roots_agree"] = shape.roots_agree()
for shape, name, want in ((w2, "w2", cap - 1), (one, "one_tree", n - 1)):
    shape.plain(d_same)(); shape.flagged(d_same)()
    checks[name + "_all_equal_masks_full"] = bool((shape.masks() == np.uint64(want)).all())
    checks[name + "_all_equal_roots_agree"] = shape.roots_agree()
stored_build(); scan()
checks["scan_equals_build"] = bool((dev.download(d_scan, 8 * w1.ntrees, dtype=np.uint64) == dev.download(d_smut, 8 * w1.ntrees, dtype=np.uint64)).all())
dev.sync()
ev = {name: [(dev.new_event(), dev.new_event()) for _ in range(a.runs)] for name, _ in forms}
for r in range(a.runs):
    for name, fn in forms:
        e0, e1 = ev[name][r]
        dev.record(e0); fn(); dev.record(e1)
dev.sync()
samples = {name: [dev.elapsed_ms(e0, e1) for e0, e1 in v] for name, v in ev.items()}
ms = {name: float(np.median(v)) for name, v in samples.items()}
scan_bytes = 32 * (n + node_hashes(w1_counts) - w1.ntrees)      # every node below a root, once
out = {"tool": "forest_mutated_timing", "leaves_log2": a.log2, "runs": a.runs, "ms": {k: round(v, 4) for k, v in ms.items()},
       "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in samples.items()}, "checks": checks,
       "w1": {"ntrees": w1.ntrees, "node_hashes": node_hashes(w1_counts)}, "w2": {"ntrees": w2.ntrees, "node_hashes": node_hashes(w2.counts)},
       "device": dev.name(), "kernel_info": dev.lib.vkmr_hip_kernel_info().decode()}
for w in ("w1", "w2", "one_tree", "w2_all_equal", "one_tree_all_equal"):
    out[f"flagged_vs_plain_{w}"] = ms[f"flagged_{w}"] / ms[f"plain_{w}"]
out["w1_target_1.05_met"] = out["flagged_vs_plain_w1"] <= 1.05
out["w2_target_1.05_met"] = out["flagged_vs_plain_w2"] <= 1.05
out["scan_w1_bytes"] = scan_bytes
out["scan_w1_GB_per_s"] = scan_bytes / (ms["scan_w1"] * 1e-3) / 1e9
out["scan_vs_stored_build_w1"] = ms["scan_w1"] / ms["stored_build_flagged_w1"]
line = json.dumps(out)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
