#!/usr/bin/env python3
"""The forest reduction (vkmr_hip_reduce_forest_async) beside the calls a user had before it, timed with HIP events: medians
of interleaved runs in one process, stamped with the build id.  Prints one JSON line (and writes it to --out).  GPU box.
    python3 tools/forest_timing.py [--log2 26] [--runs 10] [--out FILE]

  W1 mixed   2^log2 leaves, tree sizes uniform in [1, 4095] (default_rng(42)), the last tree cut to fit; beside
             vkmr_hip_reduce_levels_async over the same digests as ONE tree (the same node hashes to within ntrees)
  W2 equal   2^(log2 - 11) trees of 2^11; beside vkmr_hip_reduce_slices_async on the same buffer
  W3 small   2^(log2 - 2) leaves in trees of 1..16: node hashes per second beside W1's
  loop       the per-tree vkmr_hip_reduce_async loop over the first 1024 trees of W1 beside one forest call on the same trees"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vk_merkle_roots_amd as vk  # noqa: E402
from vk_merkle_roots_amd.engine import forest_offsets, tree_height  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log2", type=int, default=26)
ap.add_argument("--runs", type=int, default=10)
ap.add_argument("--out", default=None)
a = ap.parse_args()
dev = vk.HipDevice(0)
n = 1 << a.log2
rng = np.random.default_rng(7)
d_in = dev.alloc(32 * n)
chunk = min(n, 1 << 22)
base = rng.integers(0, 2**32, size=(chunk, 8), dtype=np.uint32)
for at in range(0, n, chunk):   # random digests, uploaded in pieces: one random piece, made different per piece
    part = base ^ np.uint32(at // chunk * 2654435761 & 0xFFFFFFFF)
    vk.check(dev.lib.vkmr_hip_memcpy_h2d_async(dev.index, dev.stream, d_in.at(32 * at), part.ctypes.data, part.nbytes), "h2d")
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
    h = np.maximum(1, np.frexp(c - 1)[1]).astype(np.int64)      # bit_length(c - 1), at least 1: engine.tree_height
    for l in range(1, int(h.max()) + 1):
        level = (level + 1) // 2
        total += int(level[h >= l].sum())
    return total


class Forest:
    def __init__(self, counts, total, max_count):
        self.counts, self.total, self.max_count = counts, total, max_count
        self.offsets, self.ntrees = forest_offsets(counts)
        self.d_off = dev.upload(self.offsets)
        self.d_scr = dev.alloc(dev.lib.vkmr_hip_forest_scratch_bytes(total, self.ntrees))
        self.d_roots, self.d_status = dev.alloc(32 * self.ntrees), dev.alloc(4)

    def run(self):
        dev.reduce_forest_async(d_in, self.total, self.d_off, self.ntrees, self.max_count, self.d_scr, self.d_roots, self.d_status)

    def roots(self):
        assert int(dev.download(self.d_status, 4)[0]) == 0
        return dev.download(self.d_roots, 32 * self.ntrees).reshape(-1, 8)


w1_counts = cut_to_fit(np.random.default_rng(42).integers(1, 4096, size=n // 1024 + 16), n)
w1 = Forest(w1_counts, n, 4095)
cap = 1 << 11
w2_trees = max(1, n // cap)
w2 = Forest([min(cap, n)] * w2_trees, n, cap)
n3 = max(16, n >> 2)
w3_counts = cut_to_fit(np.random.default_rng(43).integers(1, 17, size=n3 // 4 + 16), n3)
w3 = Forest(w3_counts, n3, 16)
loop_counts = w1_counts[:1024]
loop_total = sum(loop_counts)
w_loop = Forest(loop_counts, loop_total, 4095)

d_lscr, d_lroot = dev.reduce_scratch(n, levels_variant=True), dev.alloc(32)
d_sscr, d_sroots = dev.alloc(dev.lib.vkmr_hip_reduce_slices_scratch_bytes(cap, w2_trees)), dev.alloc(32 * w2_trees)
d_oscr, d_oroots = dev.reduce_scratch(4095), dev.alloc(32 * len(loop_counts))
loop_offsets = [int(x) for x in w_loop.offsets]
loop_heights = [tree_height(c) for c in loop_counts]


def levels_one_tree():
    dev.reduce_async(d_in, n, a.log2, d_lscr, d_lroot, levels_variant=True)


def slices():
    dev.reduce_slices_async(d_in, w2_trees, min(cap, n), min(cap, n), tree_height(min(cap, n)), d_sscr, d_sroots)


def per_tree_loop():
    fn, idx, s = dev.lib.vkmr_hip_reduce_async, dev.index, dev.stream
    for t, c in enumerate(loop_counts):
        fn(idx, s, d_in.ptr + 32 * loop_offsets[t], c, loop_heights[t], d_oscr.ptr, d_oroots.ptr + 32 * t)


forms = [("levels_one_tree", levels_one_tree), ("forest_w1_mixed", w1.run), ("slices_w2_equal", slices), ("forest_w2_equal", w2.run),
         ("forest_w3_small", w3.run), ("reduce_async_loop_1024", per_tree_loop), ("forest_1024", w_loop.run)]
# warm up until the clocks have settled, then every form in turn, run after run (tree_proofs_timing.py: a form timed alone
# is compared across a clock that drifts by several per cent)
for _ in range(10):
    levels_one_tree(); w1.run()
for _, fn in forms:
    fn()
dev.sync()
ev = {name: [(dev.new_event(), dev.new_event()) for _ in range(a.runs)] for name, _ in forms}
for r in range(a.runs):
    for name, fn in forms:
        e0, e1 = ev[name][r]
        dev.record(e0); fn(); dev.record(e1)
dev.sync()
ms = {name: float(np.median([dev.elapsed_ms(e0, e1) for e0, e1 in v])) for name, v in ev.items()}
# correctness of what was timed: the equal forest against the slices call, the 1024 trees against the loop and against W1
w1_roots = w1.roots()
ok = {"w2_equals_slices": bool((w2.roots() == dev.download(d_sroots, 32 * w2_trees).reshape(-1, 8)).all()),
      "loop_equals_forest": bool((w_loop.roots() == dev.download(d_oroots, 32 * len(loop_counts)).reshape(-1, 8)).all()),
      "w1_first_1024_equal": bool((w1_roots[: len(loop_counts)] == w_loop.roots()).all()),
      "w3_status_ok": bool(w3.roots().shape[0] == w3.ntrees)}
out = {"tool": "forest_timing", "leaves_log2": a.log2, "runs": a.runs, "ms": {k: round(v, 4) for k, v in ms.items()}, "checks": ok,
       "w1": {"ntrees": w1.ntrees, "node_hashes": node_hashes(w1_counts)}, "w2": {"ntrees": w2.ntrees, "node_hashes": node_hashes(w2.counts)},
       "w3": {"ntrees": w3.ntrees, "leaves": n3, "node_hashes": node_hashes(w3_counts)}, "loop": {"ntrees": len(loop_counts), "leaves": loop_total},
       "device": dev.name(), "kernel_info": dev.lib.vkmr_hip_kernel_info().decode()}
out["w1_vs_levels_one_tree"] = ms["forest_w1_mixed"] / ms["levels_one_tree"]
out["w1_target_1.10_met"] = out["w1_vs_levels_one_tree"] <= 1.10
out["w2_vs_slices"] = ms["forest_w2_equal"] / ms["slices_w2_equal"]
out["w2_target_1.10_met"] = out["w2_vs_slices"] <= 1.10
out["w1_node_hashes_per_s"] = out["w1"]["node_hashes"] / (ms["forest_w1_mixed"] * 1e-3)
out["w3_node_hashes_per_s"] = out["w3"]["node_hashes"] / (ms["forest_w3_small"] * 1e-3)
out["levels_one_tree_node_hashes_per_s"] = (n - 1) / (ms["levels_one_tree"] * 1e-3)
out["loop_vs_forest_1024"] = ms["reduce_async_loop_1024"] / ms["forest_1024"]
line = json.dumps(out)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
