#!/usr/bin/env python3
"""Leaf updates of a stored forest (vkmr_hip_forest_update_async) beside the two things they are measured against, timed with
HIP events: medians of interleaved runs in one process after a warm-up of every shape, stamped with the build id.  Prints one
JSON line (and writes it to --out).  GPU box.
    python3 tools/forest_update_timing.py [--log2 26] [--ks 0,10,16,20] [--runs 10] [--out FILE]

  W2 equal   2^(log2 - 11) trees of 2^11 (H = 11)
  W1 mixed   tree sizes uniform in [1, 4095] (default_rng(42)), the last tree cut to fit (H = 12): forest_timing.py's W1
  update     k random entries (k distinct cells of the leaves, as sorted (tree, index) pairs), and about 2^16 entries that fill
             whole consecutive trees
  (a)        the rebuild of the same forest, vkmr_hip_reduce_forest_tree_async
  (b)        vkmr_hip_tree_update_async with the same k, at the same cells, on ONE stored tree over the same leaves (height log2)
Every update leg reports ms, the distinct nodes it rehashes (counted on the host) and its ratios to (a) and (b); (b)'s spread
(max / median over the interleaved runs) is the margin the comparison with (b) is read with.  After the timing every update
shape is applied once more to a freshly built forest and the roots are compared with those of a fresh build over the leaves
it left."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vk_merkle_roots_amd as vk  # noqa: E402
from vk_merkle_roots_amd import provenance  # noqa: E402
from vk_merkle_roots_amd.engine import forest_offsets  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log2", type=int, default=26)
ap.add_argument("--ks", default="0,10,16,20", help="log2 of the random entry counts")
ap.add_argument("--whole-log2", type=int, default=16, help="log2 of the entries that fill whole trees")
ap.add_argument("--runs", type=int, default=10)
ap.add_argument("--out", default=None)
a = ap.parse_args()
dev = vk.HipDevice(0)
n, height = 1 << a.log2, a.log2
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


def distinct_cells(k):
    """k distinct cells of the leaves, sorted."""
    if k >= n:
        return np.arange(n, dtype=np.int64)
    u = np.unique(rng.integers(0, n, size=k + k // 8 + 16))
    while u.shape[0] < k:
        u = np.unique(np.concatenate([u, rng.integers(0, n, size=k)]))
    return np.sort(rng.choice(u, size=k, replace=False)).astype(np.int64)


ks = [min(1 << int(x), n) for x in a.ks.split(",")]
random_cells = {k: distinct_cells(k) for k in ks}
d_status = dev.alloc(4)


class Leg:
    """One update shape: the entries on the device, the nodes it rehashes."""

    def __init__(self, trees, indices, nodes):
        self.k, self.nodes = int(indices.shape[0]), nodes
        self.d_trees = dev.upload(np.ascontiguousarray(trees, dtype=np.uint32)) if trees is not None else None
        self.d_idx = dev.upload(np.ascontiguousarray(indices, dtype=np.uint64))
        self.d_new = dev.upload(rng.integers(0, 2**32, size=(self.k, 8), dtype=np.uint32))


class Forest:
    def __init__(self, counts, max_count):
        self.counts, self.max_count = np.asarray(counts, dtype=np.int64), max_count
        self.offsets, self.ntrees = forest_offsets(counts)
        self.off = self.offsets.astype(np.int64)
        self.h = np.maximum(1, np.frexp(np.maximum(self.counts, 1) - 1)[1]).astype(np.int64)   # bit_length(c - 1), at least 1
        self.d_off = dev.upload(self.offsets)
        nbytes = dev.forest_tree_bytes(n, self.ntrees, max_count)
        self.d_forest, self.d_roots = dev.alloc(nbytes), dev.alloc(32 * self.ntrees)
        self.d_forest2, self.d_roots2 = dev.alloc(nbytes), dev.alloc(32 * self.ntrees)     # the fresh build the roots are checked against
        self.handle = vk.MerkleForest(dev, d_in, n, counts, self.d_off, max_count, self.d_forest, self.d_roots)
        self.legs = {}

    def entries(self, cells):
        trees = np.searchsorted(self.off, cells, side="right") - 1
        return trees, cells - self.off[trees]

    def add(self, name, cells):
        trees, indices = self.entries(cells)
        nodes = 0
        for l in range(1, int(self.h.max()) + 1):   # distinct (tree, index >> l) with l <= h_t: the keys are sorted with the cells
            live = self.h[trees] >= l
            key = trees[live] * (1 << 13) + (indices[live] >> l)
            nodes += int(np.unique(key).shape[0])
        self.legs[name] = Leg(trees, indices, nodes)

    def rebuild(self, fresh=False):
        dev.reduce_forest_tree_async(d_in, n, self.d_off, self.ntrees, self.max_count, self.d_forest2 if fresh else self.d_forest,
                                     self.d_roots2 if fresh else self.d_roots, d_status)

    def update(self, name):
        leg = self.legs[name]
        return lambda: self.handle.update_async(leg.d_trees, leg.d_idx, leg.d_new, leg.k, d_status)

    def whole_trees(self, want):
        """The cells of consecutive whole trees from a random tree on, about `want` of them."""
        t0 = int(rng.integers(0, max(1, self.ntrees // 2)))
        t1 = t0
        while t1 < self.ntrees and self.off[t1 + 1] - self.off[t0] < want:
            t1 += 1
        t1 = min(t1 + 1, self.ntrees)
        return np.arange(self.off[t0], self.off[t1], dtype=np.int64)


cap = min(1 << 11, n)
forests = {"w2": Forest([cap] * (n // cap), cap), "w1": Forest(cut_to_fit(np.random.default_rng(42).integers(1, 4096, size=n // 1024 + 16), n), 4095)}
for f in forests.values():
    for k in ks:
        f.add(f"random_k{k}", random_cells[k])
    f.add("whole_trees", f.whole_trees(min(1 << a.whole_log2, n)))

# (b): the single stored tree over the same leaves, the same cells as its indices, and one contiguous run
d_tree = dev.alloc(dev.tree_bytes(n, height))
tree = vk.MerkleTree(dev, d_in, n, height, d_tree)


def tree_nodes(cells):
    return int(sum(np.unique(cells >> l).shape[0] for l in range(1, height + 1)))


tree_legs = {f"random_k{k}": Leg(None, random_cells[k], tree_nodes(random_cells[k])) for k in ks}
run = forests["w2"].legs["whole_trees"].k
start = int(rng.integers(0, n - run + 1))
tree_legs["run"] = Leg(None, np.arange(start, start + run, dtype=np.int64), tree_nodes(np.arange(start, start + run, dtype=np.int64)))


def tree_update(name):
    leg = tree_legs[name]
    return lambda: tree.update_async(leg.d_idx, leg.d_new, leg.k, d_status)


forms = []
for fname, f in forests.items():
    forms.append((f"rebuild_{fname}", f.rebuild))
    forms += [(f"forest_update_{fname}_{name}", f.update(name)) for name in f.legs]
forms += [(f"tree_update_{name}", tree_update(name)) for name in tree_legs]
# everything the timed legs read is formed once, untimed; then a warm-up until the clocks have settled and of every shape
dev.reduce_tree_async(d_in, n, height, d_tree)
for f in forests.values():
    f.rebuild()
for _ in range(10):
    forests["w2"].rebuild()
for _ in range(3):
    for _, fn in forms:
        fn()
dev.sync()
ev = {name: [(dev.new_event(), dev.new_event()) for _ in range(a.runs)] for name, _ in forms}
for r in range(a.runs):
    for name, fn in forms:
        e0, e1 = ev[name][r]
        dev.record(e0); fn(); dev.record(e1)
dev.sync()
times = {name: np.array([dev.elapsed_ms(e0, e1) for e0, e1 in v]) for name, v in ev.items()}
ms = {name: float(np.median(v)) for name, v in times.items()}
spread = {name: float(v.max() / np.median(v)) for name, v in times.items()}

# correctness of what was timed: every shape on a freshly built forest, its roots against a fresh build over the leaves it left
checks = {}
for fname, f in forests.items():
    f.rebuild()
    for name in f.legs:
        f.update(name)()
        status = int(dev.download(d_status, 4)[0])
        f.rebuild(fresh=True)
        same = bool((dev.download(f.d_roots, 32 * f.ntrees) == dev.download(f.d_roots2, 32 * f.ntrees)).all())
        checks[f"{fname}_{name}"] = {"status": status, "roots_equal_fresh_build": same}

info = dev.lib.vkmr_hip_kernel_info().decode()
out = {"tool": "forest_update_timing", "leaves_log2": a.log2, "runs": a.runs, "device": dev.name(), "kernel_info": info,
       "build": provenance.build_id_of(info), "single_tree_height": height, "checks": checks,
       "all_checks_ok": all(c["status"] == 0 and c["roots_equal_fresh_build"] for c in checks.values()),
       "forests": {fname: {"ntrees": f.ntrees, "H": f.handle.levels, "rebuild_ms": round(ms[f"rebuild_{fname}"], 4)} for fname, f in forests.items()},
       "tree_update": {name: {"k": leg.k, "ms": round(ms[f"tree_update_{name}"], 4), "node_hashes": leg.nodes,
                              "max_over_median": round(spread[f"tree_update_{name}"], 4)} for name, leg in tree_legs.items()},
       "forest_update": {}}
for fname, f in forests.items():
    for name, leg in f.legs.items():
        t = ms[f"forest_update_{fname}_{name}"]
        b = "run" if name == "whole_trees" else name
        out["forest_update"][f"{fname}_{name}"] = {
            "k": leg.k, "ms": round(t, 4), "node_hashes": leg.nodes, "node_hashes_per_s": leg.nodes / (t * 1e-3),
            "max_over_median": round(spread[f"forest_update_{fname}_{name}"], 4),
            "rebuild_over_update": round(ms[f"rebuild_{fname}"] / t, 3), "vs_tree_update": round(t / ms[f"tree_update_{b}"], 4)}
k16 = min(1 << 16, n)
if f"random_k{k16}" in tree_legs:   # the expectation: on W2 at k = 2^16 no slower than (b), within (b)'s own spread
    b_ms, b_spread = ms[f"tree_update_random_k{k16}"], spread[f"tree_update_random_k{k16}"]
    mine = ms[f"forest_update_w2_random_k{k16}"]
    out["expectation_w2_k65536"] = {"forest_update_ms": round(mine, 4), "tree_update_ms": round(b_ms, 4), "margin_max_over_median": round(b_spread, 4),
                                    "met": bool(mine <= b_ms * b_spread)}
line = json.dumps(out)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
