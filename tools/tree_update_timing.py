#!/usr/bin/env python3
"""Leaf updates of a stored tree at 2^k random digests against a rebuild of the whole tree, timed with HIP events: medians of
interleaved runs in one process.  Legs: the rebuild (vkmr_hip_reduce_tree_async), updates of 1, 2^10, 2^16 and 2^20 random
unique sorted leaves, and one contiguous run of 2^16 leaves.  Every leg reports ms, the distinct nodes it rehashes
(sum over l = 1..height of |unique(idx >> l)|, computed on the host) and node hashes/s.  Prints one JSON line.  GPU box.
    python3 tools/tree_update_timing.py [--log2 26] [--ks 0,10,16,20] [--runs 10]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vk_merkle_roots_amd as vk  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log2", type=int, default=26)
ap.add_argument("--ks", default="0,10,16,20", help="log2 of the random update counts")
ap.add_argument("--run-log2", type=int, default=16, help="log2 of the contiguous run's length")
ap.add_argument("--runs", type=int, default=10)
a = ap.parse_args()
dev = vk.HipDevice(0)
n, height = 1 << a.log2, a.log2
rng = np.random.default_rng(11)
d_in = dev.alloc(32 * n)
chunk = 1 << 22
for at in range(0, n, chunk):   # random digests, uploaded in pieces
    part = rng.integers(0, 2**32, size=(min(chunk, n - at), 8), dtype=np.uint32)
    vk.check(dev.lib.vkmr_hip_memcpy_h2d_async(dev.index, dev.stream, d_in.at(32 * at), part.ctypes.data, part.nbytes), "h2d")
    dev.sync()
d_tree = dev.alloc(dev.tree_bytes(n, height))
tree = vk.MerkleTree(dev, d_in, n, height, d_tree)
d_status = dev.alloc(4)


def distinct_nodes(idx):
    return int(sum(np.unique(idx >> np.uint64(l)).shape[0] for l in range(1, height + 1)))


legs = {}   # name -> (indices uint64 sorted unique, device indices, device leaves)
for lk in [int(x) for x in a.ks.split(",")]:
    k = min(1 << lk, n)
    idx = np.sort(rng.choice(n, size=k, replace=False)).astype(np.uint64)
    legs[f"update_random_k{k}"] = idx
run = min(1 << a.run_log2, n)
start = int(rng.integers(0, n - run + 1))
legs[f"update_run_k{run}"] = np.arange(start, start + run, dtype=np.uint64)
bufs = {name: (dev.upload(idx), dev.upload(rng.integers(0, 2**32, size=(idx.shape[0], 8), dtype=np.uint32))) for name, idx in legs.items()}


def rebuild():
    dev.reduce_tree_async(d_in, n, height, d_tree)


def update(name):
    d_idx, d_leaves = bufs[name]
    return lambda: tree.update_async(d_idx, d_leaves, legs[name].shape[0], d_status)


forms = [("reduce_tree_async", rebuild)] + [(name, update(name)) for name in legs]
# warm up every form until the clocks have settled, then every form in turn, run after run (tree_proofs_timing.py)
for _ in range(5):
    for _, fn in forms:
        fn()
for _ in range(15):
    rebuild()
dev.sync()
ev = {name: [(dev.new_event(), dev.new_event()) for _ in range(a.runs)] for name, _ in forms}
for r in range(a.runs):
    for name, fn in forms:
        e0, e1 = ev[name][r]
        dev.record(e0); fn(); dev.record(e1)
dev.sync()
ms = {name: float(np.median([dev.elapsed_ms(e0, e1) for e0, e1 in v])) for name, v in ev.items()}
# correctness of what was timed: after the last update leg, the tree equals a rebuild over the same (updated) leaves
status = int(dev.download(d_status, 4)[0])
root_updated = tree.root()
rebuild()
same = bool((tree.root() == root_updated).all())
nodes = {"reduce_tree_async": dev.tree_bytes(n, height) // 32}
nodes.update({name: distinct_nodes(idx) for name, idx in legs.items()})
out = {"tool": "tree_update_timing", "leaves_log2": a.log2, "height": height, "runs": a.runs, "status": status,
       "root_equals_rebuild": same, "device": dev.name(), "kernel_info": dev.lib.vkmr_hip_kernel_info().decode(), "legs": {}}
for name, _ in forms:
    out["legs"][name] = {"ms": round(ms[name], 4), "node_hashes": nodes[name], "node_hashes_per_s": nodes[name] / (ms[name] * 1e-3),
                         "vs_rebuild": round(ms[name] / ms["reduce_tree_async"], 4)}
print(json.dumps(out))
