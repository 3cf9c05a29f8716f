#!/usr/bin/env python3
"""Stored tree, proof gather and batch verification at 2^k random digests, beside the two plain reductions, timed with HIP
events: medians of interleaved runs in one process.  Prints one JSON line.  GPU box.
    python3 tools/tree_proofs_timing.py [--log2 26] [--ks 16,20] [--runs 10]"""
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
ap.add_argument("--ks", default="16,20", help="log2 of the proof counts")
ap.add_argument("--runs", type=int, default=10)
a = ap.parse_args()
dev = vk.HipDevice(0)
n, height = 1 << a.log2, a.log2
rng = np.random.default_rng(7)
d_in = dev.alloc(32 * n)
chunk = 1 << 22
for at in range(0, n, chunk):   # random digests, uploaded in pieces
    part = rng.integers(0, 2**32, size=(min(chunk, n - at), 8), dtype=np.uint32)
    vk.check(dev.lib.vkmr_hip_memcpy_h2d_async(dev.index, dev.stream, d_in.at(32 * at), part.ctypes.data, part.nbytes), "h2d")
    dev.sync()
d_scr, d_lscr, d_root, d_root2 = dev.reduce_scratch(n), dev.reduce_scratch(n, levels_variant=True), dev.alloc(32), dev.alloc(32)
d_tree = dev.alloc(dev.tree_bytes(n, height))
ks = [1 << int(x) for x in a.ks.split(",")]
kmax = max(ks)
idx = rng.integers(0, n, size=kmax, dtype=np.uint64)
d_idx = dev.upload(idx)
d_sib = dev.alloc(32 * kmax * height)
d_ok = dev.alloc(4 * kmax)
d_leaves = dev.alloc(32 * kmax)   # the proofs' leaves: gathered once below (level-0 cells at the indices)
tree = vk.MerkleTree(dev, d_in, n, height, d_tree)


def reduce():
    dev.reduce_async(d_in, n, height, d_scr, d_root)


def levels():
    dev.reduce_async(d_in, n, height, d_lscr, d_root2, levels_variant=True)


def build():
    dev.reduce_tree_async(d_in, n, height, d_tree)


def gather(k):
    return lambda: tree.proofs_async(d_idx, k, d_sib)


def verify(k):
    return lambda: dev.verify_proofs_async(d_leaves, d_idx, d_sib, k, height, d_root, 1, d_ok)


forms = [("reduce_async", reduce), ("reduce_levels_async", levels), ("reduce_tree_async", build)]
forms += [(f"tree_proofs_k{k}", gather(k)) for k in ks] + [(f"verify_proofs_k{k}", verify(k)) for k in ks]
# the leaves of the proofs, then one untimed pass of everything: the siblings the verify legs read are those of kmax proofs
build()
lv = np.ascontiguousarray(tree.level(0)[idx.astype(np.int64)])
vk.check(dev.lib.vkmr_hip_memcpy_h2d_async(dev.index, dev.stream, d_leaves.ptr, lv.ctypes.data, lv.nbytes), "h2d")
gather(kmax)()
dev.sync()
# warm up until the clocks have settled, then every form in turn, run after run (proof_timing.py: a form timed alone is
# compared across a clock that drifts by several per cent)
for _ in range(20):
    reduce(); build()
dev.sync()
ev = {name: [(dev.new_event(), dev.new_event()) for _ in range(a.runs)] for name, _ in forms}
for r in range(a.runs):
    for name, fn in forms:
        e0, e1 = ev[name][r]
        dev.record(e0); fn(); dev.record(e1)
dev.sync()
ms = {name: float(np.median([dev.elapsed_ms(e0, e1) for e0, e1 in v])) for name, v in ev.items()}
# correctness of what was timed: same root three ways, every proof ok (the last verify ran over the kmax siblings)
gather(kmax)(); verify(kmax)()
ok = dev.download(d_ok, 4 * kmax)
same = bool((dev.download(d_root, 32) == dev.download(d_root2, 32)).all() and (tree.root() == dev.download(d_root, 32)).all())
out = {"tool": "tree_proofs_timing", "leaves_log2": a.log2, "height": height, "runs": a.runs, "ms": {k: round(v, 4) for k, v in ms.items()},
       "roots_agree": same, "all_proofs_ok": bool((ok == 1).all()), "device": dev.name(), "kernel_info": dev.lib.vkmr_hip_kernel_info().decode()}
nodes = dev.tree_bytes(n, height) // 32   # node hashes of a build: the cells of levels 1..height (n - 1 for a power of two)
out["build_node_hashes_per_s"] = nodes / (ms["reduce_tree_async"] * 1e-3)
out["levels_node_hashes_per_s"] = nodes / (ms["reduce_levels_async"] * 1e-3)
out["build_vs_levels"] = ms["reduce_tree_async"] / ms["reduce_levels_async"]
for k in ks:
    out[f"verify_k{k}_node_hashes_per_s"] = k * height / (ms[f"verify_proofs_k{k}"] * 1e-3)
    out[f"verify_k{k}_vs_levels_rate"] = out[f"verify_k{k}_node_hashes_per_s"] / out["levels_node_hashes_per_s"]
    wrote = 32 * k * height
    read = 32 * k * height + 8 * k     # the cells (32 B each, scattered) and the indices
    out[f"gather_k{k}_bytes_written"] = wrote
    out[f"gather_k{k}_bytes_per_s"] = (wrote + read) / (ms[f"tree_proofs_k{k}"] * 1e-3)
    out[f"gather_k{k}_of_8TBps"] = out[f"gather_k{k}_bytes_per_s"] / 8e12
print(json.dumps(out))
