#!/usr/bin/env python3
"""One compact multiproof for leaves of many trees of a stored forest beside the path that existed before it -- k independent
proofs at one stride (vkmr_hip_forest_proofs_async + vkmr_hip_verify_forest_proofs_async) for the SAME entries -- timed with HIP
events: medians of interleaved runs in one process after a warm-up of every shape, stamped with the build id.  Prints one JSON
line (and writes it to --out).  GPU box.
    python3 tools/forest_multiproof_timing.py [--log2 26] [--ks 10,16,20] [--whole 16] [--runs 10] [--out FILE]

  E equal   2^(log2 - 11) trees of 2^11 (H = 11)
  M mixed   tree sizes uniform in [1, 4095] (default_rng(42)), the last tree cut to fit (H = 12): forest_proofs_timing.py's M
  entries   2^k random (tree, index) pairs, sorted and deduplicated (so slightly fewer), and 2^whole entries that fill whole trees
  per set   gather: vkmr_hip_forest_multiproof_async vs vkmr_hip_forest_proofs_async; verify: vkmr_hip_verify_forest_multiproof_async
            vs vkmr_hip_verify_forest_proofs_async; every ratio is compact / independent as both ran here
Bytes and node hashes of both forms are computed on the host from the entries alone and must equal what the device reported
(M, the per-level counts).  Every timed proof is verified: timed run r of a verifier writes its verdict into slot r of its
verdict buffer, and all slots are read after the timed loop (the warm-up runs write slot 0, which timed run 0 overwrites)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vk_merkle_roots_amd as vk  # noqa: E402
from vk_merkle_roots_amd import provenance  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log2", type=int, default=26)
ap.add_argument("--ks", default="10,16,20", help="log2 of the random entry counts")
ap.add_argument("--whole", type=int, default=16, help="log2 of the entries that fill whole trees")
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
    part = base ^ np.uint32((at // chunk) * 2654435761 & 0xFFFFFFFF)
    vk.check(dev.lib.vkmr_hip_memcpy_h2d_async(dev.index, dev.stream, d_in.at(32 * at), part.ctypes.data, part.nbytes), "h2d")
    dev.sync()


def leaves_at(cells):
    """[k, 8]: the digests at `cells` of d_in, formed on the host as the upload formed them."""
    cells = np.asarray(cells, dtype=np.int64)
    return np.ascontiguousarray(base[cells % chunk] ^ ((cells // chunk) * 2654435761 & 0xFFFFFFFF).astype(np.uint32)[:, None])


def cut_to_fit(sizes, total):
    ends = np.cumsum(sizes)
    k = int(np.searchsorted(ends, total))
    counts = [int(c) for c in sizes[:k]]
    if sum(counts) < total:
        counts.append(total - sum(counts))
    return counts


def host_counts(trees, indices, heights, H):
    """(per-level node counts [H], node hashes of the compact fold) from the entries alone: level by level the distinct
    (tree, node) pairs, a node for each whose sibling is not among them, a hash for each distinct parent."""
    key = (trees.astype(np.uint64) << np.uint64(32)) | indices          # indices < 2^32 here
    h = heights.astype(np.int64)
    per_level, hashes = [], 0
    for l in range(H):
        live = h > l
        key, h = key[live], h[live]
        sib = key ^ np.uint64(1)
        pos = np.searchsorted(key, sib)
        present = key[np.minimum(pos, key.shape[0] - 1)] == sib if key.shape[0] else np.zeros(0, dtype=bool)
        per_level.append(int((~present).sum()))
        tree_part = key >> np.uint64(32) << np.uint64(32)
        parent = tree_part | ((key & np.uint64(0xFFFFFFFF)) >> np.uint64(1))
        first = np.ones(parent.shape[0], dtype=bool)
        first[1:] = parent[1:] != parent[:-1]
        key, h = parent[first], h[first]
        hashes += int(key.shape[0])
    return per_level, hashes


class Slot:
    """A device pointer inside another buffer, for the wrappers that read `.ptr`."""

    def __init__(self, buf, offset):
        self.ptr = buf.at(offset)


class Entries:
    """One sorted entry set of one forest and the buffers of both forms of its proofs."""

    def __init__(self, forest, name, trees, indices):
        self.f, self.name = forest, name
        order = np.lexsort((indices, trees))
        t, i = trees[order], indices[order]
        keep = np.ones(t.shape[0], dtype=bool)
        keep[1:] = (t[1:] != t[:-1]) | (i[1:] != i[:-1])
        self.trees, self.indices = np.ascontiguousarray(t[keep].astype(np.uint32)), np.ascontiguousarray(i[keep].astype(np.uint64))
        self.k = k = int(self.trees.shape[0])
        c = forest.counts[self.trees.astype(np.int64)]
        self.heights = np.maximum(1, np.frexp(c - 1)[1]).astype(np.uint32)      # bit_length(c - 1), at least 1
        self.level_counts, self.hashes = host_counts(self.trees, self.indices, self.heights, forest.H)
        self.M = sum(self.level_counts)
        H = forest.H
        self.d_trees, self.d_idx = dev.upload(self.trees), dev.upload(self.indices)
        self.d_lv = dev.upload(leaves_at(forest.offsets[self.trees.astype(np.int64)].astype(np.int64) + self.indices.astype(np.int64)))
        self.cap = dev.lib.vkmr_hip_forest_multiproof_max_nodes(n, forest.ntrees, forest.max_count, k)
        scratch = dev.lib.vkmr_hip_forest_multiproof_scratch_bytes(k, H)
        self.d_scr, self.d_vscr = dev.alloc(scratch), dev.alloc(scratch)
        self.d_nodes, self.d_h, self.d_info, self.d_ok1 = dev.alloc(32 * self.cap), dev.alloc(4 * k), dev.alloc(8 * (2 + H)), dev.alloc(4 * a.runs)
        self.d_sib, self.d_h2, self.d_ok = dev.alloc(32 * k * H), dev.alloc(4 * k), dev.alloc(4 * k * a.runs)

    def gather(self, r=0):
        f = self.f
        dev.forest_multiproof_async(d_in, f.d_forest, n, f.d_off, f.ntrees, f.max_count, self.d_trees, self.d_idx, self.k, self.d_scr, self.d_nodes,
                                    self.cap, self.d_h, self.d_info)

    def verify(self, r=0):
        dev.verify_forest_multiproof_async(self.d_lv, self.d_trees, self.d_idx, self.d_h, self.k, self.f.H, self.d_nodes, self.M, self.f.d_roots,
                                           self.f.ntrees, self.d_vscr, Slot(self.d_ok1, 4 * r))

    def gather_independent(self, r=0):
        f = self.f
        dev.forest_proofs_async(d_in, f.d_forest, n, f.d_off, f.ntrees, f.max_count, self.d_trees, self.d_idx, self.k, self.d_sib, self.d_h2)

    def verify_independent(self, r=0):
        dev.verify_forest_proofs_async(self.d_lv, self.d_trees, self.d_idx, self.d_sib, self.d_h2, self.k, self.f.H, self.f.d_roots, self.f.ntrees,
                                       Slot(self.d_ok, 4 * self.k * r))


class Forest:
    def __init__(self, label, counts, max_count, seed):
        self.label, self.counts, self.max_count = label, np.asarray(counts, dtype=np.int64), max_count
        self.offsets, self.ntrees = vk.engine.forest_offsets(counts)
        self.d_off = dev.upload(self.offsets)
        self.d_roots, self.d_status = dev.alloc(32 * self.ntrees), dev.alloc(4)
        self.d_forest = dev.alloc(dev.forest_tree_bytes(n, self.ntrees, max_count))
        self.H = vk.tree_height(min(max_count, n))
        dev.reduce_forest_tree_async(d_in, n, self.d_off, self.ntrees, max_count, self.d_forest, self.d_roots, self.d_status)
        dev.sync()
        r = np.random.default_rng(seed)
        self.sets = []
        for lg in [int(x) for x in a.ks.split(",")]:
            k = 1 << lg
            trees = r.integers(0, self.ntrees, size=k)
            c = self.counts[trees]
            self.sets.append(Entries(self, f"random_2^{lg}", trees, np.minimum((r.random(k) * c).astype(np.int64), c - 1)))
        first = int(r.integers(0, max(1, self.ntrees // 2)))       # whole trees: consecutive ones from a random first, 2^whole leaves or just above
        last = int(np.searchsorted(np.cumsum(self.counts[first:]), 1 << a.whole)) + first + 1
        trees = np.repeat(np.arange(first, last), self.counts[first:last])
        indices = np.concatenate([np.arange(c) for c in self.counts[first:last]])
        self.sets.append(Entries(self, f"whole_trees_2^{a.whole}", trees, indices))


cap = min(1 << 11, n)
forests = [Forest("equal", [cap] * (n // cap), cap, 11),
           Forest("mixed", cut_to_fit(np.random.default_rng(42).integers(1, 4096, size=n // 1024 + 16), n), 4095, 12)]
forms = []
for f in forests:
    for e in f.sets:
        tag = f"{f.label}_{e.name}"
        forms += [(f"multiproof_{tag}", e.gather), (f"verify_multiproof_{tag}", e.verify), (f"forest_proofs_{tag}", e.gather_independent),
                  (f"verify_forest_proofs_{tag}", e.verify_independent)]
# warm up until the clocks have settled (every shape, several times), then every form in turn, run after run
for _ in range(3):
    for _, fn in forms:
        fn()
dev.sync()
ev = {name: [(dev.new_event(), dev.new_event()) for _ in range(a.runs)] for name, _ in forms}
for r in range(a.runs):
    for name, fn in forms:
        e0, e1 = ev[name][r]
        dev.record(e0); fn(r); dev.record(e1)
dev.sync()
ms = {name: float(np.median([dev.elapsed_ms(e0, e1) for e0, e1 in v])) for name, v in ev.items()}

info = dev.lib.vkmr_hip_kernel_info().decode()
out = {"tool": "forest_multiproof_timing", "leaves_log2": a.log2, "runs": a.runs, "ms": {k: round(v, 4) for k, v in ms.items()}, "sets": {},
       "device": dev.name(), "kernel_info": info, "build": provenance.build_id_of(info)}
ok = True
for f in forests:
    assert int(dev.download(f.d_status, 4)[0]) == 0
    for e in f.sets:
        tag = f"{f.label}_{e.name}"
        dinfo = dev.download(e.d_info, 8 * (2 + f.H), dtype=np.uint64)
        rec = {"ntrees": f.ntrees, "H": f.H, "k": e.k, "nodes": e.M, "level_counts": e.level_counts,
               "device_reports_the_host_counts": bool(int(dinfo[0]) == 0 and int(dinfo[1]) == e.M and [int(x) for x in dinfo[2:]] == e.level_counts),
               "heights_agree": bool((dev.download(e.d_h, 4 * e.k) == e.heights).all() and (dev.download(e.d_h2, 4 * e.k) == e.heights).all()),
               "multiproof_verifies": bool((dev.download(e.d_ok1, 4 * a.runs) == 1).all()),                 # every timed run
               "independent_proofs_verify": bool((dev.download(e.d_ok, 4 * e.k * a.runs) == 1).all()),
               "node_cells_compact": e.M, "node_cells_independent": e.k * f.H,
               "cells_ratio": e.M / (e.k * f.H),
               "node_hashes_compact": e.hashes, "node_hashes_independent": int(e.heights.astype(np.int64).sum()),
               "gather_ms": ms[f"multiproof_{tag}"], "gather_independent_ms": ms[f"forest_proofs_{tag}"],
               "gather_ratio": ms[f"multiproof_{tag}"] / ms[f"forest_proofs_{tag}"],
               "verify_ms": ms[f"verify_multiproof_{tag}"], "verify_independent_ms": ms[f"verify_forest_proofs_{tag}"],
               "verify_ratio": ms[f"verify_multiproof_{tag}"] / ms[f"verify_forest_proofs_{tag}"]}
        rec["both_ratio"] = (rec["gather_ms"] + rec["verify_ms"]) / (rec["gather_independent_ms"] + rec["verify_independent_ms"])
        rec["hashes_ratio"] = rec["node_hashes_compact"] / rec["node_hashes_independent"]
        ok = ok and rec["device_reports_the_host_counts"] and rec["heights_agree"] and rec["multiproof_verifies"] and rec["independent_proofs_verify"]
        out["sets"][tag] = rec
out["all_checks_ok"] = ok
line = json.dumps(out)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
sys.exit(0 if ok else 1)
