#!/usr/bin/env python3
"""The stored forest, its proof gather and the forest verifier beside the calls they are derived from, timed with HIP events:
medians of interleaved runs in one process after a warm-up of every shape, stamped with the build id.  Prints one JSON line
(and writes it to --out).  GPU box.
    python3 tools/forest_proofs_timing.py [--log2 26] [--ks 16,20] [--runs 10] [--out FILE]

  E equal   2^(log2 - 11) trees of 2^11 (H = 11)
  M mixed   tree sizes uniform in [1, 4095] (default_rng(42)), the last tree cut to fit (H = 12): forest_timing.py's W1
  1 build   vkmr_hip_reduce_forest_tree_async beside vkmr_hip_reduce_forest_async on the same forest (E and M)
  2 gather  vkmr_hip_forest_proofs_async (E and M) beside vkmr_hip_tree_proofs_async for the same k on ONE stored tree over the
            same leaves (height log2): per cell written, since the strides differ
  3 verify  vkmr_hip_verify_forest_proofs_async on E (every proof of height 11) beside vkmr_hip_verify_proofs_async at height
            11 on the same cells with a root per proof; on M the node-hash rate over the hashes needed, the sum of the heights"""
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
ap.add_argument("--ks", default="16,20", help="log2 of the proof counts")
ap.add_argument("--runs", type=int, default=10)
ap.add_argument("--out", default=None)
a = ap.parse_args()
dev = vk.HipDevice(0)
n = 1 << a.log2
rng = np.random.default_rng(7)
d_in = dev.alloc(32 * n)
chunk = min(n, 1 << 22)
base = rng.integers(0, 2**32, size=(chunk, 8), dtype=np.uint32)


def salt(piece):
    return np.uint32(piece * 2654435761 & 0xFFFFFFFF)


for at in range(0, n, chunk):   # random digests, uploaded in pieces: one random piece, made different per piece
    part = base ^ salt(at // chunk)
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


ks = [1 << int(x) for x in a.ks.split(",")]
kmax = max(ks)


class Forest:
    """One forest over d_in: the roots-only call, the stored build, kmax queries and what their proofs need."""

    def __init__(self, counts, max_count, seed):
        self.counts, self.max_count = np.asarray(counts, dtype=np.int64), max_count
        offsets, self.ntrees = vk.engine.forest_offsets(counts)
        self.d_off = dev.upload(offsets)
        self.d_scr = dev.alloc(dev.lib.vkmr_hip_forest_scratch_bytes(n, self.ntrees))
        self.d_roots0, self.d_roots, self.d_status = dev.alloc(32 * self.ntrees), dev.alloc(32 * self.ntrees), dev.alloc(4)
        self.d_forest = dev.alloc(dev.forest_tree_bytes(n, self.ntrees, max_count))
        self.H = vk.tree_height(min(max_count, n))
        r = np.random.default_rng(seed)
        self.trees = r.integers(0, self.ntrees, size=kmax).astype(np.uint32)
        c = self.counts[self.trees.astype(np.int64)]
        self.indices = np.minimum((r.random(kmax) * c).astype(np.int64), c - 1).astype(np.uint64)
        self.heights = np.maximum(1, np.frexp(c - 1)[1]).astype(np.int64)      # bit_length(c - 1), at least 1
        self.d_trees, self.d_idx = dev.upload(self.trees), dev.upload(self.indices)
        self.d_lv = dev.upload(leaves_at(offsets[self.trees.astype(np.int64)].astype(np.int64) + self.indices.astype(np.int64)))
        self.d_sib, self.d_h, self.d_ok = dev.alloc(32 * kmax * self.H), dev.alloc(4 * kmax), dev.alloc(4 * kmax)

    def roots_only(self):
        dev.reduce_forest_async(d_in, n, self.d_off, self.ntrees, self.max_count, self.d_scr, self.d_roots0, self.d_status)

    def build(self):
        dev.reduce_forest_tree_async(d_in, n, self.d_off, self.ntrees, self.max_count, self.d_forest, self.d_roots, self.d_status)

    def gather(self, k):
        return lambda: dev.forest_proofs_async(d_in, self.d_forest, n, self.d_off, self.ntrees, self.max_count, self.d_trees, self.d_idx, k,
                                               self.d_sib, self.d_h)

    def verify(self, k):
        return lambda: dev.verify_forest_proofs_async(self.d_lv, self.d_trees, self.d_idx, self.d_sib, self.d_h, k, self.H, self.d_roots,
                                                      self.ntrees, self.d_ok)


cap = min(1 << 11, n)
E = Forest([cap] * (n // cap), cap, 11)
M = Forest(cut_to_fit(np.random.default_rng(42).integers(1, 4096, size=n // 1024 + 16), n), 4095, 12)

# the single stored tree over the same leaves, and the single-height verifier on E's cells with a root per proof
height = a.log2
d_tree = dev.alloc(dev.tree_bytes(n, height))
tree = vk.MerkleTree(dev, d_in, n, height, d_tree)
t_idx = np.random.default_rng(13).integers(0, n, size=kmax, dtype=np.uint64)
d_tidx = dev.upload(t_idx)
d_tsib = dev.alloc(32 * kmax * height)
d_ok1 = dev.alloc(4 * kmax)


def single_gather(k):
    return lambda: tree.proofs_async(d_tidx, k, d_tsib)


# everything the timed legs read is formed once, untimed
dev.reduce_tree_async(d_in, n, height, d_tree)
for f in (E, M):
    f.roots_only(); f.build(); f.gather(kmax)()
dev.sync()
d_proof_roots = dev.upload(np.ascontiguousarray(dev.download(E.d_roots, 32 * E.ntrees).reshape(-1, 8)[E.trees.astype(np.int64)]))


def single_verify(k):
    return lambda: dev.verify_proofs_async(E.d_lv, E.d_idx, E.d_sib, k, E.H, d_proof_roots, k, d_ok1)


forms = [("forest_roots_equal", E.roots_only), ("forest_tree_equal", E.build), ("forest_roots_mixed", M.roots_only), ("forest_tree_mixed", M.build)]
for k in ks:
    forms += [(f"tree_proofs_k{k}", single_gather(k)), (f"forest_proofs_equal_k{k}", E.gather(k)), (f"forest_proofs_mixed_k{k}", M.gather(k)),
              (f"verify_proofs_h11_k{k}", single_verify(k)), (f"verify_forest_equal_k{k}", E.verify(k)), (f"verify_forest_mixed_k{k}", M.verify(k))]
# warm up until the clocks have settled, then every shape once, then every form in turn, run after run
for _ in range(10):
    E.roots_only(); E.build()
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

# correctness of what was timed: the two builds' roots agree, every proof of kmax verifies in both verifiers, the heights are the host's
checks = {}
for name, f in (("equal", E), ("mixed", M)):
    f.gather(kmax)(); f.verify(kmax)()
    checks[f"{name}_status_ok"] = bool(int(dev.download(f.d_status, 4)[0]) == 0)
    checks[f"{name}_roots_agree"] = bool((dev.download(f.d_roots, 32 * f.ntrees) == dev.download(f.d_roots0, 32 * f.ntrees)).all())
    checks[f"{name}_all_proofs_ok"] = bool((dev.download(f.d_ok, 4 * kmax) == 1).all())
    checks[f"{name}_heights_agree"] = bool((dev.download(f.d_h, 4 * kmax).astype(np.int64) == f.heights).all())
single_verify(kmax)()
checks["single_verifier_all_ok"] = bool((dev.download(d_ok1, 4 * kmax) == 1).all())

info = dev.lib.vkmr_hip_kernel_info().decode()
out = {"tool": "forest_proofs_timing", "leaves_log2": a.log2, "runs": a.runs, "ms": {k: round(v, 4) for k, v in ms.items()}, "checks": checks,
       "equal": {"ntrees": E.ntrees, "H": E.H}, "mixed": {"ntrees": M.ntrees, "H": M.H}, "single_tree_height": height,
       "device": dev.name(), "kernel_info": info, "build": provenance.build_id_of(info)}
out["build_equal_vs_roots_only"] = ms["forest_tree_equal"] / ms["forest_roots_equal"]
out["build_mixed_vs_roots_only"] = ms["forest_tree_mixed"] / ms["forest_roots_mixed"]
out["build_target_1.05_met"] = max(out["build_equal_vs_roots_only"], out["build_mixed_vs_roots_only"]) <= 1.05
for k in ks:
    per_cell_single = ms[f"tree_proofs_k{k}"] / (k * height)
    for name, f in (("equal", E), ("mixed", M)):
        out[f"gather_{name}_k{k}_per_cell_vs_tree_proofs"] = ms[f"forest_proofs_{name}_k{k}"] / (k * f.H) / per_cell_single
    out[f"gather_k{k}_target_1.25_met"] = max(out[f"gather_equal_k{k}_per_cell_vs_tree_proofs"], out[f"gather_mixed_k{k}_per_cell_vs_tree_proofs"]) <= 1.25
    out[f"verify_equal_k{k}_vs_verify_proofs"] = ms[f"verify_forest_equal_k{k}"] / ms[f"verify_proofs_h11_k{k}"]
    out[f"verify_k{k}_target_1.10_met"] = out[f"verify_equal_k{k}_vs_verify_proofs"] <= 1.10
    out[f"verify_equal_k{k}_node_hashes_per_s"] = k * E.H / (ms[f"verify_forest_equal_k{k}"] * 1e-3)
    needed = int(M.heights[:k].sum())
    out[f"verify_mixed_k{k}_node_hashes_needed"] = needed
    out[f"verify_mixed_k{k}_node_hashes_per_s"] = needed / (ms[f"verify_forest_mixed_k{k}"] * 1e-3)
    out[f"verify_mixed_k{k}_vs_equal_rate"] = out[f"verify_mixed_k{k}_node_hashes_per_s"] / out[f"verify_equal_k{k}_node_hashes_per_s"]
line = json.dumps(out)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
