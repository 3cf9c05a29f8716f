#!/usr/bin/env python3
"""What range proofs over sorted trees cost on the device (vkmr_hip_forest_range_async, vkmr_hip_verify_forest_range_async), timed
with HIP events: medians of interleaved runs in one process after a warm-up of every leg, stamped with the build id.  Prints one JSON
line (and writes it to --out).  GPU box.
    python3 tools/range_timing.py [--log2 26] [--runs 10] [--out profiles/range_timing.json]

  the shapes   2^log2 random digests, sorted on the device and stored once as trees of 2 048 and once as ONE tree
  the queries  2^10, 2^16 and 2^20 ranges of 16 leaves each (18 carried: the fences), spread evenly; 2^10 ranges of 2^16 carried leaves
               (the one tree only: a tree of 2 048 has no such range); every tree whole
  the legs     per shape and batch: the gather, the check, and the counting call (capacity 0) alone
  beside them  at 2^16 ranges on the trees of 2 048 the parent commit's only route for the same leaves: vkmr_hip_forest_multiproof_async
               over the explicit consecutive (tree, index) entries, written outside the clock, and
               vkmr_hip_verify_forest_multiproof_async; and vkmr_hip_reduce_forest_async over the whole forest beside "every tree
               whole", the same hashes; neither is code under test
Every answer is checked before the clock starts: status 0 and every verdict 1 (the old route: status 0 and ok 1).  One requirement:
at 2^16 ranges on the trees of 2 048, gather + check take no longer than the parent's gather + check."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vk_merkle_roots_amd as vk  # noqa: E402
from vk_merkle_roots_amd import provenance  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log2", type=int, default=26)
ap.add_argument("--runs", type=int, default=10)
ap.add_argument("--out", default=None)
a = ap.parse_args()
dev = vk.HipDevice(0)
n = 1 << a.log2
PER = min(2048, n)
IN, CARRIED = 16, 18
SMALL = [b for b in (10, 16, 20) if (CARRIED + 2) << b <= n]
KEY = 16 if 16 in SMALL else SMALL[-1]
gen = torch.Generator(device="cuda").manual_seed(41)


class Cells:
    """A buffer of digests that torch owns, as the engine's calls take it."""

    def __init__(self, cells):
        self.t = torch.empty((max(cells, 1), 8), dtype=torch.int32, device="cuda")
        self.ptr = self.t.data_ptr()

    def at(self, byte_offset):
        return self.ptr + int(byte_offset)

    def free(self):
        pass


raw = Cells(n)
raw.t[:n] = torch.randint(-2**31, 2**31 - 1, (n, 8), dtype=torch.int32, device="cuda", generator=gen)
torch.cuda.synchronize()


class Batch:
    """Q queries against a shape: their buffers, and the outputs of the gather and the check."""

    def __init__(self, shape, name, trees, first_cells, last_cells, carried, whole=False):
        self.shape, self.name, self.Q, self.carried = shape, name, len(trees), int(carried)
        Q, stride = self.Q, shape.stride
        self.d_trees = dev.upload(np.ascontiguousarray(trees, dtype=np.uint32))
        self.d_lo, self.d_hi = Cells(Q), Cells(Q)
        if whole:
            self.d_lo.t[:Q] = 0
            self.d_hi.t[:Q] = -1
            torch.cuda.synchronize()
        else:
            for cells, out in ((first_cells, self.d_lo), (last_cells, self.d_hi)):
                d_idx = dev.upload(np.ascontiguousarray(cells, dtype=np.uint32))
                dev.gather_digests_async(shape.d_leaves, d_idx, Q, out)
                dev.sync()
                d_idx.free()
        self.d_first, self.d_starts, self.d_h, self.d_info = dev.alloc(8 * Q), dev.alloc(8 * (Q + 1)), dev.alloc(4 * Q), dev.alloc(32)
        self.d_out, self.d_left, self.d_right = Cells(self.carried), Cells(Q * stride), Cells(Q * stride)
        self.d_gather_scratch, self.d_scratch = dev.alloc(dev.range_scratch_bytes(0, Q)), dev.alloc(dev.range_scratch_bytes(self.carried, Q))
        self.d_verdict, self.d_in_first, self.d_in_count = dev.alloc(4 * Q), dev.alloc(8 * Q), dev.alloc(8 * Q)

    def gather(self, capacity=None):
        f = self.shape.forest
        f.range_async(self.d_trees, self.d_lo, self.d_hi, self.Q, self.shape.stride, self.d_gather_scratch, self.d_first, self.d_starts,
                      self.d_out if capacity is None else None, self.carried if capacity is None else 0, self.d_left, self.d_right, self.d_h, self.d_info)

    def count(self):
        self.gather(capacity=0)

    def verify(self):
        f = self.shape.forest
        dev.verify_forest_range_enqueue(self.d_trees, self.d_lo, self.d_hi, self.d_first, self.d_starts, self.d_out, self.carried, self.d_left, self.d_right,
                                        self.d_h, self.Q, self.shape.stride, f.roots_buf, self.shape.d_counts, f.ntrees, self.d_scratch, self.d_verdict,
                                        self.d_in_first, self.d_in_count)

    def check(self, inside):
        self.count()
        counted = dev.download(self.d_info, 32, dtype=np.uint64).tolist()
        self.gather()
        self.verify()
        info = dev.download(self.d_info, 32, dtype=np.uint64).tolist()
        verdict, got = dev.download(self.d_verdict, 4 * self.Q), dev.download(self.d_in_count, 8 * self.Q, dtype=np.uint64)
        return {"status": info[0] == 0, "counting_call": counted == [1, self.carried, 0, inside * self.Q],
                "leaves_carried": info[1] == self.carried, "leaves_in_range": info[3] == inside * self.Q, "every_verdict_1": bool((verdict == 1).all()),
                "in_count": bool((got == inside).all())}


class Shape:
    def __init__(self, per):
        self.per, self.T = per, n // per
        offsets = np.arange(self.T + 1, dtype=np.uint64) * np.uint64(per)
        self.d_leaves = Cells(n)
        d_scr, d_info, d_off = dev.alloc(dev.sort_leaves_scratch_bytes(n)), dev.alloc(32), dev.upload(offsets)
        dev.forest_sort_leaves_enqueue(raw, n, d_off, self.T, per, d_scr, self.d_leaves, None, d_info)
        info = dev.download(d_info, 32, dtype=np.uint64).tolist()
        assert info[0] == 0 and info[3] == 0, info
        for b in (d_scr, d_info, d_off):
            b.free()
        self.forest = dev._build_forest_of_buffer(self.d_leaves, n, [per] * self.T, per, "range_timing")
        self.stride = self.forest.levels
        self.d_counts = dev.upload(np.full(self.T, per, dtype=np.uint64))
        self.batches = {}
        for lg in SMALL:                          # 2^lg ranges of IN leaves, in (tree, index) order, evenly spread, never touching
            Q = 1 << lg
            step = n // Q
            start = np.arange(Q, dtype=np.uint64) * np.uint64(step) + np.uint64(2)
            if step < per:                        # several a tree: keep every run inside its tree
                k = per // step
                start = (start // np.uint64(per)) * np.uint64(per) + (np.arange(Q, dtype=np.uint64) % np.uint64(k)) * np.uint64((per - CARRIED - 2) // k) + np.uint64(2)
            self.batches[f"2^{lg}_ranges_of_{IN}"] = (Batch(self, f"2^{lg}", start // np.uint64(per), start, start + np.uint64(IN - 1), CARRIED * Q), IN)
            if lg == KEY:
                self.key_start = start
        if per == n and n >= 1 << 16:             # ranges that fill a 1 024th of the tree each, fences included: 2^16 cells at 2^26 leaves
            Q = 1 << 10
            start = np.arange(Q, dtype=np.uint64) * np.uint64(n // Q) + np.uint64(1)
            m = n // Q - 2
            self.batches[f"2^10_ranges_of_{m}"] = (Batch(self, "big", start // np.uint64(per), start, start + np.uint64(m - 1), (m + 2) * Q), m)
        self.batches["every_tree_whole"] = (Batch(self, "whole", np.arange(self.T), None, None, n, whole=True), per)

    def old_route(self):
        """The parent's route for the KEY batch: the explicit entries of the same carried leaves, its buffers, and its two calls."""
        b, _ = self.batches[f"2^{KEY}_ranges_of_{IN}"]
        k = b.carried
        first = self.key_start - np.uint64(1)
        cells = (first[:, None] + np.arange(CARRIED, dtype=np.uint64)[None, :]).reshape(-1)
        lib = dev.lib
        self.k = k
        self.d_et, self.d_ei = dev.upload((cells // np.uint64(self.per)).astype(np.uint32)), dev.upload(cells % np.uint64(self.per))
        d_idx = dev.upload(cells.astype(np.uint32))
        self.d_eleaves = Cells(k)
        dev.gather_digests_async(self.d_leaves, d_idx, k, self.d_eleaves)
        dev.sync()
        d_idx.free()
        self.cap = lib.vkmr_hip_forest_multiproof_max_nodes(n, self.T, self.per, k)
        self.d_nodes, self.d_eh, self.d_minfo = Cells(self.cap), dev.alloc(4 * k), dev.alloc(8 * (2 + self.stride))
        self.d_mscr, self.d_ok = dev.alloc(lib.vkmr_hip_forest_multiproof_scratch_bytes(k, self.stride)), dev.alloc(4)
        self.old_gather()
        minfo = dev.download(self.d_minfo, 16, dtype=np.uint64).tolist()
        self.M = int(minfo[1])
        self.old_verify()
        return {"status": minfo[0] == 0, "ok": int(dev.download(self.d_ok, 4)[0]) == 1, "nodes": self.M}

    def old_gather(self):
        f = self.forest
        dev.forest_multiproof_async(f.digests, f.forest, f.total, f.offsets, f.ntrees, f.max_count, self.d_et, self.d_ei, self.k, self.d_mscr, self.d_nodes,
                                    self.cap, self.d_eh, self.d_minfo)

    def old_verify(self):
        f = self.forest
        dev.verify_forest_multiproof_async(self.d_eleaves, self.d_et, self.d_ei, self.d_eh, self.k, self.stride, self.d_nodes, self.M, f.roots_buf, f.ntrees,
                                           self.d_mscr, self.d_ok)


shapes = {"trees_of_2048": Shape(PER)}
if n > PER:
    shapes["one_tree"] = Shape(n)
forest = shapes["trees_of_2048"]

out = {"tool": "range_timing", "leaves_log2": a.log2, "runs": a.runs, "device": dev.name(), "kernel_info": dev.lib.vkmr_hip_kernel_info().decode(),
       "build": provenance.build_id_of(dev.lib.vkmr_hip_kernel_info().decode()), "torch": torch.__version__, "checks": {}, "shapes": {}}
legs = {}
for name, s in shapes.items():                    # every answer checked, and every leg warmed up
    out["checks"][name] = {}
    for bname, (b, inside) in s.batches.items():
        out["checks"][name][bname] = b.check(inside)
        legs[name, bname + "/gather"], legs[name, bname + "/verify"], legs[name, bname + "/count_only"] = b.gather, b.verify, b.count
out["checks"]["trees_of_2048"]["parent_route"] = forest.old_route()
legs["trees_of_2048", f"2^{KEY}_ranges_of_{IN}/parent_multiproof_gather"] = forest.old_gather
legs["trees_of_2048", f"2^{KEY}_ranges_of_{IN}/parent_multiproof_verify"] = forest.old_verify
d_fscr, d_froots, d_fstatus = dev.alloc(dev.lib.vkmr_hip_forest_scratch_bytes(n, forest.T)), dev.alloc(32 * forest.T), dev.alloc(4)
legs["trees_of_2048", "every_tree_whole/reduce_forest"] = lambda: dev.reduce_forest_async(forest.d_leaves, n, forest.forest.offsets, forest.T, PER, d_fscr,
                                                                                          d_froots, d_fstatus)
for key, fn in legs.items():
    if not key[1].endswith("/count_only"):        # a counting call between a gather and its check would leave no leaves to check
        fn()
dev.sync()

order = [k for k in legs if not k[1].endswith("/count_only")] + [k for k in legs if k[1].endswith("/count_only")]
ev = {key: [(dev.new_event(), dev.new_event()) for _ in range(a.runs)] for key in legs}
for r in range(a.runs):                           # every leg once per round, each waiting for the one before; the counting calls last
    for key in order:
        e0, e1 = ev[key][r]
        dev.record(e0); legs[key](); dev.record(e1)
        dev.sync()

med = {}
for (name, leg), pairs in ev.items():
    ms = [dev.elapsed_ms(e0, e1) for e0, e1 in pairs]
    med[name, leg] = float(np.median(ms))
    out["shapes"].setdefault(name, {"trees": shapes[name].T, "leaves_per_tree": shapes[name].per, "stride": shapes[name].stride, "legs": {}})["legs"][leg] = {
        "median_ms": round(med[name, leg], 4), "min_max_ms": [round(min(ms), 4), round(max(ms), 4)]}
pre = f"2^{KEY}_ranges_of_{IN}/"
new = med["trees_of_2048", pre + "gather"] + med["trees_of_2048", pre + "verify"]
old = med["trees_of_2048", pre + "parent_multiproof_gather"] + med["trees_of_2048", pre + "parent_multiproof_verify"]
out["requirement"] = {"what": f"2^{KEY} ranges of {IN} leaves on trees of 2 048: gather + check take no longer than the parent's multiproof gather + check",
                      "range_ms": round(new, 4), "parent_route_ms": round(old, 4), "ratio": round(new / old, 4), "met": bool(new <= old)}
line = json.dumps(out)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
bad = [f"{name}: {leg}" for name, group in out["checks"].items() for leg, v in group.items() if not all(x for x in v.values() if isinstance(x, bool))]
if bad:
    sys.exit(f"range_timing: failed {bad}")
