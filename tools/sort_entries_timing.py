#!/usr/bin/env python3
"""Leaf entries sorted and deduplicated on the device (vkmr_hip_forest_sort_entries_async) in front of an update of a stored
forest, beside the route through the host that a caller had before, and the sort alone beside torch.sort: medians of
interleaved runs in one process after a warm-up, stamped with the build id.  Prints one JSON line (and writes it to --out).
GPU box.
    python3 tools/sort_entries_timing.py [--log2 26] [--tree-log2 11] [--ks 10,16,20] [--runs 10] [--out FILE]

  forest     2^(log2 - tree-log2) trees of 2^tree-log2 random leaves, every level stored
  entries    k random (tree, index) entries in DEVICE memory in call order, about 1 % of them repeats of another entry and
             1 % "not found" markers, and k new leaves beside them
  (a)        the device route: sort, the 32 bytes of counters read back, the leaves gathered by `order`,
             vkmr_hip_forest_update_async over the n survivors -- events around all of it, and the wall time
  (b)        the route through the host: the entries downloaded, the markers dropped, MerkleForest._update_order (lexsort, last
             occurrence wins), the sorted entries and the permuted leaves uploaded, the same update call -- wall time; the host
             step alone is reported too
  (c)        the sort alone (events) beside torch.sort of an int64 tensor holding the same flat keys: a yardstick for a radix
             sort of this size on this part, not the code under test
After the timing the roots (a) and (b) leave are compared with each other, on what was timed."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vk_merkle_roots_amd as vk  # noqa: E402
from vk_merkle_roots_amd import provenance  # noqa: E402
from vk_merkle_roots_amd.engine import forest_offsets  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log2", type=int, default=26)
ap.add_argument("--tree-log2", type=int, default=11)
ap.add_argument("--ks", default="10,16,20", help="log2 of the entry counts")
ap.add_argument("--runs", type=int, default=10)
ap.add_argument("--out", default=None)
a = ap.parse_args()
dev = vk.HipDevice(0)
n, cap = 1 << a.log2, 1 << min(a.tree_log2, a.log2)
rng = np.random.default_rng(7)
d_in = dev.alloc(32 * n)
chunk = min(n, 1 << 22)
base = rng.integers(0, 2**32, size=(chunk, 8), dtype=np.uint32)
for at in range(0, n, chunk):   # random digests, uploaded in pieces: one random piece, made different per piece
    part = base ^ np.uint32(at // chunk * 2654435761 & 0xFFFFFFFF)
    vk.check(dev.lib.vkmr_hip_memcpy_h2d_async(dev.index, dev.stream, d_in.at(32 * at), part.ctypes.data, part.nbytes), "h2d")
    dev.sync()

counts = [cap] * (n // cap)
offsets, ntrees = forest_offsets(counts)
d_off, d_status = dev.upload(offsets), dev.alloc(4)
d_forest, d_roots = dev.alloc(dev.forest_tree_bytes(n, ntrees, cap)), dev.alloc(32 * ntrees)
forest = vk.MerkleForest(dev, d_in, n, counts, d_off, cap, d_forest, d_roots)


def rebuild():
    dev.reduce_forest_tree_async(d_in, n, d_off, ntrees, cap, d_forest, d_roots, d_status)


class Leg:
    """k entries in call order on the device, their new leaves, and the buffers of both routes."""

    def __init__(self, k):
        self.k = k
        flat = rng.integers(0, n, size=k, dtype=np.uint64)
        rep = rng.integers(0, k, size=max(1, k // 100))
        flat[rep] = flat[rng.integers(0, k, size=rep.shape[0])]
        self.trees, self.idx = (flat >> np.uint64(a.tree_log2)).astype(np.uint32), flat & np.uint64(cap - 1)
        mark = rng.integers(0, k, size=max(1, k // 100))
        self.trees[mark], self.idx[mark] = vk.NO_TREE, np.uint64(vk.NOT_FOUND)
        self.leaves = rng.integers(0, 2**32, size=(k, 8), dtype=np.uint32)
        self.flat = np.where(self.trees == vk.NO_TREE, np.uint64(n), flat)
        self.d_trees, self.d_idx, self.d_leaves = dev.upload(self.trees), dev.upload(self.idx), dev.upload(self.leaves)
        self.d_scr = dev.alloc(dev.sort_entries_scratch_bytes(n, k))
        self.d_st, self.d_si, self.d_order, self.d_info, self.d_sorted_leaves = dev.alloc(4 * k), dev.alloc(8 * k), dev.alloc(4 * k), dev.alloc(32), dev.alloc(32 * k)
        self.t_keys = torch.from_numpy(self.flat.astype(np.int64)).cuda()
        self.info, self.host_ms = None, []

    def sort(self):
        forest.sort_entries_async(self.d_trees, self.d_idx, self.k, self.d_scr, self.d_st, self.d_si, self.d_order, self.d_info)

    def device_route(self):
        self.sort()
        self.info = [int(x) for x in dev.download(self.d_info, 32, dtype=np.uint64)]
        m = self.info[0]
        dev.gather_digests_async(self.d_leaves, self.d_order, m, self.d_sorted_leaves)
        forest.update_async(self.d_st, self.d_si, self.d_sorted_leaves, m, d_status)

    def host_route(self):
        trees, idx = dev.download(self.d_trees, 4 * self.k), dev.download(self.d_idx, 8 * self.k, dtype=np.uint64)
        t0 = time.perf_counter()
        keep = trees != vk.NO_TREE
        st, si, pos = forest._update_order(trees[keep], idx[keep])
        lv = np.ascontiguousarray(self.leaves[np.flatnonzero(keep)[pos]])
        self.host_ms.append((time.perf_counter() - t0) * 1e3)
        with dev.scope() as tmp:
            forest.update_async(tmp.upload(st), tmp.upload(si), tmp.upload(lv), int(si.shape[0]), d_status)
            dev.sync()


def wall(fn):
    dev.sync()
    t0 = time.perf_counter()
    fn()
    dev.sync()
    return (time.perf_counter() - t0) * 1e3


legs = [Leg(min(1 << int(x), n)) for x in a.ks.split(",")]
rebuild()
for _ in range(3):              # a warm-up of every shape
    for leg in legs:
        leg.device_route()
        leg.host_route()
        torch.sort(leg.t_keys)
        leg.host_ms = []
dev.sync()
torch.cuda.synchronize()
ev = {(leg.k, what): [(dev.new_event(), dev.new_event()) for _ in range(a.runs)] for leg in legs for what in ("route", "sort")}
tev = {leg.k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.runs)] for leg in legs}
walls = {(leg.k, what): [] for leg in legs for what in ("device", "host")}
for r in range(a.runs):
    for leg in legs:
        e0, e1 = ev[(leg.k, "route")][r]

        def timed():
            dev.record(e0); leg.device_route(); dev.record(e1)
        walls[(leg.k, "device")].append(wall(timed))
        walls[(leg.k, "host")].append(wall(leg.host_route))
        e0, e1 = ev[(leg.k, "sort")][r]
        dev.record(e0); leg.sort(); dev.record(e1)
        dev.sync()
        t0, t1 = tev[leg.k][r]
        t0.record(); torch.sort(leg.t_keys); t1.record()
        torch.cuda.synchronize()
med = lambda v: float(np.median(np.asarray(v)))      # noqa: E731

# correctness of what was timed: both routes from a fresh build, their roots and the leaves' cells compared
checks = {}
for leg in legs:
    rebuild()
    leg.device_route()
    status_a = int(dev.download(d_status, 4)[0])
    roots_a = dev.download(d_roots, 32 * ntrees)
    rebuild()      # the leaves stay as (a) left them: (b) writes the same values again, and must reach the same roots from a fresh build
    leg.host_route()
    status_b = int(dev.download(d_status, 4)[0])
    roots_b = dev.download(d_roots, 32 * ntrees)
    checks[str(leg.k)] = {"status_device_route": status_a, "status_host_route": status_b, "roots_equal": bool((roots_a == roots_b).all()),
                          "info": leg.info, "counters_add_up": sum(leg.info) == leg.k}

info = dev.lib.vkmr_hip_kernel_info().decode()
out = {"tool": "sort_entries_timing", "leaves_log2": a.log2, "tree_log2": a.tree_log2, "ntrees": ntrees, "runs": a.runs, "device": dev.name(),
       "kernel_info": info, "build": provenance.build_id_of(info), "torch": torch.__version__, "checks": checks,
       "all_checks_ok": all(c["status_device_route"] == 0 and c["status_host_route"] == 0 and c["roots_equal"] and c["counters_add_up"]
                            for c in checks.values()),
       "legs": {}}
for leg in legs:
    route = med([dev.elapsed_ms(e0, e1) for e0, e1 in ev[(leg.k, "route")]])
    sort = med([dev.elapsed_ms(e0, e1) for e0, e1 in ev[(leg.k, "sort")]])
    tsort = med([t0.elapsed_time(t1) for t0, t1 in tev[leg.k]])
    wa, wb = med(walls[(leg.k, "device")]), med(walls[(leg.k, "host")])
    out["legs"][str(leg.k)] = {"k": leg.k, "passes": (n.bit_length() + 7) // 8, "device_route_events_ms": round(route, 4), "device_route_wall_ms": round(wa, 4),
                               "host_route_wall_ms": round(wb, 4), "host_step_alone_ms": round(med(leg.host_ms), 4), "a_over_b": round(wa / wb, 4),
                               "sort_ms": round(sort, 4), "torch_sort_ms": round(tsort, 4), "sort_over_torch_sort": round(sort / tsort, 3),
                               "sorted_entries_per_s": leg.k / (sort * 1e-3)}
line = json.dumps(out)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
