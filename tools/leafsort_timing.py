#!/usr/bin/env python3
"""What sorting the leaves on the device costs (vkmr_hip_forest_sort_leaves_async), timed with HIP events: medians of
interleaved runs in one process after a warm-up of every leg, stamped with the build id.  Prints one JSON line (and writes it to
--out).  GPU box.
    python3 tools/leafsort_timing.py [--log2 26] [--host-log2 22] [--runs 10] [--out profiles/leafsort_timing.json]

  the leaves   2^log2 random digests (hashed leaves look like that), the same for both shapes
  the shapes   trees of 2 048 leaves, and ONE tree
  the legs     per shape: the sort alone, the sort and the stored build over its output, and beside them the stored build alone
               over the unsorted leaves (vkmr_hip_reduce_forest_tree_async); the worst case of the tie step, ONE tree of
               VKMR_LEAFSORT_MAX_TIES leaves under one 64-bit prefix
  the host     the route the device sort replaces, wall clock in this process: download, vk.sort_digests, upload, at 2^host-log2
               leaves in trees of 2 048 (2^26 takes minutes; the smaller figure is a LOWER bound of the larger)
  yardstick    torch.sort of an int64 tensor of as many keys, not the code under test
Every answer is checked before the clock starts: status 0 and n leaves, the sortedness pass over the output finds every tree
strictly increasing, sampled cells of the output are the input cells `order` names, the host route's leaves are the device's.
One requirement: the device sort of 2^log2 leaves takes less than the host route of 2^host-log2."""
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
from vk_merkle_roots_amd import engine, provenance  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log2", type=int, default=26)
ap.add_argument("--host-log2", type=int, default=22)
ap.add_argument("--runs", type=int, default=10)
ap.add_argument("--out", default=None)
a = ap.parse_args()
dev = vk.HipDevice(0)
n = 1 << a.log2
TREE = 2048
MAX_TIES = engine.LEAFSORT_MAX_TIES
rng = np.random.default_rng(30)
chunk = min(n, 1 << 22)


def piece(i):
    """Leaves [i * chunk, (i + 1) * chunk): random words of their own, so that the ties a shape sees are those of n random leaves."""
    return np.random.default_rng(3000 + i).integers(0, 2**32, size=(chunk, 8), dtype=np.uint32)


d_in = dev.alloc(32 * n)
for i in range(n // chunk):
    part = np.ascontiguousarray(piece(i))
    vk.check(dev.lib.vkmr_hip_memcpy_h2d_async(dev.index, dev.stream, d_in.at(32 * i * chunk), part.ctypes.data, part.nbytes), "h2d")
    dev.sync()
d_out, d_order, d_scratch = dev.alloc(32 * n), dev.alloc(4 * n), dev.alloc(dev.sort_leaves_scratch_bytes(n))
yard = torch.randint(-2**62, 2**62, (n,), dtype=torch.int64, device="cuda")


class Shape:
    """The n leaves as trees of `per`: the offsets, the level buffers and the roots of its own."""

    def __init__(self, per):
        self.per, self.ntrees = per, n // per
        self.d_off = dev.upload(np.arange(self.ntrees + 1, dtype=np.uint64) * np.uint64(per))
        self.d_forest, self.d_roots = dev.alloc(dev.forest_tree_bytes(n, self.ntrees, per)), dev.alloc(32 * self.ntrees)
        self.d_info, self.d_status, self.d_bad, self.d_sorted = dev.alloc(32), dev.alloc(4), dev.alloc(8 * self.ntrees), dev.alloc(32)

    def sort(self):
        dev.forest_sort_leaves_enqueue(d_in, n, self.d_off, self.ntrees, self.per, d_scratch, d_out, d_order, self.d_info)

    def sort_and_build(self):
        self.sort()
        dev.reduce_forest_tree_async(d_out, n, self.d_off, self.ntrees, self.per, self.d_forest, self.d_roots, self.d_status)

    def build(self):
        dev.reduce_forest_tree_async(d_in, n, self.d_off, self.ntrees, self.per, self.d_forest, self.d_roots, self.d_status)

    STEPS = ("sort", "sort_and_build", "build")

    def check(self):
        """After sort_and_build: (checks, info) of what lies in d_out, d_order and the roots."""
        info = dev.download(self.d_info, 32, dtype=np.uint64).tolist()
        dev.forest_sorted_enqueue(d_out, n, self.d_off, self.ntrees, self.d_bad, self.d_sorted)
        is_sorted = dev.download(self.d_sorted, 32, dtype=np.uint64).tolist()
        ok = {"status_and_n": info[:2] == [0, n] and int(dev.download(self.d_status, 4)[0]) == 0,
              "strictly_increasing": is_sorted == [0, 0, 0, n - self.ntrees], "sampled_cells": True}
        for at in rng.integers(0, n - 4096, size=8).tolist():          # 8 windows of 4 096 cells: out[j] == in[order[j]], inside j's tree
            order = dev.download(d_order, 4 * 4096, offset=4 * at).astype(np.int64)
            got = dev.download(d_out, 32 * 4096, offset=32 * at).reshape(-1, 8)
            src = np.stack([dev.download(d_in, 32, offset=32 * int(o)) for o in order[::64]])
            ok["sampled_cells"] &= bool((got[::64] == src).all() and ((order // self.per) == (np.arange(at, at + 4096) // self.per)).all())
        return ok, info


class Ties:
    """ONE tree of `count` leaves under one 64-bit prefix: one run, the tie step's worst case."""

    def __init__(self, count):
        self.count = count
        rows = rng.integers(0, 2**32, size=(count, 8), dtype=np.uint32)
        rows[:, 0], rows[:, 1] = 0xC0FFEE00, 0x00C0FFEE
        self.rows = rows
        self.d_in, self.d_out, self.d_order, self.d_info = dev.upload(rows), dev.alloc(32 * count), dev.alloc(4 * count), dev.alloc(32)
        self.d_scratch = dev.alloc(dev.sort_leaves_scratch_bytes(count))

    def sort(self):
        dev.tree_sort_leaves_enqueue(self.d_in, self.count, self.d_scratch, self.d_out, self.d_order, self.d_info)

    def check(self):
        info = dev.download(self.d_info, 32, dtype=np.uint64).tolist()
        got = dev.download(self.d_out, 32 * self.count).reshape(-1, 8)
        return {"status_n_m": info[:3] == [0, self.count, self.count], "leaves": bool((got == vk.sort_digests(self.rows, [self.count])).all())}


def host_route(m):
    """Download, vk.sort_digests, upload of the first m leaves in trees of 2 048: (seconds per stage, the leaves it made)."""
    t0 = time.perf_counter()
    rows = dev.download(d_in, 32 * m).reshape(-1, 8)
    t1 = time.perf_counter()
    done = vk.sort_digests(rows, [min(TREE, m)] * (m // min(TREE, m)))
    t2 = time.perf_counter()
    buf = dev.upload(done)
    t3 = time.perf_counter()
    buf.free()
    return (t1 - t0, t2 - t1, t3 - t2), done


shapes = {"trees_of_2048": Shape(min(TREE, n)), "one_tree": Shape(n)}
ties = Ties(MAX_TIES)
for _ in range(2):                                # warm up until the clocks have settled: every leg and the yardstick
    for s in shapes.values():
        for step in Shape.STEPS:
            getattr(s, step)()
    ties.sort()
    torch.sort(yard)
dev.sync()
torch.cuda.synchronize()

out = {"tool": "leafsort_timing", "leaves_log2": a.log2, "runs": a.runs, "device": dev.name(), "kernel_info": dev.lib.vkmr_hip_kernel_info().decode(),
       "build": provenance.build_id_of(dev.lib.vkmr_hip_kernel_info().decode()), "max_ties": MAX_TIES, "scratch_bytes": dev.sort_leaves_scratch_bytes(n),
       "checks": {}, "shapes": {}}
observed = {}
for name, s in shapes.items():
    s.sort_and_build()
    dev.sync()
    out["checks"][name], observed[name] = s.check()
ties.sort()
dev.sync()
out["checks"]["ties"] = ties.check()
m_host = min(n, 1 << a.host_log2)
shapes["trees_of_2048"].sort()                    # the host route's leaves are the device's, on the leaves both have
dev.sync()
_, host_leaves = host_route(m_host)
out["checks"]["host_route_equals_device"] = bool((host_leaves == dev.download(d_out, 32 * m_host).reshape(-1, 8)).all())

ev = {(name, step): [(dev.new_event(), dev.new_event()) for _ in range(a.runs)] for name in shapes for step in Shape.STEPS}
ev_ties = [(dev.new_event(), dev.new_event()) for _ in range(a.runs)]
tev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.runs)]
for r in range(a.runs):
    for name, s in shapes.items():                # every leg once per round, each waiting for the one before
        for step in Shape.STEPS:
            e0, e1 = ev[name, step][r]
            dev.record(e0); getattr(s, step)(); dev.record(e1)
            dev.sync()
    e0, e1 = ev_ties[r]
    dev.record(e0); ties.sort(); dev.record(e1)
    dev.sync()
    t0, t1 = tev[r]
    t0.record(); torch.sort(yard); t1.record()
    torch.cuda.synchronize()
host = [host_route(m_host)[0] for _ in range(3)]

yard_ms = [t0.elapsed_time(t1) for t0, t1 in tev]
ties_ms = [dev.elapsed_ms(e0, e1) for e0, e1 in ev_ties]
for name, s in shapes.items():
    ms = {step: [dev.elapsed_ms(e0, e1) for e0, e1 in ev[name, step]] for step in Shape.STEPS}
    med = {step: float(np.median(v)) for step, v in ms.items()}
    shape = (max(0, (s.ntrees - 1).bit_length()), min(64 - (s.ntrees - 1).bit_length(), 2 * s.per.bit_length() + 8))
    out["shapes"][name] = {"trees": s.ntrees, "leaves_per_tree": s.per, "key_bits": list(shape), "passes": -(-sum(shape) // 8),
                           "sort_ms": round(med["sort"], 4), "sort_and_build_ms": round(med["sort_and_build"], 4), "build_ms": round(med["build"], 4),
                           "sort_ms_per_pass_with_the_rest": round(med["sort"] / -(-sum(shape) // 8), 4),
                           "sort_over_torch_sort": round(med["sort"] / float(np.median(yard_ms)), 3),
                           "ties_observed": int(observed[name][2]), "ties_estimate_n_over_512_max_count": round(n / (512 * s.per), 3),
                           "repeats_observed": int(observed[name][3]),
                           "min_max_ms": {step: [round(min(v), 4), round(max(v), 4)] for step, v in ms.items()}}
host_med = [float(np.median([h[j] for h in host])) for j in range(3)]
sort_ms = out["shapes"]["trees_of_2048"]["sort_ms"]
out["torch_sort_int64_ms"] = round(float(np.median(yard_ms)), 4)
out["worst_case_ties"] = {"leaves_in_one_run": MAX_TIES, "sort_ms": round(float(np.median(ties_ms)), 4), "min_max_ms": [round(min(ties_ms), 4), round(max(ties_ms), 4)],
                          "plain_sort_of_all_leaves_ms": sort_ms, "within_the_plain_sort": bool(np.median(ties_ms) <= sort_ms)}
out["host_route"] = {"leaves_log2": int(np.log2(m_host)), "download_s": round(host_med[0], 4), "sort_digests_s": round(host_med[1], 4),
                     "upload_s": round(host_med[2], 4), "total_s": round(sum(host_med), 4), "runs": 3,
                     "device_sort_of_all_leaves_s": round(sort_ms * 1e-3, 6), "host_over_device": round(sum(host_med) / (sort_ms * 1e-3), 1),
                     "note": f"the host figure is for 2^{int(np.log2(m_host))} leaves, the device figure for 2^{a.log2}"}
out["requirement"] = {"device_sort_beats_the_host_route": bool(sort_ms * 1e-3 < sum(host_med))}
line = json.dumps(out)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
bad = [k for k, v in out["checks"].items() if not (all(v.values()) if isinstance(v, dict) else v)]
if bad or not out["requirement"]["device_sort_beats_the_host_route"]:
    sys.exit(f"leafsort_timing: failed {bad or 'the requirement'}")
