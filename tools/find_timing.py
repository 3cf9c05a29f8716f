#!/usr/bin/env python3
"""What a lookup by digest costs (vkmr_hip_forest_find_async), timed with HIP events: medians of interleaved runs in one process
after a warm-up of every leg, stamped with the build id.  Prints one JSON line (and writes it to --out).  GPU box.
    python3 tools/find_timing.py [--log2 26] [--runs 10] [--before-log2 24] [--out profiles/find_timing.json]

  the forest   2^log2 random leaves in trees of 2048
  the legs     k = 1, 2^10, 2^16, 2^20 queries in random order, half of them leaves of the forest, half absent
  yardstick    beside every leg, in this process and not the code under test: torch's sum over an int32 tensor of the same
               32 * total bytes, a read-only pass; its rate is the read rate HBM is taken to give, and 32 * total bytes over it
               the floor a scan is held against
  before       once, at 2^before-log2 leaves: the route a caller had without the call -- level 0 downloaded, then looked up on
               the host (vkmr_host_cpu_forest_find, 2^10 queries); wall clock
Every leg's answers are checked before the clock starts: the present half at the positions they were taken from, the rest not
found."""
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

ap = argparse.ArgumentParser()
ap.add_argument("--log2", type=int, default=26)
ap.add_argument("--runs", type=int, default=10)
ap.add_argument("--before-log2", type=int, default=24)
ap.add_argument("--out", default=None)
a = ap.parse_args()
dev = vk.HipDevice(0)
n = 1 << a.log2
TREE = 2048
ntrees = max(1, n // TREE)
offsets = np.arange(ntrees + 1, dtype=np.uint64) * np.uint64(n // ntrees)
rng = np.random.default_rng(11)
d_leaves = dev.alloc(32 * n)
chunk = min(n, 1 << 22)
base = rng.integers(0, 2**32, size=(chunk, 8), dtype=np.uint32)


def piece(i):
    """Leaves [i * chunk, (i + 1) * chunk): one random piece, made different per piece."""
    return base ^ np.uint32(i * 2654435761 & 0xFFFFFFFF)


for i in range(n // chunk):
    part = piece(i)
    vk.check(dev.lib.vkmr_hip_memcpy_h2d_async(dev.index, dev.stream, d_leaves.at(32 * i * chunk), part.ctypes.data, part.nbytes), "h2d")
    dev.sync()
d_off = dev.upload(offsets)


class Leg:
    """k queries, half of them leaves: buffers of its own (the legs are interleaved)."""

    def __init__(self, k):
        self.k = k
        self.pos = np.unique(rng.integers(0, n, size=(k + 1) // 2)).astype(np.int64)      # sorted; a repeat drawn twice counts once
        present = self._gather()
        absent = rng.integers(0, 2**32, size=(k - self.pos.shape[0], 8), dtype=np.uint32)
        self.order = rng.permutation(k)
        self.queries = np.concatenate([present, absent])[self.order]
        self.d_q, self.d_scr = dev.upload(self.queries), dev.alloc(dev.find_scratch_bytes(k))
        self.d_trees, self.d_idx = dev.alloc(4 * k), dev.alloc(8 * k)

    def _gather(self):
        out = np.empty((self.pos.shape[0], 8), dtype=np.uint32)
        which = self.pos // chunk
        for i in np.unique(which):
            sel = which == i
            out[sel] = piece(int(i))[self.pos[sel] % chunk]
        return out

    def run(self):
        dev.forest_find_async(d_leaves, n, d_off, ntrees, self.d_q, self.k, self.d_scr, self.d_trees, self.d_idx)

    def check(self):
        trees, idx = dev.download(self.d_trees, 4 * self.k), dev.download(self.d_idx, 8 * self.k, dtype=np.uint64)
        want_t = np.full(self.k, vk.NO_TREE, dtype=np.uint32)
        want_i = np.full(self.k, vk.NOT_FOUND, dtype=np.uint64)
        per = n // ntrees
        want_t[: self.pos.shape[0]], want_i[: self.pos.shape[0]] = self.pos // per, self.pos % per
        return bool((trees == want_t[self.order]).all() and (idx == want_i[self.order]).all())


legs = [Leg(k) for k in (1, 1 << 10, 1 << 16, 1 << 20)]
yard = torch.empty(8 * n, dtype=torch.int32, device="cuda").random_()          # 32 * n bytes of its own
checks = {}
for _ in range(3):                            # warm up until the clocks have settled, every leg and the yardstick
    for leg in legs:
        leg.run()
        yard.sum()
dev.sync()
torch.cuda.synchronize()
for leg in legs:
    checks[f"k_{leg.k}_answers"] = leg.check()
ev = {leg.k: [(dev.new_event(), dev.new_event()) for _ in range(a.runs)] for leg in legs}
tev = {leg.k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.runs)] for leg in legs}
for r in range(a.runs):
    for leg in legs:                          # the leg, then its yardstick; each on its own stream, so each waits for the other to end
        e0, e1 = ev[leg.k][r]
        dev.record(e0); leg.run(); dev.record(e1)
        dev.sync()
        t0, t1 = tev[leg.k][r]
        t0.record(); yard.sum(); t1.record()
        torch.cuda.synchronize()
find_ms = {k: [dev.elapsed_ms(e0, e1) for e0, e1 in v] for k, v in ev.items()}
yard_ms = {k: [t0.elapsed_time(t1) for t0, t1 in v] for k, v in tev.items()}
out = {"tool": "find_timing", "leaves_log2": a.log2, "trees_of": n // ntrees, "ntrees": ntrees, "runs": a.runs, "bytes_read": 32 * n, "checks": checks,
       "device": dev.name(), "kernel_info": dev.lib.vkmr_hip_kernel_info().decode(), "legs": {}}
for leg in legs:
    f, y = float(np.median(find_ms[leg.k])), float(np.median(yard_ms[leg.k]))
    out["legs"][str(leg.k)] = {"find_ms": round(f, 4), "find_ms_min_max": [round(min(find_ms[leg.k]), 4), round(max(find_ms[leg.k]), 4)],
                               "yardstick_ms": round(y, 4), "yardstick_GB_per_s": round(32 * n / (y * 1e-3) / 1e9, 1),
                               "find_GB_per_s": round(32 * n / (f * 1e-3) / 1e9, 1), "find_over_yardstick": round(f / y, 3),
                               "table_bytes": 8 * max(64, 1 << (2 * leg.k - 1).bit_length())}

# the route a caller had before, once: level 0 to the host, a lookup there
m = min(n, 1 << a.before_log2)
before = legs[1]
t0 = time.perf_counter()
host = dev.download(d_leaves, 32 * m).reshape(m, 8)
t1 = time.perf_counter()
trees, idx = np.empty(before.k, dtype=np.uint32), np.empty(before.k, dtype=np.uint64)
off_m = np.array([0, m], dtype=np.uint64)
rc = vk.host_lib().vkmr_host_cpu_forest_find(host.ctypes.data, m, off_m.ctypes.data, 1, before.queries.ctypes.data, before.k, trees.ctypes.data,
                                             idx.ctypes.data)
t2 = time.perf_counter()
out["before"] = {"leaves_log2": int(np.log2(m)), "queries": before.k, "download_ms": round((t1 - t0) * 1e3, 2), "host_lookup_ms": round((t2 - t1) * 1e3, 2),
                 "download_GB_per_s": round(32 * m / (t1 - t0) / 1e9, 1), "rc": rc, "found": int((trees != vk.NO_TREE).sum())}
line = json.dumps(out)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
