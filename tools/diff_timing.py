#!/usr/bin/env python3
"""What a diff of two stored forests costs (vkmr_hip_forest_diff_async, vkmr_hip_tree_diff_async): medians of interleaved runs in
one process after a warm-up of every leg, stamped with the build id.  Prints one JSON line (and writes it to --out).  GPU box.
    python3 tools/diff_timing.py [--log2 26] [--tree-log2 11] [--runs 10] [--out profiles/diff_timing.json]

  the shapes   2^log2 random leaves as 2^(log2 - tree-log2) trees of 2^tree-log2, and the same leaves as one tree
  the legs     n = 1, 2^10, 2^16, 2^20 random differing leaves (B = A with one bit of each of those leaves flipped)
    (a) diff        the call with capacity n and B's leaves, the 32 bytes of counters read back: wall clock, the event time beside it
    (b) compare     what a caller has without the call, and not the code under test: torch over the two level-0 buffers,
                    (A != B).any(1).nonzero(), wall clock with the answer's size read back
    (c) sync_from   a working copy of A brought to B (diff, counters, update), wall clock, beside a rebuild of that copy over
                    B's leaves (a device copy of level 0 and vkmr_hip_reduce_forest_tree_async / vkmr_hip_reduce_tree_async)
Checked on what was timed: the answers of (a) and (b) are the planted positions, and the roots after (c) are B's."""
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

ap = argparse.ArgumentParser()
ap.add_argument("--log2", type=int, default=26)
ap.add_argument("--tree-log2", type=int, default=11)
ap.add_argument("--runs", type=int, default=10)
ap.add_argument("--out", default=None)
a = ap.parse_args()
dev = vk.HipDevice(0)
total = 1 << a.log2
per = 1 << min(a.tree_log2, a.log2)
ntrees = total // per
counts = [per] * ntrees
NS = [n for n in (1, 1 << 10, 1 << 16, 1 << 20) if n <= total]
gen = torch.Generator(device="cuda").manual_seed(11)


class Leaves:
    """A level-0 buffer that torch owns, as the engine's calls take it."""

    def __init__(self, tensor):
        self.t = tensor
        self.ptr = tensor.data_ptr()

    def at(self, byte_offset):
        return self.ptr + int(byte_offset)

    def free(self):
        pass


class Side:
    """One replica: its leaves, and over them a stored forest and a stored tree."""

    def __init__(self, tensor):
        self.leaves = Leaves(tensor)
        torch.cuda.synchronize()
        self.forest = dev._build_forest_of_buffer(self.leaves, total, counts, per, "diff_timing")
        self.tree = dev.build_tree(self.leaves, total)
        dev.sync()


base = torch.randint(-2**31, 2**31 - 1, (total, 8), dtype=torch.int32, device="cuda", generator=gen)
A = Side(base)
work = Side(base.clone())
rng = np.random.default_rng(11)
d_status = dev.alloc(4)


class Leg:
    def __init__(self, n):
        self.n = n
        self.pos = np.sort(rng.choice(total, size=n, replace=False)).astype(np.int64)
        tb = base.clone()
        at = torch.from_numpy(self.pos).cuda()
        tb[at, (at % 8)] ^= 1 << 7
        self.B = Side(tb)
        self.d_scr = dev.alloc(dev.diff_scratch_bytes(n))
        self.d_trees, self.d_idx, self.d_lv, self.d_info = dev.alloc(4 * n), dev.alloc(8 * n), dev.alloc(32 * n), dev.alloc(32)
        self.info = {}

    def launch(self, shape):
        if shape == "forest":
            A.forest.diff_async(self.B.forest, self.d_scr, self.d_trees, self.d_idx, self.d_lv, self.n, self.d_info)
        else:
            A.tree.diff_async(self.B.tree, self.d_scr, self.d_idx, self.d_lv, self.n, self.d_info)

    def read(self):
        return tuple(int(x) for x in dev.download(self.d_info, 32, dtype=np.uint64))       # the read-back a caller makes: syncs

    def diff(self, shape):
        self.launch(shape)
        return self.read()

    def diff_ok(self, shape):
        info = self.diff(shape)
        self.info[shape] = info
        idx = dev.download(self.d_idx, 8 * self.n, dtype=np.uint64).astype(np.int64)
        if shape == "forest":
            idx = dev.download(self.d_trees, 4 * self.n).astype(np.int64) * per + idx
        lv = torch.from_numpy(dev.download(self.d_lv, 32 * self.n).view(np.int32).reshape(self.n, 8))
        return bool(info[0] == 0 and info[1] == self.n and (idx == self.pos).all() and (lv == self.B.leaves.t[torch.from_numpy(self.pos).cuda()].cpu()).all())

    def compare(self):
        return (A.leaves.t != self.B.leaves.t).any(1).nonzero()

    def sync(self, shape):
        """work := B, then work := A again (the same work the other way round), each timed; the roots checked after the first."""
        w, b, o = (work.forest, self.B.forest, A.forest) if shape == "forest" else (work.tree, self.B.tree, A.tree)
        t0 = time.perf_counter()
        n = w.sync_from(b)
        t1 = time.perf_counter()
        same = (w.roots() == b.roots()).all() if shape == "forest" else (w.root() == b.root()).all()
        t2 = time.perf_counter()
        back = w.sync_from(o)
        t3 = time.perf_counter()
        return (t1 - t0) * 1e3, (t3 - t2) * 1e3, bool(same and n == self.n and back == self.n)

    def rebuild(self, shape):
        """What a caller without a diff does to bring `work` to B: level 0 copied, every level formed again.  Then back to A."""
        times = []
        for src in (self.B, A):
            t0 = time.perf_counter()
            work.leaves.t.copy_(src.leaves.t)
            torch.cuda.synchronize()
            if shape == "forest":
                f = work.forest
                dev.reduce_forest_tree_async(f.digests, f.total, f.offsets, f.ntrees, f.max_count, f.forest, f.roots_buf, d_status)
            else:
                dev.reduce_tree_async(work.leaves, total, work.tree.height, work.tree.tree)
            dev.sync()
            times.append((time.perf_counter() - t0) * 1e3)
        return times[0]


legs = [Leg(n) for n in NS]
SHAPES = ("forest", "tree")
checks = {}
for shape in SHAPES:                          # warm up every leg; the answers checked on the way
    for leg in legs:
        checks[f"{shape}_n_{leg.n}_diff"] = leg.diff_ok(shape)
        leg.diff(shape)
        ok = leg.sync(shape)[2]
        checks[f"{shape}_n_{leg.n}_sync_roots"] = ok
        leg.rebuild(shape)
for leg in legs:
    got = leg.compare().flatten().cpu().numpy()
    checks[f"n_{leg.n}_compare"] = bool((got == leg.pos).all())
torch.cuda.synchronize()

wall = {(s, leg.n): [] for s in SHAPES for leg in legs}
event = {(s, leg.n): [] for s in SHAPES for leg in legs}
sync_ms = {(s, leg.n): [] for s in SHAPES for leg in legs}
rebuild_ms = {(s, leg.n): [] for s in SHAPES for leg in legs}
compare_ms = {leg.n: [] for leg in legs}
e0, e1 = dev.new_event(), dev.new_event()
for r in range(a.runs):
    for leg in legs:
        for shape in SHAPES:
            t0 = time.perf_counter()
            dev.record(e0)
            leg.launch(shape)
            dev.record(e1)
            leg.read()
            wall[(shape, leg.n)].append((time.perf_counter() - t0) * 1e3)
            event[(shape, leg.n)].append(dev.elapsed_ms(e0, e1))
            there, back, ok = leg.sync(shape)
            sync_ms[(shape, leg.n)] += [there, back]
            checks[f"{shape}_n_{leg.n}_sync_roots"] &= ok
            rebuild_ms[(shape, leg.n)].append(leg.rebuild(shape))
        t0 = time.perf_counter()
        k = int(leg.compare().shape[0])
        compare_ms[leg.n].append((time.perf_counter() - t0) * 1e3)
        checks[f"n_{leg.n}_compare"] &= k == leg.n

med = lambda v: round(float(np.median(v)), 4)      # noqa: E731
info = dev.lib.vkmr_hip_kernel_info().decode()
out = {"tool": "diff_timing", "leaves_log2": a.log2, "trees_of": per, "ntrees": ntrees, "runs": a.runs, "device": dev.name(), "kernel_info": info,
       "build": provenance.build_id_of(info), "torch": torch.__version__, "checks": checks, "all_checks": all(checks.values()),
       "level0_bytes_compared": 2 * 32 * total, "legs": {}}
for leg in legs:
    row = {"compare_wall_ms": med(compare_ms[leg.n])}
    for shape in SHAPES:
        row[shape] = {"diff_wall_ms": med(wall[(shape, leg.n)]), "diff_event_ms": med(event[(shape, leg.n)]), "info": list(leg.info[shape]),
                      "diff_over_compare": round(med(wall[(shape, leg.n)]) / med(compare_ms[leg.n]), 4), "sync_from_wall_ms": med(sync_ms[(shape, leg.n)]),
                      "rebuild_wall_ms": med(rebuild_ms[(shape, leg.n)])}
    out["legs"][str(leg.n)] = row
line = json.dumps(out)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
