#!/usr/bin/env python3
"""What following a tree that grows costs a holder of its frontier alone (vkmr_hip_frontier_extend_async) beside the primary's own
extend of the stored tree (vkmr_hip_forest_extend_async, the same number of launches) and beside what such a follower could do
without a frontier: hold every leaf and reduce again (vkmr_hip_reduce_forest_async over all c + n leaves).  Every repetition of
every leg interleaved in one process, from events, after a warm-up of every leg, stamped with the build id.  Prints one JSON line
(and writes it to --out).  GPU box.
    python3 tools/frontier_extend_timing.py [--log2 26] [--room-log2 16] [--tree-log2 11] [--runs 10] [--out profiles/frontier_extend_timing.json]

  the shapes   `one_tree`: ONE tree of 2^log2 - 2^room-log2 leaves; n = 1, 2^10, 2^room-log2 arrive
               `last_of_many`: an open tree of 2^(tree-log2 - 1) leaves behind 2^log2 / 2^tree-log2 - 1 trees of 2^tree-log2;
               n = 1, 64, 2^(tree-log2 - 1) arrive at the open tree
  the legs     frontier_n       the follower: ONE frontier (the open tree's cells of its arrays), the n leaves, out of place so
                                that every repetition starts from the same frontier
               all_trees_n      (last_of_many) the follower's call over the frontiers of ALL trees, n_q == 0 for every other one
               forest_extend_n  the primary: the n leaves copied into the stored forest and its right edge rehashed (shrunk back
                                outside the timing)
               reduce_n         vkmr_hip_reduce_forest_async over all the leaves, the n new ones included: roots only
Checked on what was timed: every status word is 0, and after each step the follower's root of the open tree (for all_trees: every
root) equals the primary's.  The requirement is for `one_tree`, where the work is at most 2^-10 of the tree: at every n the
follower's slowest repetition is below the fastest full reduction.  The ratio to forest_extend is recorded, not required."""
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
ap.add_argument("--room-log2", type=int, default=16)
ap.add_argument("--tree-log2", type=int, default=11)
ap.add_argument("--runs", type=int, default=10)
ap.add_argument("--out", default=None)
a = ap.parse_args()
dev = vk.HipDevice(0)
gen = torch.Generator(device="cuda").manual_seed(24)


class Leaves:
    """A level-0 buffer that torch owns, as the engine's calls take it."""

    def __init__(self, tensor):
        self.t = tensor
        self.ptr = tensor.data_ptr()

    def at(self, byte_offset):
        return self.ptr + int(byte_offset)

    def free(self):
        pass


class At:
    """An address inside a buffer."""

    def __init__(self, ptr):
        self.ptr = ptr


d_status = dev.alloc(4)
statuses = []


class Shape:
    """The primary's stored forest with `room` free cells behind its open tree, the `room` leaves that arrive, and the follower's
    frontiers of it in device memory."""

    def __init__(self, name, counts, room, max_count, ns):
        self.name, self.counts, self.room, self.ns = name, counts, room, ns
        used = sum(counts)
        self.used, self.T, self.tree, self.count = used, len(counts), len(counts) - 1, counts[-1]
        self.leaves = Leaves(torch.randint(-2**31, 2**31 - 1, (used + room, 8), dtype=torch.int32, device="cuda", generator=gen))
        self.new = Leaves(self.leaves.t[used:].clone())
        torch.cuda.synchronize()
        self.f = dev._build_forest_of_buffer(self.leaves, used + room, counts, max_count, "frontier_extend_timing", reserve_leaves=room)
        frontier = self.f.frontier()
        self.stride = frontier.stride
        self.d_counts, self.d_peaks = dev.upload(frontier.counts), dev.upload(frontier.peaks)
        self.d_new_counts, self.d_new_peaks = dev.alloc(8 * self.T), dev.alloc(32 * self.T * self.stride)
        self.d_roots = dev.alloc(32 * self.T)
        self.scratch = dev.frontier_extend_scratch(room, self.T)
        offsets = np.array(np.concatenate([[0], np.cumsum(counts)]), dtype=np.uint64)
        self.d_one, self.d_all, self.d_grown = {}, {}, {}
        for n in ns:
            self.d_one[n] = dev.upload(np.array([0, n], dtype=np.uint64))
            self.d_all[n] = dev.upload(np.array([0] * self.T + [n], dtype=np.uint64))
            grown = offsets.copy()
            grown[-1] += n
            self.d_grown[n] = dev.upload(grown)
        self.d_reduce_scratch = dev.alloc(dev.lib.vkmr_hip_forest_scratch_bytes(used + room, self.T))
        self.d_reduce_roots = dev.alloc(32 * self.T)
        dev.sync()

    def frontier_one(self, n):
        q, s = self.tree, self.stride
        dev.frontier_extend_enqueue(At(self.d_counts.at(8 * q)), At(self.d_peaks.at(32 * q * s)), s, 1, self.new, n, self.d_one[n], n, self.scratch,
                                    At(self.d_new_counts.at(8 * q)), At(self.d_new_peaks.at(32 * q * s)), At(self.d_roots.at(32 * q)), d_status)

    def frontier_all(self, n):
        dev.frontier_extend_enqueue(self.d_counts, self.d_peaks, self.stride, self.T, self.new, n, self.d_all[n], n, self.scratch, self.d_new_counts,
                                    self.d_new_peaks, self.d_roots, d_status)

    def forest_extend(self, n):
        self.f.extend_async(self.new, n, d_status)

    def back(self, n):
        self.f.extended(n)
        self.f.shrink_async(n, d_status)
        self.f.shrunk(n)

    def reduce(self, n):
        dev.reduce_forest_async(self.leaves, self.used + n, self.d_grown[n], self.T, self.f.max_count, self.d_reduce_scratch, self.d_reduce_roots, d_status)

    def primary_roots(self):
        return dev.download(self.f.roots_buf, 32 * self.T).reshape(self.T, 8)

    def follower_roots(self):
        return dev.download(self.d_roots, 32 * self.T).reshape(self.T, 8)


def status_ok():
    return int(dev.download(d_status, 4)[0]) == 0


def timed(fn, e0, e1):
    dev.record(e0)
    fn()
    dev.record(e1)
    dev.sync()
    statuses.append(int(dev.download(d_status, 4)[0]))
    return dev.elapsed_ms(e0, e1)


per = 1 << a.tree_log2
room = 1 << a.room_log2
shapes = [Shape("one_tree", [(1 << a.log2) - room], room, 1 << a.log2, sorted({1, min(1 << 10, room), room})),
          Shape("last_of_many", [per] * ((1 << a.log2) // per - 1) + [per // 2], per // 2, per, sorted({1, min(64, per // 2), per // 2}))]
e0, e1 = dev.new_event(), dev.new_event()
checks = {}
for g in shapes:                                   # warm up every leg; the answers checked on the way
    start = g.primary_roots()
    for n in g.ns:
        g.forest_extend(n)                         # the new leaves are in the primary's level 0 from here on: the reduction reads them there
        ok = status_ok()
        want = g.primary_roots()
        g.back(n)
        ok = ok and status_ok() and bool((g.primary_roots() == start).all()) and not bool((want[g.tree] == start[g.tree]).all())
        g.frontier_one(n)
        ok = ok and status_ok()
        checks[f"{g.name}_frontier_{n}_root_is_the_primarys"] = ok and bool((g.follower_roots()[g.tree] == want[g.tree]).all())
        if g.T > 1:
            g.frontier_all(n)
            checks[f"{g.name}_all_trees_{n}_roots_are_the_primarys"] = status_ok() and bool((g.follower_roots() == want).all())
        g.reduce(n)
        checks[f"{g.name}_reduce_{n}_roots_are_the_primarys"] = status_ok() and bool((dev.download(g.d_reduce_roots, 32 * g.T).reshape(g.T, 8) == want).all())
    dev.sync()

ms = {g.name: {f"{leg}_{n}": [] for n in g.ns for leg in ("frontier", "forest_extend", "reduce") + (("all_trees",) if g.T > 1 else ())} for g in shapes}
for r in range(a.runs):
    for g in shapes:
        legs = ms[g.name]
        for n in g.ns:
            legs[f"frontier_{n}"].append(timed(lambda: g.frontier_one(n), e0, e1))
            if g.T > 1:
                legs[f"all_trees_{n}"].append(timed(lambda: g.frontier_all(n), e0, e1))
            legs[f"forest_extend_{n}"].append(timed(lambda: g.forest_extend(n), e0, e1))
            g.back(n)
            legs[f"reduce_{n}"].append(timed(lambda: g.reduce(n), e0, e1))
dev.sync()
checks["every_status_word_is_0"] = all(s == 0 for s in statuses) and status_ok()
for g in shapes:                                   # and the last repetition left the answers of the first
    n = g.ns[-1]
    g.forest_extend(n)
    want = g.primary_roots()
    g.back(n)
    g.frontier_one(n)
    checks[f"{g.name}_frontier_root_is_the_primarys_at_the_end"] = status_ok() and bool((g.follower_roots()[g.tree] == want[g.tree]).all())


def stats(v):
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(min(v)), 4), "max_ms": round(float(max(v)), 4)}


rows = {}
for g in shapes:
    legs = {k: stats(v) for k, v in ms[g.name].items()}
    rows[g.name] = {"trees": g.T, "leaves": g.used, "open_tree_leaves": g.count, "stride": g.stride, "n": g.ns, "legs": legs,
                    "frontier_slowest_below_reduce_fastest": {str(n): bool(legs[f"frontier_{n}"]["max_ms"] < legs[f"reduce_{n}"]["min_ms"]) for n in g.ns},
                    "reduce_over_frontier_median": {str(n): round(legs[f"reduce_{n}"]["median_ms"] / legs[f"frontier_{n}"]["median_ms"], 2) for n in g.ns},
                    "frontier_over_forest_extend_median": {str(n): round(legs[f"frontier_{n}"]["median_ms"] / legs[f"forest_extend_{n}"]["median_ms"], 2)
                                                           for n in g.ns}}
info = dev.lib.vkmr_hip_kernel_info().decode()
out = {"tool": "frontier_extend_timing", "leaves_log2": a.log2, "room_log2": a.room_log2, "tree_leaves": per, "runs": a.runs, "device": dev.name(),
       "kernel_info": info, "build": provenance.build_id_of(info), "torch": torch.__version__, "checks": checks, "all_checks": all(checks.values()),
       "target": "one_tree: at every n the follower's slowest frontier extend is below the fastest reduction of all the leaves; "
                 "the ratio to forest_extend, which has the same number of launches, is recorded and not required",
       "target_met": all(rows["one_tree"]["frontier_slowest_below_reduce_fastest"].values()), "forests": rows}
line = json.dumps(out)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
