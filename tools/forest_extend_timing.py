#!/usr/bin/env python3
"""What growing the open tree of a stored forest by leaves costs (vkmr_hip_forest_extend_async) beside the two routes there were
without it: dropping the open tree and appending the whole of it again in place (vkmr_hip_forest_truncate_async +
vkmr_hip_forest_append_async), and the stored build of the whole forest.  Every repetition of every leg interleaved in one
process, from events, after a warm-up of every leg, stamped with the build id.  Prints one JSON line (and writes it to --out).
GPU box.
    python3 tools/forest_extend_timing.py [--log2 26] [--room-log2 16] [--tree-log2 11] [--runs 10] [--out profiles/forest_extend_timing.json]

  the forests  `one_tree`: a forest of ONE tree with a capacity of 2^log2 leaves (a growing single tree), 2^log2 - 2^room-log2 of
               them there; extended by n = 1, 2^10, 2^room-log2
               `last_of_many`: 2^log2 cells in trees of 2^tree-log2, every tree full but the last, the open tree, which is half
               full; extended by n = 1, 64, 2^(tree-log2 - 1)
  the legs     extend_n            the n leaves copied from a buffer of their own (the default route)
               in_place_n          the same with the leaves already behind the last leaf: no copy launch
               shrink_n            the n leaves dropped again (vkmr_hip_forest_shrink_async)
               truncate_append_n   the open tree dropped and the whole of it, n new leaves included, appended in place
               rebuild             vkmr_hip_reduce_forest_tree_async over the forest after the largest extend, into the same buffers
Checked on what was timed: every status word is 0; after the extend the roots are those a rebuild over the same buffers leaves and
the forest audits clean; the truncate-and-append leaves the same roots; after the shrink the roots are those of the start.  The
requirement is for `one_tree`, where the new work is at most 2^-10 of the tree: at every n the extend's slowest repetition is below
the fastest truncate-and-append.  `last_of_many` is a handful of small launches either way: reported, no requirement."""
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
gen = torch.Generator(device="cuda").manual_seed(23)


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


def random_leaves(n):
    return torch.randint(-2**31, 2**31 - 1, (n, 8), dtype=torch.int32, device="cuda", generator=gen)


d_status = dev.alloc(4)
statuses = []


class Open:
    """A stored forest whose open tree holds `count` leaves with `room` free cells behind them, and the `room` new leaves both in
    a buffer of their own and in place."""

    def __init__(self, name, counts, room, max_count, ns):
        self.name, self.counts, self.room, self.ns = name, counts, room, ns
        used = sum(counts)
        self.leaves = Leaves(random_leaves(used + room))
        self.new = Leaves(self.leaves.t[used:].clone())
        torch.cuda.synchronize()
        self.f = dev._build_forest_of_buffer(self.leaves, used + room, counts, max_count, "forest_extend_timing", reserve_leaves=room)
        self.tree, self.count = len(counts) - 1, counts[-1]
        self.place = At(self.leaves.at(32 * used))
        self.tree_start = At(self.leaves.at(32 * (used - self.count)))
        self.d_off = {n: dev.upload(np.array([0, self.count + n], dtype=np.uint64)) for n in ns}
        dev.sync()

    def extend(self, n, in_place=False):
        self.f.extend_async(self.place if in_place else self.new, n, d_status)

    def shrink(self, n):
        self.f.shrink_async(n, d_status)

    def truncate_append(self, n):
        """What there was without the call: the open tree dropped, and all of it appended again where it lies."""
        self.f.truncate_async(self.tree)
        self.f.append_async(self.tree_start, self.count + n, self.d_off[n], 1, d_status)

    def rebuild(self):
        f = self.f
        dev.reduce_forest_tree_async(f.digests, f.total, f.offsets, f.ntrees, f.max_count, f.forest, f.roots_buf, d_status)

    def roots(self):
        return dev.download(self.f.roots_buf, 32 * self.f.ntrees)


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
forests = [Open("one_tree", [(1 << a.log2) - room], room, 1 << a.log2, sorted({1, min(1 << 10, room), room})),
           Open("last_of_many", [per] * ((1 << a.log2) // per - 1) + [per // 2], per // 2, per, sorted({1, min(64, per // 2), per // 2}))]
e0, e1 = dev.new_event(), dev.new_event()
checks = {}
for g in forests:                                  # warm up every leg; the answers checked on the way
    start = g.roots()
    for n in g.ns:
        for in_place in (False, True):
            g.extend(n, in_place)
            ok = status_ok()
            g.f.extended(n)
            grown = g.roots()
            clean = bool(g.f.audit().clean)
            g.rebuild()
            key = f"{g.name}_{'in_place' if in_place else 'extend'}_{n}_roots_are_the_rebuilds_and_the_audit_is_clean"
            checks[key] = ok and clean and status_ok() and bool((g.roots() == grown).all()) and not bool((grown == start).all())
            g.shrink(n)
            ok = status_ok()
            g.f.shrunk(n)
            checks[f"{g.name}_shrink_{n}_roots_are_those_of_the_start"] = ok and bool((g.roots() == start).all()) and bool(g.f.audit().clean)
        g.truncate_append(n)
        ok = status_ok()
        g.f.appended([g.count + n])
        checks[f"{g.name}_truncate_append_{n}_roots_are_the_extends"] = ok and bool((g.roots() == grown).all())
        g.shrink(n)
        g.f.shrunk(n)
    dev.sync()

ms = {g.name: {**{f"{leg}_{n}": [] for n in g.ns for leg in ("extend", "in_place", "shrink", "truncate_append")}, "rebuild": []} for g in forests}
for r in range(a.runs):
    for g in forests:
        legs = ms[g.name]
        for n in g.ns:
            for in_place in (False, True):
                legs[f"{'in_place' if in_place else 'extend'}_{n}"].append(timed(lambda: g.extend(n, in_place), e0, e1))
                g.f.extended(n)
                if in_place:
                    legs[f"shrink_{n}"].append(timed(lambda: g.shrink(n), e0, e1))
                else:
                    g.shrink(n)
                g.f.shrunk(n)
            legs[f"truncate_append_{n}"].append(timed(lambda: g.truncate_append(n), e0, e1))
            g.f.appended([g.count + n])
            if n == g.ns[-1]:
                legs["rebuild"].append(timed(g.rebuild, e0, e1))   # the offsets are those after the largest extend
            g.shrink(n)
            g.f.shrunk(n)
dev.sync()
checks["every_status_word_is_0"] = all(s == 0 for s in statuses) and status_ok()
for g in forests:
    checks[f"{g.name}_clean_at_the_end"] = bool(g.f.audit().clean)


def stats(v):
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(min(v)), 4), "max_ms": round(float(max(v)), 4)}


rows = {}
for g in forests:
    legs = {k: stats(v) for k, v in ms[g.name].items()}
    rows[g.name] = {"trees": g.f.ntrees, "capacity_leaves": g.f.total, "open_tree_leaves": g.count, "levels": g.f.levels, "n": g.ns, "legs": legs,
                    "extend_slowest_below_truncate_append_fastest": {str(n): bool(max(legs[f"extend_{n}"]["max_ms"], legs[f"in_place_{n}"]["max_ms"])
                                                                                  < legs[f"truncate_append_{n}"]["min_ms"]) for n in g.ns},
                    "truncate_append_over_extend_median": {str(n): round(legs[f"truncate_append_{n}"]["median_ms"] / legs[f"extend_{n}"]["median_ms"], 2)
                                                           for n in g.ns}}
info = dev.lib.vkmr_hip_kernel_info().decode()
out = {"tool": "forest_extend_timing", "leaves_log2": a.log2, "room_log2": a.room_log2, "tree_leaves": per, "runs": a.runs, "device": dev.name(),
       "kernel_info": info, "build": provenance.build_id_of(info), "torch": torch.__version__, "checks": checks, "all_checks": all(checks.values()),
       "target": "one_tree: at every n the slowest extend (leaves copied or in place) is below the fastest truncate-and-append of the whole tree; "
                 "last_of_many: a handful of small launches either way, reported, no requirement",
       "target_met": all(rows["one_tree"]["extend_slowest_below_truncate_append_fastest"].values()), "forests": rows}
line = json.dumps(out)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
