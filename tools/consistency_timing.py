#!/usr/bin/env python3
"""What a consistency proof costs: the primary's gather out of a stored forest (vkmr_hip_forest_consistency_async: the status
word, one check, one gather) and the monitor's check (vkmr_hip_verify_consistency_async: one launch, a lane per query), beside the
nearest existing one-lane-per-tree walk over the same Q (vkmr_hip_verify_frontier_async over the proofs' peaks rows) and beside
what a follower does instead of checking a proof: take the c2 - c leaves and extend its frontier (vkmr_hip_frontier_extend_async).
Every repetition of every leg interleaved in one process, from events, after a warm-up of every leg, stamped with the build id.
Prints one JSON line (and writes it to --out).  GPU box.  Nothing is required of the numbers: they are recorded.
    python3 tools/consistency_timing.py [--log2 26] [--room-log2 16] [--tree-log2 11] [--runs 10] [--out profiles/consistency_timing.json]

  the shapes   `many_trees`: 2^log2 leaves in trees of 2^tree-log2, ONE query per tree at a random old count
               `one_tree_q1`, `one_tree_q65536`: ONE tree of 2^log2 - 2^room-log2 leaves (the shape of tools/frontier_extend_timing.py),
               Q = 1 and Q = 2^room-log2 queries at random old counts
  the legs     gather            the proofs of all Q queries out of the stored levels: no hash
               verify            the check of all Q proofs under the old roots and the roots now
               verify_frontier   vkmr_hip_verify_frontier_async over (old counts, peaks) under the old roots: the first of the two walks
               frontier_extend   the follower's alternative: the c2 - c leaves of every query, gathered back to back outside the
                                 timing, through vkmr_hip_frontier_extend_async from the frontier (old count, peaks).  Not run where the
                                 leaves would not fit in memory (2^16 queries into one tree of 2^26: about 2^41 leaves)
Checked on what was timed: every status word is 0, every proof verifies, verify_frontier accepts every peaks row, and the
follower's extended roots are the roots now."""
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
gen = torch.Generator(device="cuda").manual_seed(26)
rng = np.random.default_rng(26)
EXTEND_LIMIT = 1 << 27                              # leaves the follower's alternative may take in one call here


class Leaves:
    """A level-0 buffer that torch owns, as the engine's calls take it."""

    def __init__(self, tensor):
        self.t = tensor
        self.ptr = tensor.data_ptr()

    def at(self, byte_offset):
        return self.ptr + int(byte_offset)

    def free(self):
        pass


d_status = dev.alloc(4)
statuses = []


class Shape:
    """Q queries (tree, old count) into the stored forest `f`, the buffers of their proofs, the old roots (from the proofs' own
    peaks, checked against the verifier) and the roots now per query."""

    def __init__(self, name, f, leaves, offsets, trees, old):
        self.name, self.f, self.Q = name, f, len(trees)
        Q, self.stride = self.Q, max(1, min(f.max_count, f.total).bit_length())
        s = self.stride
        self.trees, self.old = np.asarray(trees, dtype=np.uint32), np.asarray(old, dtype=np.uint64)
        self.d_trees, self.d_old = dev.upload(self.trees), dev.upload(self.old)
        self.d_new, self.d_peaks, self.d_rights = dev.alloc(8 * Q), dev.alloc(32 * Q * s), dev.alloc(32 * Q * s)
        self.d_old_roots, self.d_ok, self.d_ok_frontier = dev.alloc(32 * Q), dev.alloc(4 * Q), dev.alloc(4 * Q)
        self.gather()
        dev.frontier_roots_enqueue(self.d_old, self.d_peaks, s, Q, self.d_old_roots)         # the root every tree had at its old count
        now = dev.download(f.roots_buf, 32 * f.ntrees).reshape(f.ntrees, 8)
        self.d_new_roots = dev.upload(now[self.trees.astype(np.int64)])
        self.new = dev.download(self.d_new, 8 * Q, dtype=np.uint64)
        # the follower's alternative: the c2 - c leaves of every query back to back
        take = (self.new - self.old).astype(np.int64)
        self.extend_leaves = int(take.sum())
        self.extend = self.extend_leaves <= EXTEND_LIMIT
        if self.extend:
            starts = offsets[self.trees.astype(np.int64)].astype(np.int64) + self.old.astype(np.int64)
            ext = np.concatenate([[0], np.cumsum(take)]).astype(np.int64)
            index = torch.from_numpy(np.repeat(starts - ext[:-1], take) + np.arange(self.extend_leaves, dtype=np.int64)).cuda()
            self.more = Leaves(leaves.t[index].contiguous())
            self.d_ext = dev.upload(ext.astype(np.uint64))
            self.max_new = int(take.max()) if Q else 0
            self.scratch = dev.frontier_extend_scratch(self.extend_leaves, Q)
            self.d_ext_counts, self.d_ext_peaks, self.d_ext_roots = dev.alloc(8 * Q), dev.alloc(32 * Q * s), dev.alloc(32 * Q)
        torch.cuda.synchronize()
        dev.sync()

    def gather(self):
        f = self.f
        dev.forest_consistency_enqueue(f.digests, f.forest, f.total, f.offsets, f.ntrees, f.max_count, f.roots_buf, self.d_trees, self.d_old, self.Q,
                                       self.stride, self.d_new, self.d_peaks, self.d_rights, d_status)

    def verify(self):
        dev.verify_consistency_enqueue(self.d_old, self.d_new, self.d_peaks, self.d_rights, self.stride, self.Q, self.d_old_roots, self.d_new_roots, self.d_ok)

    def verify_frontier(self):
        dev.verify_frontier_enqueue(self.d_old, self.d_peaks, self.stride, self.Q, self.d_old_roots, self.d_ok_frontier)

    def frontier_extend(self):
        dev.frontier_extend_enqueue(self.d_old, self.d_peaks, self.stride, self.Q, self.more, self.extend_leaves, self.d_ext, self.max_new, self.scratch,
                                    self.d_ext_counts, self.d_ext_peaks, self.d_ext_roots, d_status)

    def legs(self):
        return [("gather", self.gather), ("verify", self.verify), ("verify_frontier", self.verify_frontier)] + (
            [("frontier_extend", self.frontier_extend)] if self.extend else [])

    def checks(self):
        ok = {"status_0": int(dev.download(d_status, 4)[0]) == 0,
              "every_proof_verifies": bool((dev.download(self.d_ok, 4 * self.Q) == 1).all()),
              "every_peaks_row_is_a_frontier_of_the_old_root": bool((dev.download(self.d_ok_frontier, 4 * self.Q) == 1).all())}
        if self.extend:
            ok["the_extended_roots_are_the_roots_now"] = bool((dev.download(self.d_ext_roots, 32 * self.Q) == dev.download(self.d_new_roots, 32 * self.Q)).all())
        return ok


def forest_of(counts, max_count, what):
    total = int(sum(counts))
    leaves = Leaves(torch.randint(-2**31, 2**31 - 1, (total, 8), dtype=torch.int32, device="cuda", generator=gen))
    torch.cuda.synchronize()
    return dev._build_forest_of_buffer(leaves, total, counts, max_count, what), leaves, np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)


def timed(fn, e0, e1):
    dev.record(e0)
    fn()
    dev.record(e1)
    dev.sync()
    statuses.append(int(dev.download(d_status, 4)[0]))
    return dev.elapsed_ms(e0, e1)


per, room = 1 << a.tree_log2, 1 << a.room_log2
many, many_leaves, many_offsets = forest_of([per] * ((1 << a.log2) // per), per, "consistency_timing")
one_count = (1 << a.log2) - room
one, one_leaves, one_offsets = forest_of([one_count], 1 << a.log2, "consistency_timing")
shapes = [Shape("many_trees", many, many_leaves, many_offsets, np.arange(many.ntrees), rng.integers(0, per + 1, size=many.ntrees)),
          Shape("one_tree_q1", one, one_leaves, one_offsets, [0], rng.integers(one_count - room, one_count, size=1)),
          Shape(f"one_tree_q{room}", one, one_leaves, one_offsets, np.zeros(room, np.uint32), rng.integers(0, one_count + 1, size=room))]
e0, e1 = dev.new_event(), dev.new_event()
checks = {}
for g in shapes:                                   # warm up every leg; the answers checked on the way
    for _, fn in g.legs():
        fn()
    dev.sync()
    checks.update({f"{g.name}_{k}": v for k, v in g.checks().items()})

ms = {g.name: {leg: [] for leg, _ in g.legs()} for g in shapes}
for r in range(a.runs):
    for g in shapes:
        for leg, fn in g.legs():
            ms[g.name][leg].append(timed(fn, e0, e1))
dev.sync()
checks["every_status_word_is_0"] = all(s == 0 for s in statuses)
for g in shapes:                                   # and the last repetition left the answers of the first
    checks.update({f"{g.name}_{k}_at_the_end": v for k, v in g.checks().items()})


def stats(v):
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(min(v)), 4), "max_ms": round(float(max(v)), 4)}


rows = {}
for g in shapes:
    legs = {k: stats(v) for k, v in ms[g.name].items()}
    rows[g.name] = {"trees": g.f.ntrees, "leaves": g.f.total, "queries": g.Q, "stride": g.stride, "legs": legs,
                    "frontier_extend_leaves": g.extend_leaves if g.extend else None,
                    "frontier_extend_not_run": None if g.extend else f"{g.extend_leaves} leaves to take: more than one call is given here",
                    "verify_over_verify_frontier_median": round(legs["verify"]["median_ms"] / legs["verify_frontier"]["median_ms"], 2)}
info = dev.lib.vkmr_hip_kernel_info().decode()
out = {"tool": "consistency_timing", "leaves_log2": a.log2, "room_log2": a.room_log2, "tree_leaves": per, "runs": a.runs, "device": dev.name(),
       "kernel_info": info, "build": provenance.build_id_of(info), "torch": torch.__version__, "checks": checks, "all_checks": all(checks.values()),
       "target": "none: recorded, nothing required", "forests": rows}
line = json.dumps(out)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
