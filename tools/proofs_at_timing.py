#!/usr/bin/env python3
"""What an inclusion proof as of an earlier count costs: vkmr_hip_forest_proofs_at_async out of a stored forest (the status word,
one check, one edge launch with a lane per epoch, one gather with a lane per (query, level)) beside what it replaces, measured by
this tool on the same machine: a SECOND stored forest built from the prefix leaves (vkmr_hip_reduce_forest_tree_async over the
first c leaves of every epoch's tree, gathered back to back outside the timing) plus vkmr_hip_forest_proofs_async on it.  Every
repetition of every leg interleaved in one process, from events, after a warm-up of every leg, stamped with the build id.  Prints
one JSON line (and writes it to --out).  GPU box.  Nothing is required of the numbers: they are recorded.
    python3 tools/proofs_at_timing.py [--log2 26] [--room-log2 16] [--tree-log2 11] [--per-epoch 32] [--runs 10] [--out profiles/proofs_at_timing.json]

  the shapes   `many_trees`: 2^log2 leaves in trees of 2^tree-log2, ONE epoch per tree at a random old count >= 1, --per-epoch
               queries an epoch at random leaves
               `one_tree_e1`: ONE tree of 2^log2 - 2^room-log2 leaves, E = 1 at a random old count in the last 2^room-log2, k = 2^20
               `one_tree_e65536`: the same tree, E = k = 2^room-log2: an epoch per query, at random old counts
  the legs     proofs_at         the whole call: edges, old roots, siblings, heights
               roots_at          the call with k == 0: the edges and the old roots alone
               verify            vkmr_hip_verify_forest_proofs_async over the k proofs under the returned old roots
               rebuild           the second stored forest from the prefix leaves (not run where they do not fit: 2^16 epochs into
                                 one tree of 2^26 are about 2^41 leaves)
               rebuild_gather    vkmr_hip_forest_proofs_async on the rebuilt forest
Checked on what was timed: every status word is 0, every proof verifies under its old root, the old roots are the rebuilt
forest's roots and the first 4096 proofs are, cell for cell, the rebuilt forest's."""
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
ap.add_argument("--per-epoch", type=int, default=32)
ap.add_argument("--runs", type=int, default=10)
ap.add_argument("--out", default=None)
a = ap.parse_args()
dev = vk.HipDevice(0)
gen = torch.Generator(device="cuda").manual_seed(27)
rng = np.random.default_rng(27)
REBUILD_LIMIT = 1 << 27                             # prefix leaves the alternative may take here
SAMPLE = 4096


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
    """E epochs (tree, old count) and k queries (epoch, leaf) into the stored forest `f`, the buffers of the answer, and the
    alternative: the prefix leaves back to back, a tree per epoch, and the buffers of a stored forest over them."""

    def __init__(self, name, f, leaves, offsets, epoch_trees, epoch_counts, epochs, indices):
        self.name, self.f, self.E, self.k = name, f, len(epoch_trees), len(epochs)
        E, k = self.E, self.k
        self.stride = s = max(1, min(f.max_count, f.total).bit_length())
        self.epoch_trees, self.epoch_counts = np.asarray(epoch_trees, dtype=np.uint32), np.asarray(epoch_counts, dtype=np.uint64)
        self.epochs, self.indices = np.asarray(epochs, dtype=np.uint32), np.asarray(indices, dtype=np.uint64)
        self.d_epoch_trees, self.d_epoch_counts = dev.upload(self.epoch_trees), dev.upload(self.epoch_counts)
        self.d_epochs, self.d_indices = dev.upload(self.epochs), dev.upload(self.indices)
        self.d_edges, self.d_old_roots = dev.alloc(32 * E * s), dev.alloc(32 * E)
        self.d_edges_only, self.d_old_roots_only = dev.alloc(32 * E * s), dev.alloc(32 * E)
        self.d_siblings, self.d_heights, self.d_ok = dev.alloc(32 * k * s), dev.alloc(4 * k), dev.alloc(4 * k)
        where = offsets[self.epoch_trees[self.epochs.astype(np.int64)].astype(np.int64)].astype(np.int64) + self.indices.astype(np.int64)
        self.proved = Leaves(leaves.t[torch.from_numpy(where).cuda()].contiguous())              # the leaf every query proves
        # the alternative: the first c leaves of every epoch's tree back to back, a tree per epoch
        take = self.epoch_counts.astype(np.int64)
        self.prefix_leaves = int(take.sum())
        self.rebuild_run = self.prefix_leaves <= REBUILD_LIMIT
        if self.rebuild_run:
            starts = offsets[self.epoch_trees.astype(np.int64)].astype(np.int64)
            ext = np.concatenate([[0], np.cumsum(take)]).astype(np.int64)
            index = torch.from_numpy(np.repeat(starts - ext[:-1], take) + np.arange(self.prefix_leaves, dtype=np.int64)).cuda()
            self.prefix = Leaves(leaves.t[index].contiguous())
            self.prefix_max = int(take.max())
            self.d_prefix_offsets = dev.upload(ext.astype(np.uint64))
            self.d_prefix_forest = dev.alloc(dev.forest_tree_bytes(self.prefix_leaves, E, self.prefix_max))
            self.d_prefix_roots = dev.alloc(32 * E)
            self.prefix_levels = vk.tree_height(min(self.prefix_max, self.prefix_leaves))        # the cells per proof of vkmr_hip_forest_proofs_async
            self.d_prefix_siblings, self.d_prefix_heights = dev.alloc(32 * k * self.prefix_levels), dev.alloc(4 * k)
        torch.cuda.synchronize()
        dev.sync()

    def proofs_at(self):
        f = self.f
        dev.forest_proofs_at_enqueue(f.digests, f.forest, f.total, f.offsets, f.ntrees, f.max_count, f.roots_buf, self.d_epoch_trees, self.d_epoch_counts,
                                     self.E, self.d_epochs, self.d_indices, self.k, self.stride, self.d_edges, self.d_old_roots, self.d_siblings,
                                     self.d_heights, d_status)

    def roots_at(self):
        f = self.f
        dev.forest_proofs_at_enqueue(f.digests, f.forest, f.total, f.offsets, f.ntrees, f.max_count, f.roots_buf, self.d_epoch_trees, self.d_epoch_counts,
                                     self.E, None, None, 0, self.stride, self.d_edges_only, self.d_old_roots_only, None, None, d_status)

    def verify(self):
        dev.verify_forest_proofs_async(self.proved, self.d_epochs, self.d_indices, self.d_siblings, self.d_heights, self.k, self.stride, self.d_old_roots,
                                       self.E, self.d_ok)

    def rebuild(self):
        dev.reduce_forest_tree_async(self.prefix, self.prefix_leaves, self.d_prefix_offsets, self.E, self.prefix_max, self.d_prefix_forest,
                                     self.d_prefix_roots, d_status)

    def rebuild_gather(self):
        dev.forest_proofs_async(self.prefix, self.d_prefix_forest, self.prefix_leaves, self.d_prefix_offsets, self.E, self.prefix_max, self.d_epochs,
                                self.d_indices, self.k, self.d_prefix_siblings, self.d_prefix_heights)

    def legs(self):
        return [("proofs_at", self.proofs_at), ("roots_at", self.roots_at), ("verify", self.verify)] + (
            [("rebuild", self.rebuild), ("rebuild_gather", self.rebuild_gather)] if self.rebuild_run else [])

    def checks(self):
        E, k, s = self.E, self.k, self.stride
        old_roots = dev.download(self.d_old_roots, 32 * E)
        ok = {"status_0": int(dev.download(d_status, 4)[0]) == 0,
              "every_proof_verifies_under_its_old_root": bool((dev.download(self.d_ok, 4 * k) == 1).all()),
              "roots_at_gives_the_same_edges_and_roots": bool((dev.download(self.d_old_roots_only, 32 * E) == old_roots).all()
                                                              and (dev.download(self.d_edges_only, 32 * E * s) == dev.download(self.d_edges, 32 * E * s)).all())}
        if self.rebuild_run:
            n, w = min(k, SAMPLE), self.prefix_levels
            mine = dev.download(self.d_siblings, 32 * n * s).reshape(n, s, 8)
            theirs = dev.download(self.d_prefix_siblings, 32 * n * w).reshape(n, w, 8)
            ok["the_old_roots_are_the_rebuilt_forests_roots"] = bool((dev.download(self.d_prefix_roots, 32 * E) == old_roots).all())
            ok["the_heights_are_the_rebuilt_forests"] = bool((dev.download(self.d_prefix_heights, 4 * k) == dev.download(self.d_heights, 4 * k)).all())
            ok["the_first_proofs_are_the_rebuilt_forests_cell_for_cell"] = bool((mine[:, :min(s, w)] == theirs[:, :min(s, w)]).all()
                                                                                and not mine[:, w:].any() and not theirs[:, s:].any())
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


def leaves_below(counts, per):
    """`per` random leaf indices below every count."""
    return (rng.random((len(counts), per)) * np.asarray(counts, dtype=np.float64)[:, None]).astype(np.uint64).reshape(-1)


per, room = 1 << a.tree_log2, 1 << a.room_log2
many, many_leaves, many_offsets = forest_of([per] * ((1 << a.log2) // per), per, "proofs_at_timing")
one_count = (1 << a.log2) - room
one, one_leaves, one_offsets = forest_of([one_count], 1 << a.log2, "proofs_at_timing")
many_counts = rng.integers(1, per + 1, size=many.ntrees)
one_c = int(rng.integers(one_count - room, one_count))
K1 = 1 << 20
room_counts = rng.integers(1, one_count + 1, size=room)
shapes = [Shape("many_trees", many, many_leaves, many_offsets, np.arange(many.ntrees), many_counts, np.repeat(np.arange(many.ntrees), a.per_epoch),
                leaves_below(many_counts, a.per_epoch)),
          Shape("one_tree_e1", one, one_leaves, one_offsets, [0], [one_c], np.zeros(K1, np.uint32), rng.integers(0, one_c, size=K1)),
          Shape(f"one_tree_e{room}", one, one_leaves, one_offsets, np.zeros(room, np.uint32), room_counts, np.arange(room), leaves_below(room_counts, 1))]
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
    rows[g.name] = {"trees": g.f.ntrees, "leaves": g.f.total, "epochs": g.E, "queries": g.k, "stride": g.stride,
                    "node_hashes_of_the_edges": int(sum(0 if (c & (c - 1)) == 0 and c >= 2 else vk.tree_height(c) - ((c & -c).bit_length() - 1)
                                                        for c in g.epoch_counts.tolist())),
                    "legs": legs, "prefix_leaves": g.prefix_leaves if g.rebuild_run else None,
                    "rebuild_not_run": None if g.rebuild_run else f"{g.prefix_leaves} prefix leaves: more than fit here",
                    "rebuild_plus_gather_over_proofs_at_median": round((legs["rebuild"]["median_ms"] + legs["rebuild_gather"]["median_ms"])
                                                                       / legs["proofs_at"]["median_ms"], 2) if g.rebuild_run else None}
info = dev.lib.vkmr_hip_kernel_info().decode()
out = {"tool": "proofs_at_timing", "leaves_log2": a.log2, "room_log2": a.room_log2, "tree_leaves": per, "per_epoch": a.per_epoch, "runs": a.runs,
       "device": dev.name(), "kernel_info": info, "build": provenance.build_id_of(info), "torch": torch.__version__, "checks": checks,
       "all_checks": all(checks.values()), "target": "none: recorded, nothing required", "forests": rows}
line = json.dumps(out)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
