#!/usr/bin/env python3
"""What merging a batch into sorted trees costs on the device (vkmr_hip_forest_merge_leaves_async, vkmr_hip_tree_merge_leaves_async),
timed with HIP events: medians of interleaved runs in one process after a warm-up of every leg, stamped with the build id.  Prints
one JSON line (and writes it to --out).  GPU box.
    python3 tools/merge_timing.py [--log2 26] [--runs 10] [--out profiles/merge_timing.json]

  A            2^log2 random digests, sorted on the device once as trees of 2 048 and once as ONE tree (the one-tree twin)
  the batches  2^10, 2^16, 2^20 and 2^24 NEW random digests spread evenly over the trees and sorted per tree (union), and 2^16
               digests that ARE leaves, taken from A at even steps (difference)
  the legs     per shape: the union with each batch, the difference at 2^16, the union at 2^16 with the origin written; for the
               trees of 2 048 also the union at 2^16 followed by the stored build from out_offsets, and that build alone
  beside them  the only device route the parent commit has for "insert 2^16 digests": the concatenation laid per tree (made outside
               the clock) sorted again by vkmr_hip_forest_sort_leaves_async, which does not even remove duplicates; and
               vkmr_hip_forest_copy_trees_async over the 2^26 leaves as a stored forest (MerkleForest.append_from_async), the
               memory-bound yardstick; neither is code under test
Every answer is checked before the clock starts: status 0, the n_out identity from info, and the sortedness pass over the output
(every tree strictly increasing).  One requirement: the union of 2^16 into the trees of 2 048 takes less than the parent's route."""
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
BATCHES = [b for b in (10, 16, 20, 24) if (1 << b) <= n]
KEY = 16 if 16 in BATCHES else BATCHES[-1]            # the batch of the requirement and of the extra legs
b_max = 1 << BATCHES[-1]
gen = torch.Generator(device="cuda").manual_seed(31)


class Cells:
    """A buffer of digests that torch owns, as the engine's calls take it."""

    def __init__(self, cells):
        self.t = torch.empty((max(cells, 1), 8), dtype=torch.int32, device="cuda")
        self.ptr = self.t.data_ptr()

    def at(self, byte_offset):
        return self.ptr + int(byte_offset)

    def free(self):
        pass


class At:
    def __init__(self, buf, byte_offset):
        self.ptr = buf.at(byte_offset)


def random_cells(cells):
    c = Cells(cells)
    c.t[:cells] = torch.randint(-2**31, 2**31 - 1, (cells, 8), dtype=torch.int32, device="cuda", generator=gen)
    torch.cuda.synchronize()
    return c


def even_counts(total, trees):
    counts = np.full(trees, total // trees, dtype=np.uint64)
    counts[: total % trees] += np.uint64(1)
    return counts


def offsets_of(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)


def sorted_on_device(src, cells, offsets, out):
    """The trees at `offsets` over the first `cells` cells of src, sorted into `out` (outside every clock)."""
    d_scr, d_info = dev.alloc(dev.sort_leaves_scratch_bytes(cells)), dev.alloc(32)
    d_off = dev.upload(offsets)
    dev.forest_sort_leaves_enqueue(src, cells, d_off, len(offsets) - 1, int(np.diff(offsets).max()), d_scr, out, None, d_info)
    info = dev.download(d_info, 32, dtype=np.uint64).tolist()
    assert info[0] == 0 and info[1] == cells and info[3] == 0, info
    for b in (d_scr, d_info, d_off):
        b.free()


raw = random_cells(n)


class Shape:
    """A as trees of `per` leaves, its batches, and the buffers of its legs."""

    def __init__(self, per):
        self.per, self.T = per, n // per
        self.one_tree = self.T == 1
        self.a_off_host = np.arange(self.T + 1, dtype=np.uint64) * np.uint64(per)
        self.d_ab = Cells(n + b_max)                                             # A, and room behind it for the one tree's concatenation
        sorted_on_device(raw, n, self.a_off_host, self.d_ab)
        self.d_aoff = dev.upload(self.a_off_host)
        self.batches = {}
        for lg in BATCHES:
            nb = 1 << lg
            counts = even_counts(nb, self.T)
            off = offsets_of(counts)
            d_b = Cells(nb)
            sorted_on_device(random_cells(nb), nb, off, d_b)
            self.batches["union", lg] = (d_b, nb, dev.upload(off), off)
        nb = 1 << KEY                                                            # 2^KEY leaves of A, at even steps: in order, and spread as evenly
        cells = (np.arange(nb, dtype=np.uint64) * np.uint64(n // nb) + np.uint64(min(7, n // nb - 1))).astype(np.uint32)
        counts = np.bincount((cells // per).astype(np.int64), minlength=self.T).astype(np.uint64)
        d_b, d_idx = Cells(nb), dev.upload(cells)
        dev.gather_digests_async(self.d_ab, d_idx, nb, d_b)
        dev.sync()
        d_idx.free()
        self.batches["difference", KEY] = (d_b, nb, dev.upload(offsets_of(counts)), offsets_of(counts))
        cap = n + b_max
        self.cap = cap
        self.d_out, self.d_origin, self.d_ooff = Cells(cap), dev.alloc(8 * (n + (1 << KEY))), dev.alloc(8 * (self.T + 1))
        self.d_scratch = dev.alloc(dev.merge_leaves_scratch_bytes(n, b_max, self.T))
        self.d_info, self.d_status, self.d_bad, self.d_sorted = dev.alloc(32), dev.alloc(4), dev.alloc(8 * self.T), dev.alloc(32)
        # the parent's route: the concatenation laid per tree, sorted again
        nb = 1 << KEY
        self.cat_cells = n + nb
        b_off = self.batches["union", KEY][3]
        cat_off = self.a_off_host + b_off
        self.cat_max = int(np.diff(cat_off).max())
        if self.one_tree:                                                        # A followed by B: in place behind A
            d_idx = dev.upload(np.arange(nb, dtype=np.uint32))
            dev.gather_digests_async(self.batches["union", KEY][0], d_idx, nb, At(self.d_ab, 32 * n))
            dev.sync()
            d_idx.free()
            self.d_cat = self.d_ab
        else:
            tree = np.repeat(np.arange(self.T, dtype=np.int64), np.diff(cat_off).astype(np.int64))
            local = np.arange(self.cat_cells, dtype=np.int64) - cat_off[tree].astype(np.int64)
            from_a = local < per
            idx = np.where(from_a, tree * per + local, n + b_off[tree].astype(np.int64) + local - per).astype(np.uint32)
            joined = Cells(n + nb)                                               # A and the batch in one buffer, for one gather
            joined.t[:n] = self.d_ab.t[:n]
            joined.t[n: n + nb] = self.batches["union", KEY][0].t[:nb]
            torch.cuda.synchronize()
            self.d_cat = Cells(self.cat_cells)
            d_idx = dev.upload(idx)
            dev.gather_digests_async(joined, d_idx, self.cat_cells, self.d_cat)
            dev.sync()
            d_idx.free()
            del joined
        self.d_cat_off = dev.upload(cat_off)
        self.d_cat_out, self.d_cat_scratch = Cells(self.cat_cells), dev.alloc(dev.sort_leaves_scratch_bytes(self.cat_cells))
        if not self.one_tree:                                                    # the stored build over the merge's output
            self.build_cells = n + nb
            self.build_max = per + int(np.diff(b_off).max())
            self.d_out2, self.d_ooff2 = Cells(self.build_cells), dev.alloc(8 * (self.T + 1))
            self.d_forest, self.d_roots = dev.alloc(dev.forest_tree_bytes(self.build_cells, self.T, self.build_max)), dev.alloc(32 * self.T)

    def merge(self, what, lg, origin=False, second=False):
        d_b, nb, d_boff, _ = self.batches[what, lg]
        op = 0 if what == "union" else 1
        cap = (n + nb) if op == 0 else n
        out, ooff = (self.d_out2, self.d_ooff2) if second else (self.d_out, self.d_ooff)
        if self.one_tree:
            dev.tree_merge_leaves_enqueue(self.d_ab, n, d_b, nb, op, self.d_scratch, out, cap, self.d_origin if origin else None, self.d_info)
        else:
            dev.forest_merge_leaves_enqueue(self.d_ab, n, self.d_aoff, d_b, nb, d_boff, self.T, op, self.d_scratch, out, cap, ooff,
                                            self.d_origin if origin else None, self.d_info)

    def build(self):
        dev.reduce_forest_tree_async(self.d_out2, self.build_cells, self.d_ooff2, self.T, self.build_max, self.d_forest, self.d_roots, self.d_status)

    def merge_and_build(self):
        self.merge("union", KEY, second=True)
        self.build()

    def parent_route(self):
        dev.forest_sort_leaves_enqueue(self.d_cat, self.cat_cells, self.d_cat_off, self.T, self.cat_max, self.d_cat_scratch, self.d_cat_out, None, self.d_info)

    def legs(self):
        out = {f"union_2^{lg}": (lambda lg=lg: self.merge("union", lg)) for lg in BATCHES}
        out[f"difference_2^{KEY}"] = lambda: self.merge("difference", KEY)
        out[f"union_2^{KEY}_with_origin"] = lambda: self.merge("union", KEY, origin=True)
        out[f"parent_route_sort_of_the_concatenation_2^{KEY}"] = self.parent_route
        if not self.one_tree:
            out[f"union_2^{KEY}_and_stored_build"] = self.merge_and_build
            out["stored_build_alone"] = self.build
        return out

    def check(self, what, lg):
        """After merge(what, lg): status 0, the n_out identity, every tree of the output strictly increasing."""
        _, nb, _, _ = self.batches[what, lg]
        status, n_out, matches, repeats = dev.download(self.d_info, 32, dtype=np.uint64).tolist()
        want = n + nb - matches - repeats if what == "union" else n - matches
        if self.one_tree:
            d_off = dev.upload(np.array([0, n_out], dtype=np.uint64))
        else:
            d_off = self.d_ooff
        dev.forest_sorted_enqueue(self.d_out, self.cap, d_off, self.T, self.d_bad, self.d_sorted)
        is_sorted = dev.download(self.d_sorted, 32, dtype=np.uint64).tolist()
        ends = n_out if self.one_tree else int(dev.download(self.d_ooff, 8 * (self.T + 1), dtype=np.uint64)[-1])
        return {"status": status == 0, "n_out_identity": n_out == want and ends == n_out, "matches": int(matches), "repeats": int(repeats), "n_out": int(n_out),
                "strictly_increasing": is_sorted[:3] == [0, 0, 0]}


shapes = {"trees_of_2048": Shape(PER)}
if n > PER:
    shapes["one_tree"] = Shape(n)
forest = shapes["trees_of_2048"]

# the yardstick: every tree of the stored forest over A copied into an empty forest
src = dev._build_forest_of_buffer(forest.d_ab, n, [PER] * forest.T, PER, "merge_timing")
dst_leaves = Cells(n)
dst = vk.MerkleForest(dev, dst_leaves, n, np.zeros(forest.T, dtype=np.uint64), dev.upload(np.zeros(forest.T + 1, dtype=np.uint64)), PER,
                      dev.alloc(dev.forest_tree_bytes(n, forest.T, PER)), dev.upload(np.zeros((forest.T, 8), dtype=np.uint32)), used_trees=0)
d_sel, d_copy_off, d_copy_status = dev.upload(np.arange(forest.T, dtype=np.uint32)), dev.upload(forest.a_off_host), dev.alloc(4)


def copy_all():
    dst.append_from_async(src, d_sel, forest.T, n, d_copy_off, d_copy_status)


out = {"tool": "merge_timing", "leaves_log2": a.log2, "runs": a.runs, "device": dev.name(), "kernel_info": dev.lib.vkmr_hip_kernel_info().decode(),
       "build": provenance.build_id_of(dev.lib.vkmr_hip_kernel_info().decode()), "torch": torch.__version__,
       "scratch_bytes": {name: dev.merge_leaves_scratch_bytes(n, b_max, s.T) for name, s in shapes.items()}, "checks": {}, "shapes": {}}
for name, s in shapes.items():                    # every answer checked, and every leg warmed up
    out["checks"][name] = {}
    for what, lg in s.batches:
        s.merge(what, lg)
        dev.sync()
        out["checks"][name][f"{what}_2^{lg}"] = s.check(what, lg)
    for fn in s.legs().values():
        fn()
    dev.sync()
    if not s.one_tree:
        out["checks"][name]["stored_build_status"] = {"status": int(dev.download(s.d_status, 4)[0]) == 0}
    s.parent_route()
    out["checks"][name]["parent_route"] = {"status": dev.download(s.d_info, 32, dtype=np.uint64).tolist()[:2] == [0, s.cat_cells]}
copy_statuses = []
for _ in range(2):
    dst.truncate_async(0)                         # the destination empty again, outside every clock
    copy_all()
    copy_statuses.append(int(dev.download(d_copy_status, 4)[0]))

legs = {(name, leg): fn for name, s in shapes.items() for leg, fn in s.legs().items()}
legs["trees_of_2048", "forest_copy_trees_all"] = copy_all
ev = {key: [(dev.new_event(), dev.new_event()) for _ in range(a.runs)] for key in legs}
for r in range(a.runs):                           # every leg once per round, each waiting for the one before
    for key, fn in legs.items():
        e0, e1 = ev[key][r]
        if fn is copy_all:
            dst.truncate_async(0)
        dev.record(e0); fn(); dev.record(e1)
        dev.sync()
        if fn is copy_all:
            copy_statuses.append(int(dev.download(d_copy_status, 4)[0]))
out["checks"]["trees_of_2048"]["forest_copy_trees_all"] = {"every_status_0": all(x == 0 for x in copy_statuses),
                                                           "leaves_are_the_sources": bool(torch.equal(dst_leaves.t[:n], forest.d_ab.t[:n]))}

med = {}
for (name, leg), pairs in ev.items():
    ms = [dev.elapsed_ms(e0, e1) for e0, e1 in pairs]
    med[name, leg] = float(np.median(ms))
    out["shapes"].setdefault(name, {"trees": shapes[name].T, "leaves_per_tree": shapes[name].per, "legs": {}})["legs"][leg] = {
        "median_ms": round(med[name, leg], 4), "min_max_ms": [round(min(ms), 4), round(max(ms), 4)]}
copy_ms = med["trees_of_2048", "forest_copy_trees_all"]
for name in shapes:
    union, parent = med[name, f"union_2^{KEY}"], med[name, f"parent_route_sort_of_the_concatenation_2^{KEY}"]
    out["shapes"][name]["union_over_parent_route"] = round(union / parent, 4)
    out["shapes"][name]["union_over_forest_copy_trees_all"] = round(union / copy_ms, 3)
union, parent = med["trees_of_2048", f"union_2^{KEY}"], med["trees_of_2048", f"parent_route_sort_of_the_concatenation_2^{KEY}"]
out["requirement"] = {"what": f"the union of 2^{KEY} new digests into 2^{a.log2} leaves in trees of 2 048 takes less than the parent's route",
                      "union_ms": round(union, 4), "parent_route_ms": round(parent, 4), "ratio": round(union / parent, 4), "met": bool(union < parent)}
line = json.dumps(out)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
bad = [f"{name}: {leg}" for name, group in out["checks"].items() for leg, v in group.items() if not all(x for x in v.values() if isinstance(x, bool))]
if bad or not out["requirement"]["met"]:
    sys.exit(f"merge_timing: failed {bad or 'the requirement'}")
