#!/usr/bin/env python3
"""What the partial Merkle trees of a rescan cost: vkmr_hip_forest_merkleblocks_async out of a stored forest (the status word, one
check, nine kernels; output ready for the wire) beside the path that existed before it, measured by this tool in the same loop
on the same entries: vkmr_hip_forest_multiproof_async, the download of its nodes and of the matched leaves, and a reordering on
the host.  Every repetition of every leg interleaved in one process, from events (the host leg from the wall clock), after a
warm-up of every leg, stamped with the build id.  Prints one JSON line (and writes it to --out).  GPU box.  Nothing is required
of the numbers: they are recorded.
    python3 tools/merkleblocks_timing.py [--log2 26] [--tree-log2 11] [--runs 10] [--out profiles/merkleblocks_timing.json]

  the forest   2^log2 leaves as 2^(log2 - tree-log2) trees of 2^tree-log2
  the shapes   `random_1024`, `random_65536`, `random_1048576`: that many distinct random (tree, leaf) entries
               `whole_trees_65536`: 65536 entries that fill whole trees (every leaf of 2^16 / 2^tree-log2 trees)
  the legs     merkleblocks         the whole call
               merkleblocks_d2h     the download of what it wrote: the per-block arrays, the hashes, the flag bytes
               multiproof           vkmr_hip_forest_multiproof_async on the same entries
               multiproof_d2h       the download of its nodes and heights, and of the matched leaves (gathered by torch on the
                                    device, outside the timing)
               host_reorder         the gather of a reordering on the host: the downloaded nodes and leaves brought into the walk's
                                    order, edge nodes dropped, with numpy through an index map made OUTSIDE the timing (by matching
                                    the digests with the device's output).  Computing that map -- the index arithmetic of a
                                    reordering -- and forming the flag bits are NOT timed: this leg is a part of the old path's
                                    host work, not all of it
Checked on what was timed: every status word is 0; after EVERY repetition, outside the timed intervals, a sample of blocks of the
result just downloaded is extracted on the host (vkmr_host_cpu_merkleblock_extract): the root is the forest's root of that tree
and the matched set is the entries; and the reordered cells are, cell for cell, the hashes the device wrote."""
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
ap.add_argument("--sample", type=int, default=64)
ap.add_argument("--out", default=None)
a = ap.parse_args()
dev = vk.HipDevice(0)
gen = torch.Generator(device="cuda").manual_seed(28)
rng = np.random.default_rng(28)


class Leaves:
    """A level-0 buffer that torch owns, as the engine's calls take it."""

    def __init__(self, tensor):
        self.t = tensor
        self.ptr = tensor.data_ptr()

    def at(self, byte_offset):
        return self.ptr + int(byte_offset)

    def free(self):
        pass


per = 1 << a.tree_log2
ntrees = (1 << a.log2) // per
leaves = Leaves(torch.randint(-2**31, 2**31 - 1, (ntrees * per, 8), dtype=torch.int32, device="cuda", generator=gen))
torch.cuda.synchronize()
forest = dev._build_forest_of_buffer(leaves, ntrees * per, [per] * ntrees, per, "merkleblocks_timing")
roots = forest.roots()
statuses = []


class Shape:
    def __init__(self, name, cells):
        cells = np.unique(np.asarray(cells, dtype=np.int64))              # sorted (tree, index) pairs: a cell is tree * per + index
        self.name, self.k = name, int(cells.shape[0])
        k = self.k
        self.trees, self.indices = (cells // per).astype(np.uint32), (cells % per).astype(np.uint64)
        self.d_trees, self.d_indices = dev.upload(self.trees), dev.upload(self.indices)
        self.cap_h, self.cap_b, scratch = forest._merkleblocks_sizes(k)
        self.d_scr = dev.alloc(scratch)
        self.d_rows = [dev.alloc(4 * k), dev.alloc(8 * k), dev.alloc(8 * k), dev.alloc(8 * (k + 1)), dev.alloc(8 * (k + 1))]
        self.d_hashes, self.d_flags, self.d_info = dev.alloc(32 * self.cap_h), dev.alloc(self.cap_b), dev.alloc(32)
        self.cap_m, mp_scratch = forest._multiproof_sizes(k)
        self.d_mp_scr, self.d_nodes, self.d_heights = dev.alloc(mp_scratch), dev.alloc(32 * self.cap_m), dev.alloc(4 * k)
        self.d_mp_info = dev.alloc(8 * (2 + forest.levels))
        self.matched = Leaves(leaves.t[torch.from_numpy(cells).cuda()].contiguous())
        torch.cuda.synchronize()
        self.result = self.M = None

    def merkleblocks(self):
        forest.merkleblocks_async(self.d_trees, self.d_indices, self.k, self.d_scr, *self.d_rows, self.d_hashes, self.cap_h, self.d_flags, self.cap_b,
                                  self.d_info)

    def merkleblocks_d2h(self):
        status, B, n, m = (int(x) for x in dev.download(self.d_info, 32, dtype=np.uint64))
        statuses.append(status)
        cols = (np.uint32, np.uint64, np.uint64)
        t, c, bits = (dev.download(b, np.dtype(d).itemsize * B, dtype=d) for b, d in zip(self.d_rows[:3], cols))
        self.result = vk.PartialMerkleTrees(t, c, bits, dev.download(self.d_rows[3], 8 * (B + 1), dtype=np.uint64),
                                            dev.download(self.d_rows[4], 8 * (B + 1), dtype=np.uint64), dev.download(self.d_hashes, 32 * n).reshape(n, 8),
                                            dev.download(self.d_flags, m, dtype=np.uint8))

    def multiproof(self):
        forest.multiproof_async(self.d_trees, self.d_indices, self.k, self.d_mp_scr, self.d_nodes, self.cap_m, self.d_heights, self.d_mp_info)

    def multiproof_d2h(self):
        info = dev.download(self.d_mp_info, 16, dtype=np.uint64)
        statuses.append(int(info[0]))
        self.M = int(info[1])
        self.cells = np.concatenate([dev.download(self.d_nodes, 32 * self.M).reshape(-1, 8), dev.download(self.matched, 32 * self.k).reshape(-1, 8)])
        dev.download(self.d_heights, 4 * self.k)

    def index_map(self):
        """For every hash of the device's output its cell among the downloaded nodes and leaves: made once, outside the timing,
        from the digests themselves (their first 64 bits as the key; checks() compares whole cells)."""
        keys = np.ascontiguousarray(self.cells[:, :2]).view(np.uint64).reshape(-1)
        order = np.argsort(keys, kind="stable")
        want = np.ascontiguousarray(self.result.hashes[:, :2]).view(np.uint64).reshape(-1)
        self.src = order[np.minimum(np.searchsorted(keys[order], want), keys.shape[0] - 1)]

    def host_reorder(self):
        self.reordered = self.cells[self.src]

    def legs(self):
        return [("merkleblocks", self.merkleblocks, True), ("merkleblocks_d2h", self.merkleblocks_d2h, False), ("multiproof", self.multiproof, True),
                ("multiproof_d2h", self.multiproof_d2h, False), ("host_reorder", self.host_reorder, False)]

    def checks(self):
        r = self.result
        pick = sorted(set(rng.integers(0, len(r), size=min(a.sample, len(r))).tolist()))
        first = np.searchsorted(self.trees, r.trees)                          # the entries are sorted: a tree's are one run
        last = np.searchsorted(self.trees, r.trees, side="right")
        ok = True
        for b in pick:
            t = int(r.trees[b])
            root, found, _ = r[b].extract()
            ok = ok and bool((root == roots[t]).all()) and found.tolist() == self.indices[first[b]: last[b]].tolist()
        return {"sampled_blocks_extract_to_the_forests_roots_and_the_entries": ok, "blocks": len(r) == len(np.unique(self.trees)),
                "the_reordered_cells_are_the_devices_hashes": self.reordered.shape == r.hashes.shape and bool((self.reordered == r.hashes).all())}


def timed(fn, on_device, e0, e1):
    if on_device:
        dev.record(e0)
        fn()
        dev.record(e1)
        dev.sync()
        return dev.elapsed_ms(e0, e1)
    dev.sync()
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


total = ntrees * per
shapes = [Shape(f"random_{k}", rng.choice(total, size=k, replace=False)) for k in (1 << 10, 1 << 16, 1 << 20) if k <= total // 2]
whole = rng.choice(ntrees, size=max(1, (1 << 16) // per), replace=False)
shapes.append(Shape("whole_trees_65536", (whole[:, None].astype(np.int64) * per + np.arange(per)[None, :]).reshape(-1)))
e0, e1 = dev.new_event(), dev.new_event()
checks = {}
for g in shapes:                                   # warm up every leg; the answers checked on the way
    for leg, fn, _ in g.legs():
        if leg == "host_reorder":
            g.index_map()
        fn()
    dev.sync()
    checks.update({f"{g.name}_{k}": v for k, v in g.checks().items()})

ms = {g.name: {leg: [] for leg, _, _ in g.legs()} for g in shapes}
for r in range(a.runs):
    for g in shapes:
        for leg, fn, on_device in g.legs():
            ms[g.name][leg].append(timed(fn, on_device, e0, e1))
        for k, v in g.checks().items():            # every repetition's result, outside the timed intervals
            checks[f"{g.name}_{k}_in_every_repetition"] = checks.get(f"{g.name}_{k}_in_every_repetition", True) and v
dev.sync()
checks["every_status_word_is_0"] = all(s == 0 for s in statuses)


def stats(v):
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(min(v)), 4), "max_ms": round(float(max(v)), 4)}


rows = {}
for g in shapes:
    legs = {k: stats(v) for k, v in ms[g.name].items()}
    new = legs["merkleblocks"]["median_ms"] + legs["merkleblocks_d2h"]["median_ms"]
    old = legs["multiproof"]["median_ms"] + legs["multiproof_d2h"]["median_ms"] + legs["host_reorder"]["median_ms"]
    rows[g.name] = {"entries": g.k, "blocks": len(g.result), "hashes": int(g.result.hashes.shape[0]), "flag_bytes": int(g.result.flags.shape[0]),
                    "multiproof_nodes": g.M, "legs": legs, "device_call_multiproof_over_merkleblocks_median": round(legs["multiproof"]["median_ms"] /
                                                                                                                  legs["merkleblocks"]["median_ms"], 2),
                    "to_the_host_old_path_without_its_index_arithmetic_over_new_median": round(old / new, 2)}
info = dev.lib.vkmr_hip_kernel_info().decode()
out = {"tool": "merkleblocks_timing", "leaves_log2": a.log2, "tree_leaves": per, "trees": ntrees, "runs": a.runs, "device": dev.name(), "kernel_info": info,
       "build": provenance.build_id_of(info), "torch": torch.__version__, "checks": checks, "all_checks": all(checks.values()),
       "target": "none: recorded, nothing required",
       "note": "host_reorder times the gather of a real reordering (index map made outside the timing); the index arithmetic and the flag bits are not timed",
       "shapes": rows}
line = json.dumps(out)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
