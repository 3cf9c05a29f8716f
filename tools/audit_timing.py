#!/usr/bin/env python3
"""What an audit of a stored forest or tree costs (vkmr_hip_forest_audit_async, vkmr_hip_tree_audit_async) beside the build of
the same structure: medians of interleaved runs in one process, from events, after a warm-up of every leg, stamped with the
build id.  Prints one JSON line (and writes it to --out).  GPU box.
    python3 tools/audit_timing.py [--log2 26] [--tree-log2 11] [--runs 10] [--updates-log2 16] [--out profiles/audit_timing.json]

  the shapes   2^log2 random leaves as 2^(log2 - tree-log2) trees of 2^tree-log2, as trees of 1 .. 4095 leaves, and as one tree
  the legs     (a) masks    the audit with capacity 0: one launch per level, masks and counters
               (b) build    vkmr_hip_reduce_forest_tree_async / vkmr_hip_reduce_tree_async over the same leaves into the same buffers
               (c) list     the audit with capacity n after n = 1 and n = 2^16 scattered leaves had one bit flipped (each is one
                            bad level-1 node): the levels again, the three ranking launches, one emit launch per level
Checked on what was timed: the fresh structure audits clean with the host-derived node count; after 2^updates-log2 random leaf
updates it still does; every planted corruption is listed at its position, and the structure audits clean once they are undone."""
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
ap.add_argument("--tree-log2", type=int, default=11)
ap.add_argument("--runs", type=int, default=10)
ap.add_argument("--updates-log2", type=int, default=16)
ap.add_argument("--out", default=None)
a = ap.parse_args()
dev = vk.HipDevice(0)
total = 1 << a.log2
per = 1 << min(a.tree_log2, a.log2)
rng = np.random.default_rng(20)
gen = torch.Generator(device="cuda").manual_seed(20)
NS = [n for n in (1, 1 << 16) if 4 * n <= total]


class Leaves:
    """A level-0 buffer that torch owns, as the engine's calls take it."""

    def __init__(self, tensor):
        self.t = tensor
        self.ptr = tensor.data_ptr()

    def at(self, byte_offset):
        return self.ptr + int(byte_offset)

    def free(self):
        pass


def mixed_counts():
    """Trees of 1 .. 4095 leaves in a shuffled order, repeated until 2^log2 leaves are used up."""
    out, left = [], total
    while left:
        for c in rng.permutation(np.arange(1, 4096)):
            c = min(int(c), left)
            out.append(c)
            left -= c
            if not left:
                break
    return out


def nodes_of(counts):
    """The nodes an audit checks, from the counts alone: levels 1 .. h of every tree."""
    c = np.asarray(counts, dtype=np.int64)
    nodes, live = 0, c > 0
    while live.any():
        c = np.where(live, (c + 1) // 2, c)
        nodes += int(c[live].sum())
        live &= c > 1
    return nodes + int((np.asarray(counts) == 0).sum())


base = torch.randint(-2**31, 2**31 - 1, (total, 8), dtype=torch.int32, device="cuda", generator=gen)
d_status = dev.alloc(4)


class Shape:
    def __init__(self, name, counts):
        self.name, self.forest = name, counts is not None
        self.leaves = Leaves(base.clone())
        torch.cuda.synchronize()
        if self.forest:
            self.counts = np.asarray(counts, dtype=np.int64)
            self.starts = np.concatenate([[0], np.cumsum(self.counts)])
            self.s = dev._build_forest_of_buffer(self.leaves, total, counts, int(self.counts.max()), "audit_timing")
            self.ntrees, self.want_checked = len(counts), nodes_of(counts)
            self.d_masks = dev.alloc(8 * self.ntrees)
        else:
            self.s = dev.build_tree(self.leaves, total)
            self.ntrees, self.want_checked = 1, nodes_of([total])
        self.d_info = dev.alloc(32)
        self.bufs = {}
        dev.sync()

    def lists(self, n):
        if n not in self.bufs:
            self.bufs[n] = (dev.alloc(dev.audit_scratch_bytes(total, self.ntrees, n)), dev.alloc(4 * n), dev.alloc(4 * n), dev.alloc(8 * n))
        return self.bufs[n]

    def audit(self, n=0):
        d_scr, d_t, d_l, d_n = self.lists(n) if n else (None, None, None, None)
        if self.forest:
            self.s.audit_async(d_scr, self.d_masks, d_t, d_l, d_n, n, self.d_info)
        else:
            self.s.audit_async(d_scr, d_l, d_n, n, self.d_info)

    def info(self):
        return [int(x) for x in dev.download(self.d_info, 32, dtype=np.uint64)]

    def build(self):
        s = self.s
        if self.forest:
            dev.reduce_forest_tree_async(s.digests, s.total, s.offsets, s.ntrees, s.max_count, s.forest, s.roots_buf, d_status)
        else:
            dev.reduce_tree_async(s.digests, s.count, s.height, s.tree)

    def entries(self, flat):
        """(trees, indices) of flat leaf positions."""
        if not self.forest:
            return np.zeros(flat.shape[0], dtype=np.uint32), flat.astype(np.uint64)
        t = np.searchsorted(self.starts, flat, side="right") - 1
        return t.astype(np.uint32), (flat - self.starts[t]).astype(np.uint64)

    def plant(self, n):
        """n leaves with distinct level-1 parents, one bit of each flipped: (flat positions, the bad nodes they make, in order)."""
        flat = np.unique(rng.choice(total, size=2 * n, replace=False).astype(np.int64))
        t, i = self.entries(flat)
        _, first = np.unique(np.stack([t.astype(np.int64), (i >> np.uint64(1)).astype(np.int64)]), axis=1, return_index=True)
        keep = np.sort(first)[:n]
        flat, t, i = flat[keep], t[keep], i[keep]
        assert flat.shape[0] == n
        return flat, (t, (i >> np.uint64(1)))

    def flip(self, flat):
        at = torch.from_numpy(flat).cuda()
        self.leaves.t[at, 0] ^= 1 << 9
        torch.cuda.synchronize()

    def listed_ok(self, n, want):
        d_scr, d_t, d_l, d_n = self.lists(n)
        info = self.info()
        ok = info[:2] == [0, n] and info[3] == self.want_checked and (dev.download(d_l, 4 * n) == 1).all()
        ok = ok and (dev.download(d_n, 8 * n, dtype=np.uint64) == want[1]).all()
        if self.forest:
            ok = ok and (dev.download(d_t, 4 * n) == want[0]).all() and info[2] == np.unique(want[0]).shape[0]
        return bool(ok)


def timed(fn, e0, e1):
    dev.record(e0)
    fn()
    dev.record(e1)
    dev.sync()
    return dev.elapsed_ms(e0, e1)


shapes = [Shape(f"trees_of_{per}", [per] * (total // per)), Shape("trees_of_1_to_4095", mixed_counts()), Shape("one_tree", None)]
checks, rows = {}, {}
e0, e1 = dev.new_event(), dev.new_event()
for sh in shapes:
    sh.audit()
    checks[f"{sh.name}_fresh_clean"] = sh.info() == [0, 0, 0, sh.want_checked]
    k = min(1 << a.updates_log2, total // 4)
    flat = np.unique(rng.choice(total, size=k, replace=False).astype(np.int64))
    new = rng.integers(0, 2**32, size=(flat.shape[0], 8), dtype=np.uint32)
    t, i = sh.entries(flat)
    sh.s.update(t, i, new) if sh.forest else sh.s.update(i, new)
    sh.audit()
    checks[f"{sh.name}_clean_after_{flat.shape[0]}_updates"] = sh.info() == [0, 0, 0, sh.want_checked]
    planted = {n: sh.plant(n) for n in NS}
    for n, (flat, want) in planted.items():          # warm up the list form; the answers checked on the way
        sh.flip(flat)
        sh.audit(n)
        checks[f"{sh.name}_list_{n}_found_at_its_position"] = sh.listed_ok(n, want)
        sh.flip(flat)
    sh.build()
    sh.audit()
    checks[f"{sh.name}_clean_once_undone"] = sh.info() == [0, 0, 0, sh.want_checked]
    ms = {"masks": [], "build": [], **{f"list_{n}": [] for n in NS}}
    for r in range(a.runs):
        ms["masks"].append(timed(sh.audit, e0, e1))
        ms["build"].append(timed(sh.build, e0, e1))
        for n, (flat, want) in planted.items():
            sh.flip(flat)
            ms[f"list_{n}"].append(timed(lambda: sh.audit(n), e0, e1))
            sh.flip(flat)
    med = {k: round(float(np.median(v)), 4) for k, v in ms.items()}
    rows[sh.name] = {"ntrees": sh.ntrees, "levels": sh.s.stride, "nodes_checked": sh.want_checked, "audit_masks_event_ms": med["masks"],
                     "build_event_ms": med["build"], "audit_over_build": round(med["masks"] / med["build"], 4),
                     "within_10_percent_of_the_build": bool(med["masks"] <= 1.10 * med["build"]),
                     **{f"audit_list_{n}_event_ms": med[f"list_{n}"] for n in NS},
                     "scratch_bytes_of_the_list": int(dev.audit_scratch_bytes(total, sh.ntrees, 1))}

info = dev.lib.vkmr_hip_kernel_info().decode()
out = {"tool": "audit_timing", "leaves_log2": a.log2, "runs": a.runs, "device": dev.name(), "kernel_info": info, "build": provenance.build_id_of(info),
       "torch": torch.__version__, "checks": checks, "all_checks": all(checks.values()), "target": "audit_masks_event_ms <= 1.10 * build_event_ms",
       "shapes": rows}
line = json.dumps(out)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
