#!/usr/bin/env python3
"""What sorted trees cost (vkmr_hip_forest_sorted_async, _lower_bound_async, _absence_async, vkmr_hip_verify_forest_absence_async),
timed with HIP events: medians of interleaved runs in one process after a warm-up of every leg, stamped with the build id.
Prints one JSON line (and writes it to --out).  GPU box.
    python3 tools/absence_timing.py [--log2 26] [--runs 10] [--out profiles/absence_timing.json]

  the leaves   2^log2 digests, strictly increasing over the whole buffer (a 64-bit prefix that grows with the position, random
               bits behind it), so every tree of either shape is sorted
  the shapes   the same leaves stored once as trees of 2 048 and once as ONE tree
  the legs     Q = 2^10, 2^16, 2^20 queries in random order, half of them leaves, half absent (a leaf with one bit of word 7
               turned); every leg times the sorted pass, the lower bound, the gather and the verifier
  yardsticks   beside them, in this process and not the code under test: for the sorted pass torch's sum over an int32 tensor of
               the same 32 * total bytes, a read-only pass; for the verifier vkmr_hip_verify_forest_proofs_async over 2 Q plain
               proofs, what a verifier without the compact form would fold
Every leg's answers are checked before the clock starts: the pass finds every tree sorted, the present half is found where it was
taken from and proven present, the absent half proven absent, the plain proofs all hold.  No ratio is fixed in advance."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vk_merkle_roots_amd as vk  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log2", type=int, default=26)
ap.add_argument("--runs", type=int, default=10)
ap.add_argument("--out", default=None)
a = ap.parse_args()
dev = vk.HipDevice(0)
n = 1 << a.log2
TREE = 2048
rng = np.random.default_rng(29)
chunk = min(n, 1 << 22)
base = rng.integers(0, 2**32, size=(chunk, 8), dtype=np.uint32)
low_bits = 64 - a.log2
jitter = rng.integers(0, 1 << min(low_bits, 62), size=chunk, dtype=np.uint64)


def piece(i):
    """Leaves [i * chunk, (i + 1) * chunk): words 0 and 1 the position in the top bits of 64 and random bits below, so that the
    leaves increase strictly over the whole buffer; words 2..7 random, made different per piece."""
    out = base ^ np.uint32(i * 2654435761 & 0xFFFFFFFF)
    prefix = ((np.arange(chunk, dtype=np.uint64) + np.uint64(i * chunk)) << np.uint64(low_bits)) | jitter
    out[:, 0], out[:, 1] = (prefix >> np.uint64(32)).astype(np.uint32), (prefix & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return out


def leaves_at(pos):
    out = np.empty((pos.shape[0], 8), dtype=np.uint32)
    which = pos // chunk
    for i in np.unique(which):
        sel = which == i
        out[sel] = piece(int(i))[pos[sel] % chunk]
    return out


d_leaves = dev.alloc(32 * n)
for i in range(n // chunk):
    part = piece(i)
    vk.check(dev.lib.vkmr_hip_memcpy_h2d_async(dev.index, dev.stream, d_leaves.at(32 * i * chunk), part.ctypes.data, part.nbytes), "h2d")
    dev.sync()
yard = torch.empty(8 * n, dtype=torch.int32, device="cuda").random_()          # 32 * n bytes of its own


class Leg:
    """Q queries into one stored shape, half of them leaves: buffers of its own (the legs are interleaved)."""

    def __init__(self, forest, per, Q):
        self.forest, self.per, self.Q, self.stride = forest, per, Q, forest.levels
        pos = np.unique(rng.integers(0, n, size=Q // 2)).astype(np.int64)
        gone = rng.integers(0, n, size=Q - pos.shape[0]).astype(np.int64)
        absent = leaves_at(gone)
        absent[:, 7] ^= np.uint32(1)                                             # not a leaf: the prefixes of the leaves are all different
        self.present, self.pos = pos.shape[0], np.concatenate([pos, gone])
        self.order = rng.permutation(Q)
        queries, trees = np.concatenate([leaves_at(pos), absent])[self.order], (self.pos // per).astype(np.uint32)[self.order]
        self.d_q, self.d_t = dev.upload(queries), dev.upload(trees)
        self.d_idx, self.d_found, self.d_h, self.d_verdict = dev.alloc(8 * Q), dev.alloc(4 * Q), dev.alloc(4 * Q), dev.alloc(4 * Q)
        self.d_nb, self.d_main, self.d_low = dev.alloc(64 * Q), dev.alloc(32 * Q * self.stride), dev.alloc(32 * Q * self.stride)
        self.d_bad, self.d_info = dev.alloc(8 * forest.ntrees), dev.alloc(32)
        self.d_counts = dev.upload(forest.counts)
        # the yardstick of the verifier: 2 Q plain proofs, of every query's position and of the leaf in front of it
        at = (self.pos % per)[self.order]
        plain_i = np.concatenate([at, np.maximum(at, 1) - 1]).astype(np.uint64)
        plain_t = np.concatenate([trees, trees])
        self.d_pt, self.d_pi = dev.upload(plain_t), dev.upload(plain_i)
        self.d_pl, self.d_ps, self.d_ph, self.d_ok = dev.upload(leaves_at(plain_t.astype(np.int64) * per + plain_i.astype(np.int64))), dev.alloc(64 * Q * self.stride), dev.alloc(8 * Q), dev.alloc(8 * Q)
        forest.proofs_async(self.d_pt, self.d_pi, 2 * Q, self.d_ps, self.d_ph)
        dev.sync()

    def sorted(self):
        self.forest.sorted_async(self.d_bad, self.d_info)

    def lower_bound(self):
        self.forest.lower_bound_async(self.d_t, self.d_q, self.Q, self.d_idx, self.d_found)

    def gather(self):
        self.forest.absence_async(self.d_t, self.d_q, self.Q, self.stride, self.d_idx, self.d_nb, self.d_main, self.d_low, self.d_h)

    def verify(self):
        dev.verify_forest_absence_enqueue(self.d_q, self.d_t, self.d_idx, self.d_nb, self.d_main, self.d_low, self.d_h, self.Q, self.stride,
                                          self.forest.roots_buf, self.d_counts, self.forest.ntrees, self.d_verdict)

    def plain(self):
        dev.verify_forest_proofs_async(self.d_pl, self.d_pt, self.d_pi, self.d_ps, self.d_ph, 2 * self.Q, self.stride, self.forest.roots_buf,
                                       self.forest.ntrees, self.d_ok)

    STEPS = ("sorted", "lower_bound", "gather", "verify", "plain")

    def check(self):
        info = dev.download(self.d_info, 32, dtype=np.uint64).tolist()
        idx, found = dev.download(self.d_idx, 8 * self.Q, dtype=np.uint64), dev.download(self.d_found, 4 * self.Q)
        verdict, ok = dev.download(self.d_verdict, 4 * self.Q), dev.download(self.d_ok, 8 * self.Q)
        is_leaf = np.zeros(self.Q, bool)
        is_leaf[: self.present] = True
        is_leaf, at = is_leaf[self.order], (self.pos % self.per)[self.order]
        tops = np.array([(int(i) & -int(i)).bit_length() - 1 for i in idx[~is_leaf][:4096] if 0 < int(i) < self.per])
        return {"sorted": info[:3] == [0, 0, 0] and info[3] == n - self.forest.ntrees, "found": bool((found == is_leaf).all()),
                "indices": bool((idx[is_leaf] == at[is_leaf]).all() and (np.abs(idx[~is_leaf].astype(np.int64) - at[~is_leaf]) <= 1).all()),
                "verdicts": bool((verdict == np.where(is_leaf, 2, 1)).all()), "plain_proofs": bool((ok == 1).all())}, float(tops.mean()) if tops.size else None


def measure(per):
    ntrees = n // per
    forest = dev._build_forest_of_buffer(d_leaves, n, [per] * ntrees, per, "absence_timing")
    legs = [Leg(forest, per, Q) for Q in (1 << 10, 1 << 16, 1 << 20)]
    for _ in range(3):                            # warm up until the clocks have settled, every step of every leg and the yardstick
        for leg in legs:
            for step in Leg.STEPS:
                getattr(leg, step)()
            yard.sum()
    dev.sync()
    torch.cuda.synchronize()
    out = {"trees": ntrees, "leaves_per_tree": per, "stride": forest.levels, "checks": {}, "legs": {}}
    mean_top = {}
    for leg in legs:
        out["checks"][str(leg.Q)], mean_top[leg.Q] = leg.check()
    ev = {(leg.Q, step): [(dev.new_event(), dev.new_event()) for _ in range(a.runs)] for leg in legs for step in Leg.STEPS}
    tev = {leg.Q: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.runs)] for leg in legs}
    for r in range(a.runs):
        for leg in legs:                          # every step of the leg, then the read-only yardstick; each waits for the one before
            for step in Leg.STEPS:
                e0, e1 = ev[leg.Q, step][r]
                dev.record(e0); getattr(leg, step)(); dev.record(e1)
                dev.sync()
            t0, t1 = tev[leg.Q][r]
            t0.record(); yard.sum(); t1.record()
            torch.cuda.synchronize()
    for leg in legs:
        ms = {step: [dev.elapsed_ms(e0, e1) for e0, e1 in ev[leg.Q, step]] for step in Leg.STEPS}
        med = {step: float(np.median(v)) for step, v in ms.items()}
        y = float(np.median([t0.elapsed_time(t1) for t0, t1 in tev[leg.Q]]))
        out["legs"][str(leg.Q)] = {
            "sorted_ms": round(med["sorted"], 4), "sorted_GB_per_s": round(32 * n / (med["sorted"] * 1e-3) / 1e9, 1), "read_yardstick_ms": round(y, 4),
            "read_yardstick_GB_per_s": round(32 * n / (y * 1e-3) / 1e9, 1), "sorted_over_yardstick": round(med["sorted"] / y, 3),
            "lower_bound_ms": round(med["lower_bound"], 4), "gather_ms": round(med["gather"], 4), "verify_ms": round(med["verify"], 4),
            "plain_verify_2Q_ms": round(med["plain"], 4), "verify_over_plain": round(med["verify"] / med["plain"], 3),
            "mean_top_of_two_sided_absent": None if mean_top[leg.Q] is None else round(mean_top[leg.Q], 3),
            "min_max_ms": {step: [round(min(v), 4), round(max(v), 4)] for step, v in ms.items()}}
    for leg in legs:
        for name, buf in vars(leg).items():
            if name.startswith("d_"):
                buf.free()
    forest.free()
    return out


out = {"tool": "absence_timing", "leaves_log2": a.log2, "runs": a.runs, "bytes_read_by_the_sorted_pass": 32 * n, "device": dev.name(),
       "kernel_info": dev.lib.vkmr_hip_kernel_info().decode(),
       "hashes_per_proof": "H + top against 2 H of two plain proofs: a derivation (csrc/absence_plan.hpp), not a measurement",
       "shapes": {"trees_of_2048": measure(min(TREE, n)), "one_tree": measure(n)}}
line = json.dumps(out)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
