#!/usr/bin/env python3
"""A holder of the roots alone follows k leaf updates from one multiproof (vkmr_hip_apply_forest_multiproof_async) beside what
existed before it, timed with HIP events: medians of interleaved runs in one process after a warm-up of every shape, stamped
with the build id.  Prints one JSON line (and writes it to --out).  GPU box.
    python3 tools/multiproof_apply_timing.py [--log2 26] [--ks 16,20] [--runs 10] [--out FILE]

  forest   2^(log2 - 11) trees of 2^11 (H = 11), and the same leaves as ONE tree of 2^log2 (height log2)
  entries  2^k random positions, sorted and deduplicated (so slightly fewer); new leaves random
  1  apply against vkmr_hip_verify_forest_multiproof_async on the same proof: twice the node hashes over nearly the same loads
  2  apply against vkmr_hip_reduce_forest_async over the whole forest: what a follower without a witness pays
  3  vkmr_hip_apply_multiproof_async against the forest call, both on the one tree of 2^log2
Every timed apply writes its verdict into slot r of its verdict buffer and its roots into a buffer of its own; after the timed
loop the primary's update runs (vkmr_hip_forest_update_async, vkmr_hip_tree_update_async), the applied roots must equal the
updated structure's, and the old leaves are put back before the next set is checked."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vk_merkle_roots_amd as vk  # noqa: E402
from vk_merkle_roots_amd import provenance  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log2", type=int, default=26)
ap.add_argument("--ks", default="16,20", help="log2 of the random entry counts")
ap.add_argument("--runs", type=int, default=10)
ap.add_argument("--out", default=None)
a = ap.parse_args()
dev = vk.HipDevice(0)
n = 1 << a.log2
rng = np.random.default_rng(7)
d_in = dev.alloc(32 * n)
chunk = min(n, 1 << 22)
base = rng.integers(0, 2**32, size=(chunk, 8), dtype=np.uint32)
for at in range(0, n, chunk):   # random digests, uploaded in pieces: one random piece, made different per piece
    part = base ^ np.uint32((at // chunk) * 2654435761 & 0xFFFFFFFF)
    vk.check(dev.lib.vkmr_hip_memcpy_h2d_async(dev.index, dev.stream, d_in.at(32 * at), part.ctypes.data, part.nbytes), "h2d")
    dev.sync()


def leaves_at(cells):
    """[k, 8]: the digests at `cells` of d_in, formed on the host as the upload formed them."""
    cells = np.asarray(cells, dtype=np.int64)
    return np.ascontiguousarray(base[cells % chunk] ^ ((cells // chunk) * 2654435761 & 0xFFFFFFFF).astype(np.uint32)[:, None])


class Slot:
    """A device pointer inside another buffer, for the wrappers that read `.ptr`."""

    def __init__(self, buf, offset):
        self.ptr = buf.at(offset)


cap = min(1 << 11, n)
ntrees, H = n // cap, vk.tree_height(cap)
offsets, _ = vk.engine.forest_offsets([cap] * ntrees)
d_off = dev.upload(offsets)
d_roots, d_status, d_forest = dev.alloc(32 * ntrees), dev.alloc(4), dev.alloc(dev.forest_tree_bytes(n, ntrees, cap))
dev.reduce_forest_tree_async(d_in, n, d_off, ntrees, cap, d_forest, d_roots, d_status)
d_reduce_scr, d_reduce_roots, d_reduce_status = dev.alloc(dev.lib.vkmr_hip_forest_scratch_bytes(n, ntrees)), dev.alloc(32 * ntrees), dev.alloc(4)
d_tree = dev.alloc(dev.tree_bytes(n, a.log2))
dev.reduce_tree_async(d_in, n, a.log2, d_tree)
d_tree_root = Slot(d_tree, dev.tree_bytes(n, a.log2) - 32)
dev.sync()
assert int(dev.download(d_status, 4)[0]) == 0


class Entries:
    """One sorted set of positions, as entries of the forest and as indices of the one tree, the proofs of both gathered once."""

    def __init__(self, lg):
        self.name = f"random_2^{lg}"
        cells = np.unique(np.random.default_rng(100 + lg).integers(0, n, size=1 << lg).astype(np.uint64))
        self.k = k = int(cells.shape[0])
        self.cells = cells
        self.trees, self.indices = (cells // np.uint64(cap)).astype(np.uint32), cells % np.uint64(cap)
        self.old, self.new = leaves_at(cells), np.random.default_rng(200 + lg).integers(0, 2**32, size=(k, 8), dtype=np.uint32)
        self.d_old, self.d_new = dev.upload(self.old), dev.upload(self.new)
        self.d_trees, self.d_idx, self.d_cells = dev.upload(self.trees), dev.upload(self.indices), dev.upload(cells)
        self.d_counts, self.d_zero = dev.upload(np.full(k, cap, dtype=np.uint64)), dev.upload(np.zeros(k, dtype=np.uint32))
        self.d_one_count = dev.upload(np.full(k, n, dtype=np.uint64))
        # the forest's proof and the one tree's, gathered once
        fcap = dev.lib.vkmr_hip_forest_multiproof_max_nodes(n, ntrees, cap, k)
        self.d_nodes, self.d_h, d_info = dev.alloc(32 * fcap), dev.alloc(4 * k), dev.alloc(8 * (2 + H))
        dev.forest_multiproof_async(d_in, d_forest, n, d_off, ntrees, cap, self.d_trees, self.d_idx, k,
                                    dev.alloc(dev.lib.vkmr_hip_forest_multiproof_scratch_bytes(k, H)), self.d_nodes, fcap, self.d_h, d_info)
        info = dev.download(d_info, 8 * (2 + H), dtype=np.uint64)
        assert int(info[0]) == 0
        self.M = int(info[1])
        tcap = dev.lib.vkmr_hip_multiproof_max_nodes(n, a.log2, k)
        self.d_tnodes, d_tinfo = dev.alloc(32 * tcap), dev.alloc(8 * (2 + a.log2))
        dev.tree_multiproof_async(d_in, d_tree, n, a.log2, self.d_cells, k, dev.alloc(dev.lib.vkmr_hip_multiproof_scratch_bytes(k, a.log2)), self.d_tnodes,
                                  tcap, d_tinfo)
        tinfo = dev.download(d_tinfo, 8 * (2 + a.log2), dtype=np.uint64)
        assert int(tinfo[0]) == 0
        self.TM = int(tinfo[1])
        self.hashes = sum(int(np.unique(cells >> np.uint64(l)).shape[0]) for l in range(1, H + 1))     # distinct (tree, index >> l), 1 <= l <= H
        self.d_scr, self.d_vscr = dev.alloc(dev.apply_multiproof_scratch_bytes(k, H)), dev.alloc(dev.lib.vkmr_hip_forest_multiproof_scratch_bytes(k, H))
        self.d_tscr, self.d_fscr = (dev.alloc(dev.apply_multiproof_scratch_bytes(k, a.log2)) for _ in range(2))
        self.d_ok = {what: dev.alloc(4 * a.runs) for what in ("apply", "verify", "tree", "one")}
        self.d_out, self.d_tree_out, self.d_one_out = dev.alloc(32 * ntrees), dev.alloc(32), dev.alloc(32)

    def apply(self, r=0):
        dev.apply_forest_multiproof_enqueue(self.d_old, self.d_new, self.d_trees, self.d_idx, self.d_counts, self.k, H, self.d_nodes, self.M, d_roots,
                                            ntrees, self.d_scr, Slot(self.d_ok["apply"], 4 * r), self.d_out)

    def verify(self, r=0):
        dev.verify_forest_multiproof_async(self.d_old, self.d_trees, self.d_idx, self.d_h, self.k, H, self.d_nodes, self.M, d_roots, ntrees,
                                           self.d_vscr, Slot(self.d_ok["verify"], 4 * r))

    def apply_tree(self, r=0):
        dev.apply_multiproof_enqueue(self.d_old, self.d_new, self.d_cells, self.k, n, a.log2, self.d_tnodes, self.TM, d_tree_root, self.d_tscr,
                                     Slot(self.d_ok["tree"], 4 * r), self.d_tree_out)

    def apply_forest_of_one(self, r=0):
        dev.apply_forest_multiproof_enqueue(self.d_old, self.d_new, self.d_zero, self.d_cells, self.d_one_count, self.k, a.log2, self.d_tnodes, self.TM,
                                            d_tree_root, 1, self.d_fscr, Slot(self.d_ok["one"], 4 * r), self.d_one_out)


def reduce_forest(r=0):
    dev.reduce_forest_async(d_in, n, d_off, ntrees, cap, d_reduce_scr, d_reduce_roots, d_reduce_status)


sets = [Entries(int(x)) for x in a.ks.split(",")]
forms = [("reduce_forest", reduce_forest)]
for e in sets:
    forms += [(f"apply_{e.name}", e.apply), (f"verify_{e.name}", e.verify), (f"apply_tree_{e.name}", e.apply_tree),
              (f"apply_forest_of_one_tree_{e.name}", e.apply_forest_of_one)]
# warm up until the clocks have settled (every shape, several times), then every form in turn, run after run
for _ in range(3):
    for _, fn in forms:
        fn()
dev.sync()
ev = {name: [(dev.new_event(), dev.new_event()) for _ in range(a.runs)] for name, _ in forms}
for r in range(a.runs):
    for name, fn in forms:
        e0, e1 = ev[name][r]
        dev.record(e0); fn(r); dev.record(e1)
dev.sync()
ms = {name: float(np.median([dev.elapsed_ms(e0, e1) for e0, e1 in v])) for name, v in ev.items()}

info = dev.lib.vkmr_hip_kernel_info().decode()
out = {"tool": "multiproof_apply_timing", "leaves_log2": a.log2, "ntrees": ntrees, "H": H, "runs": a.runs, "ms": {k: round(v, 4) for k, v in ms.items()},
       "sets": {}, "device": dev.name(), "kernel_info": info, "build": provenance.build_id_of(info)}
old_roots = dev.download(d_roots, 32 * ntrees).reshape(-1, 8)
ok = bool(int(dev.download(d_reduce_status, 4)[0]) == 0 and (dev.download(d_reduce_roots, 32 * ntrees).reshape(-1, 8) == old_roots).all())
out["reduce_forest_gives_the_stored_roots"] = ok
d_ustatus = dev.alloc(4)
for e in sets:
    applied, one = dev.download(e.d_out, 32 * ntrees).reshape(-1, 8), (dev.download(e.d_tree_out, 32), dev.download(e.d_one_out, 32))
    verdicts = {what: bool((dev.download(b, 4 * a.runs) == 1).all()) for what, b in e.d_ok.items()}      # every timed run
    # the primary's side: the update itself, compared, and the old leaves put back
    dev.forest_update_async(d_in, d_forest, n, d_off, ntrees, cap, e.d_trees, e.d_idx, e.d_new, e.k, d_roots, d_ustatus)
    dev.tree_update_async(d_in, d_tree, n, a.log2, e.d_cells, e.d_new, e.k, d_ustatus)
    new_roots, new_root = dev.download(d_roots, 32 * ntrees).reshape(-1, 8), dev.download(d_tree, 32, offset=dev.tree_bytes(n, a.log2) - 32)
    dev.forest_update_async(d_in, d_forest, n, d_off, ntrees, cap, e.d_trees, e.d_idx, e.d_old, e.k, d_roots, d_ustatus)
    dev.tree_update_async(d_in, d_tree, n, a.log2, e.d_cells, e.d_old, e.k, d_ustatus)
    restored = bool((dev.download(d_roots, 32 * ntrees).reshape(-1, 8) == old_roots).all())
    named = np.unique(e.trees).astype(np.int64)
    rec = {"k": e.k, "nodes": e.M, "nodes_one_tree": e.TM, "trees_named": int(named.shape[0]), "node_hashes_verify": e.hashes,
           "node_hashes_apply": 2 * e.hashes, "every_timed_run_accepted": verdicts,
           "applied_roots_equal_the_updated_forest_s": bool((applied[named] == new_roots[named]).all()),
           "tree_call_and_forest_call_give_the_updated_tree_s_root": bool((one[0] == new_root).all() and (one[1] == new_root).all()),
           "old_leaves_put_back": restored,
           "apply_ms": ms[f"apply_{e.name}"], "verify_ms": ms[f"verify_{e.name}"], "reduce_forest_ms": ms["reduce_forest"],
           "apply_over_verify": ms[f"apply_{e.name}"] / ms[f"verify_{e.name}"],
           "apply_over_reduce_forest": ms[f"apply_{e.name}"] / ms["reduce_forest"],
           "apply_tree_ms": ms[f"apply_tree_{e.name}"], "apply_forest_of_one_tree_ms": ms[f"apply_forest_of_one_tree_{e.name}"],
           "tree_call_over_forest_call": ms[f"apply_tree_{e.name}"] / ms[f"apply_forest_of_one_tree_{e.name}"]}
    ok = ok and all(verdicts.values()) and rec["applied_roots_equal_the_updated_forest_s"] and restored and \
        rec["tree_call_and_forest_call_give_the_updated_tree_s_root"]
    out["sets"][e.name] = rec
out["all_checks_ok"] = ok
line = json.dumps(out)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
sys.exit(0 if ok else 1)
