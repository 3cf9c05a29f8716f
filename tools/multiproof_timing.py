#!/usr/bin/env python3
"""One multiproof against k independent proofs of the same leaves, on a stored tree of 2^k random digests, timed with HIP
events: medians of interleaved runs in one process, after a warm-up of every shape.  Legs per index set (random sorted unique
k = 2^10, 2^16, 2^20 and one contiguous run of 2^16): (a) vkmr_hip_tree_multiproof_async, (b) vkmr_hip_verify_multiproof_async,
(c) vkmr_hip_tree_proofs_async, (d) vkmr_hip_verify_proofs_async.  Every leg reports ms; every set reports M, the bound, the
node hashes sum |A_l| and the bytes, computed on the host from the indices alone, and what the device reported.  Prints one
JSON line.  GPU box.
    python3 tools/multiproof_timing.py [--log2 26] [--ks 10,16,20] [--run-log2 16] [--runs 10]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vk_merkle_roots_amd as vk  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log2", type=int, default=26)
ap.add_argument("--ks", default="10,16,20", help="log2 of the random index counts")
ap.add_argument("--run-log2", type=int, default=16, help="log2 of the contiguous run's length")
ap.add_argument("--runs", type=int, default=10)
a = ap.parse_args()
dev = vk.HipDevice(0)
n, height = 1 << a.log2, a.log2
rng = np.random.default_rng(11)
sets = {}
for lk in [int(x) for x in a.ks.split(",")]:
    k = min(1 << lk, n)
    sets[f"random_k{k}"] = np.sort(rng.choice(n, size=k, replace=False)).astype(np.uint64)
run = min(1 << a.run_log2, n)
start = int(rng.integers(0, n - run + 1))
sets[f"run_k{run}"] = np.arange(start, start + run, dtype=np.uint64)
leaves = {name: np.empty((idx.shape[0], 8), dtype=np.uint32) for name, idx in sets.items()}
d_in = dev.alloc(32 * n)
chunk = min(1 << 22, n)
for at in range(0, n, chunk):   # random digests, uploaded in pieces; the proved leaves are kept on the way
    part = rng.integers(0, 2**32, size=(chunk, 8), dtype=np.uint32)
    vk.check(dev.lib.vkmr_hip_memcpy_h2d_async(dev.index, dev.stream, d_in.at(32 * at), part.ctypes.data, part.nbytes), "h2d")
    dev.sync()
    for name, idx in sets.items():
        lo, hi = np.searchsorted(idx, [at, at + chunk])
        leaves[name][lo:hi] = part[(idx[lo:hi] - np.uint64(at)).astype(np.int64)]
tree = dev.build_tree(d_in, n, height)


def structure(idx):
    """(per-level node counts, node hashes) of the multiproof of idx, from the indices alone."""
    counts, hashes, cur = [], 0, idx
    for _ in range(height):
        counts.append(int((~np.isin(cur ^ np.uint64(1), cur)).sum()))
        cur = np.unique(cur >> np.uint64(1))
        hashes += int(cur.shape[0])
    return counts, hashes


kmax = max(idx.shape[0] for idx in sets.values())
d_root = dev.upload(tree.root())
d_scr = dev.alloc(dev.lib.vkmr_hip_multiproof_scratch_bytes(kmax, height))
d_nodes = dev.alloc(32 * dev.lib.vkmr_hip_multiproof_max_nodes(n, height, kmax))
d_info, d_ok1 = dev.alloc(8 * (2 + height)), dev.alloc(4)
d_sib, d_ok = dev.alloc(32 * kmax * height), dev.alloc(4 * kmax)     # the single proofs of the largest set: freed with the process
bufs = {name: (dev.upload(idx), dev.upload(leaves[name])) for name, idx in sets.items()}
want = {name: structure(idx) for name, idx in sets.items()}
forms, report = [], {}
for name, idx in sets.items():
    k = int(idx.shape[0])
    d_idx, d_leaves = bufs[name]
    cap = dev.lib.vkmr_hip_multiproof_max_nodes(n, height, k)
    m = sum(want[name][0])

    def gather(d_idx=d_idx, k=k, cap=cap):
        tree.multiproof_async(d_idx, k, d_scr, d_nodes, cap, d_info)

    def verify(d_idx=d_idx, d_leaves=d_leaves, k=k, m=m):
        dev.verify_multiproof_async(d_leaves, d_idx, k, height, d_nodes, m, d_root, d_scr, d_ok1)

    def proofs(d_idx=d_idx, k=k):
        tree.proofs_async(d_idx, k, d_sib)

    def verify_single(d_idx=d_idx, d_leaves=d_leaves, k=k):
        dev.verify_proofs_async(d_leaves, d_idx, d_sib, k, height, d_root, 1, d_ok)

    # a set's four legs stay together: (b) reads the nodes of its own (a), (d) the siblings of its own (c)
    forms += [(f"{name}/multiproof", gather), (f"{name}/verify_multiproof", verify), (f"{name}/tree_proofs", proofs),
              (f"{name}/verify_proofs", verify_single)]
    # correctness of what is timed, once, outside the timed window
    gather(); verify(); proofs(); verify_single()
    info = dev.download(d_info, 8 * (2 + height), dtype=np.uint64)
    report[name] = {"k": k, "status": int(info[0]), "M": int(info[1]), "M_expected": m, "bound": cap,
                    "level_counts_match": [int(x) for x in info[2:]] == want[name][0], "multiproof_ok": int(dev.download(d_ok1, 4)[0]) == 1,
                    "single_proofs_ok": bool((dev.download(d_ok, 4 * k) == 1).all()), "bytes": 32 * m, "bytes_single": 32 * k * height,
                    "node_hashes": want[name][1], "node_hashes_single": k * height}
for _ in range(5):             # warm up every shape until the clocks have settled
    for _, fn in forms:
        fn()
dev.sync()
ev = {name: [(dev.new_event(), dev.new_event()) for _ in range(a.runs)] for name, _ in forms}
for r in range(a.runs):        # every form in turn, run after run
    for name, fn in forms:
        e0, e1 = ev[name][r]
        dev.record(e0); fn(); dev.record(e1)
dev.sync()
ms = {name: float(np.median([dev.elapsed_ms(e0, e1) for e0, e1 in v])) for name, v in ev.items()}
for name in sets:
    r = report[name]
    r["ms"] = {leg: round(ms[f"{name}/{leg}"], 4) for leg in ("multiproof", "verify_multiproof", "tree_proofs", "verify_proofs")}
    r["ms_multiproof_path"] = round(r["ms"]["multiproof"] + r["ms"]["verify_multiproof"], 4)
    r["ms_single_path"] = round(r["ms"]["tree_proofs"] + r["ms"]["verify_proofs"], 4)
    r["multiproof_vs_single"] = round(r["ms_multiproof_path"] / r["ms_single_path"], 4)
out = {"tool": "multiproof_timing", "leaves_log2": a.log2, "height": height, "runs": a.runs, "device": dev.name(),
       "kernel_info": dev.lib.vkmr_hip_kernel_info().decode(), "sets": report}
print(json.dumps(out))
