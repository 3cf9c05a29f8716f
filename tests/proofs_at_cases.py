"""Inclusion proofs as of an earlier count (vkmr_hip_forest_proofs_at_async, vkmr_host_cpu_forest_proofs_at,
MerkleForest.proofs_at / roots_at): the rule restated with hashlib over full level lists -- the old tree's right edge and root
(model_epoch) and the cells of a proof (model_proofs) --, the shapes, the drivers of the CPU twin and of the replay
(tests/c/proofs_at_plan_test.cpp) and the refusal table that tests/test_proofs_at_model.py, tests/test_proofs_at_abi.py (no GPU)
and tests/test_gpu_proofs_at.py share.  A plain module: no fixtures, no GPU.

An EPOCH is (tree, old count c).  Its edge row is [stride, 8] uint32: cell l the last node E_l of the old tree's level l for
ctz(c) < l < H(c), every other cell zero.  The proof of leaf i < c is H(c) cells of a [stride, 8] row: cell l the sibling of the
path node at level l IN THE TREE OF c LEAVES, read from the tree of c2 >= c leaves where that node is complete, else E_l."""
import os
import subprocess

import numpy as np

from consistency_cases import CANARY, GPU_COUNTS, REFUSAL_COUNTS, REFUSALS, STRIDE, ZERO, Forest, cnt, ctz, square  # noqa: F401
from merkle_model import ROOT, build_plan_exe, node, tree_height

HEIGHT_FILL = 0xA5A5A5A5


def hashes(c):
    """Node hashes of one epoch, from the rule alone: H(c) - ctz(c), none for a power of two of at least 2 (and for c == 0)."""
    if c == 0 or (c >= 2 and c & (c - 1) == 0):
        return 0
    return tree_height(c) - ctz(c)


def edge_levels(c):
    """The levels whose cell of the edge row holds a node."""
    return [] if hashes(c) == 0 else list(range(ctz(c) + 1, tree_height(c)))


def model_epoch(levels, c, stride=STRIDE):
    """(edge row [stride, 8], old root [8], node hashes) of the epoch of count c of the tree whose level lists NOW are `levels`
    (merkle_model.cpu_levels of its c2 >= c leaves): the issue's rule, level by level from ctz(c) + 1 up."""
    edge = np.zeros((stride, 8), np.uint32)
    if c == 0:
        return edge, ZERO.copy(), 0
    c2 = int(levels[0].shape[0])
    assert c <= c2 and c2.bit_length() <= stride
    H, l0 = tree_height(c), ctz(c)
    if c >= 2 and c & (c - 1) == 0:
        return edge, levels[H][0].copy(), 0                  # node 0 of level H(c) of the new tree; the root itself for c2 == c
    E, n = None, 0
    for l in range(l0 + 1, H + 1):
        if (c >> (l - 1)) & 1:
            P = levels[l - 1][(c >> (l - 1)) - 1]
            E = node(P, P if l - 1 == l0 else E)
        else:
            E = node(E, E)
        n += 1
        if l < H:
            edge[l] = E
    return edge, np.array(E, dtype=np.uint32), n


def model_proofs(levels, edge, c, indices, stride=STRIDE):
    """(siblings [k, stride, 8], heights [k]) of leaves `indices` as of count c; an index >= c: height 0 and zero cells."""
    indices = np.asarray(indices, dtype=np.int64).reshape(-1)
    cells, heights = np.zeros((indices.shape[0], stride, 8), np.uint32), np.zeros(indices.shape[0], np.uint32)
    good = indices < c
    if c == 0 or not good.any():
        return cells, heights
    H = tree_height(c)
    heights[good] = H
    i = indices[good]
    for l in range(H):
        j = i >> l
        s = np.where((j ^ 1) < cnt(c, l), j ^ 1, j)
        complete = ((s + 1) << l) <= c
        got = np.empty((i.shape[0], 8), np.uint32)
        got[complete] = levels[l][s[complete]]
        got[~complete] = edge[l]
        cells[good, l] = got
    return cells, heights


def forest_model(forest, epoch_trees, epoch_counts, epochs, indices, stride=STRIDE):
    """(edges [E, stride, 8], old roots [E, 8], siblings [k, stride, 8], heights [k]) for a consistency_cases.Forest."""
    E = len(epoch_trees)
    rows = [model_epoch(forest.levels(int(t)), int(c), stride) if forest.counts[int(t)] else (np.zeros((stride, 8), np.uint32), ZERO.copy(), 0)
            for t, c in zip(epoch_trees, epoch_counts)]
    edges = np.stack([r[0] for r in rows]) if E else np.zeros((0, stride, 8), np.uint32)
    old_roots = np.stack([r[1] for r in rows]) if E else np.zeros((0, 8), np.uint32)
    epochs, indices = np.asarray(epochs, dtype=np.int64).reshape(-1), np.asarray(indices, dtype=np.uint64).reshape(-1)
    siblings, heights = np.zeros((epochs.shape[0], stride, 8), np.uint32), np.zeros(epochs.shape[0], np.uint32)
    order = np.argsort(epochs, kind="stable")                # the queries of one epoch side by side
    first = np.searchsorted(epochs[order], np.arange(E + 1))
    for e in range(E):
        mine = order[first[e]: first[e + 1]]
        c, t = int(epoch_counts[e]), int(epoch_trees[e])
        if mine.size and c:
            ok = mine[indices[mine] < c]                     # model_proofs takes int64 indices: the bad ones stay zero
            siblings[ok], heights[ok] = model_proofs(forest.levels(t), edges[e], c, indices[ok].astype(np.int64), stride)
    return edges, old_roots, siblings, heights


# ---- the shapes ------------------------------------------------------------------------------------------------------------------
def every_epoch(counts, top=None):
    """(epoch trees, epoch counts): an epoch for every c in 1..count of every tree (of every tree up to `top` leaves)."""
    pairs = [(t, c) for t, n in enumerate(counts) if top is None or n <= top for c in range(1, n + 1)]
    return np.array([t for t, _ in pairs], dtype=np.uint32), np.array([c for _, c in pairs], dtype=np.uint64)


def every_leaf(epoch_counts):
    """(epochs, indices): a query for every leaf i < c of every epoch."""
    epochs = np.repeat(np.arange(len(epoch_counts), dtype=np.uint32), np.asarray(epoch_counts, dtype=np.int64))
    indices = np.concatenate([np.arange(int(c), dtype=np.uint64) for c in epoch_counts] + [np.zeros(0, np.uint64)])
    return epochs, indices


def powers(n):
    return {(1 << k) + d for k in range(n.bit_length()) for d in (-1, 0, 1)}


def gpu_epochs_and_queries(counts=GPU_COUNTS, seed=502, bad=64):
    """The issue's fixed lists.  Epochs: every c <= count for the trees up to 129 leaves (c == 0 included); 1, count - 1, count,
    2^k and 2^k +- 1 for the larger ones.  Queries: every i < c for c <= 129; 0, 1, c - 2, c - 1, 2^k and 2^k +- 1 for larger c;
    `bad` queries with an epoch outside the list and `bad` with an index at or above the count; shuffled."""
    rng = np.random.default_rng(seed)
    epochs = []
    for t, n in enumerate(counts):
        if n <= 129:
            epochs += [(t, c) for c in range(n + 1)]
        else:
            epochs += [(t, c) for c in sorted({1, n - 1, n} | powers(n)) if 1 <= c <= n]
    queries = []
    for e, (_, c) in enumerate(epochs):
        if c <= 129:
            queries += [(e, i) for i in range(c)]
        else:
            queries += [(e, i) for i in sorted({0, 1, c - 2, c - 1} | powers(c)) if 0 <= i < c]
    E = len(epochs)
    queries += [(E + int(rng.integers(0, 3)) * 1000003, int(rng.integers(0, 5))) for _ in range(bad)]
    for _ in range(bad):
        e = int(rng.integers(0, E))
        queries.append((e, epochs[e][1] + int(rng.integers(0, 3)) * (1 << 40)))
    order = rng.permutation(len(queries))
    return (np.array([t for t, _ in epochs], dtype=np.uint32), np.array([c for _, c in epochs], dtype=np.uint64),
            np.array([queries[i][0] for i in order], dtype=np.uint32), np.array([queries[i][1] for i in order], dtype=np.uint64))


# ---- the CPU twin (libvkmr_host.so) ----------------------------------------------------------------------------------------------
def host_proofs_at(leaves, offsets, epoch_trees, epoch_counts, epochs, indices, stride=STRIDE):
    """(status, edges [E, stride, 8], old roots [E, 8], siblings [k, stride, 8], heights [k]) of vkmr_host_cpu_forest_proofs_at;
    the outputs start as the canary."""
    import vk_merkle_roots_amd as vk
    leaves = np.ascontiguousarray(leaves, dtype=np.uint32).reshape(-1, 8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    epoch_trees, epoch_counts = np.ascontiguousarray(epoch_trees, dtype=np.uint32), np.ascontiguousarray(epoch_counts, dtype=np.uint64)
    epochs, indices = np.ascontiguousarray(epochs, dtype=np.uint32), np.ascontiguousarray(indices, dtype=np.uint64)
    E, k = int(epoch_trees.shape[0]), int(epochs.shape[0])
    assert epoch_counts.shape == (E,) and indices.shape == (k,)
    edges, old_roots = np.full((E, stride, 8), CANARY, np.uint32), np.full((E, 8), CANARY, np.uint32)
    siblings, heights = np.full((k, stride, 8), CANARY, np.uint32), np.full(k, HEIGHT_FILL, np.uint32)
    status = vk.host_lib().vkmr_host_cpu_forest_proofs_at(leaves.ctypes.data if leaves.size else None, offsets.ctypes.data, int(offsets.shape[0]) - 1,
                                                          epoch_trees.ctypes.data, epoch_counts.ctypes.data, E, epochs.ctypes.data if k else None,
                                                          indices.ctypes.data if k else None, k, stride, edges.ctypes.data, old_roots.ctypes.data,
                                                          siblings.ctypes.data if k else None, heights.ctypes.data if k else None)
    return status, edges, old_roots, siblings, heights


# ---- the replay ------------------------------------------------------------------------------------------------------------------
def build_proofs_at_plan_exe(directory, sanitize=True):
    """tests/c/proofs_at_plan_test.cpp as a program of its own, by default with AddressSanitizer and UBSan."""
    if not sanitize:
        return build_plan_exe(directory, "proofs_at_plan_test")
    exe = os.path.join(str(directory), "proofs_at_plan_test_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "vk_merkle_roots_amd", "csrc"), os.path.join(ROOT, "tests", "c", "proofs_at_plan_test.cpp"), "-o", exe])
    return exe


def plan_replay(exe, directory, cases):
    """One line per (first_offset, stride, counts, [(tree, old count), ..]) through tests/c/proofs_at_plan_test.cpp: per case
    (edge cells, node hashes, proofs, status); the C test has checked sources, bounds, the written set and every cell of every
    proof on the way."""
    path = os.path.join(str(directory), "proofs_at_cases.txt")
    with open(path, "w") as f:
        for first, stride, counts, epochs in cases:
            words = [first, stride, len(counts)] + list(counts) + [len(epochs)] + [v for e in epochs for v in e]
            f.write(" ".join(str(int(x)) for x in words) + "\n")
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    text = r.stdout.decode()
    assert r.returncode == 0 and "FAIL" not in text and f"ok: {len(cases)} cases" in text, text[-2000:]
    return [tuple(int(x) for x in line.split()) for line in text.splitlines()[: len(cases)]]
