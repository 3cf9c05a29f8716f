"""Frontiers: trees followed by a count and one peak per set bit of it (vkmr_hip_frontier_extend_async, vkmr_hip_frontier_roots_async,
vkmr_hip_verify_frontier_async, vkmr_hip_forest_frontier_async, vk.Frontier).  The two rules restated with hashlib on top of
merkle_model, the case tables, the drivers of the CPU twins and of the replay (tests/c/frontier_plan_test.cpp) that
tests/test_frontier_abi.py (no GPU) and tests/test_gpu_frontier.py share.  A plain module: no fixtures, no GPU.

A frontier here is (c, peaks): peaks a [stride, 8] uint32 array, cell l the node (c >> l) - 1 of level l for a set bit l of c,
zero for a clear bit."""
import functools
import os
import subprocess

import numpy as np

from merkle_model import build_plan_exe, cpu_levels, node, random_leaves, tree_height

STRIDE = 64
CANARY = 0xA5A5A5A5
MAX_COUNT = 1 << 58


def cnt(x, l):
    """Nodes of level l of a tree of x leaves."""
    return -(-x >> l)


def brute_frontier(leaves, stride=STRIDE):
    """(peaks [stride, 8], root [8]) of the tree over `leaves` ([c, 8]) from all of its levels; the zero root for no leaf."""
    c = int(leaves.shape[0])
    peaks = np.zeros((stride, 8), np.uint32)
    if c == 0:
        return peaks, np.zeros(8, np.uint32)
    levels = cpu_levels(leaves)
    for l in range(c.bit_length()):
        if (c >> l) & 1:
            peaks[l] = levels[l][(c >> l) - 1]
    return peaks, levels[-1][0]


def model_root(c, peaks):
    """The first rule: the root from a frontier."""
    if c == 0:
        return np.zeros(8, np.uint32)
    carry = None
    H = tree_height(c)
    for l in range(H):
        if (c >> l) & 1:
            carry = node(peaks[l], peaks[l] if carry is None else carry)
        elif carry is not None:
            carry = node(carry, carry)
    return np.array(peaks[H] if carry is None else carry, dtype=np.uint32)


def model_extend(c, peaks, new, stride=STRIDE):
    """The second rule: the frontier (c, peaks) takes the leaves `new` ([n, 8], n >= 0): (c2, new peaks [stride, 8], root), formed
    level by level from the new leaves and the named old peaks alone; asserts the node bound and that no other child is read.
    n == 0 runs through the same ranges; the one tree they form no root for (a power of two, no new leaf) takes P_H(c)."""
    n = int(new.shape[0])
    c2 = c + n
    out = np.zeros((stride, 8), np.uint32)
    if c2 == 0:
        return 0, out, np.zeros(8, np.uint32)
    below = {c + i: new[i] for i in range(n)}             # level 0's nodes [c, c2)
    root = None
    for l in range(stride):                               # the new peaks, level by level: `below` is level l's formed nodes
        if (c2 >> l) & 1:
            if (c2 >> l) == (c >> l):
                out[l] = peaks[l]
            else:
                out[l] = below[(c2 >> l) - 1]
        if l + 1 > tree_height(c2):
            continue
        formed = {}
        for j in range(c >> (l + 1), cnt(c2, l + 1)):
            kids = []
            for k in (2 * j, min(2 * j + 1, cnt(c2, l) - 1)):
                if k >= (c >> l):
                    kids.append(below[k])
                else:                                     # the only other child that ever occurs
                    assert k == (c >> l) - 1 and k == 2 * j and (c >> l) & 1, (c, n, l, j, k)
                    kids.append(peaks[l])
            formed[j] = node(kids[0], kids[1])
        assert len(formed) <= (n >> (l + 1)) + 2, (c, n, l)
        if l + 1 == tree_height(c2) and 0 in formed:
            root = formed[0]
        below = formed
    if root is None:
        assert n == 0 and c >= 2 and c & (c - 1) == 0, (c, n)
        root = peaks[tree_height(c)]
    return c2, out, np.array(root, dtype=np.uint32)


# ---- the case tables -------------------------------------------------------------------------------------------------------------
SQUARE = [(c, n) for c in range(41) for n in range(41)]                                  # every (c, n) in one batch: T = 1 681
EDGES = [(c, n) for c in (0, 1, 62, 63, 64, 65, 126, 127, 128, 129) for n in (0, 1, 2, 63, 64, 65, 66, 127, 128, 129)]   # wavefront edges
BIG = ((1 << 40) + (1 << 33) + 7, 70)                                                    # peaks are random digests: no leaf below c exists


class Batch:
    """T trees, tree q going from c_q leaves to c_q + n_q: the old frontiers by brute force over random leaves, the new leaves, and
    what the MODEL gives for the new counts, peaks and roots (the brute-force tree beside it where `check`)."""

    def __init__(self, pairs, seed, stride=STRIDE, check=True):
        rng = np.random.default_rng(seed)
        self.stride, self.T = stride, len(pairs)
        self.counts = np.array([c for c, _ in pairs], dtype=np.uint64)
        self.new_counts = [n for _, n in pairs]
        self.offsets = np.concatenate([[0], np.cumsum(self.new_counts)]).astype(np.uint64)
        self.peaks = np.zeros((self.T, stride, 8), np.uint32)
        self.leaves = random_leaves(rng, int(self.offsets[-1]))
        self.want_counts = np.array([c + n for c, n in pairs], dtype=np.uint64)
        self.want_peaks = np.zeros((self.T, stride, 8), np.uint32)
        self.want_roots = np.zeros((self.T, 8), np.uint32)
        for q, (c, n) in enumerate(pairs):
            new = self.leaves[int(self.offsets[q]): int(self.offsets[q + 1])]
            if c > 5000:                                   # a tree nobody can build: its peaks are random digests
                old = None
                for l in range(c.bit_length()):
                    if (c >> l) & 1:
                        self.peaks[q, l] = random_leaves(rng, 1)[0]
            else:
                old = random_leaves(rng, c)
                self.peaks[q] = brute_frontier(old, stride)[0]
            c2, self.want_peaks[q], self.want_roots[q] = model_extend(c, self.peaks[q], new, stride)
            assert c2 == c + n
            if check and old is not None:                  # the rule against the tree built from every leaf
                peaks, root = brute_frontier(np.concatenate([old, new]), stride)
                assert (peaks == self.want_peaks[q]).all() and (root == self.want_roots[q]).all(), (c, n)
                assert (model_root(c2, peaks) == root).all(), (c, n)


@functools.lru_cache(maxsize=None)
def square():
    return Batch(SQUARE, seed=301)


@functools.lru_cache(maxsize=None)
def edges():
    return Batch(EDGES, seed=302)


@functools.lru_cache(maxsize=None)
def big():
    return Batch([BIG, (5, 3)], seed=303)


# ---- the CPU twins (libvkmr_host.so) ---------------------------------------------------------------------------------------------
def host_roots(counts, peaks):
    """(return code, roots [T, 8]) of vkmr_host_cpu_frontier_roots; the roots start as the canary."""
    import vk_merkle_roots_amd as vk
    counts = np.ascontiguousarray(counts, dtype=np.uint64)
    peaks = np.ascontiguousarray(peaks, dtype=np.uint32)
    T, stride = counts.shape[0], peaks.shape[1]
    roots = np.full((T, 8), CANARY, np.uint32)
    rc = vk.host_lib().vkmr_host_cpu_frontier_roots(counts.ctypes.data, peaks.ctypes.data, stride, T, roots.ctypes.data)
    return rc, roots


def host_extend(counts, peaks, leaves, offsets, max_new=None, total_new=None, in_place=False):
    """(status, new counts, new peaks, roots) of vkmr_host_cpu_frontier_extend; the outputs start as the canary (in place: as
    copies of the inputs)."""
    import vk_merkle_roots_amd as vk
    counts = np.ascontiguousarray(counts, dtype=np.uint64)
    peaks = np.ascontiguousarray(peaks, dtype=np.uint32)
    leaves = np.ascontiguousarray(leaves, dtype=np.uint32).reshape(-1, 8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    T, stride = counts.shape[0], peaks.shape[1]
    new_counts = counts.copy() if in_place else np.full(T, 0xA5A5A5A5A5A5A5A5, np.uint64)
    new_peaks = peaks.copy() if in_place else np.full(peaks.shape, CANARY, np.uint32)
    roots = np.full((T, 8), CANARY, np.uint32)
    diffs = np.diff(offsets.astype(np.int64)) if T else np.zeros(0, np.int64)
    max_new = int(max(0, diffs.max())) if max_new is None and T else (max_new or 0)
    total_new = int(leaves.shape[0]) if total_new is None else total_new
    src_counts, src_peaks = (new_counts, new_peaks) if in_place else (counts, peaks)
    status = vk.host_lib().vkmr_host_cpu_frontier_extend(src_counts.ctypes.data, src_peaks.ctypes.data, stride, T, leaves.ctypes.data if leaves.size else None,
                                                         total_new, offsets.ctypes.data, max_new, new_counts.ctypes.data, new_peaks.ctypes.data,
                                                         roots.ctypes.data)
    return status, new_counts, new_peaks, roots


def host_forest_frontier(leaves, counts, stride=STRIDE):
    """(return code, counts, peaks) of vkmr_host_cpu_forest_frontier over the trees `counts` of `leaves`."""
    import vk_merkle_roots_amd as vk
    leaves = np.ascontiguousarray(leaves, dtype=np.uint32).reshape(-1, 8)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    T = len(counts)
    out_counts, out_peaks = np.full(T, 0xA5A5A5A5A5A5A5A5, np.uint64), np.full((T, stride, 8), CANARY, np.uint32)
    rc = vk.host_lib().vkmr_host_cpu_forest_frontier(leaves.ctypes.data if leaves.size else None, offsets.ctypes.data, T, stride, out_counts.ctypes.data,
                                                     out_peaks.ctypes.data)
    return rc, out_counts, out_peaks


# The refusals of the extend, each alone: (what, the status word, old counts, offsets, max_new, stride); total_new is 6 leaves.
REFUSALS = [
    ("decreasing offsets", 1, [3, 4, 5], [0, 4, 2, 6], 4, 8),
    ("offsets[T] != total_new", 1, [3, 4, 5], [0, 2, 4, 5], 4, 8),
    ("offsets[0] != 0", 1, [3, 4, 5], [1, 2, 4, 6], 4, 8),
    ("n_q > max_new", 2, [3, 4, 5], [0, 1, 5, 6], 3, 8),
    ("a new count of more bits than stride", 8, [3, 250, 5], [0, 0, 6, 6], 6, 8),
    ("a sum above 2^58", 4, [3, MAX_COUNT - 2, 5], [0, 1, 4, 6], 4, 64),
]


def refusal_frontier(counts, stride, seed=311):
    """Old frontiers for a refusal case: random digests in the cells of set bits (no tree of 2^58 leaves can be built)."""
    rng = np.random.default_rng(seed)
    peaks = np.zeros((len(counts), stride, 8), np.uint32)
    for q, c in enumerate(counts):
        for l in range(min(stride, int(c).bit_length())):
            if (int(c) >> l) & 1:
                peaks[q, l] = random_leaves(rng, 1)[0]
    return np.array(counts, dtype=np.uint64), peaks, random_leaves(rng, 6)


# ---- the replay ------------------------------------------------------------------------------------------------------------------
def build_frontier_plan_exe(directory):
    return build_plan_exe(directory, "frontier_plan_test")


def plan_replay(exe, directory, batches):
    """One line per (stride, [(c, n), ..]) through tests/c/frontier_plan_test.cpp: per batch (launches, scratch cells touched,
    hashes, lanes); the C test has checked the lanes, the reads, the writes and the values on the way."""
    path = os.path.join(str(directory), "frontier_batches.txt")
    with open(path, "w") as f:
        for stride, pairs in batches:
            f.write(" ".join(str(int(x)) for x in [stride] + [v for pair in pairs for v in pair]) + "\n")
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    text = r.stdout.decode()
    assert r.returncode == 0 and "FAIL" not in text and f"ok: {len(batches)} batches" in text, text[-2000:]
    return [tuple(int(x) for x in line.split()) for line in text.splitlines()[: len(batches)]]
