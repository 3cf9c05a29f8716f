"""Consistency proofs (vkmr_hip_forest_consistency_async, vkmr_hip_verify_consistency_async, vk.ConsistencyProof,
MerkleForest.consistency): the rule restated with hashlib over full level lists -- which cells a proof holds (model_gather) and
what a holder of two roots checks (model_check, which also records the cells it reads) --, the shapes, the drivers of the CPU
twins and of the replay (tests/c/consistency_plan_test.cpp) and the refusal table that tests/test_consistency_model.py,
tests/test_consistency_abi.py (no GPU) and tests/test_gpu_consistency.py share.  A plain module: no fixtures, no GPU.

A proof of "the tree of c2 leaves extends the tree of c leaves" is two [stride, 8] uint32 rows: peaks, cell l the node
(c >> l) - 1 of level l for a set bit l of c; rights, cell l the right neighbour of the node the walk from P_l0 (l0 the lowest
set bit of c) to the root stands on at level l, where that node is a left child and has one.  Every other cell is zero."""
import functools
import hashlib
import os
import subprocess

import numpy as np

from merkle_model import ROOT, build_plan_exe, cpu_levels, node, random_leaves, tree_height

STRIDE = 64
CANARY = 0xA5A5A5A5
COUNT_FILL = 0xA5A5A5A5A5A5A5A5
MAX_COUNT = 1 << 58
ZERO = np.zeros(8, np.uint32)


def cnt(x, l):
    """Nodes of level l of a tree of x >= 1 leaves."""
    return ((x - 1) >> l) + 1


def ctz(c):
    return (c & -c).bit_length() - 1


def walk(c, c2):
    """The new-root walk of 1 <= c <= c2, level by level from l0 to H(c2) - 1: (l, what the accumulator is hashed with) --
    "right": rights[l] behind it; "self": itself, the level ends with it; "peak": P_l in front of it."""
    l0, out = ctz(c), []
    for l in range(l0, tree_height(c2)):
        j = (c >> l0) - 1 if l == l0 else c >> l
        if l == l0 or not (c >> l) & 1:
            assert j % 2 == 0
            out.append((l, "right" if j + 1 < cnt(c2, l) else "self"))
        else:
            assert j % 2 == 1 and j - 1 == (c >> l) - 1
            out.append((l, "peak"))
    return out


def model_gather(levels, c, stride=STRIDE):
    """(peaks, rights) of the proof that the tree with the level lists `levels` (merkle_model.cpu_levels of its c2 leaves) extends
    what it was at c <= c2 leaves."""
    c2 = int(levels[0].shape[0])
    assert 0 <= c <= c2 and c2.bit_length() <= stride
    peaks, rights = np.zeros((stride, 8), np.uint32), np.zeros((stride, 8), np.uint32)
    if c == 0:
        return peaks, rights
    for l in range(c.bit_length()):
        if (c >> l) & 1:
            peaks[l] = levels[l][(c >> l) - 1]
    l0 = ctz(c)
    for l, what in walk(c, c2):
        if what == "right":
            rights[l] = levels[l][((c >> l0) - 1 if l == l0 else c >> l) + 1]
    return peaks, rights


def model_walk(c, c2, peaks, rights, reads=None):
    """(old root, new root) that the two walks of a checkable pair 1 <= c <= c2 form from the rows alone.  `reads` (a set)
    collects the cells they read as ("peaks" | "rights", l)."""
    reads = set() if reads is None else reads

    def P(l):
        reads.add(("peaks", l))
        return peaks[l]

    def R(l):
        reads.add(("rights", l))
        return rights[l]

    carry = None                                            # the old root: the root of the frontier (c, peaks)
    for l in range(tree_height(c)):
        if (c >> l) & 1:
            p = P(l)
            carry = node(p, p if carry is None else carry)
        elif carry is not None:
            carry = node(carry, carry)
    if carry is None:
        carry = P(tree_height(c))
    acc = P(ctz(c))                                         # the new root: from P_l0 up
    for l, what in walk(c, c2):
        acc = node(acc, R(l)) if what == "right" else node(acc, acc) if what == "self" else node(P(l), acc)
    return np.array(carry, dtype=np.uint32), np.array(acc, dtype=np.uint32)


def model_check(c, c2, peaks, rights, old_root, new_root, reads=None):
    """0 or 1: the check of a holder of old_root (at c leaves) and new_root (at c2 leaves); `reads` as model_walk's."""
    c, c2, stride = int(c), int(c2), int(peaks.shape[0])
    if c > c2 or c2 > MAX_COUNT or c2.bit_length() > stride:
        return 0
    if c == 0:
        return int(not np.asarray(old_root).any())
    old, new = model_walk(c, c2, peaks, rights, reads)
    return int(bool((old == old_root).all()) and bool((new == new_root).all()))


def read_set(c, c2):
    """The cells the check of a checkable pair reads, from the rule alone."""
    if c == 0:
        return set()
    cells = {("peaks", l) for l in range(c.bit_length()) if (c >> l) & 1}
    return cells | {("rights", l) for l, what in walk(c, c2) if what == "right"}


def hashes(c, c2):
    """Node hashes of one check."""
    if c == 0:
        return 0
    low = ctz(c)
    return sum(1 for l in range(tree_height(c)) if l >= low) + len(walk(c, c2))


def built_root(rows):
    """The root of the tree BUILT FROM the leaves `rows` (a list of 32-byte strings, at least one): level by level, on bytes."""
    cur = rows
    while True:
        n = len(cur)
        cur = [hashlib.sha256(hashlib.sha256(cur[2 * p] + cur[min(2 * p + 1, n - 1)]).digest()).digest() for p in range((n + 1) // 2)]
        if len(cur) == 1:
            return np.frombuffer(cur[0], dtype=">u4").astype(np.uint32)


def leaf_rows(leaves):
    return [bytes(r) for r in np.asarray(leaves, dtype=np.uint32).astype(">u4")]


def prefix_roots(leaves):
    """[c2 + 1, 8]: row c the root of the tree built from the first c leaves (row 0: zero); tests/test_consistency_model.py
    anchors it to merkle_model.cpu_levels."""
    rows = leaf_rows(leaves)
    out = np.zeros((len(rows) + 1, 8), np.uint32)
    for c in range(1, len(rows) + 1):
        out[c] = built_root(rows[:c])
    return out


# ---- the shapes ------------------------------------------------------------------------------------------------------------------
class Forest:
    """Trees of `counts` leaves over random digests, `first` cells in front of tree 0: the leaves, the offsets, and per tree --
    computed once, when first asked for -- its level lists and the roots of all of its prefixes."""

    def __init__(self, counts, seed, first=3):
        self.counts, self.ntrees, self.first = [int(c) for c in counts], len(counts), int(first)
        self.offsets = (np.concatenate([[0], np.cumsum(self.counts)]) + first).astype(np.uint64)
        self.leaves = random_leaves(np.random.default_rng(seed), int(self.offsets[-1]))
        self._levels, self._rows, self._old = {}, {}, {}

    def tree(self, t):
        return self.leaves[int(self.offsets[t]): int(self.offsets[t + 1])]

    def levels(self, t):
        if t not in self._levels:
            self._levels[t] = cpu_levels(self.tree(t))
        return self._levels[t]

    def old_root(self, t, c):
        """The root of the tree built from the first c leaves of tree t; computed once."""
        if (t, c) not in self._old:
            if t not in self._rows:
                self._rows[t] = leaf_rows(self.tree(t))
            self._old[t, c] = built_root(self._rows[t][:c]) if c else ZERO
        return self._old[t, c]

    def roots(self):
        return np.stack([self.levels(t)[-1][0] if c else ZERO for t, c in enumerate(self.counts)])

    def proofs(self, trees, old_counts, stride=STRIDE):
        """The model's (new counts, peaks [Q, stride, 8], rights) for the queries."""
        new_counts = np.array([self.counts[t] for t in trees], dtype=np.uint64)
        rows = [model_gather(self.levels(t), int(c), stride) if self.counts[t] else (np.zeros((stride, 8), np.uint32),) * 2 for t, c in zip(trees, old_counts)]
        return new_counts, np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])

    def query_roots(self, trees, old_counts):
        """(old roots, new roots) per query: the trees built from the first c leaves, and the trees as they are."""
        now = self.roots()
        return np.stack([self.old_root(int(t), int(c)) for t, c in zip(trees, old_counts)]), np.stack([now[t] for t in trees])


def every_pair(counts):
    """(trees, old counts): a query for every c in 0..count of every tree."""
    pairs = [(t, c) for t, n in enumerate(counts) for c in range(n + 1)]
    return np.array([t for t, _ in pairs], dtype=np.uint32), np.array([c for _, c in pairs], dtype=np.uint64)


def square_counts(top):
    """A tree of every count 1..top, an empty tree in front of every seventh."""
    out = []
    for n in range(1, top + 1):
        out += [0, n] if n % 7 == 0 else [n]
    return out


@functools.lru_cache(maxsize=None)
def square(top=130):
    return Forest(square_counts(top), seed=401)


GPU_COUNTS = [0, 1, 2, 3, 4, 5, 8, 63, 64, 65, 127, 128, 129, 0, 1024, 2047, 2048]


def gpu_queries(counts=GPU_COUNTS, seed=402):
    """Every c for the trees up to 129 leaves; 0, 1, count - 1, count, 2^k and 2^k +- 1 for the larger ones; shuffled."""
    pairs = []
    for t, n in enumerate(counts):
        if n <= 129:
            pairs += [(t, c) for c in range(n + 1)]
        else:
            cs = {0, 1, n - 1, n} | {(1 << k) + d for k in range(n.bit_length()) for d in (-1, 0, 1)}
            pairs += [(t, c) for c in sorted(cs) if 0 <= c <= n]
    order = np.random.default_rng(seed).permutation(len(pairs))
    return np.array([pairs[i][0] for i in order], dtype=np.uint32), np.array([pairs[i][1] for i in order], dtype=np.uint64)


# The refusals of the gather, each alone, over a forest of counts [5, 0, 9, 129]: (what, the status word, trees, old counts,
# stride, max_count as the call is told it).  Bit 2 needs a caller that understates max_count: the host refuses a stride below
# the bits of the max_count it is given.
REFUSAL_COUNTS = [5, 0, 9, 129]
REFUSALS = [
    ("a tree index >= ntrees", 1, [0, 4, 2], [3, 0, 9], 8, 129),
    ("an old count above the count", 2, [0, 2, 3], [5, 10, 7], 8, 129),
    ("an old count above an empty tree", 2, [1], [1], 8, 129),
    ("a count of more bits than stride", 4, [0, 3], [2, 100], 7, 100),
    ("all three", 7, [7, 0, 3], [0, 6, 1], 7, 100),
]


# ---- the CPU twins (libvkmr_host.so) ---------------------------------------------------------------------------------------------
def host_gather(leaves, offsets, trees, old_counts, stride=STRIDE):
    """(status, new counts, peaks [Q, stride, 8], rights) of vkmr_host_cpu_forest_consistency; the outputs start as the canary."""
    import vk_merkle_roots_amd as vk
    leaves = np.ascontiguousarray(leaves, dtype=np.uint32).reshape(-1, 8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    trees, old_counts = np.ascontiguousarray(trees, dtype=np.uint32), np.ascontiguousarray(old_counts, dtype=np.uint64)
    Q = int(trees.shape[0])
    new_counts = np.full(Q, COUNT_FILL, np.uint64)
    peaks, rights = np.full((Q, stride, 8), CANARY, np.uint32), np.full((Q, stride, 8), CANARY, np.uint32)
    status = vk.host_lib().vkmr_host_cpu_forest_consistency(leaves.ctypes.data if leaves.size else None, offsets.ctypes.data, int(offsets.shape[0]) - 1,
                                                            trees.ctypes.data, old_counts.ctypes.data, Q, stride, new_counts.ctypes.data,
                                                            peaks.ctypes.data, rights.ctypes.data)
    return status, new_counts, peaks, rights


def host_verify(old_counts, new_counts, peaks, rights, old_roots, new_roots):
    """ok uint32 [Q] of vkmr_host_cpu_verify_consistency; starts as the canary."""
    import vk_merkle_roots_amd as vk
    old_counts, new_counts = np.ascontiguousarray(old_counts, dtype=np.uint64), np.ascontiguousarray(new_counts, dtype=np.uint64)
    peaks, rights = np.ascontiguousarray(peaks, dtype=np.uint32), np.ascontiguousarray(rights, dtype=np.uint32)
    old_roots, new_roots = np.ascontiguousarray(old_roots, dtype=np.uint32), np.ascontiguousarray(new_roots, dtype=np.uint32)
    Q, stride = int(old_counts.shape[0]), int(peaks.shape[1])
    assert peaks.shape == rights.shape == (Q, stride, 8) and old_roots.shape == new_roots.shape == (Q, 8) and new_counts.shape == (Q,)
    ok = np.full(Q, CANARY, np.uint32)
    rc = vk.host_lib().vkmr_host_cpu_verify_consistency(old_counts.ctypes.data, new_counts.ctypes.data, peaks.ctypes.data, rights.ctypes.data, stride, Q,
                                                        old_roots.ctypes.data, new_roots.ctypes.data, ok.ctypes.data)
    assert rc == 0
    return ok


# ---- the read set: one flipped bit per cell ----------------------------------------------------------------------------------------
class Flips:
    """For every pair 1 <= c <= c2 <= top over one tree per c2 (prefixes of one leaf list): the honest proof, and one copy of it
    per cell of both rows up to `stride` with one bit of that cell flipped; `want` says what the model answers for each (0 for
    a cell the rule reads, 1 for every other), batched as one verify call."""

    def __init__(self, top, seed, stride=None):
        stride = top.bit_length() if stride is None else stride
        rng = np.random.default_rng(seed)
        leaves = random_leaves(rng, top)
        roots = prefix_roots(leaves)
        rows = []                                   # (c, c2, peaks, rights, want, what)
        for c2 in range(1, top + 1):
            levels = cpu_levels(leaves[:c2])
            assert (levels[-1][0] == roots[c2]).all()
            for c in range(1, c2 + 1):
                peaks, rights = model_gather(levels, c, stride)
                rows.append((c, c2, peaks, rights, 1, None))
                cells = read_set(c, c2)
                for row in ("peaks", "rights"):
                    for l in range(stride):
                        flipped = [peaks.copy(), rights.copy()]
                        flipped[row == "rights"][l, int(rng.integers(0, 8))] ^= np.uint32(1 << int(rng.integers(0, 32)))
                        rows.append((c, c2, flipped[0], flipped[1], 0 if (row, l) in cells else 1, (row, l)))
        self.rows, self.stride = rows, stride
        self.old_counts = np.array([r[0] for r in rows], dtype=np.uint64)
        self.new_counts = np.array([r[1] for r in rows], dtype=np.uint64)
        self.peaks, self.rights = np.stack([r[2] for r in rows]), np.stack([r[3] for r in rows])
        self.want = np.array([r[4] for r in rows], dtype=np.uint32)
        self.old_roots, self.new_roots = roots[self.old_counts.astype(np.int64)], roots[self.new_counts.astype(np.int64)]


@functools.lru_cache(maxsize=None)
def flips(top):
    return Flips(top, seed=403 + top)


# ---- the replay ------------------------------------------------------------------------------------------------------------------
def build_consistency_plan_exe(directory, sanitize=True):
    """tests/c/consistency_plan_test.cpp as a program of its own, by default with AddressSanitizer and UBSan."""
    if not sanitize:
        return build_plan_exe(directory, "consistency_plan_test")
    exe = os.path.join(str(directory), "consistency_plan_test_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "vk_merkle_roots_amd", "csrc"), os.path.join(ROOT, "tests", "c", "consistency_plan_test.cpp"), "-o", exe])
    return exe


def plan_replay(exe, directory, cases):
    """One line per (first_offset, stride, counts, [(tree, old count), ..]) through tests/c/consistency_plan_test.cpp: per case
    (cells read, node hashes, status); the C test has checked sources, bounds, trees and the hash bound on the way."""
    path = os.path.join(str(directory), "consistency_cases.txt")
    with open(path, "w") as f:
        for first, stride, counts, queries in cases:
            words = [first, stride, len(counts)] + list(counts) + [len(queries)] + [v for q in queries for v in q]
            f.write(" ".join(str(int(x)) for x in words) + "\n")
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    text = r.stdout.decode()
    assert r.returncode == 0 and "FAIL" not in text and f"ok: {len(cases)} cases" in text, text[-2000:]
    return [tuple(int(x) for x in line.split()) for line in text.splitlines()[: len(cases)]]
