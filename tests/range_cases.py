"""Range proofs over sorted trees (vkmr_hip_forest_range_async, vkmr_hip_verify_forest_range_async, vk.RangeProofs,
MerkleForest.ranges): the rule restated with hashlib (merkle_model), Python's tuple compare and bisect, independent of
csrc/range_plan.hpp -- the run a closed interval carries, the cells of its two rows and the verdict of its check --, ONE forest with
its queries, the verifier's negatives, the drivers of the CPU twins and of the replay (tests/c/range_plan_test.cpp), shared by
tests/test_range_abi.py (no GPU) and tests/test_gpu_range.py.  A plain module: no fixtures, no GPU.

A query is (t, lo, hi), closed on both sides.  i0 = leaves below lo, i1 = leaves at or below hi; the run is leaves [a, b] with
a = max(i0 - 1, 0), b = min(i1, c - 1): the leaves in range and the neighbour on either side, where there is one."""
import bisect
import functools
import os
import subprocess

import numpy as np

from absence_cases import CANARY, INDEX_FILL, NONE, ONES, ZERO, as_int, from_int, height, key, sorted_rows
from merkle_model import ROOT, cpu_levels, node, random_leaves

COUNTS = [0, 1, 2, 3, 5, 8, 9, 64, 65, 257, 0, 1000, 2500]
STRIDE = 12                                             # H(2500)
SMALL = 9                                               # trees up to this many leaves get every pair of gaps as bounds


# ---- the rule ----------------------------------------------------------------------------------------------------------------------
def model_run(leaves, lo, hi):
    """(first, m, leaves in range) for a tree that is there and hi >= lo."""
    keys = [key(r) for r in leaves]
    c = len(keys)
    if c == 0:
        return 0, 0, 0
    i0, i1 = bisect.bisect_left(keys, key(lo)), bisect.bisect_right(keys, key(hi))
    a, b = max(i0 - 1, 0), min(i1, c - 1)
    return a, b - a + 1, i1 - i0


def model_rows(levels, a, b, c, stride):
    """(left [stride, 8], right): the node in front of the run's first at every level where that one is a right child, the node
    behind its last where that one is a left child and has a sibling; zero otherwise."""
    left, right = np.zeros((stride, 8), np.uint32), np.zeros((stride, 8), np.uint32)
    for l in range(height(c)):
        if (a >> l) & 1:
            left[l] = levels[l][(a >> l) - 1]
        if not (b >> l) & 1 and (b >> l) + 1 < len(levels[l]):
            right[l] = levels[l][(b >> l) + 1]
    return left, right


def model_verdict(t, ntrees, lo, hi, first, run, left, right, h, root, c, reads=None):
    """(verdict, in_first, in_count) with hashlib; `reads` (a set) collects the row cells read as ("left" | "right", l)."""
    reads = set() if reads is None else reads
    no = (0, 0, 0)
    a, m, c, h = int(first), len(run), int(c), int(h)
    if t >= ntrees or h != height(c) or h > left.shape[0] or c > 1 << 58 or a + m > c or key(hi) < key(lo) or (m == 0 and c > 0):
        return no
    if c == 0:
        return (1, 0, 0) if not np.asarray(root).any() else no
    keys = [key(r) for r in run]
    if any(not keys[j - 1] < keys[j] for j in range(1, m)):
        return no
    b = a + m - 1
    below, above = keys[0] < key(lo), keys[-1] > key(hi)
    if not (below or a == 0) or not (above or b == c - 1):
        return no
    if m >= 2 and ((below and keys[1] < key(lo)) or (above and keys[-2] > key(hi))):
        return no
    have = {a + j: run[j] for j in range(m)}             # node index -> value, level by level
    for l in range(h):
        n = ((c - 1) >> l) + 1
        al, bl = a >> l, b >> l
        up = {}
        for p in range(al >> 1, (bl >> 1) + 1):
            if 2 * p < al:
                reads.add(("left", l))
                x = left[l]
            else:
                x = have[2 * p]
            if 2 * p + 1 <= bl:
                y = have[2 * p + 1]
            elif 2 * p + 1 < n:
                reads.add(("right", l))
                y = right[l]
            else:
                y = x
            up[p] = node(x, y)
        have = up
    if key(have[0]) != key(root):
        return no
    return 1, a + int(below), m - int(below) - int(above)


# ---- the forest ---------------------------------------------------------------------------------------------------------------------
class Forest:
    """COUNTS trees of random digests sorted per tree, with the crafted leaves: in the tree of 64 two leaves equal in words 0..6; in
    the tree of 65 the neighbours 0x7FFFFFFF FFFFFFFF.. / 0x80000000 00000000..; in the tree of 257 the all-zero and the all-ones
    digest as first and last leaf."""

    def __init__(self, seed=701):
        rng = np.random.default_rng(seed)
        self.counts, self.ntrees = list(COUNTS), len(COUNTS)
        trees = [random_leaves(rng, c) for c in COUNTS]
        trees[7][1] = trees[7][0]
        trees[7][0][7], trees[7][1][7] = 5, 6
        self.word7 = (trees[7][0].copy(), trees[7][1].copy())
        trees[8][0] = np.array([0x7FFFFFFF] + [0xFFFFFFFF] * 7, dtype=np.uint32)
        trees[8][1] = np.array([0x80000000] + [0] * 7, dtype=np.uint32)
        trees[9][0], trees[9][1] = ZERO, ONES
        self.trees = [sorted_rows(t) if len(t) else np.zeros((0, 8), np.uint32) for t in trees]
        for t in self.trees:
            keys = [key(r) for r in t]
            assert all(keys[i - 1] < keys[i] for i in range(1, len(keys)))
        self.total = sum(COUNTS)
        self.offsets0 = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.uint64)
        self.levels = [cpu_levels(t) if len(t) else None for t in self.trees]
        self.roots = np.stack([lv[-1][0] if lv else ZERO for lv in self.levels])
        self.filler = random_leaves(rng, 137)

    def placed(self, first=0, slack=0):
        """(cells [first + total + slack, 8], offsets uint64 [ntrees + 1]): the leaves laid at cell `first`."""
        body = np.concatenate(self.trees)
        cells = np.concatenate([self.filler[:first], body, self.filler[37: 37 + slack]]) if first or slack else body
        return np.ascontiguousarray(cells), self.offsets0 + np.uint64(first)

    def gap(self, t, g):
        """A digest strictly between leaf g - 1 and leaf g of tree t (below the first: g == 0, above the last: g == c), or None
        where there is none."""
        leaves = self.trees[t]
        lo = as_int(leaves[g - 1]) if g > 0 else -1
        hi = as_int(leaves[g]) if g < len(leaves) else 1 << 256
        return from_int(lo + (hi - lo) // 2) if hi - lo >= 2 else None

    @functools.lru_cache(maxsize=None)
    def queries(self):
        """(what [Q], trees uint32 [Q], lo [Q, 8], hi [Q, 8]), shuffled."""
        rng = np.random.default_rng(702)
        out = []
        for t, leaves in enumerate(self.trees):
            c = len(leaves)
            out += [("whole", t, ZERO, ONES), ("hi < lo", t, ONES, ZERO)]
            if c == 0:
                x = random_leaves(rng, 1)[0]
                out.append(("empty tree, lo == hi", t, x, x))
            elif c <= SMALL:
                gaps = [self.gap(t, g) for g in range(c + 1)]
                for g1 in range(c + 1):
                    for g2 in range(g1, c + 1):
                        if gaps[g1] is not None and gaps[g2] is not None:
                            out.append((f"gaps {g1}..{g2}", t, gaps[g1], gaps[g2]))
                for i in range(c):
                    out.append(("lo == hi on a leaf", t, leaves[i], leaves[i]))
            else:
                mid = c // 2
                for what, lo, hi in (("empty below leaf 0", self.gap(t, 0), self.gap(t, 0)), ("empty in a gap", self.gap(t, mid), self.gap(t, mid)),
                                     ("empty above the last", self.gap(t, c), self.gap(t, c)), ("lo == hi on a leaf", leaves[mid], leaves[mid]),
                                     ("lo a leaf", leaves[mid - 3], self.gap(t, mid + 2)), ("hi a leaf", self.gap(t, mid - 3), leaves[mid + 2]),
                                     ("both ends leaves", leaves[1], leaves[c - 2]), ("to the odd edge", self.gap(t, c - 5), ONES),
                                     ("from the start", ZERO, self.gap(t, 6)), ("first leaf alone", leaves[0], leaves[0]),
                                     ("last leaf alone", leaves[c - 1], leaves[c - 1])):
                    if lo is not None and hi is not None:
                        out.append((what, t, lo, hi))
        big = self.trees[12]
        for n in (255, 256, 257, 1025):
            for s in (10, 11):
                out.append((f"{n} leaves from {s}", 12, big[s], big[s + n - 1]))
        out.append(("word 7 decides", 7, self.word7[0], self.word7[0]))
        out.append(("word 7 decides, both", 7, self.word7[0], self.word7[1]))
        low, high = np.array([0x7FFFFFFF] + [0xFFFFFFFF] * 7, dtype=np.uint32), np.array([0x80000000] + [0] * 7, dtype=np.uint32)
        out += [("0x7FFF.. alone", 8, low, low), ("0x8000.. alone", 8, high, high), ("0x7FFF.. to 0x8000..", 8, low, high)]
        x, y = self.gap(11, 300), self.gap(11, 340)
        out += [("same bounds, tree 11", 11, x, y), ("same bounds, tree 12", 12, x, y), ("same bounds, tree 9", 9, x, y)]
        for t in (self.ntrees, self.ntrees + 5, 0xFFFFFFFF):
            out.append(("no such tree", t, ZERO, ONES))
        order = rng.permutation(len(out))
        return ([out[j][0] for j in order], np.array([out[j][1] for j in order], dtype=np.uint32), np.stack([out[j][2] for j in order]).astype(np.uint32),
                np.stack([out[j][3] for j in order]).astype(np.uint32))

    @functools.lru_cache(maxsize=None)
    def expected(self, stride=STRIDE):
        """What the model gives for queries(): (firsts, leaf_starts, leaves, left, right, heights, info, verdict, in_first, in_count)."""
        _, trees, lo, hi = self.queries()
        Q = len(trees)
        firsts, heights = np.zeros(Q, np.uint64), np.zeros(Q, np.uint32)
        starts, runs = np.zeros(Q + 1, np.uint64), []
        left, right = np.zeros((Q, stride, 8), np.uint32), np.zeros((Q, stride, 8), np.uint32)
        verdict, in_first, in_count = np.zeros(Q, np.uint32), np.zeros(Q, np.uint64), np.zeros(Q, np.uint64)
        refused = inside = 0
        seen = set()
        for q, t in enumerate(trees.tolist()):
            run = np.zeros((0, 8), np.uint32)
            if t >= self.ntrees or key(hi[q]) < key(lo[q]):
                firsts[q] = NONE
                refused += 1
            else:
                leaves, c = self.trees[t], len(self.trees[t])
                a, m, n = model_run(leaves, lo[q], hi[q])
                firsts[q], heights[q] = a, height(c)
                inside += n
                if m:
                    run = leaves[a: a + m]
                    left[q], right[q] = model_rows(self.levels[t], a, a + m - 1, c, stride)
                    seen.add((c, a, a + m - 1))
                verdict[q], in_first[q], in_count[q] = model_verdict(t, self.ntrees, lo[q], hi[q], a, run, left[q], right[q], heights[q], self.roots[t], c)
                assert verdict[q] == 1 and in_count[q] == n, (q, t)
                assert n == 0 or key(leaves[int(in_first[q])]) >= key(lo[q])
            runs.append(run)
            starts[q + 1] = starts[q] + np.uint64(len(run))
        for c in (1, 2, 3, 5, 8, 9):                     # every run a small tree can carry occurs: any a < b, and a fence alone at either end
            assert all((c, a, b) in seen for a in range(c) for b in range(a + 1, c)) and (c, 0, 0) in seen and (c, c - 1, c - 1) in seen, c
        info = np.array([0, int(starts[Q]), refused, inside], dtype=np.uint64)
        return firsts, starts, np.concatenate(runs), left, right, heights, info, verdict, in_first, in_count


@functools.lru_cache(maxsize=None)
def forest():
    return Forest()


# ---- the verifier's negatives --------------------------------------------------------------------------------------------------------
def honest(t, a, b, lo, hi, stride=STRIDE):
    """The proof that carries leaves [a, b] of tree t for (lo, hi), rows gathered honestly for that run, as a dict."""
    f = forest()
    c = len(f.trees[t])
    left, right = model_rows(f.levels[t], a, b, c, stride)
    return {"t": t, "lo": lo, "hi": hi, "first": a, "leaves": f.trees[t][a: b + 1].copy(), "left": left, "right": right, "h": height(c), "root": f.roots[t], "c": c}


def negatives(stride=STRIDE):
    """[(what, want, proof)]: honest proofs (want 1), each bent copy (want 0), and the bent copies that stay 1."""
    f = forest()
    out = []

    def bent(p, **changes):
        q = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in p.items()}
        q.update(changes)
        return q

    t = 12
    lo, hi = f.gap(t, 100), f.gap(t, 141)                # leaves 100 .. 140 are in range; 99 and 141 fence them
    p = honest(t, 99, 141, lo, hi)
    out.append(("honest, mid-tree", 1, p))
    out.append(("an in-range leaf left out of the middle", 0, bent(p, leaves=np.delete(p["leaves"], 20, axis=0))))
    out.append(("the last in-range leaf left out, right row regathered", 0, honest(t, 99, 139, lo, hi)))
    out.append(("the first in-range leaf left out, left row regathered", 0, honest(t, 101, 141, lo, hi)))
    altered = p["leaves"].copy()
    altered[7, 7] ^= np.uint32(1)
    out.append(("one leaf altered", 0, bent(p, leaves=altered)))
    swapped = p["leaves"].copy()
    swapped[[11, 12]] = swapped[[12, 11]]
    out.append(("two leaves swapped", 0, bent(p, leaves=swapped)))
    reads = set()
    assert model_verdict(t, f.ntrees, lo, hi, 99, p["leaves"], p["left"], p["right"], p["h"], p["root"], p["c"], reads)[0] == 1
    for row in ("left", "right"):
        l = min(l for r, l in reads if r == row)
        cells = p[row].copy()
        cells[l, 2] ^= np.uint32(1 << 20)
        out.append((f"a read cell of the {row} row altered", 0, bent(p, **{row: cells})))
        for l in range(stride):
            if (row, l) not in reads:
                cells = p[row].copy()
                cells[l] = 0xDEADBEEF
                out.append((f"{row}[{l}], never read, altered", 1, bent(p, **{row: cells})))
    out.append(("first moved by +1", 0, bent(p, first=100)))
    out.append(("first moved by -1", 0, bent(p, first=98)))
    out.append(("a wrong height", 0, bent(p, h=p["h"] + 1)))
    out.append(("a height below", 0, bent(p, h=p["h"] - 1)))
    out.append(("an extra out-of-range leaf in front", 0, honest(t, 98, 141, lo, hi)))
    out.append(("an extra out-of-range leaf behind", 0, honest(t, 99, 142, lo, hi)))
    out.append(("a root of another tree", 0, bent(p, root=f.roots[11])))
    out.append(("hi < lo", 0, bent(p, lo=hi, hi=lo)))
    t = 8                                                # 65 leaves: the last level-0 node has no sibling
    lo = f.gap(t, 40)
    e = honest(t, 39, 64, lo, ONES)
    out.append(("honest, to the odd edge", 1, e))
    out.append(("a count of c + 1", 0, bent(e, c=66)))
    out.append(("a count of c - 1", 0, bent(e, c=64)))
    for l in range(e["h"], stride):
        left, right = e["left"].copy(), e["right"].copy()
        left[l] = right[l] = 0xDEADBEEF
        out.append((f"both rows at level {l}, at or above H, altered", 1, bent(e, left=left, right=right)))
    out.append(("the last leaf left out at the edge", 0, honest(t, 39, 63, lo, ONES)))
    return out


def batch(proofs, stride=STRIDE):
    """Proof dicts as the arrays of one verify call over a table of one root and one count per PROOF (tree q of Q): (trees, lo, hi,
    firsts, leaf_starts, leaves, left, right, heights, roots, counts)."""
    Q = len(proofs)
    col = lambda k, dtype, *shape: np.array([p[k] for p in proofs], dtype=dtype).reshape(Q, *shape)
    starts = np.concatenate([[0], np.cumsum([len(p["leaves"]) for p in proofs])]).astype(np.uint64)
    return (np.arange(Q, dtype=np.uint32), col("lo", np.uint32, 8), col("hi", np.uint32, 8), col("first", np.uint64), starts,
            np.concatenate([p["leaves"] for p in proofs]).astype(np.uint32), col("left", np.uint32, stride, 8), col("right", np.uint32, stride, 8),
            col("h", np.uint32), col("root", np.uint32, 8), col("c", np.uint64))


# ---- the CPU twins (libvkmr_host.so) -------------------------------------------------------------------------------------------------
def _ptr(a):
    return a.ctypes.data if a.size else None


def host_range(cells, offsets, trees, lo, hi, stride=STRIDE, capacity=None, guard=3):
    """(rc, firsts, leaf_starts, leaves [capacity + guard, 8], left, right, heights, info) of vkmr_host_cpu_forest_range; the outputs
    start as the canary.  capacity None: a counting call first, as MerkleForest.ranges does."""
    import vk_merkle_roots_amd as vk
    cells, offsets = np.ascontiguousarray(cells, dtype=np.uint32).reshape(-1, 8), np.ascontiguousarray(offsets, dtype=np.uint64)
    trees, lo, hi = np.ascontiguousarray(trees, dtype=np.uint32), np.ascontiguousarray(lo, dtype=np.uint32), np.ascontiguousarray(hi, dtype=np.uint32)
    Q = int(trees.shape[0])
    if capacity is None:
        counted = host_range(cells, offsets, trees, lo, hi, stride, 0)
        if counted[0] != 0:
            return counted
        capacity = int(counted[7][1])
    firsts, starts, heights, info = np.full(Q, INDEX_FILL, np.uint64), np.full(Q + 1, INDEX_FILL, np.uint64), np.full(Q, CANARY, np.uint32), np.full(4, INDEX_FILL, np.uint64)
    leaves = np.full((capacity + guard, 8), CANARY, np.uint32)
    left, right = np.full((Q, stride, 8), CANARY, np.uint32), np.full((Q, stride, 8), CANARY, np.uint32)
    rc = vk.host_lib().vkmr_host_cpu_forest_range(_ptr(cells), int(cells.shape[0]), offsets.ctypes.data, int(offsets.shape[0]) - 1, trees.ctypes.data,
                                                  lo.ctypes.data, hi.ctypes.data, Q, stride, firsts.ctypes.data, starts.ctypes.data, leaves.ctypes.data, capacity,
                                                  left.ctypes.data, right.ctypes.data, heights.ctypes.data, info.ctypes.data)
    return rc, firsts, starts, leaves, left, right, heights, info


def host_verify(trees, lo, hi, firsts, starts, leaves, left, right, heights, roots, counts):
    """(verdict, in_first, in_count) of vkmr_host_cpu_verify_range; they start as the canary."""
    import vk_merkle_roots_amd as vk
    trees, heights = np.ascontiguousarray(trees, dtype=np.uint32), np.ascontiguousarray(heights, dtype=np.uint32)
    lo, hi, leaves = (np.ascontiguousarray(x, dtype=np.uint32).reshape(-1, 8) for x in (lo, hi, leaves))
    firsts, starts = np.ascontiguousarray(firsts, dtype=np.uint64), np.ascontiguousarray(starts, dtype=np.uint64)
    left, right = np.ascontiguousarray(left, dtype=np.uint32), np.ascontiguousarray(right, dtype=np.uint32)
    roots, counts = np.ascontiguousarray(roots, dtype=np.uint32).reshape(-1, 8), np.ascontiguousarray(counts, dtype=np.uint64)
    Q = int(trees.shape[0])
    assert left.shape == right.shape == (Q, left.shape[1], 8) and roots.shape[0] == counts.shape[0] and starts.shape[0] == Q + 1
    verdict, in_first, in_count = np.full(Q, CANARY, np.uint32), np.full(Q, INDEX_FILL, np.uint64), np.full(Q, INDEX_FILL, np.uint64)
    rc = vk.host_lib().vkmr_host_cpu_verify_range(trees.ctypes.data, lo.ctypes.data, hi.ctypes.data, firsts.ctypes.data, starts.ctypes.data, _ptr(leaves),
                                                  int(leaves.shape[0]), left.ctypes.data, right.ctypes.data, heights.ctypes.data, Q, int(left.shape[1]),
                                                  _ptr(roots), _ptr(counts), int(roots.shape[0]), verdict.ctypes.data, in_first.ctypes.data,
                                                  in_count.ctypes.data)
    assert rc == 0
    return verdict, in_first, in_count


# ---- the replay ------------------------------------------------------------------------------------------------------------------------
def build_range_plan_exe(directory):
    """tests/c/range_plan_test.cpp as a program of its own, with AddressSanitizer and UBSan."""
    exe = os.path.join(str(directory), "range_plan_test_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "vk_merkle_roots_amd", "csrc"), os.path.join(ROOT, "tests", "c", "range_plan_test.cpp"), "-o", exe])
    return exe
