"""Sorted trees (vkmr_hip_forest_sorted_async, vkmr_hip_forest_lower_bound_async, vkmr_hip_forest_absence_async,
vkmr_hip_verify_forest_absence_async, vk.AbsenceProofs, MerkleForest.absence): the rules restated with hashlib
(merkle_model) and Python's tuple compare -- the order, the first pair out of order, the lower bound's loop, the cells of an
absence proof and the verdict of its check --, ONE forest with its queries, the drivers of the CPU twins and of the replay
(tests/c/absence_plan_test.cpp), shared by tests/test_absence_abi.py (no GPU) and tests/test_gpu_absence.py.  A plain module: no
fixtures, no GPU.

A digest is eight uint32 words; a < b is the compare of the tuples of their words, word 0 first, every word unsigned.  A proof
of (tree t of c leaves, x) with i the lower bound: index i; pred = leaf i - 1, succ = leaf i (zero where there is none); main,
the inclusion proof of the anchor (leaf i, or leaf c - 1 for i == c); low, for 0 < i < c, the siblings of leaf i - 1 below
top = ctz(i), zero from there up."""
import functools
import os
import subprocess

import numpy as np

from merkle_model import ROOT, cpu_levels, node, proof_path, random_leaves, tree_height

NONE = 0xFFFFFFFFFFFFFFFF
CANARY = 0xA5A5A5A5
INDEX_FILL = 0xA5A5A5A5A5A5A5A5
ZERO = np.zeros(8, np.uint32)
ONES = np.full(8, 0xFFFFFFFF, np.uint32)
NOT_PROVEN, ABSENT, PRESENT = 0, 1, 2
COUNTS = [1, 2, 3, 0, 4, 5, 7, 8, 9, 0, 63, 64, 65, 130]
STRIDE = 8                                              # H(130)


def key(d):
    """A digest as what Python compares: the tuple of its words."""
    return tuple(int(w) for w in np.asarray(d).reshape(8))


def as_int(d):
    """The digest as one 256-bit number, word 0 the most significant: the same order."""
    n = 0
    for w in key(d):
        n = (n << 32) | w
    return n


def from_int(n):
    return np.array([(n >> (32 * (7 - w))) & 0xFFFFFFFF for w in range(8)], dtype=np.uint32)


def height(c):
    return tree_height(c) if c else 0


def ctz(i):
    return (i & -i).bit_length() - 1


def model_first_bad(leaves):
    """The lowest i >= 1 with not leaf[i-1] < leaf[i], or NONE; and whether that pair is equal."""
    keys = [key(r) for r in leaves]
    for i in range(1, len(keys)):
        if not keys[i - 1] < keys[i]:
            return i, keys[i - 1] == keys[i]
    return NONE, False


def model_lower_bound(leaves, x):
    """The rule's loop, on whatever leaves: (i, found)."""
    keys, kx = [key(r) for r in leaves], key(x)
    lo, hi = 0, len(keys)
    while lo < hi:
        mid = lo + (hi - lo) // 2
        if keys[mid] < kx:
            lo = mid + 1
        else:
            hi = mid
    return lo, lo < len(keys) and keys[lo] == kx


def model_proof(leaves, levels, x, stride):
    """(index, pred, succ, main [stride, 8], low, height) of the proof of x in the tree with `leaves` and its level lists."""
    c = len(leaves)
    main, low = np.zeros((stride, 8), np.uint32), np.zeros((stride, 8), np.uint32)
    if c == 0:
        return 0, ZERO, ZERO, main, low, 0
    i, _ = model_lower_bound(leaves, x)
    h = height(c)
    main[:h] = proof_path(levels, i if i < c else c - 1, h)
    if 0 < i < c:
        top = ctz(i)
        low[:top] = proof_path(levels, i - 1, h)[:top]
    return i, (leaves[i - 1] if i > 0 else ZERO), (leaves[i] if i < c else ZERO), main, low, h


def model_verdict(x, t, ntrees, index, pred, succ, main, low, h, root, c, reads=None):
    """The nine checks with hashlib; `reads` (a set) collects the cells read as ("main" | "low", l)."""
    reads = set() if reads is None else reads
    index, c, h = int(index), int(c), int(h)
    if t >= ntrees or h != height(c) or h > main.shape[0] or index > c:
        return NOT_PROVEN
    if c == 0:
        return ABSENT if not np.asarray(root).any() else NOT_PROVEN
    present = index < c and key(x) == key(succ)
    if not present:
        if index > 0 and not key(pred) < key(x):
            return NOT_PROVEN
        if index < c and not key(x) < key(succ):
            return NOT_PROVEN
        if 0 < index < c:
            top, cur = ctz(index), pred
            for l in range(top):
                reads.add(("low", l))
                cur = node(low[l], cur)
            if key(cur) != key(main[top]):
                return NOT_PROVEN
    a, cur = (index if index < c else c - 1), (succ if index < c else pred)
    for l in range(h):
        reads.add(("main", l))
        cur = node(main[l], cur) if (a >> l) & 1 else node(cur, main[l])
    if key(cur) != key(root):
        return NOT_PROVEN
    return PRESENT if present else ABSENT


# ---- the forest -------------------------------------------------------------------------------------------------------------------
def sorted_rows(rows):
    return np.array(sorted((key(r) for r in rows)), dtype=np.uint32).reshape(-1, 8)


class Forest:
    """COUNTS trees of random digests sorted per tree, with the crafted leaves: in the tree of 9 a run of three equal in words 0..6;
    in the tree of 7 the neighbours 0x7FFFFFFF FFFFFFFF.. / 0x80000000 00000000..; in the tree of 8 the all-zero and the all-ones
    digest as first and last leaf.  `first` cells lie in front of tree 0 and `slack` behind the last tree; they hold digests that
    are out of order with everything, and belong to no tree."""

    def __init__(self, seed=601):
        rng = np.random.default_rng(seed)
        self.counts, self.ntrees = list(COUNTS), len(COUNTS)
        trees = [random_leaves(rng, c) for c in COUNTS]
        run = random_leaves(rng, 1)[0]
        for j, w7 in enumerate((5, 6, 9)):
            trees[8][j] = run
            trees[8][j][7] = w7
        self.run = [trees[8][j].copy() for j in range(3)]
        trees[6][0] = np.array([0x7FFFFFFF] + [0xFFFFFFFF] * 7, dtype=np.uint32)
        trees[6][1] = np.array([0x80000000] + [0] * 7, dtype=np.uint32)
        trees[7][0], trees[7][1] = ZERO, ONES
        self.trees = [sorted_rows(t) if len(t) else np.zeros((0, 8), np.uint32) for t in trees]
        for t in self.trees:
            assert model_first_bad(t)[0] == NONE
        assert key(self.trees[7][0]) == key(ZERO) and key(self.trees[7][-1]) == key(ONES)
        self.offsets0 = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.uint64)
        self.levels = [cpu_levels(t) if len(t) else None for t in self.trees]
        self.roots = np.stack([lv[-1][0] if lv else ZERO for lv in self.levels])
        self.filler = random_leaves(rng, 16)

    def placed(self, first=0, slack=0):
        """(cells [first + total + slack, 8], offsets uint64 [ntrees + 1]): the leaves laid at cell `first`."""
        body = np.concatenate(self.trees)
        cells = np.concatenate([self.filler[:first][::-1], body, self.filler[8: 8 + slack]]) if first or slack else body
        return np.ascontiguousarray(cells), self.offsets0 + np.uint64(first)

    def tree_of(self, rows):
        """The same counts over other leaves (for the unsorted cases): a list of per-tree arrays."""
        at, out = 0, []
        for c in self.counts:
            out.append(rows[at: at + c])
            at += c
        return out

    @functools.lru_cache(maxsize=None)
    def queries(self):
        """(trees uint32 [Q], digests [Q, 8]): per tree every leaf; every gap (below the first, between neighbours, above the
        last) by the digest halfway, and by pred with word 7 + 1 where that is still below succ; succ but for word 0 and succ but
        for word 7, one up and one down; the all-zero and the all-ones digest; for the empty trees those two and a random one;
        the same three for two trees outside the forest."""
        rng = np.random.default_rng(602)
        out = []
        for t, leaves in enumerate(self.trees):
            c = len(leaves)
            out += [(t, ZERO), (t, ONES), (t, random_leaves(rng, 1)[0])]
            ints = [as_int(r) for r in leaves]
            for i in range(c):
                out.append((t, leaves[i]))
                for w in (0, 7):
                    for d in (-1, 1):
                        near = leaves[i].copy()
                        near[w] = np.uint32((int(near[w]) + d) & 0xFFFFFFFF)
                        out.append((t, near))
            bounds = [-1] + ints + [1 << 256]
            for i in range(c + 1):
                lo, hi = bounds[i], bounds[i + 1]
                if hi - lo >= 2:
                    out.append((t, from_int(lo + (hi - lo) // 2)))
                if i > 0 and int(leaves[i - 1][7]) != 0xFFFFFFFF and lo + 1 < hi:
                    out.append((t, from_int(lo + 1)))
        for t in (self.ntrees, self.ntrees + 5, 0xFFFFFFFF):
            out += [(t, ZERO), (t, ONES), (t, random_leaves(rng, 1)[0])]
        order = rng.permutation(len(out))
        return np.array([out[j][0] for j in order], dtype=np.uint32), np.stack([out[j][1] for j in order]).astype(np.uint32)

    @functools.lru_cache(maxsize=None)
    def expected(self, stride=STRIDE):
        """What the model gives for queries(): (indices, found, pred, succ, main, low, heights, verdicts)."""
        trees, digests = self.queries()
        Q = len(trees)
        idx, found, heights, verdicts = np.full(Q, NONE, np.uint64), np.zeros(Q, np.uint32), np.zeros(Q, np.uint32), np.zeros(Q, np.uint32)
        pred, succ = np.zeros((Q, 8), np.uint32), np.zeros((Q, 8), np.uint32)
        main, low = np.zeros((Q, stride, 8), np.uint32), np.zeros((Q, stride, 8), np.uint32)
        for q, (t, x) in enumerate(zip(trees.tolist(), digests)):
            if t >= self.ntrees:
                continue
            leaves = self.trees[t]
            i, pred[q], succ[q], main[q], low[q], heights[q] = model_proof(leaves, self.levels[t], x, stride)
            idx[q], found[q] = i, int(model_lower_bound(leaves, x)[1])
            verdicts[q] = model_verdict(x, t, self.ntrees, i, pred[q], succ[q], main[q], low[q], heights[q], self.roots[t], len(leaves))
            assert verdicts[q] == (PRESENT if found[q] else ABSENT), (q, t)
        return idx, found, pred, succ, main, low, heights, verdicts


@functools.lru_cache(maxsize=None)
def forest():
    return Forest()


# ---- the sortedness cases: (what, per-tree leaves, first_bad per tree, trees not sorted, of those equal) -------------------------------
def sortedness_cases():
    f = forest()
    rng = np.random.default_rng(603)
    clean = [t.copy() for t in f.trees]
    cases = [("clean", clean)]

    def bent(change):
        trees = [t.copy() for t in clean]
        change(trees)
        return trees

    def equal_pair(trees):
        trees[11][30] = trees[11][29]

    def first_pair(trees):
        trees[10][[0, 1]] = trees[10][[1, 0]]

    def last_pair(trees):
        trees[12][[63, 64]] = trees[12][[64, 63]]

    def two(trees):
        trees[13][[100, 101]] = trees[13][[101, 100]]
        trees[13][41] = trees[13][40]

    def boundary(trees):                                 # every tree stays sorted; tree 5 ends above where tree 6 begins
        assert key(trees[5][-1]) > key(trees[6][0]) or key(trees[4][-1]) > key(trees[5][0])

    def pair_of_one(trees):                              # the two leaves of the tree of 2, between an empty tree's neighbours
        trees[1][[0, 1]] = trees[1][[1, 0]]
        trees[4][[2, 3]] = trees[4][[3, 2]]              # the tree behind the first empty tree, its last pair

    for what, change in (("one equal pair", equal_pair), ("a descent at the first pair of a tree", first_pair),
                         ("a descent at the last pair of a tree", last_pair), ("two offences in one tree", two),
                         ("a descent across a tree boundary only", boundary), ("empty trees on either side", pair_of_one)):
        cases.append((what, bent(change)))
    big = sorted_rows(random_leaves(rng, 300))
    for at in (64, 256):
        one = big.copy()
        one[[at - 1, at]] = one[[at, at - 1]]
        cases.append((f"indices {at - 1}/{at} of one tree", [np.zeros((0, 8), np.uint32), one, np.zeros((0, 8), np.uint32)]))
    out = []
    for what, trees in cases:
        want = [model_first_bad(t) for t in trees]
        out.append((what, trees, np.array([w[0] for w in want], dtype=np.uint64), sum(w[0] != NONE for w in want), sum(w[1] for w in want),
                    sum(max(len(t) - 1, 0) for t in trees)))
    return out


def lay(trees, first=0, slack=0):
    """(cells, offsets) of per-tree leaf arrays laid at cell `first`, `slack` cells behind; the cells outside descend."""
    body = np.concatenate(trees) if sum(len(t) for t in trees) else np.zeros((0, 8), np.uint32)
    pad = np.array([[0xFFFFFFFF - j] * 8 for j in range(first + slack)], dtype=np.uint32).reshape(-1, 8)
    cells = np.concatenate([pad[:first], body, pad[first:]])
    offsets = (np.concatenate([[0], np.cumsum([len(t) for t in trees])]) + first).astype(np.uint64)
    return np.ascontiguousarray(cells), offsets


# ---- the verifier's negatives ----------------------------------------------------------------------------------------------------------
def negatives(stride=STRIDE):
    """[(what, want, x, t, index, pred, succ, main, low, height, root, count)]: proofs out of the tree of 65 (tree 12) and the
    tree of 130 (tree 13) of forest(), each honest one (want 1) followed by its bent copies (want 0), and the one that stays 1."""
    f = forest()
    out = []

    def honest(t, i):
        leaves = f.trees[t]
        lo = as_int(leaves[i - 1]) if i > 0 else -1
        hi = as_int(leaves[i]) if i < len(leaves) else 1 << 256
        x = from_int(lo + (hi - lo) // 2)
        got = model_proof(leaves, f.levels[t], x, stride)
        assert got[0] == i
        return [x, t, *got, f.roots[t], len(leaves)]

    def add(what, want, p):
        out.append((what, want, *p))

    t, i = 13, 48                                        # top = 4, H = 8
    p = honest(t, i)
    add("honest, two-sided", ABSENT, p)
    add("pred and succ swapped", NOT_PROVEN, p[:3] + [p[4], p[3]] + p[5:])
    q = honest(t, i)
    q[2] = i + 1                                         # the index off by one, every cell true: the neighbours are not adjacent
    q[4] = f.trees[t][i + 1]
    q[5] = model_proof(f.trees[t], f.levels[t], f.trees[t][i + 1], stride)[3]
    add("index off by one with true proofs", NOT_PROVEN, q)
    add("x == pred", NOT_PROVEN, [p[3]] + p[1:])
    above = from_int(as_int(p[4]) + 1)
    add("x above succ", NOT_PROVEN, [above] + p[1:])
    add("a wrong height", NOT_PROVEN, p[:7] + [p[7] + 1] + p[8:])
    bent = p[6].copy()
    bent[2, 3] ^= np.uint32(1 << 9)
    add("one low cell below top flipped", NOT_PROVEN, p[:6] + [bent] + p[7:])
    other = p[5].copy()
    other[4] = f.levels[t][4][5]                         # another stored node of level top
    assert key(other[4]) != key(p[5][4])
    add("main[top] replaced by another stored node", NOT_PROVEN, p[:5] + [other] + p[6:])
    add("a root of another tree", NOT_PROVEN, p[:8] + [f.roots[12]] + p[9:])
    junk = p[6].copy()
    junk[4:] = 0xDEADBEEF
    add("garbage in the low row at and above top", ABSENT, p[:6] + [junk] + p[7:])
    last = honest(12, 65)                                # above the last leaf of the tree of 65: H(65) == H(66) == 7
    add("honest, above the last leaf", ABSENT, last)
    add("count off by one, above the last", NOT_PROVEN, last[:9] + [66])
    add("count off by one the other way", NOT_PROVEN, last[:9] + [64])
    first = honest(12, 0)
    add("honest, below the first leaf", ABSENT, first)
    add("below the first leaf, a nonzero index", NOT_PROVEN, first[:2] + [1] + first[3:])
    return out


# ---- the CPU twins (libvkmr_host.so) ---------------------------------------------------------------------------------------------------
def _ptr(a):
    return a.ctypes.data if a.size else None


def host_sorted(cells, offsets):
    """(rc, first_bad uint64 [ntrees], info uint64 [4]) of vkmr_host_cpu_forest_sorted; the outputs start as the canary."""
    import vk_merkle_roots_amd as vk
    cells, offsets = np.ascontiguousarray(cells, dtype=np.uint32).reshape(-1, 8), np.ascontiguousarray(offsets, dtype=np.uint64)
    ntrees = int(offsets.shape[0]) - 1
    bad, info = np.full(ntrees, INDEX_FILL, np.uint64), np.full(4, INDEX_FILL, np.uint64)
    rc = vk.host_lib().vkmr_host_cpu_forest_sorted(_ptr(cells), int(cells.shape[0]), offsets.ctypes.data, ntrees, _ptr(bad), info.ctypes.data)
    return rc, bad, info


def host_lower_bound(cells, offsets, trees, digests):
    """(indices, found) of vkmr_host_cpu_forest_lower_bound."""
    import vk_merkle_roots_amd as vk
    cells, offsets = np.ascontiguousarray(cells, dtype=np.uint32).reshape(-1, 8), np.ascontiguousarray(offsets, dtype=np.uint64)
    trees, digests = np.ascontiguousarray(trees, dtype=np.uint32), np.ascontiguousarray(digests, dtype=np.uint32).reshape(-1, 8)
    Q = int(trees.shape[0])
    idx, found = np.full(Q, INDEX_FILL, np.uint64), np.full(Q, CANARY, np.uint32)
    rc = vk.host_lib().vkmr_host_cpu_forest_lower_bound(_ptr(cells), int(cells.shape[0]), offsets.ctypes.data, int(offsets.shape[0]) - 1, trees.ctypes.data,
                                                        digests.ctypes.data, Q, idx.ctypes.data, found.ctypes.data)
    assert rc == 0
    return idx, found


def host_absence(cells, offsets, trees, digests, stride=STRIDE):
    """(rc, indices, pred, succ, main, low, heights) of vkmr_host_cpu_forest_absence; the outputs start as the canary."""
    import vk_merkle_roots_amd as vk
    cells, offsets = np.ascontiguousarray(cells, dtype=np.uint32).reshape(-1, 8), np.ascontiguousarray(offsets, dtype=np.uint64)
    trees, digests = np.ascontiguousarray(trees, dtype=np.uint32), np.ascontiguousarray(digests, dtype=np.uint32).reshape(-1, 8)
    Q = int(trees.shape[0])
    idx, heights = np.full(Q, INDEX_FILL, np.uint64), np.full(Q, CANARY, np.uint32)
    nb = np.full((Q, 2, 8), CANARY, np.uint32)
    main, low = np.full((Q, stride, 8), CANARY, np.uint32), np.full((Q, stride, 8), CANARY, np.uint32)
    rc = vk.host_lib().vkmr_host_cpu_forest_absence(_ptr(cells), int(cells.shape[0]), offsets.ctypes.data, int(offsets.shape[0]) - 1, trees.ctypes.data,
                                                    digests.ctypes.data, Q, stride, idx.ctypes.data, nb.ctypes.data, main.ctypes.data, low.ctypes.data,
                                                    heights.ctypes.data)
    return rc, idx, nb[:, 0].copy(), nb[:, 1].copy(), main, low, heights


def host_verify(digests, trees, indices, pred, succ, main, low, heights, roots, counts):
    """verdict uint32 [Q] of vkmr_host_cpu_verify_absence; starts as the canary."""
    import vk_merkle_roots_amd as vk
    digests, trees = np.ascontiguousarray(digests, dtype=np.uint32).reshape(-1, 8), np.ascontiguousarray(trees, dtype=np.uint32)
    indices, heights = np.ascontiguousarray(indices, dtype=np.uint64), np.ascontiguousarray(heights, dtype=np.uint32)
    Q = int(trees.shape[0])
    nb = np.ascontiguousarray(np.stack([np.asarray(pred, dtype=np.uint32).reshape(Q, 8), np.asarray(succ, dtype=np.uint32).reshape(Q, 8)], axis=1))
    main, low = np.ascontiguousarray(main, dtype=np.uint32), np.ascontiguousarray(low, dtype=np.uint32)
    roots, counts = np.ascontiguousarray(roots, dtype=np.uint32).reshape(-1, 8), np.ascontiguousarray(counts, dtype=np.uint64)
    assert main.shape == low.shape == (Q, main.shape[1], 8) and roots.shape[0] == counts.shape[0]
    verdict = np.full(Q, CANARY, np.uint32)
    rc = vk.host_lib().vkmr_host_cpu_verify_absence(digests.ctypes.data, trees.ctypes.data, indices.ctypes.data, nb.ctypes.data, main.ctypes.data,
                                                    low.ctypes.data, heights.ctypes.data, Q, int(main.shape[1]), _ptr(roots), _ptr(counts),
                                                    int(roots.shape[0]), verdict.ctypes.data)
    assert rc == 0
    return verdict


def negatives_batch(stride=STRIDE):
    """negatives() as the arrays of one verify call over a table of one root and one count per PROOF (tree q of Q): (what, want,
    digests, trees, indices, pred, succ, main, low, heights, roots, counts)."""
    rows = negatives(stride)
    Q = len(rows)
    col = lambda j, dtype, *shape: np.array([r[j] for r in rows], dtype=dtype).reshape(Q, *shape)
    return ([r[0] for r in rows], col(1, np.uint32), col(2, np.uint32, 8), np.arange(Q, dtype=np.uint32), col(4, np.uint64), col(5, np.uint32, 8),
            col(6, np.uint32, 8), col(7, np.uint32, stride, 8), col(8, np.uint32, stride, 8), col(9, np.uint32), col(10, np.uint32, 8), col(11, np.uint64))


# ---- the replay ------------------------------------------------------------------------------------------------------------------------
def build_absence_plan_exe(directory):
    """tests/c/absence_plan_test.cpp as a program of its own, with AddressSanitizer and UBSan."""
    exe = os.path.join(str(directory), "absence_plan_test_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "vk_merkle_roots_amd", "csrc"), os.path.join(ROOT, "tests", "c", "absence_plan_test.cpp"), "-o", exe])
    return exe
