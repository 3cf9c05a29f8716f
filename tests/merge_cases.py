"""Two sorted forests merged tree by tree (vkmr_hip_forest_merge_leaves_async, vkmr_hip_tree_merge_leaves_async, their CPU twins,
HipDevice.merge_leaves, MerkleForest.inserted / removed / common): the rule restated in Python, the cases and the drivers of the
twins and of the replay (tests/c/merge_plan_test.cpp), shared by tests/test_merge_abi.py (no GPU) and tests/test_gpu_merge.py.  A
plain module: no fixtures, no GPU.

THE MODEL is Python's `sorted(set(...))` and list comprehensions on the tuples of a digest's eight unsigned words, per tree:
union = sorted(set(A_t) | set(B_t)), difference = [a for a in A_t if a not in B_t], intersection = [a for a in A_t if a in B_t].
origin: A's cell for a digest of A, else (1 << 63) | the cell of B's FIRST leaf with that digest.  info = [status, n_out, matches,
repeats]: matches the distinct digests of B_t that are in A_t, repeats the leaves of B_t equal to the one in front of them."""
import functools
import os
import subprocess
from typing import NamedTuple

import numpy as np

import leafsort_cases as lc
from merkle_model import ROOT, random_leaves

CANARY, INFO_FILL = lc.CANARY, lc.INFO_FILL
OFFSET_FILL = 0xA5A5A5A5A5A5A5A5
COUNTS = lc.COUNTS                                   # the forest A: the counts that serve the leaf sort as well
OPS = (0, 1, 2)
OP_NAMES = ("union", "difference", "intersection")
BAD_A_OFFSETS, BAD_B_OFFSETS, A_NOT_INCREASING, B_DECREASES, SHORT_OUTPUT = 1, 2, 4, 8, 16
FROM_B = 1 << 63
A_PLACEMENTS = ((0, 0), (37, 100))                   # (offsets[0], slack cells behind) of A
B_PLACEMENTS = ((0, 0), (11, 7))                     # and of B beside it
ZERO, ONES = (0,) * 8, (0xFFFFFFFF,) * 8
HALF_BELOW, HALF = (0x7FFFFFFF,) + (0xFFFFFFFF,) * 7, (0x80000000,) + (0,) * 7
words = lc.words


def as_int(row):
    v = 0
    for w in row:
        v = (v << 32) | int(w)
    return v


def from_int(v):
    return tuple((v >> (32 * (7 - i))) & 0xFFFFFFFF for i in range(8))


def rows_of(tuples):
    return np.array(list(tuples), dtype=np.uint32).reshape(-1, 8)


# ---- the plan, restated ----------------------------------------------------------------------------------------------------------------

SCAN_ROW, HEADER_WORDS = 8192, 8                     # VKMR_MERGE_SCAN_ROW, VKMR_MERGE_HEADER_WORDS: tests/test_merge_abi.py holds them to the header


def scratch_bytes(a_total, b_total):
    """The layout of merge_plan.hpp written out."""
    n = a_total + b_total + 2
    if a_total >= 1 << 32 or b_total >= 1 << 32 or n >= 1 << 32:
        return 0
    up = lambda x: (x + 15) // 16 * 16                                                # noqa: E731
    rows = -(-n // SCAN_ROW)
    return 4 * rows * SCAN_ROW + up(4 * rows) + 16 + up(4 * b_total) + 8 * HEADER_WORDS


def n_out_of_counts(op, na, nb, matches, repeats):
    return (na + nb - matches - repeats, na - matches, matches)[op]


# ---- the model -------------------------------------------------------------------------------------------------------------------------

class Case(NamedTuple):
    name: str
    a_cells: np.ndarray        # [a_total, 8]: A's buffer, filler outside the trees
    a_offsets: np.ndarray      # uint64 [ntrees + 1]
    b_cells: np.ndarray
    b_offsets: np.ndarray


def offsets_bad(off, total):
    return any(b < a for a, b in zip(off, off[1:])) or off[-1] > total


def model_merge(case, op, capacity=None):
    """(out [capacity, 8], out_offsets [ntrees + 1], origin [capacity], info [4]) by the rule; what is not written holds the
    canary.  capacity None: nA + nB for union, nA for the other two."""
    a, b = case.a_cells.reshape(-1, 8), case.b_cells.reshape(-1, 8)
    ao, bo = [int(o) for o in case.a_offsets], [int(o) for o in case.b_offsets]
    ntrees = len(ao) - 1
    status = (BAD_A_OFFSETS if offsets_bad(ao, a.shape[0]) else 0) | (BAD_B_OFFSETS if offsets_bad(bo, b.shape[0]) else 0)
    if capacity is None:
        capacity = 0 if status else (ao[-1] - ao[0]) + ((bo[-1] - bo[0]) if op == 0 else 0)
    out, origin = np.full((capacity, 8), CANARY, np.uint32), np.full(capacity, OFFSET_FILL, np.uint64)
    out_offsets = np.full(ntrees + 1, OFFSET_FILL, np.uint64)

    def refused(status, n=0, matches=0, repeats=0):
        return out, out_offsets, origin, np.array([status, n, matches, repeats], dtype=np.uint64)
    if status:
        return refused(status)
    A = [[words(a[j]) for j in range(ao[t], ao[t + 1])] for t in range(ntrees)]
    B = [[words(b[j]) for j in range(bo[t], bo[t + 1])] for t in range(ntrees)]
    if any(not x < y for rows in A for x, y in zip(rows, rows[1:])):
        status |= A_NOT_INCREASING
    if any(y < x for rows in B for x, y in zip(rows, rows[1:])):
        status |= B_DECREASES
    if status:
        return refused(status)
    got, src, starts, matches, repeats = [], [], [0], 0, 0
    for t in range(ntrees):
        in_a = {d: ao[t] + i for i, d in enumerate(A[t])}
        in_b = {}
        for j, d in enumerate(B[t]):
            in_b.setdefault(d, FROM_B | (bo[t] + j))
        matches += len(set(in_a) & set(in_b))
        repeats += sum(x == y for x, y in zip(B[t], B[t][1:]))
        if op == 0:
            mine = sorted(set(in_a) | set(in_b))
        elif op == 1:
            mine = [d for d in A[t] if d not in in_b]
        else:
            mine = [d for d in A[t] if d in in_b]
        got += mine
        src += [in_a[d] if d in in_a else in_b[d] for d in mine]
        starts.append(len(got))
    na, nb = ao[-1] - ao[0], bo[-1] - bo[0]
    assert len(got) == n_out_of_counts(op, na, nb, matches, repeats)
    if len(got) > capacity:
        return refused(SHORT_OUTPUT, len(got), matches, repeats)
    if got:
        out[: len(got)] = rows_of(got)
        origin[: len(got)] = np.array(src, dtype=np.uint64)
    out_offsets[:] = np.array(starts, dtype=np.uint64)
    return out, out_offsets, origin, np.array([0, len(got), matches, repeats], dtype=np.uint64)


# ---- the cases -------------------------------------------------------------------------------------------------------------------------

def lay(trees, first=0, slack=0, seed=7):
    return lc.lay([rows_of(t) for t in trees], first, slack, seed)


def between(lo, n):
    """n digests lo + 1 .. lo + n: their order is decided in word 7 unless a carry reaches further."""
    return [from_int(as_int(lo) + 1 + i) for i in range(n)]


@functools.lru_cache(maxsize=None)
def forest_sides():
    """(A's trees, B's trees) as lists of word tuples: A strictly increasing, B non-decreasing.  tests/test_merge_abi.py checks
    what is where."""
    rng = np.random.default_rng(801)
    A = []
    for c in COUNTS:
        rows = random_leaves(rng, c)
        rows[:, 0] = (rows[:, 0] >> np.uint32(3)) + np.uint32(0x10000000)             # room below the first and above the last leaf, gaps in between
        A.append(sorted(set(words(r) for r in rows)))
    assert [len(t) for t in A] == COUNTS
    A[6] = A[6][:5] + [HALF_BELOW[:7] + (0xFFFFFFF0,), HALF[:7] + (5,)]              # the random leaves lie below; these two on either side of word 0's sign bit
    A[17][0], A[17][-1] = ZERO, ONES                                                  # the lowest and the highest digest there is, as leaves
    B = [[] for _ in COUNTS]
    below = lambda t, n: between(from_int(as_int(A[t][0]) - n - 1), n)                # noqa: E731   n digests directly below the first leaf
    B[0] = []                                                                         # B empty
    B[1] = below(1, 2)                                                                # entirely below A's first leaf
    B[2] = between(A[2][-1], 2)                                                       # entirely above A's last leaf: the end slot
    B[3] = below(4, 4) + [A[4][0]]                                                    # into an empty tree of A; its last digest ...
    B[4] = list(A[4])                                                                 # ... is the first of the next tree: leaf for leaf equal to A
    B[5] = sorted(set(A[5][::2] + [d for a in A[5] for d in between(a, 7)]))          # larger than A: 3 matches, 35 others
    B[6] = sorted([A[6][0], HALF_BELOW, HALF, A[6][4]] + between(A[6][1], 1))         # across the sign bit: words 0 differ, both orders wrong if signed
    # runs of 2 at slot 0, 5 behind the first leaf, 65 in the middle, 1 at the end slot; B's flat cells 63 and 64 are A[7][1] and the digest above it
    B[7] = sorted(below(7, 2) + between(A[7][0], 5) + [A[7][1]] + between(A[7][1], 1) + between(A[7][3], 65) + between(A[7][-1], 1))
    B[8] = sorted([A[8][3]] * 2 + between(A[8][5], 1) * 2 + [A[8][7]])               # a repeat that matches A, a pair that does not
    B[9] = []                                                                         # both sides empty

    def alternating(t):                                                               # every even leaf, and a digest just above every odd one
        return [A[t][i] if i % 2 == 0 else between(A[t][i], 1)[0] for i in range(len(A[t]))]
    B[10] = sorted(below(10, 64) + alternating(10))                                   # 64 at slot 0
    B[11] = sorted([ZERO] + alternating(11)[:-1] + between(A[11][-1], 65))            # the all-zero digest, 65 at the end slot
    B[12] = sorted(below(12, 1) + alternating(12)[:30] + between(A[12][30], 64) + alternating(12)[32:])
    run40 = between(A[13][100], 1) * 40                                               # a run of 40 equal leaves
    B[13] = sorted(alternating(13)[:50] + between(A[13][60], 257) + run40 + between(A[13][-1], 64))
    B[14] = sorted(alternating(14) + between(A[14][-1], 257))                         # 257 at the end slot
    B[15] = sorted(below(15, 257) + alternating(15) + between(A[15][511], 2)[1:])     # 257 at slot 0, 2 in the middle
    B[16] = sorted(below(16, 65) + alternating(16)[:-1] + [ONES])                                    # the all-ones digest above the last leaf
    B[17] = sorted([ZERO] + alternating(17)[1:-1] + between(A[17][1200], 66)[1:])     # 65 in the middle of the largest tree; ZERO matches
    for t in range(len(COUNTS)):
        assert all(x < y for x, y in zip(A[t], A[t][1:])) and all(x <= y for x, y in zip(B[t], B[t][1:])), t
    return A, B


def forest_cases():
    A, B = forest_sides()
    return [Case(f"the forest: A at {fa} with {sa} behind, B at {fb} with {sb} behind", *lay(A, fa, sa), *lay(B, fb, sb, seed=8))
            for (fa, sa), (fb, sb) in zip(A_PLACEMENTS, B_PLACEMENTS)]


def shape_cases():
    A, B = forest_sides()
    rng = np.random.default_rng(802)

    def small(count):                                                                 # `count` increasing digests of a 5-letter alphabet in word 7
        return [ZERO[:7] + (int(v),) for v in sorted(rng.choice(5, size=count, replace=False))]
    many_a = [small(int(c)) for c in rng.integers(0, 4, size=257)]
    many_b = [sorted(small(int(c)) + small(int(d))) for c, d in rng.integers(0, 4, size=(257, 2))]     # repeats among them
    many_b = [t[:3] for t in many_b]
    one = sorted(set(words(r) for r in random_leaves(rng, 1500)))
    other = sorted(one[100:400:3] + [words(r) for r in random_leaves(rng, 200)])
    x, y = words(random_leaves(rng, 1)[0]), words(random_leaves(rng, 1)[0])
    return [Case("one tree", *lay([one], 3, 5), *lay([other], 2, 0, seed=9)),
            Case("one leaf against the same leaf", *lay([[x]]), *lay([[x]])),
            Case("one leaf against another", *lay([[x]]), *lay([[y]], 1, 1)),
            Case("257 trees of 0 to 3 leaves on each side", *lay(many_a, 1, 3), *lay(many_b, 0, 2, seed=9)),
            Case("every tree empty on both sides", *lay([[], [], []], 4, 4), *lay([[], [], []])),
            Case("an empty A: the distinct leaves of a batch that repeats", *lay([[], []]), *lay([sorted(other[:50] * 2 + other[:5]), [x, x, x]])),
            Case("an empty B", *lay([one[:70], one[70:75]], 0, 2), *lay([[], []], 3, 0)),
            Case("the tree of 2 500 alone", *lay([A[17]]), *lay([B[17]]))]


def all_cases():
    return forest_cases() + shape_cases()


def is_one_tree(case):
    """The one-tree twin takes it: one tree a side, both at cell 0 with nothing behind."""
    return (len(case.a_offsets) == 2 and int(case.a_offsets[0]) == 0 == int(case.b_offsets[0]) and int(case.a_offsets[1]) == case.a_cells.shape[0]
            and int(case.b_offsets[1]) == case.b_cells.shape[0])


def default_capacity(case, op):
    na, nb = int(case.a_offsets[-1]) - int(case.a_offsets[0]), int(case.b_offsets[-1]) - int(case.b_offsets[0])
    return na + nb if op == 0 else na


# ---- what is refused --------------------------------------------------------------------------------------------------------------------

def disordered(case):
    """(A with two leaves of its largest tree swapped, B with two unequal neighbours swapped), as cases."""
    a, b = case.a_cells.copy(), case.b_cells.copy()
    i = int(case.a_offsets[-1]) - 100
    a[[i, i + 1]] = a[[i + 1, i]]
    j = int(case.b_offsets[-1]) - 100
    assert (b[j] != b[j + 1]).any()
    b[[j, j + 1]] = b[[j + 1, j]]
    return case._replace(a_cells=a), case._replace(b_cells=b), case._replace(a_cells=a, b_cells=b)


REFUSALS = ("A's offsets decrease", "B's offsets end behind its cells", "both offsets", "A not increasing", "A with an equal pair", "B decreasing",
            "A and B out of order", "a short output")


def refusal(name):
    """(case, capacity or None, the status, n_out) of a refusal, on the second placement of the forest."""
    c = forest_cases()[1]
    down = np.concatenate([c.a_offsets[:5], c.a_offsets[5:6] - 9, c.a_offsets[6:]]).astype(np.uint64)
    behind = np.concatenate([c.b_offsets[:-1], [c.b_cells.shape[0] + 1]]).astype(np.uint64)
    bad_a, bad_b, bad_both = disordered(c)
    equal = c.a_cells.copy()
    equal[int(c.a_offsets[-1]) - 7] = equal[int(c.a_offsets[-1]) - 8]
    return {"A's offsets decrease": (c._replace(a_offsets=down), 20, 1, 0), "B's offsets end behind its cells": (c._replace(b_offsets=behind), 20, 2, 0),
            "both offsets": (c._replace(a_offsets=down, b_offsets=behind), 20, 3, 0), "A not increasing": (bad_a, None, 4, 0),
            "A with an equal pair": (c._replace(a_cells=equal), None, 4, 0), "B decreasing": (bad_b, None, 8, 0), "A and B out of order": (bad_both, None, 12, 0),
            "a short output": (c, -1, 16, None)}[name]


# ---- the CPU twins (libvkmr_host.so) ----------------------------------------------------------------------------------------------------

def _ptr(a):
    return a.ctypes.data if a.size else None


def host_merge(case, op, capacity=None, with_origin=True, one_tree=False):
    """(rc, out, out_offsets, origin, info) of vkmr_host_cpu_forest_merge_leaves (or the one-tree twin: the offsets stay the
    fill); the outputs start as the canary."""
    import vk_merkle_roots_amd as vk
    a, b = np.ascontiguousarray(case.a_cells, dtype=np.uint32).reshape(-1, 8), np.ascontiguousarray(case.b_cells, dtype=np.uint32).reshape(-1, 8)
    ao, bo = np.ascontiguousarray(case.a_offsets, dtype=np.uint64), np.ascontiguousarray(case.b_offsets, dtype=np.uint64)
    capacity = default_capacity(case, op) if capacity is None else capacity
    out, origin = np.full((capacity, 8), CANARY, np.uint32), np.full(capacity, OFFSET_FILL, np.uint64)
    out_offsets, info = np.full(ao.shape[0], OFFSET_FILL, np.uint64), np.full(4, INFO_FILL, np.uint64)
    if one_tree:
        rc = vk.host_lib().vkmr_host_cpu_tree_merge_leaves(_ptr(a), a.shape[0], _ptr(b), b.shape[0], op, _ptr(out), capacity,
                                                           _ptr(origin) if with_origin else None, info.ctypes.data)
    else:
        rc = vk.host_lib().vkmr_host_cpu_forest_merge_leaves(_ptr(a), a.shape[0], ao.ctypes.data, _ptr(b), b.shape[0], bo.ctypes.data, ao.shape[0] - 1, op,
                                                             _ptr(out), capacity, out_offsets.ctypes.data, _ptr(origin) if with_origin else None,
                                                             info.ctypes.data)
    return rc, out, out_offsets, origin, info


# ---- the replay -------------------------------------------------------------------------------------------------------------------------

def build_merge_plan_exe(directory):
    """tests/c/merge_plan_test.cpp as a program of its own, with AddressSanitizer and UBSan."""
    exe = os.path.join(str(directory), "merge_plan_test_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "vk_merkle_roots_amd", "csrc"), os.path.join(ROOT, "tests", "c", "merge_plan_test.cpp"), "-o", exe])
    return exe
