"""The leaves of a forest sorted on the device (vkmr_hip_forest_sort_leaves_async, vkmr_hip_tree_sort_leaves_async, their CPU
twins, HipDevice.sort_leaves / build_sorted_forest, vk.sorted_forest_packed): the rule restated in Python, the cases and the
drivers of the twins and of the replay (tests/c/leafsort_plan_test.cpp), shared by tests/test_leafsort_abi.py (no GPU) and
tests/test_gpu_leafsort.py.  A plain module: no fixtures, no GPU.

THE MODEL is Python's stable `sorted` on the tuple of a digest's eight unsigned words, per tree: out[offsets[t] + i] is the i-th
of tree t's leaves in that order, order[...] the flat cell it came from; cells outside [offsets[0], offsets[ntrees]) stay as they
were.  info = [status, n, m, repeats]: m the sorted leaves whose KEY (csrc/leafsort_plan.hpp, restated in key_of) equals that of
the leaf before or behind, repeats the leaves equal in all eight words to an earlier leaf of their tree."""
import functools
import os
import re
import subprocess
from typing import NamedTuple

import numpy as np

from merkle_model import ROOT, random_leaves

CANARY = 0xA5A5A5A5
INFO_FILL = 0xA5A5A5A5A5A5A5A5
ZERO = np.zeros(8, np.uint32)
ONES = np.full(8, 0xFFFFFFFF, np.uint32)
COUNTS = [1, 2, 3, 0, 4, 5, 7, 8, 9, 0, 63, 64, 65, 130, 1023, 1024, 1025, 2500]     # trees end before, at and behind a tile edge
PLACEMENTS = ((0, 0), (37, 100))                                                      # (offsets[0], slack cells behind)
RUN = 40                                                                              # the leaves equal in words 0..6
BAD_OFFSETS, ABOVE_MAX_COUNT, TOO_MANY_TIES = 1, 2, 4


# ---- the plan, read / restated --------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def plan_constants():
    """{name: value} of the VKMR_LEAFSORT_* and VKMR_SORT_* constants, read from the headers' text."""
    out = {}
    for header in ("leafsort_plan.hpp", "sort_plan.hpp"):
        text = open(os.path.join(ROOT, "vk_merkle_roots_amd", "csrc", header)).read()
        out.update({name: int(value) for name, value in re.findall(r"#define\s+(VKMR_(?:LEAF)?SORT_\w+)\s+(\d+)u(?:ll)?\b", text)})
    return out


def max_ties():
    return plan_constants()["VKMR_LEAFSORT_MAX_TIES"]


def tile_keys():
    c = plan_constants()
    return c["VKMR_SORT_THREADS"] * c["VKMR_SORT_KEYS_PER_LANE"]


def shape(ntrees, max_count):
    """(bits_T, P, passes) of a call."""
    bits_t = (ntrees - 1).bit_length() if ntrees else 0
    p = min(64 - bits_t, 2 * int(max_count).bit_length() + 8)
    return bits_t, p, -(-(bits_t + p) // 8)


def key_of(tree, row, p):
    prefix = (int(row[0]) << 32) | int(row[1])
    return ((tree << p) | (prefix >> (64 - p))) & 0xFFFFFFFFFFFFFFFF if p < 64 else prefix


def scratch_bytes(total):
    """The layout of leafsort_plan.hpp written out: sort_plan.hpp's for k = total, dest, the header."""
    if total == 0 or total >= 1 << 32:
        return 0
    c = plan_constants()
    up = lambda n: (n + 15) // 16 * 16                                                # noqa: E731
    words = -(-total // 64)
    sort = (2 * up(8 * total) + 2 * up(4 * total) + up(4 * c["VKMR_SORT_BINS"] * -(-total // tile_keys())) + up(4 * c["VKMR_SORT_BINS"]) + 2 * up(8 * words) +
            up(8 * -(-words // c["VKMR_SORT_RANK_BLOCK_WORDS"])) + 32)
    return sort + up(4 * total) + 8 * c["VKMR_LEAFSORT_HEADER_WORDS"]


def words(row):
    return tuple(int(w) for w in row)


# ---- the model ------------------------------------------------------------------------------------------------------------------------

def model_sort(cells, offsets, max_count, tie_limit=None, out=None, order=None):
    """(out cells, order uint32 [total], info uint64 [4]) by the rule; `out` and `order` as they were before the call (the canary
    when None).  tie_limit None: the twins' rule, which always sorts."""
    cells = np.asarray(cells, dtype=np.uint32).reshape(-1, 8)
    total, ntrees = int(cells.shape[0]), len(offsets) - 1
    off = [int(o) for o in offsets]
    out = np.full((total, 8), CANARY, np.uint32) if out is None else out.copy()
    order = np.full(total, CANARY, np.uint32) if order is None else order.copy()
    status = 0
    if any(b < a for a, b in zip(off, off[1:])) or off[-1] > total:
        status |= BAD_OFFSETS
    if any(b >= a and b - a > max_count for a, b in zip(off, off[1:])):
        status |= ABOVE_MAX_COUNT
    n = 0 if status & BAD_OFFSETS else off[-1] - off[0]
    if status:
        return out, order, np.array([status, n, 0, 0], dtype=np.uint64)
    p = shape(ntrees, max_count)[1]
    new_order, keys, repeats = [], [], 0
    for t in range(ntrees):
        rows = [words(cells[j]) for j in range(off[t], off[t + 1])]
        by = sorted(range(len(rows)), key=lambda i: rows[i])                          # stable
        new_order += [off[t] + i for i in by]
        keys += [key_of(t, rows[i], p) for i in by]
        repeats += sum(rows[a] == rows[b] for a, b in zip(by, by[1:]))
    m = sum((j > 0 and keys[j - 1] == keys[j]) or (j + 1 < n and keys[j + 1] == keys[j]) for j in range(n))
    if tie_limit is not None and m > tie_limit:
        return out, order, np.array([TOO_MANY_TIES, n, m, 0], dtype=np.uint64)
    if n:
        out[off[0]: off[-1]] = cells[new_order]
        order[off[0]: off[-1]] = new_order
    return out, order, np.array([0, n, m, repeats], dtype=np.uint64)


# ---- the cases ------------------------------------------------------------------------------------------------------------------------

class Case(NamedTuple):
    name: str
    cells: np.ndarray          # [total, 8]: the input buffer, filler outside the trees
    offsets: np.ndarray        # uint64 [ntrees + 1]
    max_count: int


def lay(trees, first=0, slack=0, seed=7):
    """(cells, offsets) of per-tree leaf arrays laid at cell `first`, `slack` random cells behind and `first` in front."""
    filler = random_leaves(np.random.default_rng(seed), first + slack)
    body = [np.asarray(t, dtype=np.uint32).reshape(-1, 8) for t in trees]
    cells = np.concatenate([filler[:first]] + body + [filler[first:]])
    offsets = (np.concatenate([[0], np.cumsum([len(t) for t in trees])]) + first).astype(np.uint64)
    return np.ascontiguousarray(cells), offsets


@functools.lru_cache(maxsize=None)
def forest_trees():
    """COUNTS trees of random leaves with the crafted ones among them (tests/test_leafsort_abi.py checks what is where)."""
    rng = np.random.default_rng(701)
    trees = [random_leaves(rng, c) for c in COUNTS]
    # the tree of 1 023 holds flat positions 361 .. 1 383 of the placement at 0: RUN leaves equal in words 0..6, descending in word 7,
    # at input indices 643 .. 682 (flat 1 004 .. 1 043), under a prefix that 643 other leaves of the tree lie below
    t14 = trees[14]
    others = sorted(words(r) for r in np.delete(t14, np.s_[643: 643 + RUN], axis=0))
    pivot = np.array(others[642], dtype=np.uint32)
    for j in range(RUN):
        t14[643 + j] = pivot
        t14[643 + j][7] = np.uint32(1000 + RUN - j)
    at = [words(r) for r in t14].index(tuple(pivot))
    t14[at][7] = 0                                                                    # the pivot itself below the run, under the same prefix
    # the same 64-bit prefix in the last leaves of the tree of 1 024 and the first of the tree of 1 025
    for row in list(trees[15][-3:]) + list(trees[16][:3]):
        row[0], row[1] = 0x13572468, 0x9ABCDEF0
    trees[6][2] = np.array([0x80000000] + [0] * 7, dtype=np.uint32)
    trees[6][5] = np.array([0x7FFFFFFF] + [0xFFFFFFFF] * 7, dtype=np.uint32)
    trees[17][100], trees[17][7], trees[17][2499] = ONES, ZERO, ONES                  # the last tree
    for at in (5, 60, 129):                                                           # three equal digests, scattered
        trees[13][at] = trees[13][60]
    return trees


def forest_cases():
    trees = forest_trees()
    return [Case(f"the forest at {first} with {slack} behind", *lay(trees, first, slack), max(COUNTS)) for first, slack in PLACEMENTS]


def shape_cases():
    rng = np.random.default_rng(702)
    many = [int(c) for c in rng.integers(0, 4, size=257)]
    many[0], many[255], many[256] = 3, 2, 3                                           # trees on both sides of the digit at 2^8
    sentinel = [random_leaves(rng, 5), random_leaves(rng, 6)]
    sentinel[1][1], sentinel[1][4], sentinel[1][3] = ONES, ONES, ZERO
    sentinel[1][2] = np.array([0xFFFFFFFF, 0xFFFFFFFF, 0, 0, 0, 0, 0, 0], dtype=np.uint32)
    forest = forest_trees()
    return [Case("one tree", *lay([random_leaves(rng, 1500)], 3, 5), 1500),
            Case("one leaf", *lay([random_leaves(rng, 1)]), 1),
            Case("one leaf behind empty trees", *lay([[], [], random_leaves(rng, 1), []], 2, 2), 1),
            Case("every tree empty", *lay([[], [], []], 4, 4), 1),
            Case("257 trees of 0 to 3 leaves", *lay([random_leaves(rng, c) for c in many], 1, 3), 3),
            Case("max_count 1 000 times too large", *lay(forest, *PLACEMENTS[1]), 1000 * max(COUNTS)),
            Case("keys that equal the sentinel: the last of two trees, P = 63", *lay(sentinel, 3, 50), 1 << 40),
            Case("keys that equal the sentinel: one tree, P = 64", *lay(sentinel[1:], 0, 1500), 1 << 28)]


def all_cases():
    return forest_cases() + shape_cases()


def tie_batch(extra=0):
    """One tree of MAX_TIES + extra leaves under ONE 64-bit prefix: one run, the worst case of the place step."""
    n = max_ties() + extra
    rows = random_leaves(np.random.default_rng(703 + extra), n)
    rows[:, 0], rows[:, 1] = 0xC0FFEE00, 0x00C0FFEE
    rows[n // 2] = rows[n // 3]                                                       # and one repeat in it
    return Case(f"{n} leaves in one run", *lay([rows]), n)


# ---- the CPU twins (libvkmr_host.so) --------------------------------------------------------------------------------------------------

def _ptr(a):
    return a.ctypes.data if a.size else None


def host_sort(cells, offsets, max_count, with_order=True):
    """(rc, out, order, info) of vkmr_host_cpu_forest_sort_leaves; the outputs start as the canary."""
    import vk_merkle_roots_amd as vk
    cells, offsets = np.ascontiguousarray(cells, dtype=np.uint32).reshape(-1, 8), np.ascontiguousarray(offsets, dtype=np.uint64)
    total = int(cells.shape[0])
    out, order, info = np.full((total, 8), CANARY, np.uint32), np.full(total, CANARY, np.uint32), np.full(4, INFO_FILL, np.uint64)
    rc = vk.host_lib().vkmr_host_cpu_forest_sort_leaves(_ptr(cells), total, offsets.ctypes.data, int(offsets.shape[0]) - 1, int(max_count), _ptr(out),
                                                        _ptr(order) if with_order else None, info.ctypes.data)
    return rc, out, order, info


def host_tree_sort(rows):
    """(rc, out, order, info) of vkmr_host_cpu_tree_sort_leaves."""
    import vk_merkle_roots_amd as vk
    rows = np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1, 8)
    n = int(rows.shape[0])
    out, order, info = np.full((n, 8), CANARY, np.uint32), np.full(n, CANARY, np.uint32), np.full(4, INFO_FILL, np.uint64)
    rc = vk.host_lib().vkmr_host_cpu_tree_sort_leaves(_ptr(rows), n, _ptr(out), _ptr(order), info.ctypes.data)
    return rc, out, order, info


# ---- the replay -----------------------------------------------------------------------------------------------------------------------

def build_leafsort_plan_exe(directory):
    """tests/c/leafsort_plan_test.cpp as a program of its own, with AddressSanitizer and UBSan."""
    exe = os.path.join(str(directory), "leafsort_plan_test_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "vk_merkle_roots_amd", "csrc"), os.path.join(ROOT, "tests", "c", "leafsort_plan_test.cpp"), "-o", exe])
    return exe
