"""The lookup by digest (vkmr_hip_forest_find_async, vkmr_hip_tree_find_async and their CPU twins) restated as a Python dict of
first occurrences, and the case tables tests/test_find_abi.py and tests/test_gpu_find.py share.  A plain module: no fixtures,
no GPU.

A case is a Case: the cells of a digests buffer, the offsets of the trees inside it, the queries, and the model's answer."""
import bisect
import functools
import os
import re
import zlib

import numpy as np

import forest_cases as fc
import merkle_model

NO_TREE = 0xFFFFFFFF
NOT_FOUND = 0xFFFFFFFFFFFFFFFF
ZERO = np.zeros(8, dtype=np.uint32)
ONES = np.full(8, 0xFFFFFFFF, dtype=np.uint32)


# ---- the sizes of csrc/find_plan.hpp, restated / read ----------------------------------------------------------------------

def plan_constants():
    """{name: value} of the VKMR_FIND_* launch constants, read from the header's text."""
    text = open(os.path.join(merkle_model.ROOT, "vk_merkle_roots_amd", "csrc", "find_plan.hpp")).read()
    return {name: int(value) for name, value in re.findall(r"#define\s+(VKMR_FIND_\w+)\s+(\d+)u?\b", text)}


def table_slots(k):
    """The smallest power of two >= max(64, 2k)."""
    t = 64
    while t < 2 * k:
        t *= 2
    return t


def scratch_bytes(k):
    """T slots of 8 bytes, k best positions of 8, k representatives of 4; in whole 16-byte units."""
    return (8 * table_slots(k) + 8 * k + 4 * k + 15) // 16 * 16


def second_trip_total(compute_units):
    """The smallest number of leaves at which one workgroup of the scan, its grid capped for `compute_units`, takes a second
    trip of its grid-stride loop: one leaf more than the capped grid covers in one."""
    c = plan_constants()
    return compute_units * c["VKMR_FIND_GROUPS_PER_CU"] * c["VKMR_FIND_THREADS"] * c["VKMR_FIND_LEAVES_PER_LANE"] + 1


# ---- the model --------------------------------------------------------------------------------------------------------------

def model(cells, offsets, queries):
    """(trees uint32 [k], indices uint64 [k]): for every query the lowest flat position p in [offsets[0], offsets[-1]) whose
    cell equals it, as the tree that holds p and p's index inside it; NO_TREE and NOT_FOUND when there is none.  A dict of
    first occurrences; `offsets` may be empty or hold one entry (no tree)."""
    off = [int(x) for x in offsets]
    lo, hi = (off[0], off[-1]) if len(off) >= 2 else (0, 0)
    raw = np.ascontiguousarray(cells, dtype=np.uint32).tobytes()
    keys = [raw[32 * p: 32 * p + 32] for p in range(hi - 1, lo - 1, -1)]
    first = dict(zip(keys, range(hi - 1, lo - 1, -1)))         # descending positions: the lowest is written last
    queries = np.ascontiguousarray(queries, dtype=np.uint32).reshape(-1, 8)
    trees = np.full(queries.shape[0], NO_TREE, dtype=np.uint32)
    indices = np.full(queries.shape[0], NOT_FOUND, dtype=np.uint64)
    for q in range(queries.shape[0]):
        p = first.get(queries[q].tobytes())
        if p is not None:
            t = bisect.bisect_right(off, p) - 1                # the last tree that starts at or before p: never an empty one
            trees[q], indices[q] = t, p - off[t]
    return trees, indices


class Case:
    def __init__(self, cells, offsets, queries, notes=None):
        self.cells = np.ascontiguousarray(cells, dtype=np.uint32).reshape(-1, 8)
        self.offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        self.queries = np.ascontiguousarray(queries, dtype=np.uint32).reshape(-1, 8)
        self.total, self.ntrees, self.k = int(self.cells.shape[0]), int(self.offsets.shape[0]) - 1, int(self.queries.shape[0])
        self.notes = notes or {}
        self.trees, self.indices = model(self.cells, self.offsets, self.queries)

    def found(self):
        return self.trees != NO_TREE


def seed_of(*parts):
    return zlib.crc32(repr(parts).encode())


# ---- forests with the full query set ------------------------------------------------------------------------------------------

# the count tables of forest_cases that put tree starts inside wavefronts (the first two), fill wavefronts with one tree (the
# next two) and mix empty trees in (the rest); then (first offset, slack behind the last tree, counts) of the two forests of
# this module: a window inside the buffer, and empty trees in front, behind and side by side
FORESTS = {name: (0, 0, fc.CASES[name]) for name in ("power_of_two_edges", "sizes_1_to_130", "one_tree_of_5000", "one_big_among_small",
                                                      "empty_first", "empty_last", "empty_adjacent")}
FORESTS["window"] = (7, 9, [5, 130, 0, 64, 1, 77])
FORESTS["empties_everywhere"] = (0, 0, [0, 0, 5, 0, 0, 0, 3, 64, 0, 130, 0, 0])
VARIANTS = ("zero_is_a_leaf", "ones_is_a_leaf")       # the other of the two is queried all the same, and is absent


@functools.lru_cache(maxsize=None)
def forest_case(name, variant):
    """The forest `name` with the whole query set planted.  notes: name -> query number(s), for the tests that point at one."""
    first, slack, counts = FORESTS[name]
    rng = np.random.default_rng(seed_of(name, variant))
    off = fc.offsets_of(counts) + np.uint64(first)
    lo, hi = int(off[0]), int(off[-1])
    total = hi + slack
    cells = merkle_model.random_leaves(rng, total)
    live = [t for t, c in enumerate(counts) if c]
    starts = {int(off[t]) for t in live} | {int(off[t + 1]) - 1 for t in live}
    free = [int(p) for p in rng.permutation(np.arange(lo, hi)) if int(p) not in starts]       # cells to plant in, each used once
    queries, notes = [], {}

    def ask(what, digest):
        notes.setdefault(what, []).append(len(queries))
        queries.append(np.array(digest, dtype=np.uint32))

    # planted first, so that everything read from the cells below is final
    special = ZERO if variant == "zero_is_a_leaf" else ONES
    cells[free.pop()] = special
    twice = merkle_model.random_leaves(rng, 2)
    big = max(live, key=lambda t: counts[t])                   # two positions of one tree
    inside = [p for p in free if int(off[big]) <= p < int(off[big + 1])][:2]
    for p in inside:
        cells[p] = twice[0]
        free.remove(p)
    room, starts_of = {}, [int(x) for x in off]                # and two different trees, where two have a cell to spare
    for p in free:
        if len(room) == 2:
            break
        t = bisect.bisect_right(starts_of, p) - 1
        if t != big:
            room.setdefault(t, p)
    others = sorted(room) if len(room) == 2 else []
    for t in others:
        cells[room[t]] = twice[1]
        free.remove(room[t])
    if slack:                                                  # the cells outside the window carry a digest that is queried
        outside = merkle_model.random_leaves(rng, 1)[0]
        cells[:lo] = outside
        cells[hi:] = outside
        ask("outside_the_window", outside)
        cells[lo - 1], cells[hi] = cells[lo + 3], cells[hi - 4]       # and leaves of the window again, just outside it
    ask("first_of_forest", cells[lo])
    ask("last_of_forest", cells[hi - 1])
    mid = live[len(live) // 2]
    ask("first_of_a_tree", cells[int(off[mid])])
    ask("last_of_a_tree", cells[int(off[mid + 1]) - 1])
    beside = [t for t in live if (t > 0 and counts[t - 1] == 0) or (t + 1 < len(counts) and counts[t + 1] == 0)]
    for t in beside[:2]:
        ask("beside_an_empty_tree", cells[int(off[t])])
        ask("beside_an_empty_tree", cells[int(off[t + 1]) - 1])
    for d in merkle_model.random_leaves(rng, 8):
        ask("absent", d)
    near = cells[free.pop()].copy()
    near[7] ^= 1                                               # slot and tag match: the full compare must reject it
    ask("absent_but_for_word_7", near)
    near = cells[free.pop()].copy()
    near[0] ^= 0x80000000
    ask("absent_but_for_word_0", near)
    ask("zero", ZERO)
    ask("ones", ONES)
    again = cells[free.pop()].copy()
    for _ in range(3):
        ask("three_times", again)
    ask("twice_in_one_tree", twice[0])
    ask("in_two_trees", twice[1])
    small = min((t for t in live if counts[t] >= 2), key=lambda t: counts[t], default=live[0])
    levels = merkle_model.cpu_levels(cells[int(off[small]): int(off[small + 1])])
    ask("a_root", levels[-1][0])
    ask("a_level_1_node", levels[1][0])
    order = rng.permutation(len(queries))
    case = Case(cells, off, np.stack(queries)[order], {what: [int(np.nonzero(order == q)[0][0]) for q in qs] for what, qs in notes.items()})
    case.counts, case.inside, case.big, case.others = counts, sorted(inside), big, others
    return case


# ---- chains: k queries that all start at one slot -----------------------------------------------------------------------------

CHAIN_K = (1, 2, 31, 32, 33, 1000)        # T doubles between 32 and 33: both sit at the edge of the load-factor bound
CHAIN_COUNTS = [100, 0, 157, 300]


@functools.lru_cache(maxsize=None)
def chain_case(k, wrap, parity):
    """k queries with one word 0, so that they form one chain of k slots -- from slot 5, or with `wrap` from the table's last
    slot, so that the chain goes round its end.  Query q is a leaf iff q % 2 == parity: the last one in one parity, not in the
    other.  Leaves that share the word but equal no query walk the whole chain for nothing."""
    rng = np.random.default_rng(seed_of("chain", k, wrap, parity))
    word0 = 0xABCD0000 | ((table_slots(k) - 1) if wrap else 5)
    off = fc.offsets_of(CHAIN_COUNTS)
    cells = merkle_model.random_leaves(rng, int(off[-1]))
    queries = merkle_model.random_leaves(rng, k)
    queries[:, 0] = word0
    where = rng.permutation(int(off[-1]))
    present = [q for q in range(k) if q % 2 == parity]
    for i, q in enumerate(present):
        cells[where[i % where.shape[0]]] = queries[q]          # k = 1000: more plants than cells, a later one overwrites an earlier one
    for p in where[-10:]:
        cells[p, 0] = word0                                    # these only share the chain (and may undo a plant: the model says)
    return Case(cells, off, queries, {"present": present})


# ---- every leaf equal ---------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def all_equal_case():
    counts = [0, 0, 1200, 0, 800, 3000]
    rng = np.random.default_rng(seed_of("all_equal"))
    d = merkle_model.random_leaves(rng, 1)[0]
    return Case(np.tile(d, (sum(counts), 1)), fc.offsets_of(counts), np.stack([d, merkle_model.random_leaves(rng, 1)[0], d]))


# ---- sizes ---------------------------------------------------------------------------------------------------------------------

TOTALS = (1, 63, 64, 65, 5000)
KS = (1, 63, 64, 65, 4097)


@functools.lru_cache(maxsize=None)
def size_case(total, k):
    """`total` random leaves in three trees, the middle one empty; k queries in random order, half of them leaves (the first
    and the last leaf among them), the rest absent."""
    rng = np.random.default_rng(seed_of("size", total, k))
    cells = merkle_model.random_leaves(rng, total)
    queries = merkle_model.random_leaves(rng, k)
    picks = np.concatenate([[0, total - 1], rng.integers(0, total, size=k)])[: (k + 1) // 2]
    queries[: picks.shape[0]] = cells[picks]
    return Case(cells, fc.offsets_of([total // 3, 0, total - total // 3]), queries[rng.permutation(k)])


# ---- the CPU twins -------------------------------------------------------------------------------------------------------------

def host_cpu_forest_find(case):
    """(return code, trees, indices) of vkmr_host_cpu_forest_find; the outputs start as a 0xA5 pattern."""
    import vk_merkle_roots_amd as vk
    trees = np.full(case.k, 0xA5A5A5A5, dtype=np.uint32)
    indices = np.full(case.k, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    rc = vk.host_lib().vkmr_host_cpu_forest_find(case.cells.ctypes.data if case.total else None, case.total, case.offsets.ctypes.data, case.ntrees,
                                                 case.queries.ctypes.data, case.k, trees.ctypes.data, indices.ctypes.data)
    return rc, trees, indices


def host_cpu_tree_find(cells, queries):
    """(return code, indices) of vkmr_host_cpu_tree_find over all of `cells`."""
    import vk_merkle_roots_amd as vk
    cells = np.ascontiguousarray(cells, dtype=np.uint32).reshape(-1, 8)
    queries = np.ascontiguousarray(queries, dtype=np.uint32).reshape(-1, 8)
    indices = np.full(queries.shape[0], 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    rc = vk.host_lib().vkmr_host_cpu_tree_find(cells.ctypes.data if cells.size else None, cells.shape[0], queries.ctypes.data, queries.shape[0],
                                               indices.ctypes.data)
    return rc, indices
