"""The audit of a stored forest or tree (vkmr_hip_forest_audit_async, vkmr_hip_tree_audit_async, vkmr_host_cpu_forest_audit,
vkmr_host_cpu_tree_audit) restated with hashlib on host arrays, the shapes the CPU and GPU tests share, and the
single-cell corruptions they apply.  A plain module: no fixtures, no GPU.

The rule.  With S(0, i) leaf i of tree t and S(l, j), 1 <= l <= h_t, the STORED cell of node j of tree t's level l, node
(t, l, j) is bad when S(l, j) != SHA-256d(S(l - 1, 2j) || S(l - 1, min(2j + 1, n_{l-1} - 1))): the children as they are stored,
not as a rebuild would make them.  An empty tree's one checkable node (t, 1, 0) is bad when roots[t] is not all zero.

`Forest` and `Tree` mirror the device layout (forest_plan.hpp, tree_plan.hpp) in three / two host arrays, so that a test can
write one cell on both sides and compare everything the call returns.  Cells that are no node of a tree hold PADDING."""
import hashlib

import numpy as np

from merkle_model import tree_height

PADDING = 0x5A5A5A5A


def _bytes(cell):
    return np.asarray(cell, dtype=np.uint32).astype(">u4").tobytes()


def hash_pair(l, r):
    """SHA-256d(l || r) of two word-valued cells, as 8 words."""
    d = hashlib.sha256(hashlib.sha256(_bytes(l) + _bytes(r)).digest()).digest()
    return np.frombuffer(d, dtype=">u4").astype(np.uint32)


def level_count(c, l):
    return 0 if c == 0 else ((c - 1) >> l) + 1


def right_child(j, n):
    return 2 * j + 1 if 2 * j + 1 < n else 2 * j


class Report:
    """What an audit returns: the four counters, the masks and the (cut) list."""

    def __init__(self, bad, masks, checked, capacity, forest):
        self.n_bad, self.checked, self.masks = len(bad), checked, np.asarray(masks, dtype=np.uint64)
        self.flagged = int(np.count_nonzero(self.masks)) if forest else int(self.masks[0])
        self.status = 4 if capacity and self.n_bad > capacity else 0
        cut = bad[: min(self.n_bad, capacity or 0)]
        self.trees = np.array([t for _, t, _ in cut], dtype=np.uint32)
        self.levels = np.array([l for l, _, _ in cut], dtype=np.uint32)
        self.nodes = np.array([j for _, _, j in cut], dtype=np.uint64)
        self.info = np.array([self.status, self.n_bad, self.flagged, self.checked], dtype=np.uint64)


class Forest:
    """A stored forest on the host: `leaves` [total, 8] (tree t at cells offsets[t] .. offsets[t+1]; `first` cells in front of
    tree 0 and `slack` behind the last are no leaves), `forest` [stored cells, 8] and `roots` [ntrees, 8]."""

    def __init__(self, counts, seed=0, first=0, slack=0, max_count=None):
        self.counts = [int(c) for c in counts]
        self.ntrees = len(self.counts)
        self.offsets = np.zeros(self.ntrees + 1, dtype=np.uint64)
        self.offsets[0] = first
        np.cumsum(np.asarray(self.counts, dtype=np.uint64), out=self.offsets[1:])
        self.offsets[1:] += np.uint64(first)
        self.total = int(self.offsets[-1]) + slack
        self.max_count = int(max_count) if max_count is not None else max(max(self.counts, default=0), 1)
        m = min(self.max_count, self.total)
        self.levels = 1 if m <= 1 else tree_height(m)
        rng = np.random.default_rng(seed)
        self.leaves = rng.integers(0, 2**32, size=(self.total, 8), dtype=np.uint32)
        self.forest = np.full((self.level_base(self.levels + 1), 8), PADDING, dtype=np.uint32)
        self.roots = np.full((self.ntrees, 8), PADDING, dtype=np.uint32)
        self.build()

    # -- forest_plan.hpp ------------------------------------------------------------------------------------------------------
    def level_cells(self, l):
        return (self.total >> l) + self.ntrees

    def level_base(self, l):
        return sum(self.level_cells(j) for j in range(1, l))

    def pos(self, t, l):
        o = int(self.offsets[t])
        return o if l == 0 else (o >> l) + t

    def height(self, t):
        return tree_height(self.counts[t]) if self.counts[t] else 1

    def cell(self, t, l, j):
        """(array, index) of S(l, j) of tree t: the leaves, the roots or the level buffers."""
        if l == 0:
            return self.leaves, self.pos(t, 0) + j
        if l == self.height(t):
            return self.roots, t
        return self.forest, self.level_base(l) + self.pos(t, l) + j

    def get(self, t, l, j):
        a, i = self.cell(t, l, j)
        return a[i]

    def want(self, t, l, j):
        """What S(l, j) must be, from the stored cells beneath it."""
        if self.counts[t] == 0:
            return np.zeros(8, dtype=np.uint32)
        n_in = level_count(self.counts[t], l - 1)
        return hash_pair(self.get(t, l - 1, 2 * j), self.get(t, l - 1, right_child(j, n_in)))

    def node_ids(self):
        """Every checkable node as (l, t, j), in the order of the list."""
        for l in range(1, self.levels + 1):
            for t, c in enumerate(self.counts):
                if l <= self.height(t):
                    for j in range(level_count(c, l) if c else 1):
                        yield l, t, j

    def build(self):
        for l, t, j in self.node_ids():
            a, i = self.cell(t, l, j)
            a[i] = self.want(t, l, j)

    def rehash_above(self, t, l, j):
        """Every ancestor of node (l, j) of tree t formed again from the stored cells: a forgery made consistent."""
        for up in range(l + 1, self.height(t) + 1):
            j >>= 1
            a, i = self.cell(t, up, j)
            a[i] = self.want(t, up, j)

    def is_bad(self, l, t, j):
        return not np.array_equal(self.get(t, l, j), self.want(t, l, j))

    def audit(self, capacity=0, only=None):
        """The Report of the rule over every node; `only`: the (l, t, j) that may be bad (a structure known to be consistent but
        for cells whose own node and parent they are), the others being counted unread."""
        ids = list(self.node_ids())
        if only is not None:
            only = sorted(n for n in set(only) if 1 <= n[0] <= self.height(n[1]) and n[2] < max(level_count(self.counts[n[1]], n[0]), 1))
        bad = [n for n in (ids if only is None else only) if self.is_bad(*n)]
        masks = [0] * self.ntrees
        for l, t, _ in bad:
            masks[t] |= 1 << (l - 1)
        return Report(bad, masks, len(ids), capacity, True)

    def arrays(self):
        return self.leaves, self.forest, self.roots


class Tree:
    """One stored tree on the host: `leaves` [count, 8] and `tree` [cells, 8], levels 1 .. height back to back (tree_plan.hpp);
    a level above ceil(log2 count) is one node, hash(a, a) of the node below."""

    def __init__(self, count, height=None, seed=0, leaves=None):
        self.count = int(count)
        self.height = tree_height(count) if height is None else int(height)
        self.leaves = np.random.default_rng(seed).integers(0, 2**32, size=(count, 8), dtype=np.uint32) if leaves is None else leaves
        self.off = [0] * (self.height + 2)
        for l in range(1, self.height + 1):
            self.off[l + 1] = self.off[l] + self.level_size(l)
        self.tree = np.full((self.off[self.height + 1], 8), PADDING, dtype=np.uint32)
        if leaves is None:
            self.build()

    def level_size(self, l):
        return -(-self.count >> l)

    def cell(self, l, j):
        return (self.leaves, j) if l == 0 else (self.tree, self.off[l] + j)

    def get(self, l, j):
        a, i = self.cell(l, j)
        return a[i]

    def want(self, l, j):
        return hash_pair(self.get(l - 1, 2 * j), self.get(l - 1, right_child(j, self.level_size(l - 1))))

    def node_count(self):
        return self.off[self.height + 1]

    def node_ids(self):
        for l in range(1, self.height + 1):
            for j in range(self.level_size(l)):
                yield l, 0, j

    def build(self):
        for l, _, j in self.node_ids():
            self.tree[self.off[l] + j] = self.want(l, j)

    def rehash_above(self, l, j):
        for up in range(l + 1, self.height + 1):
            j >>= 1
            self.tree[self.off[up] + j] = self.want(up, j)

    def is_bad(self, l, _t, j):
        return not np.array_equal(self.get(l, j), self.want(l, j))

    def audit(self, capacity=0, only=None):
        if only is not None:
            only = sorted(n for n in set(only) if 1 <= n[0] <= self.height and n[2] < self.level_size(n[0]))
        bad = [n for n in (self.node_ids() if only is None else only) if self.is_bad(*n)]
        mask = 0
        for l, _, _ in bad:
            mask |= 1 << (l - 1)
        return Report(bad, [mask], self.node_count(), capacity, False)


def touched(ids):
    """The nodes whose verdict a write to the cells `ids` ((l, t, j), l = 0 a leaf) can change: each cell's own node and its
    parent.  Levels outside the tree are dropped by the caller's shape."""
    out = []
    for l, t, j in ids:
        if l >= 1:
            out.append((l, t, j))
        out.append((l + 1, t, j >> 1))
    return out


# ---- the shapes ---------------------------------------------------------------------------------------------------------------
# Forests: (name, counts, first offset, slack).  Level l of tree t starts at cell (offsets[t] >> l) + t: the counts below put a
# tree's first cell inside a wavefront at level 1 and at level 2, and a wavefront boundary inside a tree.
FORESTS = [
    ("tiny", [0, 1, 2, 3], 0, 0),
    ("around_64", [63, 64, 65], 0, 0),
    ("around_128", [127, 128, 129], 0, 0),
    ("begins_inside_a_wavefront", [70, 200, 9, 300, 5], 0, 0),
    ("first_offset", [5, 0, 66, 3], 37, 11),
    ("one_tree", [77], 0, 0),
    ("one_leaf", [1], 0, 0),
    ("no_leaf", [0, 0, 0], 0, 0),
    ("mixed_1_to_4095", [1, 4095, 2, 1024, 3, 129, 0, 1000, 64, 2049, 7, 513], 0, 0),
]

# Trees: (count, height); None: the count's own.  600 001 is past every power-of-two edge and ragged on most levels.
TREES = [(1, 1), (2, None), (3, None), (5, None), (64, None), (65, None), (5, 6), (65, 9)]
BIG_TREE = (600001, None)


def flip(struct, where, word=3, bit=0x00010000):
    """One bit of one stored cell flipped, on the host mirror: `where` is (array, index) of Forest.cell / Tree.cell."""
    a, i = where
    a[i, word] ^= np.uint32(bit)


def forest_corruptions(f):
    """[(name, cells written as (l, t, j), a function that writes them into the mirror, expected number of bad nodes or None)]
    for a built Forest: every kind of single-cell damage the shape has room for."""
    out = []
    live = [t for t, c in enumerate(f.counts) if c]
    odd = [t for t in live if f.counts[t] % 2 == 1 and f.counts[t] > 1]
    tall = [t for t in live if f.height(t) >= 2]

    def write(ids):
        def go():
            for l, t, j in ids:
                flip(f, f.cell(t, l, j))
        return go

    if live:
        out.append(("first_leaf", [(0, live[0], 0)], 1))
        out.append(("a_root", [(f.height(live[-1]), live[-1], 0)], 1))
    if odd:
        out.append(("last_leaf_of_an_odd_tree", [(0, odd[0], f.counts[odd[0]] - 1)], 1))
    for t in tall:
        for l in range(1, f.height(t)):
            n = level_count(f.counts[t], l)
            if n % 2 == 1 and n > 1:
                out.append((f"ragged_edge_t{t}_l{l}", [(l, t, n - 1)], 2))
                break
    if tall:
        t = max(tall, key=f.height)
        for l in range(1, f.height(t)):
            out.append((f"inner_t{t}_l{l}", [(l, t, level_count(f.counts[t], l) // 2)], 2))
        out.append((f"siblings_t{t}", [(1, t, 0), (1, t, 1)], 3))
    empty = [t for t, c in enumerate(f.counts) if c == 0]
    if empty:
        out.append(("an_empty_trees_root", [(1, empty[0], 0)], 1))
    out = [(name, ids, write(ids), n) for name, ids, n in out]
    if tall:
        t = max(tall, key=f.height)
        j = level_count(f.counts[t], 1) - 1

        def forge():
            flip(f, f.cell(t, 1, j))
            f.rehash_above(t, 1, j)
        out.append((f"consistent_forgery_t{t}", [(l, t, j >> (l - 1)) for l in range(1, f.height(t) + 1)], forge, 1))
    pads = np.flatnonzero((f.forest == PADDING).all(axis=1))
    if pads.size:
        def pad():
            f.forest[pads[pads.size // 2], 0] ^= np.uint32(1)
        out.append(("a_padding_cell", [], pad, 0))
    return out


def tree_corruptions(tr):
    out = [("first_leaf", [(0, 0, 0)], 1), ("the_root", [(tr.height, 0, 0)], 1)]
    if tr.count % 2 == 1 and tr.count > 1:
        out.append(("last_leaf", [(0, 0, tr.count - 1)], 1))
    for l in range(1, tr.height):
        n = tr.level_size(l)
        out.append((f"inner_l{l}", [(l, 0, n // 2)], 2))
        if n % 2 == 1 and n > 1:
            out.append((f"ragged_edge_l{l}", [(l, 0, n - 1)], 2))
    if tr.level_size(1) >= 2 and tr.height >= 2:
        out.append(("siblings", [(1, 0, 0), (1, 0, 1)], 3))

    def write(ids):
        def go():
            for l, _, j in ids:
                flip(tr, tr.cell(l, j))
        return go

    out = [(name, ids, write(ids), n) for name, ids, n in out]
    if tr.height >= 2:
        j = tr.level_size(1) - 1

        def forge():
            flip(tr, tr.cell(1, j))
            tr.rehash_above(1, j)
        out.append(("consistent_forgery", [(l, 0, j >> (l - 1)) for l in range(1, tr.height + 1)], forge, 1))
    return out


# ---- the CPU counterparts -----------------------------------------------------------------------------------------------------
GUARD = 8              # cells of pattern on both sides of every output
FILL32, FILL64 = 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5


def _ptr(a):
    return a.ctypes.data if a.size else None


def host_forest_audit(f, capacity, max_count=None, offsets=None):
    """(return code, Report-like arrays) of vkmr_host_cpu_forest_audit on the mirror `f`; outputs pre-filled, guards checked."""
    import vk_merkle_roots_amd as vk
    masks = np.full(f.ntrees + 2 * GUARD, FILL64, dtype=np.uint64)
    trees, levels = (np.full(capacity + 2 * GUARD, FILL32, dtype=np.uint32) for _ in range(2))
    nodes = np.full(capacity + 2 * GUARD, FILL64, dtype=np.uint64)
    info = np.full(4, FILL64, dtype=np.uint64)
    offsets = f.offsets if offsets is None else np.ascontiguousarray(offsets, dtype=np.uint64)
    before = [a.copy() for a in f.arrays()]
    rc = vk.host_lib().vkmr_host_cpu_forest_audit(_ptr(f.leaves), _ptr(f.forest), _ptr(f.roots), f.total, offsets.ctypes.data, f.ntrees,
                                                  f.max_count if max_count is None else max_count, masks[GUARD:].ctypes.data,
                                                  trees[GUARD:].ctypes.data if capacity else None, levels[GUARD:].ctypes.data if capacity else None,
                                                  nodes[GUARD:].ctypes.data if capacity else None, capacity, info.ctypes.data)
    assert all(np.array_equal(a, b) for a, b in zip(f.arrays(), before)), "the audit wrote to the structure"
    for a, fill, n in ((masks, FILL64, f.ntrees), (trees, FILL32, capacity), (levels, FILL32, capacity), (nodes, FILL64, capacity)):
        assert (a[:GUARD] == fill).all() and (a[GUARD + n:] == fill).all(), "guard words"
    return rc, info, masks[GUARD: GUARD + f.ntrees], trees[GUARD: GUARD + capacity], levels[GUARD: GUARD + capacity], nodes[GUARD: GUARD + capacity]


def host_tree_audit(tr, capacity):
    import vk_merkle_roots_amd as vk
    levels = np.full(capacity + 2 * GUARD, FILL32, dtype=np.uint32)
    nodes = np.full(capacity + 2 * GUARD, FILL64, dtype=np.uint64)
    info = np.full(4, FILL64, dtype=np.uint64)
    before = tr.leaves.copy(), tr.tree.copy()
    rc = vk.host_lib().vkmr_host_cpu_tree_audit(_ptr(tr.leaves), _ptr(tr.tree), tr.count, tr.height, levels[GUARD:].ctypes.data if capacity else None,
                                                nodes[GUARD:].ctypes.data if capacity else None, capacity, info.ctypes.data)
    assert np.array_equal(tr.leaves, before[0]) and np.array_equal(tr.tree, before[1]), "the audit wrote to the structure"
    for a, fill in ((levels, FILL32), (nodes, FILL64)):
        assert (a[:GUARD] == fill).all() and (a[GUARD + capacity:] == fill).all(), "guard words"
    return rc, info, levels[GUARD: GUARD + capacity], nodes[GUARD: GUARD + capacity]


def assert_matches(want, info, masks, trees, levels, nodes, what=""):
    """Everything an audit wrote against the model's Report: the counters, the masks, the list up to min(n, capacity), and the
    fill pattern behind it."""
    assert [int(x) for x in info] == [int(x) for x in want.info], (what, list(info), list(want.info))
    if masks is not None:
        assert np.array_equal(masks, want.masks), (what, masks, want.masks)
    m = want.trees.shape[0]
    if trees is not None:
        assert np.array_equal(trees[:m], want.trees) and (trees[m:] == FILL32).all(), (what, trees, want.trees)
    assert np.array_equal(levels[:m], want.levels) and (levels[m:] == FILL32).all(), (what, levels, want.levels)
    assert np.array_equal(nodes[:m], want.nodes) and (nodes[m:] == FILL64).all(), (what, nodes, want.nodes)
