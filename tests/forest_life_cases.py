"""The life of a stored forest: ONE model of the whole MerkleForest in plain Python over hashlib, and a walk that puts every
operation directly after every other.  tests/test_forest_life_model.py (no GPU) anchors the model to the host library's CPU
twins along every walk and asserts that the walks reach what they are meant to reach; tests/test_gpu_forest_life.py drives a
resident forest, its twin and two followers through the same walks and compares everything they answer with the model.  A
plain module: no fixtures, no GPU.

ModelForest.  Its state is the capacity (ntrees, total, max_count), the leaves of every tree in use (`trees`, a list of
[c, 8] uint32 arrays; a dropped tree holds none) and the front (`dropped_trees`, `dropped_leaves`).  Everything else -- the
handle's books, the device's offsets, roots, every stored node and its cell, masks, frontiers, proofs, find's answers, the
audit's count -- is derived from that state alone.  `image` is level 0 as it lies in memory, stale cells included (leaves
behind used_leaves after a shrink or truncate, leaves in front after a drop_front): it is no state, only what the CPU twins
read and where find's questions about cells that no tree holds come from.

The open tree.  A tree dropped from the front is never the open tree: open_tree is None when used_trees == dropped_trees.

The walk.  CIRCUIT is a closed sequence of the eleven KINDS in which every ordered pair of kinds, each kind after itself
included, occurs once: an Eulerian circuit of the complete digraph, 121 steps; SEQUENCE repeats its first kind at the end so
that the 121 pairs are all performed.  Life(seed, config) draws each step's parameters from its seed, from the model's state
and from the kind that comes next in the fixed sequence -- never from what a device answered -- so every step is feasible;
where a kind has nothing it can do the step is performed in its degenerate form (an extend by 0, an append of no tree, a
refused extend where no tree is open) and counted.  The kind is never swapped for another.  The draws keep the forest alive:
growth steps aim at TARGET_LIVE live trees, a truncate or drop_front takes every tree where the next kind brings new ones, and
CIRCUIT_SEED and SEEDS are the circuit and the walks for which the model alone meets the conditions that
tests/test_forest_life_model.py asserts (every pair, at most a quarter of a kind's steps degenerate, every one of EVENTS)."""
import collections

import numpy as np

import audit_cases
import find_cases as fd
import forest_multiproof_cases as fm
import forest_mutation_cases as fmu
import frontier_cases as fr
from merkle_model import cpu_levels, digest_of, proof_path, stored_node_cell, tree_height

NO_TREE, NOT_FOUND = fd.NO_TREE, fd.NOT_FOUND
KINDS = ("update", "replace", "witness", "append", "truncate", "extend", "shrink", "drop_front", "repack", "append_from", "sync")
STRUCTURAL = ("append", "truncate", "extend", "shrink", "drop_front", "repack", "append_from")      # what the twin receives too
GROWTH = ("append", "extend", "append_from")
REFILLS = ("append", "append_from")       # a truncate or drop_front in front of one of these takes every tree: the next step brings new ones

_LEVELS = {}


def levels_of(leaves):
    """cpu_levels(leaves), kept per leaf list: a walk asks for the same trees step after step."""
    key = leaves.tobytes()
    if key not in _LEVELS:
        if len(_LEVELS) > 20000:
            _LEVELS.clear()
        _LEVELS[key] = cpu_levels(leaves.copy())          # a copy: an update writes into the tree's own array
        for level in _LEVELS[key]:
            level.setflags(write=False)
    return _LEVELS[key]


def _no_leaves():
    return np.zeros((0, 8), dtype=np.uint32)


class _Shape(audit_cases.Forest):
    """audit_cases.Forest for its node_ids() alone: the nodes an audit checks, nothing hashed."""

    def build(self):
        pass


class ModelForest:
    """A stored forest in plain Python: the module docstring says what is state and what is derived."""

    def __init__(self, ntrees, total, max_count, trees=()):
        self.ntrees, self.total, self.max_count = int(ntrees), int(total), int(max_count)
        self.trees = [np.array(t, dtype=np.uint32).reshape(-1, 8) for t in trees]
        self.dropped_trees = self.dropped_leaves = 0
        self.image = np.zeros((self.total, 8), dtype=np.uint32)
        self._settle()

    def copy(self):
        other = ModelForest(self.ntrees, self.total, self.max_count, self.trees)
        other.dropped_trees, other.dropped_leaves = self.dropped_trees, self.dropped_leaves
        other.image = self.image.copy()
        return other

    def _settle(self):
        """The checks every state passes, and the live leaves written into the image where they lie."""
        assert self.dropped_trees <= self.used_trees <= self.ntrees and self.used_leaves <= self.total
        assert all(t.shape[0] <= self.max_count for t in self.trees) and not any(t.shape[0] for t in self.trees[: self.dropped_trees])
        off = self.offsets()
        for t, leaves in enumerate(self.trees):
            self.image[int(off[t]): int(off[t + 1])] = leaves

    # ---- the handle's books ---------------------------------------------------------------------------------------------
    used_trees = property(lambda self: len(self.trees))
    counts = property(lambda self: [int(t.shape[0]) for t in self.trees] + [0] * (self.ntrees - len(self.trees)))
    live_leaves = property(lambda self: sum(self.counts))
    used_leaves = property(lambda self: self.dropped_leaves + self.live_leaves)
    free_trees = property(lambda self: self.ntrees - self.used_trees)
    free_leaves = property(lambda self: self.total - self.used_leaves)
    open_tree = property(lambda self: self.used_trees - 1 if self.used_trees > self.dropped_trees else None)
    levels = property(lambda self: tree_height(min(self.max_count, self.total)) if self.total else 1)
    frontier_stride = property(lambda self: max(1, min(self.max_count, self.total).bit_length()))

    def books(self):
        return {"ntrees": self.ntrees, "total": self.total, "max_count": self.max_count, "levels": self.levels, "counts": self.counts,
                "used_trees": self.used_trees, "dropped_trees": self.dropped_trees, "dropped_leaves": self.dropped_leaves,
                "used_leaves": self.used_leaves, "live_leaves": self.live_leaves, "free_trees": self.free_trees,
                "free_leaves": self.free_leaves, "open_tree": self.open_tree}

    # ---- what the device holds ------------------------------------------------------------------------------------------
    def offsets(self):
        """uint64 [ntrees + 1]: dropped trees where the first kept tree begins, trees not in use at used_leaves."""
        off = np.zeros(self.ntrees + 1, dtype=np.uint64)
        off[0] = self.dropped_leaves
        off[1:] = self.dropped_leaves + np.cumsum(self.counts)
        return off

    def tree_levels(self, t):
        return levels_of(self.trees[t])

    def roots(self):
        out = np.zeros((self.ntrees, 8), dtype=np.uint32)
        for t, leaves in enumerate(self.trees):
            if leaves.shape[0]:
                out[t] = self.tree_levels(t)[-1][0]
        return out

    def nodes(self):
        """(cells, digests): every live node of levels 1 .. h_t - 1 of every tree and the cell of the level buffers it lies at."""
        off = self.offsets()
        cells, digests = [], []
        for t, leaves in enumerate(self.trees):
            if leaves.shape[0]:
                lv = self.tree_levels(t)
                for l in range(1, len(lv) - 1):
                    for j in range(lv[l].shape[0]):
                        cells.append(stored_node_cell(self.total, self.ntrees, off[t], t, l, j))
                        digests.append(lv[l][j])
        assert len(set(cells)) == len(cells)
        return np.array(cells, dtype=np.int64), np.array(digests, dtype=np.uint32).reshape(-1, 8)

    def live_cells(self):
        """The cells of level 0 that hold a live leaf: [dropped_leaves, used_leaves)."""
        return np.arange(self.dropped_leaves, self.used_leaves, dtype=np.int64)

    def checked(self):
        """The nodes an audit hashes and compares: audit_cases.Forest's counting rule over this shape."""
        shape = _Shape(self.counts, first=self.dropped_leaves, slack=self.free_leaves, max_count=self.max_count)
        assert shape.total == self.total and shape.levels == self.levels
        return sum(1 for _ in shape.node_ids())

    def masks(self):
        out = np.zeros(self.ntrees, dtype=np.uint64)
        for t, leaves in enumerate(self.trees):
            if leaves.shape[0]:
                out[t] = fmu.tree_root_and_mask(leaves)[1]
        return out

    def frontier(self, stride=None):
        """(counts uint64 [ntrees], peaks [ntrees, stride, 8]) as frontier_cases.brute_frontier gives them tree by tree."""
        stride = self.frontier_stride if stride is None else stride
        peaks = np.zeros((self.ntrees, stride, 8), dtype=np.uint32)
        for t, leaves in enumerate(self.trees):
            peaks[t] = fr.brute_frontier(leaves, stride)[0]
        return np.array(self.counts, dtype=np.uint64), peaks

    def proofs(self, trees, indices):
        """(siblings [k, levels, 8], heights [k]); an entry that names no leaf gets height 0 and zero cells."""
        k, counts = len(trees), self.counts
        sib, heights = np.zeros((k, self.levels, 8), dtype=np.uint32), np.zeros(k, dtype=np.uint32)
        for q, (t, i) in enumerate(zip(trees, indices)):
            t, i = int(t), int(i)
            if t < self.ntrees and i < counts[t]:
                lv = self.tree_levels(t)
                heights[q] = len(lv) - 1
                sib[q, : len(lv) - 1] = proof_path(lv, i, len(lv) - 1)
        return sib, heights

    def find(self, queries):
        """(trees, indices): the lowest position among the leaves that live trees hold; the image's other cells never answer."""
        return fd.model(self.image, self.offsets(), queries)

    def multiproof(self, trees, indices):
        """(nodes, heights, level counts) of sorted in-range entries, by forest_multiproof_cases.make over the live leaves."""
        nodes, heights, level_counts, _ = fm.make(self.image, self.offsets(), trees, indices, self.levels)
        return nodes, heights, level_counts

    def entries(self):
        """Every live leaf as (tree, index), in order."""
        return [(t, i) for t, c in enumerate(self.counts) for i in range(c)]

    def leaves_at(self, trees, indices):
        off = self.offsets().astype(np.int64)
        return self.image[off[np.asarray(trees, dtype=np.int64)] + np.asarray(indices, dtype=np.int64)]

    def stale_digests(self):
        """The digests that lie in a cell no tree holds -- in front of dropped_leaves or behind used_leaves -- and in no live
        leaf: what find must not answer with."""
        live = {d.tobytes() for d in self.image[self.dropped_leaves: self.used_leaves]}
        out = {}
        for cell in np.concatenate([self.image[: self.dropped_leaves], self.image[self.used_leaves:]]):
            if cell.any() and cell.tobytes() not in live:
                out.setdefault(cell.tobytes(), cell)
        return list(out.values())

    # ---- the mutating operations, with the Python layer's semantics ---------------------------------------------------------
    def update(self, trees, indices, values):
        """Entries in call order, a repeated pair taking its last value; a NO_TREE marker is left out.  (leaves written,
        markers, repeats dropped): what update_entries counts."""
        last, markers, n = {}, 0, 0
        for t, i, v in zip(trees, indices, values):
            if int(t) == NO_TREE:
                markers += 1
                continue
            assert int(t) >= self.dropped_trees and int(i) < self.counts[int(t)], (t, i)
            last[(int(t), int(i))] = v
            n += 1
        for (t, i), v in last.items():
            self.trees[t][i] = v
        self._settle()
        return len(last), markers, n - len(last)

    def replace(self, old, new):
        """find's lowest position of each old digest, on the forest as it is before the call, takes the new one; two equal old
        digests take the last.  (leaves written, old digests that are no leaf)."""
        trees, indices = self.find(old)
        applied, missing, _ = self.update(trees, indices, new)
        return applied, missing

    def append(self, new_trees):
        new_trees = [np.array(t, dtype=np.uint32).reshape(-1, 8) for t in new_trees]
        assert len(new_trees) <= self.free_trees and sum(t.shape[0] for t in new_trees) <= self.free_leaves
        first = self.used_trees
        self.trees += new_trees
        self._settle()
        return list(range(first, first + len(new_trees)))

    def truncate(self, keep):
        assert self.dropped_trees <= keep <= self.used_trees
        del self.trees[keep:]
        self._settle()

    def extend(self, leaves):
        t = self.open_tree
        assert t is not None and leaves.shape[0] <= self.free_leaves
        self.trees[t] = np.concatenate([self.trees[t], np.asarray(leaves, dtype=np.uint32).reshape(-1, 8)])
        self._settle()
        return self.counts[t]

    def shrink(self, r):
        t = self.open_tree
        assert t is not None and r <= self.counts[t]
        self.trees[t] = self.trees[t][: self.counts[t] - r].copy()
        self._settle()
        return self.counts[t]

    def drop_front(self, k):
        assert k <= self.used_trees
        for t in range(self.dropped_trees, k):
            self.dropped_leaves += self.counts[t]
            self.trees[t] = _no_leaves()
        self.dropped_trees = max(self.dropped_trees, k)
        self._settle()

    def repacked(self, trees=None, reserve_trees=0, reserve_leaves=0):
        """A new model of trees `trees` (the trees in use that were not dropped when None) with fresh reserves."""
        sel = list(range(self.dropped_trees, self.used_trees)) if trees is None else [int(t) for t in trees]
        chosen = [self.trees[t] if t < self.used_trees else _no_leaves() for t in sel]
        return ModelForest(len(sel) + reserve_trees, sum(t.shape[0] for t in chosen) + reserve_leaves, self.max_count, chosen)

    def append_from(self, src, sel):
        return self.append([src.trees[int(t)] if int(t) < src.used_trees else _no_leaves() for t in sel])

    def diff(self, other):
        """(trees, indices) of the live leaves in which this forest and `other`, of the same shape, differ."""
        assert self.counts == other.counts and self.dropped_leaves == other.dropped_leaves and self.total == other.total
        pairs = [(t, i) for t, i in self.entries() if (self.trees[t][i] != other.trees[t][i]).any()]
        return np.array([t for t, _ in pairs], dtype=np.uint32), np.array([i for _, i in pairs], dtype=np.uint64)

    def sync_from(self, other):
        n = int(self.diff(other)[0].shape[0])
        self.trees = [t.copy() for t in other.trees]
        self._settle()
        return n


# ---- the circuit ---------------------------------------------------------------------------------------------------------------

def eulerian_circuit(n, seed):
    """A closed walk over 0 .. n - 1 that takes every ordered pair (a, b), a == b included, exactly once: n * n steps
    (Hierholzer over the complete digraph, the order of each vertex's edges shuffled by `seed`)."""
    rng = np.random.default_rng(seed)
    out = {a: [int(b) for b in rng.permutation(n)] for a in range(n)}
    stack, walk = [0], []
    while stack:
        a = stack[-1]
        if out[a]:
            stack.append(out[a].pop())
        else:
            walk.append(stack.pop())
    walk.reverse()
    assert len(walk) == n * n + 1 and walk[0] == walk[-1]
    return walk[:-1]


CIRCUIT_SEED = 9


def sequence_of(circuit_seed):
    circuit = tuple(KINDS[v] for v in eulerian_circuit(len(KINDS), circuit_seed))
    return circuit, circuit + circuit[:1]


CIRCUIT, SEQUENCE = sequence_of(CIRCUIT_SEED)          # 122 steps: the closing pair is performed too


def pairs_of(sequence):
    return set(zip(sequence, sequence[1:]))


# ---- the configs ---------------------------------------------------------------------------------------------------------------

Config = collections.namedtuple("Config", "name max_count trees cells")
CONFIGS = {"roomy": Config("roomy", 70, 12, 400), "tight": Config("tight", 9, 12, 60)}
SEEDS = {"roomy": (3, 4, 7), "tight": (1, 2, 5)}           # walks that meet the conditions of tests/test_forest_life_model.py

TARGET_LIVE = 6                           # the live trees a growth step aims at: room for five removals in a row
POOL = np.random.default_rng(977).integers(0, 2**32, size=(4, 8), dtype=np.uint32)       # the four digests that come again and again

EVENTS = ("shrink to 0", "extend from 0", "open tree 1->2", "open tree 2->3", "open tree 3->2", "a power of two crossed upwards",
          "a power of two crossed downwards", "a tree at max_count", "free_leaves == 0 by growth", "free_trees == 0 by growth",
          "an empty tree appended", "a one-leaf tree appended", "drop_front of every tree in use", "truncate down to dropped_trees",
          "growth directly behind a drop_front", "repack with a middle tree deleted", "update of the last leaf of an odd level",
          "a nonzero mutation mask", "find of a digest only in dropped or freed cells", "extend or shrink refused behind a dropped front")


def second_forest(config):
    """The small fixed forest append_from copies trees of: an empty tree, a lone leaf, a tree of max_count, pool digests."""
    rng = np.random.default_rng(4099)
    counts = [3, 0, 1, config.max_count, 2, 4, 7]
    trees = [rng.integers(0, 2**32, size=(c, 8), dtype=np.uint32) for c in counts]
    trees[0][1], trees[4][0], trees[4][1], trees[6][5] = POOL[0], POOL[1], POOL[1], POOL[2]          # tree 4 is [x, x]: a mask
    return ModelForest(len(counts), sum(counts), config.max_count, trees)


def touches_odd_edge(count, index):
    """Is some ancestor-or-self of leaf `index` the last node of a level of odd size above 1 -- the node hashed with itself?"""
    return any(n > 1 and n % 2 == 1 and (index >> l) == n - 1 for l in range(tree_height(count)) for n in [-(-count >> l)])


def crossed(c, c2):
    """Does some power of two 2^k, k >= 1, lie in [min, max) of the two counts?"""
    lo, hi = min(c, c2), max(c, c2)
    return any(lo <= (1 << k) < hi for k in range(1, 62))


def reached_max(before, after):
    """Did a growth step take a tree to exactly max_count?"""
    return any(c == after.max_count and was != c for was, c in zip(before.counts, after.counts))


class Life:
    """One walk: the model of the forest under test (`a`), of its twin (`b`, which receives the STRUCTURAL steps alone), the
    fixed second forest (`src`), and the counters the CPU test asserts over.  steps() yields (number, kind, parameters) with
    the models as they are BEFORE the step; the caller performs the step and then calls apply(), which moves the models and
    returns what the Python layer is to return."""

    def __init__(self, seed, config, sequence=SEQUENCE):
        self.seed, self.config, self.sequence = seed, config, tuple(sequence)
        self.rng = np.random.default_rng([seed, config.max_count])
        self.ask = np.random.default_rng([seed, config.max_count, 1])         # the questions asked after a step: another stream
        self.src = second_forest(config)
        self.serial = 0
        counts = [int(c) for c in self.rng.choice([0, 1, 2, 3, config.max_count, int(self.rng.integers(2, config.max_count))], size=5)] + [3]
        while sum(counts) > config.cells // 2:
            counts[int(np.argmax(counts))] //= 2
        self.a = ModelForest(config.trees, config.cells, config.max_count, [self.fresh(c) for c in counts])
        self.b = self.a.copy()
        self.events, self.done, self.degenerate, self.pairs = set(), collections.Counter(), collections.Counter(), set()
        self.last = None

    # -- what the forest is made of ---------------------------------------------------------------------------------------
    def fresh(self, n, plant=False):
        """n leaf digests: about one in eight from POOL, the others random; `plant`: two equal siblings at level 0."""
        out = self.rng.integers(0, 2**32, size=(n, 8), dtype=np.uint32)
        for j in np.flatnonzero(self.rng.integers(0, 8, size=n) == 0):
            out[j] = POOL[int(self.rng.integers(0, 4))]
        if plant and n >= 2:
            j = 2 * int(self.rng.integers(0, n // 2))
            out[j + 1] = out[j]
        return out

    def strings(self, n, plant=False):
        """n strings no two walks share, and their digests; `plant`: two equal strings side by side."""
        out = []
        for _ in range(n):
            self.serial += 1
            out.append(b"life %d %d %d" % (self.seed, self.serial, int(self.rng.integers(0, 10**9))))
        if plant and n >= 2:
            j = 2 * int(self.rng.integers(0, n // 2))
            out[j + 1] = out[j]
        return out, np.array([digest_of(s) for s in out], dtype=np.uint32).reshape(-1, 8)

    # -- the steps --------------------------------------------------------------------------------------------------------
    def steps(self):
        for number, kind in enumerate(self.sequence):
            assert sum(self.done.values()) == number, "apply() the step before asking for the next"
            self.next_kind = self.sequence[number + 1] if number + 1 < len(self.sequence) else None
            yield number, kind, getattr(self, "_draw_" + kind)()

    def _pick(self, most):
        """Up to `most` live leaves, the last leaf of a tree often among them, and the first of them again at the end."""
        live = self.a.entries()
        if not live:
            return []
        k = min(len(live), int(self.rng.integers(1, most + 1)))
        picks = [live[int(j)] for j in self.rng.choice(len(live), size=k, replace=False)]
        if self.rng.integers(0, 2):
            t = int(self.rng.choice([t for t, c in enumerate(self.a.counts) if c]))
            picks.append((t, self.a.counts[t] - 1))
        return picks + picks[:1]

    def _draw_update(self):
        form = ("update", "update_packed", "update_entries")[int(self.rng.integers(0, 3))]
        picks = self._pick(6)
        p = {"form": form, "trees": [t for t, _ in picks], "indices": [i for _, i in picks], "degenerate": not picks}
        if form == "update_packed":
            p["strings"], p["values"] = self.strings(len(picks))
        else:
            p["values"] = self.fresh(len(picks))
        if form == "update_entries" and picks:
            order = self.rng.permutation(len(picks))
            p["trees"], p["indices"], p["values"] = [p["trees"][j] for j in order], [p["indices"][j] for j in order], p["values"][order]
            at = int(self.rng.integers(0, len(picks) + 1))
            p["trees"].insert(at, NO_TREE)
            p["indices"].insert(at, NOT_FOUND)
            p["values"] = np.insert(p["values"], at, self.fresh(1), axis=0)
        return p

    def _draw_replace(self):
        a = self.a
        live = a.image[a.dropped_leaves: a.used_leaves]
        old = [live[int(j)] for j in self.rng.choice(live.shape[0], size=min(live.shape[0], int(self.rng.integers(1, 4))), replace=False)] if live.shape[0] else []
        held = {d.tobytes() for d in live}
        old += [d for d in POOL if d.tobytes() in held][:1]                      # a digest that several leaves may hold
        unknown = self.rng.integers(0, 2**32, size=8, dtype=np.uint32)           # one that no leaf holds
        old.insert(int(self.rng.integers(0, len(old) + 1)), unknown)
        old.append(old[0])                                                       # and one that the queries hold twice
        old = np.array(old, dtype=np.uint32).reshape(-1, 8)
        return {"old": old, "new": self.fresh(old.shape[0]), "degenerate": live.shape[0] == 0}

    def _draw_witness(self):
        picks = self._pick(5)
        return {"trees": [t for t, _ in picks], "indices": [i for _, i in picks], "values": self.fresh(len(picks)), "degenerate": not picks}

    def _wanted(self, most):
        """How many trees a growth step brings: what takes the live trees back to about TARGET_LIVE, `most` at the most."""
        live = self.a.used_trees - self.a.dropped_trees
        return min(self.a.free_trees, max(1, min(most, TARGET_LIVE - live + int(self.rng.integers(0, 2)))))

    def _draw_append(self):
        a, c = self.a, self.config
        form = ("append", "append_packed")[int(self.rng.integers(0, 2))]
        room, counts = a.free_leaves, []
        ntr = self._wanted(4) if room >= 8 else min(1, a.free_trees)
        for j in range(ntr):
            want = int(self.rng.integers(2, c.max_count))                        # 2 .. max_count - 1
            if j < ntr - 1 and self.rng.integers(0, 4) == 0:                     # the last one becomes the open tree: no edge case
                want = int(self.rng.choice([0, 1, c.max_count]))
            counts.append(min(want, room, max(1, c.cells // 8)) if want != c.max_count else min(want, room))
            room -= counts[-1]
        p = {"form": form, "counts": counts, "degenerate": not counts, "mutated": form == "append" and bool(self.rng.integers(0, 2))}
        plant = bool(self.rng.integers(0, 3) == 0)
        parts = [self.strings(n, plant) if form == "append_packed" else (None, self.fresh(n, plant)) for n in counts]
        p["leaves"] = np.concatenate([d for _, d in parts] + [_no_leaves()])
        if form == "append_packed":
            p["strings"] = [s for strs, _ in parts for s in strs]
        return p

    def _draw_truncate(self):
        lo, hi = self.a.dropped_trees, self.a.used_trees
        if hi == lo:
            return {"keep": hi, "degenerate": True}
        keep = lo if self.next_kind in REFILLS or self.rng.integers(0, 16) == 0 else hi - (2 if hi - lo >= 4 and self.rng.integers(0, 4) == 0 else 1)
        return {"keep": keep, "degenerate": False}

    def _draw_extend(self):
        a = self.a
        form = ("extend", "extend_packed")[int(self.rng.integers(0, 2))]
        p = {"form": form, "mutated": form == "extend" and bool(self.rng.integers(0, 2)), "refused": a.open_tree is None}
        room = 0 if a.open_tree is None else min(a.free_leaves, a.max_count - a.counts[a.open_tree])
        n = 0 if room == 0 else int(self.rng.choice([1, 1, room, int(self.rng.integers(1, room + 1))] + [int(self.rng.integers(1, min(room, 4) + 1))] * 4))
        if room and a.counts[a.open_tree] in (1, 2):
            n = 1                                                                # the 1 -> 2 and 2 -> 3 edges
        if 0 < room == a.free_leaves <= 4:
            n = room                                                             # a reserve used to the last cell
        p["degenerate"] = n == 0
        if form == "extend_packed":
            p["strings"], p["leaves"] = self.strings(n)
        else:
            p["leaves"] = self.fresh(n)
        return p

    def _draw_shrink(self):
        a = self.a
        count = 0 if a.open_tree is None else a.counts[a.open_tree]
        r = 0 if count == 0 else int(self.rng.choice([1, 1, 1, int(self.rng.integers(1, count + 1)), int(self.rng.integers(1, min(count, 3) + 1))]))
        if count >= 2 and self.rng.integers(0, 4) == 0:
            r = count - int(self.rng.integers(1, min(count - 1, 3) + 1))         # down to 1, 2 or 3 leaves: the small edges come next
        if count == 3 and self.rng.integers(0, 2):
            r = 1                                                                # 3 -> 2
        if count and self.rng.integers(0, 10) == 0:
            r = count                                                            # down to an empty tree that stays in use
        return {"r": r, "mutated": bool(self.rng.integers(0, 2)), "refused": a.open_tree is None, "degenerate": r == 0}

    def _draw_drop_front(self):
        lo, hi = self.a.dropped_trees, self.a.used_trees
        if hi == lo:
            return {"k": lo, "degenerate": True}
        k = hi if self.a.free_trees >= 3 and (self.next_kind in REFILLS + ("extend",) or self.rng.integers(0, 16) == 0) else lo + (2 if hi - lo >= 4 and self.rng.integers(0, 4) == 0 else 1)
        return {"k": k, "degenerate": False}

    def _draw_repack(self):
        a, c = self.a, self.config
        live = list(range(a.dropped_trees, a.used_trees))
        trees = None
        if len(live) >= 3 and self.rng.integers(0, 2):
            trees = list(live)
            del trees[int(self.rng.integers(1, len(live) - 1))]
        m = len(live if trees is None else trees)
        n = sum(a.counts[t] for t in (live if trees is None else trees))
        reserve_trees = max(c.trees - m - int(self.rng.integers(0, 3)), 1 if m == 0 else 0)
        reserve_leaves = max(c.cells - n - int(self.rng.integers(0, 8)), 0)
        if self.next_kind == "extend":
            reserve_leaves = int(self.rng.integers(1, 4))                       # a reserve that is used to the last cell
        return {"trees": trees, "reserve_trees": reserve_trees, "reserve_leaves": reserve_leaves, "mutated": bool(self.rng.integers(0, 2)),
                "degenerate": False}

    def _draw_append_from(self):
        a, src = self.a, self.src
        if a.free_trees == 0:
            return {"sel": [], "mutated": False, "degenerate": True}
        want = [int(t) for t in self.rng.integers(0, src.ntrees, size=self._wanted(3))]
        if len(want) >= 2 and self.rng.integers(0, 2):
            want[0] = want[1]                                                    # a repeat
        if self.rng.integers(0, 3) == 0:
            want.insert(0, 1)                                                    # the empty tree
        want[-1] = int(self.rng.choice([0, 4, 5, 6]))                            # the last one becomes the open tree: no edge case
        sel, room = [], a.free_leaves
        for t in want[-a.free_trees:] if a.free_trees else []:
            if src.counts[t] <= room:
                sel.append(t)
                room -= src.counts[t]
        return {"sel": sel, "mutated": bool(self.rng.integers(0, 2)), "degenerate": not sel}

    def _draw_sync(self):
        return {"degenerate": self.a.diff(self.b)[0].shape[0] == 0}

    # -- the model moved --------------------------------------------------------------------------------------------------
    def apply(self, kind, p):
        """The models after the step, the counters and events kept; what the Python layer is to return."""
        a, b, ev = self.a, self.b, self.events
        before = a.copy()
        was_open = None if a.open_tree is None else a.counts[a.open_tree]
        out = {}
        if kind in ("update", "witness"):
            out["roots_before"] = a.roots()
            for t, i in zip(p["trees"], p["indices"]):
                if t != NO_TREE and touches_odd_edge(a.counts[t], i):
                    ev.add("update of the last leaf of an odd level")
            out["counted"] = a.update(p["trees"], p["indices"], p["values"])
        elif kind == "replace":
            out["counted"] = a.replace(p["old"], p["new"])
        elif kind == "append":
            new = np.split(p["leaves"], np.cumsum(p["counts"])[:-1]) if p["counts"] else []
            out["numbers"] = a.append(new)
            b.append(new)
        elif kind == "truncate":
            if p["keep"] == a.dropped_trees and a.used_trees > a.dropped_trees:
                ev.add("truncate down to dropped_trees")
            a.truncate(p["keep"])
            b.truncate(p["keep"])
        elif kind == "extend":
            if p["refused"] and a.dropped_trees:
                ev.add("extend or shrink refused behind a dropped front")
            if not p["refused"]:
                out["count"] = a.extend(p["leaves"])
                b.extend(p["leaves"])
        elif kind == "shrink":
            if p["refused"] and a.dropped_trees:
                ev.add("extend or shrink refused behind a dropped front")
            if not p["refused"]:
                out["count"] = a.shrink(p["r"])
                b.shrink(p["r"])
        elif kind == "drop_front":
            if p["k"] == a.used_trees and a.used_trees > a.dropped_trees:
                ev.add("drop_front of every tree in use")
            a.drop_front(p["k"])
            b.drop_front(p["k"])
        elif kind == "repack":
            if p["trees"] is not None:
                ev.add("repack with a middle tree deleted")
            self.a = a.repacked(p["trees"], p["reserve_trees"], p["reserve_leaves"])
            self.b = b.repacked(p["trees"], p["reserve_trees"], p["reserve_leaves"])
        elif kind == "append_from":
            out["numbers"] = a.append_from(self.src, p["sel"])
            b.append_from(self.src, p["sel"])
        elif kind == "sync":
            out["diff"] = a.diff(b)
            out["n"] = b.sync_from(a)
        else:
            raise ValueError(kind)
        a = self.a
        out["masks"] = a.masks()
        if kind in ("extend", "shrink") and not p["refused"]:
            now = a.counts[a.open_tree]
            for name, pair in (("open tree 1->2", (1, 2)), ("open tree 2->3", (2, 3)), ("open tree 3->2", (3, 2))):
                if (was_open, now) == pair:
                    ev.add(name)
            if was_open == 0 and now > 0:
                ev.add("extend from 0")
            if was_open > 0 and now == 0:
                ev.add("shrink to 0")
            if crossed(was_open, now):
                ev.add("a power of two crossed upwards" if now > was_open else "a power of two crossed downwards")
        grew = kind in GROWTH and not p["degenerate"]
        if grew:
            if a.free_leaves == 0 and before.free_leaves:
                ev.add("free_leaves == 0 by growth")
            if a.free_trees == 0 and before.free_trees:
                ev.add("free_trees == 0 by growth")
            if reached_max(before, a):
                ev.add("a tree at max_count")
            if self.last == "drop_front":
                ev.add("growth directly behind a drop_front")
        if kind in ("append", "append_from") and grew:
            new_counts = a.counts[before.used_trees: a.used_trees]
            if 0 in new_counts:
                ev.add("an empty tree appended")
            if 1 in new_counts:
                ev.add("a one-leaf tree appended")
        if out["masks"].any():
            ev.add("a nonzero mutation mask")
        self.done[kind] += 1
        self.degenerate[kind] += bool(p["degenerate"])
        if self.last is not None:
            self.pairs.add((self.last, kind))
        self.last = kind
        return out

    # -- the questions asked after every step --------------------------------------------------------------------------------
    def find_queries(self):
        """A sample of live leaves with duplicates among them, every digest that lies only in dropped or freed cells (16 at
        the most), one random digest."""
        a = self.a
        live = a.image[a.dropped_leaves: a.used_leaves]
        stale = a.stale_digests()[:16]
        if stale:
            self.events.add("find of a digest only in dropped or freed cells")
        q = [live[int(j)] for j in self.ask.integers(0, live.shape[0], size=min(12, live.shape[0]))] if live.shape[0] else []
        q = q + q[:2] + stale + [self.ask.integers(0, 2**32, size=8, dtype=np.uint32)]
        return np.array(q, dtype=np.uint32).reshape(-1, 8)

    def entry_set(self):
        """A random set of live leaves, sorted, each once: (trees uint32, indices uint64); empty when no leaf is live."""
        live = self.a.entries()
        if not live:
            return np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint64)
        k = min(len(live), int(self.ask.integers(1, 10)))
        return fm.sorted_entries(live[int(j)] for j in self.ask.choice(len(live), size=k, replace=False))


def walk(seed, config):
    """(kind, parameters) of every step of the walk, the model moved along."""
    life = Life(seed, config)
    for _, kind, p in life.steps():
        yield kind, p
        life.apply(kind, p)
