"""The life of a sorted set and every small shape of a sorted tree: ONE model of a forest whose trees are strictly increasing,
in plain Python over the rules that tests/absence_cases.py, tests/range_cases.py and tests/merge_cases.py restate with hashlib and
the tuple compare; EVERY, the forest of 41 trees of 0 .. 40 leaves with the two query tables that take every leaf, every gap and
every pair of gaps of every tree; and a walk that puts every sorted operation directly after every other.
tests/test_sorted_set_model.py (no GPU) anchors the model to the host library's CPU twins along every walk and over EVERY and
asserts that the walks reach what they are meant to reach; tests/test_gpu_sorted_set.py drives the device through the same tables
and walks and compares everything it answers with the model.  A plain module: no fixtures, no GPU.

ModelSet.  Its state is `trees`, per tree in use the leaves as a list of 8-word tuples -- sorted and distinct, but for the middle
of a disorder step --, and the capacity the last step asked for: `reserve_trees` empty trees behind them, `total` cells of level 0
and `max_count`.  Counts, offsets, level 0 as it lies in memory, the levels and roots of every tree, `levels`, and what is_sorted,
lower_bound, absence, ranges, find and the two verifiers answer are derived from that state alone.

The walk.  CIRCUIT is an Eulerian circuit over the six KINDS (forest_life_cases.eulerian_circuit): every ordered pair of kinds,
each kind after itself included, occurs once; SEQUENCE repeats its first kind at the end, 37 steps.  SetLife(seed, config) draws
every step's parameters from its seed, from the model's state and from the kind that comes next, never from what a device answered;
a kind is never swapped for another, and a step that has nothing to do (a sort of no leaf, a removal from a forest without one, an
update where no leaf has room to move, a disorder where no tree has two leaves) is performed in that degenerate form and counted.
CIRCUIT_SEED and SEEDS are the circuit and the walks for which the model alone meets what tests/test_sorted_set_model.py asserts:
every pair, at most a quarter of a kind's steps degenerate, every one of EVENTS over the three seeds of a config.

One stored MerkleTree (`life.tree`, a model of its own) receives tree 0's share of every merge step through the one-tree methods;
where nothing would be left of it the ValueError is what the step asserts and the tree stays as it is."""
import collections
import functools

import numpy as np

import absence_cases as ac
import find_cases as fd
import merge_cases as mc
import range_cases as rc
from forest_life_cases import eulerian_circuit
from merkle_model import cpu_levels, random_leaves, tree_height

NONE, NOT_PROVEN, ABSENT, PRESENT = ac.NONE, ac.NOT_PROVEN, ac.ABSENT, ac.PRESENT
NO_TREE, NOT_FOUND = fd.NO_TREE, fd.NOT_FOUND
ZERO, ONES = mc.ZERO, mc.ONES                           # as word tuples
A_NOT_INCREASING = mc.A_NOT_INCREASING                  # status bit 2: what a merge out of a disordered forest is refused with
KINDS = ("sort_build", "insert", "remove", "common", "update_in_order", "disorder")
MERGES = {"insert": 0, "remove": 1, "common": 2}        # the kind -> the op of merge_cases
METHODS = {"insert": "inserted", "remove": "removed", "common": "common"}

_LEVELS = {}


def rows_of(tuples):
    return mc.rows_of(tuples)


def levels_of(rows):
    """cpu_levels(rows), kept per leaf list: a walk asks for the same trees step after step, a table for the same tree query
    after query."""
    key = rows.tobytes()
    if key not in _LEVELS:
        if len(_LEVELS) > 20000:
            _LEVELS.clear()
        _LEVELS[key] = cpu_levels(rows.copy())
        for level in _LEVELS[key]:
            level.setflags(write=False)
    return _LEVELS[key]


@functools.lru_cache(maxsize=4096)
def _rows(leaves):
    rows = rows_of(leaves)
    rows.setflags(write=False)
    return rows


class _Trees:
    """What rc.Forest.gap reads of a forest: its trees."""

    def __init__(self, trees):
        self.trees = trees


def alterations(roots, counts):
    """[(name, roots, counts)]: the verifier's tables as they are, and the three ways in which a holder's tables are wrong."""
    roots, counts = np.asarray(roots, dtype=np.uint32).reshape(-1, 8), np.asarray(counts, dtype=np.uint64)
    return [("true", roots, counts), ("counts + 1", roots, counts + np.uint64(1)),
            ("counts - 1", roots, counts - (counts >= 1).astype(np.uint64)), ("roots rotated", np.roll(roots, 1, axis=0), counts)]


ALTERATIONS = ("true", "counts + 1", "counts - 1", "roots rotated")


class ModelSet:
    """A forest of sorted trees in plain Python: the module docstring says what is state and what is derived."""

    def __init__(self, trees, reserve_trees=0, total=None, max_count=None):
        self.trees = [[tuple(int(w) for w in r) for r in t] for t in trees]
        self.reserve_trees = int(reserve_trees)
        live = sum(len(t) for t in self.trees)
        self.total = live if total is None else int(total)
        self.max_count = max([1] + [len(t) for t in self.trees]) if max_count is None else int(max_count)
        assert self.total >= live and all(len(t) <= self.max_count for t in self.trees)

    def copy(self):
        return ModelSet(self.trees, self.reserve_trees, self.total, self.max_count)

    # ---- the handle's books --------------------------------------------------------------------------------------------------
    used_trees = property(lambda self: len(self.trees))
    ntrees = property(lambda self: len(self.trees) + self.reserve_trees)
    counts = property(lambda self: [len(t) for t in self.trees] + [0] * self.reserve_trees)
    live = property(lambda self: sum(len(t) for t in self.trees))
    levels = property(lambda self: tree_height(min(self.max_count, self.total)) if self.total else 1)

    def books(self):
        return {"counts": self.counts, "used_trees": self.used_trees, "ntrees": self.ntrees, "total": self.total, "max_count": self.max_count,
                "levels": self.levels}

    # ---- what the device holds -----------------------------------------------------------------------------------------------
    def offsets(self):
        return np.concatenate([[0], np.cumsum(self.counts)]).astype(np.uint64)

    def rows(self, t):
        return _rows(tuple(self.trees[t]) if t < self.used_trees else ())

    def image(self):
        """Level 0 as it lies in memory: the live leaves back to back from cell 0; what lies behind them is nobody's."""
        return rows_of([r for t in self.trees for r in t])

    def tree_levels(self, t):
        return levels_of(self.rows(t)) if t < self.used_trees and self.trees[t] else None

    def roots(self):
        out = np.zeros((self.ntrees, 8), np.uint32)
        for t, leaves in enumerate(self.trees):
            if leaves:
                out[t] = self.tree_levels(t)[-1][0]
        return out

    def gap(self, t, g):
        """A digest strictly between leaf g - 1 and leaf g of tree t, or None where there is none: rc.Forest.gap, the one
        rule, called on a stand-in that holds what that method reads of its forest today -- `trees` and nothing else.  Should it
        come to read more, this call fails or _Trees has to follow; range_cases is not this module's to change."""
        return rc.Forest.gap(_Trees({t: self.rows(t)}), t, g)

    # ---- the sortedness pass ----------------------------------------------------------------------------------------------------
    def first_bad(self):
        """(first_bad uint64 [ntrees], info [status, trees out of order, of those with an equal pair first, pairs looked at])."""
        want = [ac.model_first_bad(self.rows(t)) for t in range(self.ntrees)]
        return (np.array([w[0] for w in want], dtype=np.uint64),
                [0, sum(w[0] != NONE for w in want), sum(w[1] for w in want), sum(max(c - 1, 0) for c in self.counts)])

    def is_sorted(self):
        return self.first_bad()[1][1] == 0

    # ---- the readers ------------------------------------------------------------------------------------------------------------
    def lower_bound(self, trees, digests):
        """(indices uint64 [Q], found uint32 [Q]); NONE and 0 for a tree outside the forest."""
        Q = len(trees)
        idx, found = np.full(Q, NONE, np.uint64), np.zeros(Q, np.uint32)
        for q, t in enumerate(int(t) for t in trees):
            if t < self.ntrees:
                idx[q], found[q] = ac.model_lower_bound(self.rows(t), digests[q])
        return idx, found

    def absence(self, trees, digests, stride=None):
        """(indices, pred, succ, main [Q, stride, 8], low, heights): ac.model_proof per query, zero cells and NONE for a tree
        outside the forest."""
        stride, Q = self.levels if stride is None else stride, len(trees)
        idx, heights = np.full(Q, NONE, np.uint64), np.zeros(Q, np.uint32)
        pred, succ = np.zeros((Q, 8), np.uint32), np.zeros((Q, 8), np.uint32)
        main, low = np.zeros((Q, stride, 8), np.uint32), np.zeros((Q, stride, 8), np.uint32)
        for q, t in enumerate(int(t) for t in trees):
            if t < self.ntrees:
                idx[q], pred[q], succ[q], main[q], low[q], heights[q] = ac.model_proof(self.rows(t), self.tree_levels(t), digests[q], stride)
        return idx, pred, succ, main, low, heights

    def ranges(self, trees, lo, hi, stride=None):
        """(firsts, leaf_starts, leaves, left, right, heights, info) by rc.model_run and rc.model_rows; a tree outside the forest
        or hi < lo: NONE, no leaf, counted in info[2]."""
        stride, Q = self.levels if stride is None else stride, len(trees)
        firsts, heights = np.zeros(Q, np.uint64), np.zeros(Q, np.uint32)
        starts, runs = np.zeros(Q + 1, np.uint64), [np.zeros((0, 8), np.uint32)]
        left, right = np.zeros((Q, stride, 8), np.uint32), np.zeros((Q, stride, 8), np.uint32)
        refused = inside = 0
        for q, t in enumerate(int(t) for t in trees):
            m = 0
            if t >= self.ntrees or ac.key(hi[q]) < ac.key(lo[q]):
                firsts[q] = NONE
                refused += 1
            else:
                leaves = self.rows(t)
                a, m, n = rc.model_run(leaves, lo[q], hi[q])
                firsts[q], heights[q] = a, ac.height(len(leaves))
                inside += n
                if m:
                    runs.append(leaves[a: a + m])
                    left[q], right[q] = rc.model_rows(self.tree_levels(t), a, a + m - 1, len(leaves), stride)
            starts[q + 1] = starts[q] + np.uint64(m)
        return firsts, starts, np.concatenate(runs), left, right, heights, np.array([0, int(starts[Q]), refused, inside], dtype=np.uint64)

    def find(self, digests):
        """(trees, indices) by find_cases.model: the lowest position of the forest at which the digest is a leaf."""
        return fd.model(self.image(), self.offsets(), digests)


def absence_verdicts(trees, digests, proofs, roots, counts):
    """uint32 [Q]: ac.model_verdict of every proof (indices, pred, succ, main, low, heights) under the holder's roots and counts."""
    idx, pred, succ, main, low, heights = proofs
    ntrees = len(counts)
    return np.array([ac.model_verdict(digests[q], t, ntrees, idx[q], pred[q], succ[q], main[q], low[q], heights[q], roots[min(t, ntrees - 1)],
                                      counts[min(t, ntrees - 1)]) for q, t in enumerate(int(t) for t in trees)], dtype=np.uint32).reshape(-1)


def range_verdicts(trees, lo, hi, proofs, roots, counts):
    """(verdict uint32 [Q], in_first uint64 [Q], in_count uint64 [Q]): rc.model_verdict of every proof (firsts, leaf_starts, leaves,
    left, right, heights) under the holder's roots and counts."""
    firsts, starts, leaves, left, right, heights = proofs[:6]
    ntrees = len(counts)
    out = [rc.model_verdict(t, ntrees, lo[q], hi[q], firsts[q], leaves[int(starts[q]): int(starts[q + 1])], left[q], right[q], heights[q],
                            roots[min(t, ntrees - 1)], counts[min(t, ntrees - 1)])
           for q, t in enumerate(int(t) for t in trees)]
    return (np.array([o[0] for o in out], dtype=np.uint32).reshape(-1), np.array([o[1] for o in out], dtype=np.uint64).reshape(-1),
            np.array([o[2] for o in out], dtype=np.uint64).reshape(-1))


# ---- EVERY: every small shape ------------------------------------------------------------------------------------------------------

EVERY_COUNTS = list(range(41))
EVERY_STRIDE = 6                                        # H(40)
EVERY_IN_RANGE = 123410                                 # C(43, 4): the leaves that the range table's 12 341 queries have in range
EVERY_CARRIED = 146370                                  # and the leaves their runs carry, the fences on either side included
EVERY_TRIPLES = (1, 22, 40)                             # the trees that the one-tree twins take


class Every(ModelSet):
    """41 trees, tree t of t random digests from a fixed seed, sorted: 820 leaves, max_count 40, heights 0 .. 6; and the two
    query tables."""

    def __init__(self, seed=901):
        rng = np.random.default_rng(seed)
        super().__init__([ac.sorted_rows(random_leaves(rng, c)) if c else [] for c in EVERY_COUNTS])
        assert self.counts == EVERY_COUNTS and self.total == 820 and self.max_count == 40 and self.levels == EVERY_STRIDE and self.is_sorted()
        self.filler = random_leaves(rng, 137)

    def placed(self, first=0, slack=0):
        """(cells [first + 820 + slack, 8], offsets uint64 [42]): the leaves laid at cell `first`, random cells around them."""
        cells = np.concatenate([self.filler[:first], self.image(), self.filler[37: 37 + slack]])
        return np.ascontiguousarray(cells), self.offsets() + np.uint64(first)

    @functools.lru_cache(maxsize=None)
    def absence_queries(self):
        """(trees uint32 [1681], digests [1681, 8], present bool [1681]): per tree every leaf and every gap 0 .. c, shuffled."""
        out = []
        for t, c in enumerate(self.counts):
            rows = self.rows(t)
            out += [(t, rows[i], True) for i in range(c)] + [(t, self.gap(t, g), False) for g in range(c + 1)]
        assert len(out) == 1681 and all(x is not None for _, x, _ in out)
        order = np.random.default_rng(902).permutation(len(out))
        return (np.array([out[j][0] for j in order], dtype=np.uint32), np.stack([out[j][1] for j in order]).astype(np.uint32),
                np.array([out[j][2] for j in order], dtype=bool))

    @functools.lru_cache(maxsize=None)
    def range_queries(self):
        """(trees uint32 [12341], lo, hi, (a, b) of the run or None): per tree every pair of gaps g1 <= g2, shuffled."""
        out = []
        for t, c in enumerate(self.counts):
            gaps = [self.gap(t, g) for g in range(c + 1)]
            out += [(t, gaps[g1], gaps[g2]) for g1 in range(c + 1) for g2 in range(g1, c + 1)]
        assert len(out) == 12341
        order = np.random.default_rng(903).permutation(len(out))
        return (np.array([out[j][0] for j in order], dtype=np.uint32), np.stack([out[j][1] for j in order]).astype(np.uint32),
                np.stack([out[j][2] for j in order]).astype(np.uint32))

    @functools.lru_cache(maxsize=None)
    def absence_expected(self):
        """(indices, found, pred, succ, main, low, heights) of absence_queries() at EVERY_STRIDE."""
        trees, digests, _ = self.absence_queries()
        idx, found = self.lower_bound(trees, digests)
        got = self.absence(trees, digests, EVERY_STRIDE)
        assert (got[0] == idx).all()
        return (idx, found) + got[1:]

    @functools.lru_cache(maxsize=None)
    def range_expected(self):
        """(firsts, leaf_starts, leaves, left, right, heights, info) of range_queries() at EVERY_STRIDE."""
        return self.ranges(*self.range_queries(), EVERY_STRIDE)

    @functools.lru_cache(maxsize=None)
    def absence_verdicts_under(self, name):
        """The verdicts of the absence table's proofs under alteration `name` of the true roots and counts."""
        trees, digests, _ = self.absence_queries()
        _, roots, counts = alterations(self.roots(), self.counts)[ALTERATIONS.index(name)]
        e = self.absence_expected()
        return absence_verdicts(trees, digests, e[:1] + e[2:], roots, counts)

    @functools.lru_cache(maxsize=None)
    def range_verdicts_under(self, name):
        """(verdict, in_first, in_count) of the range table's proofs under alteration `name`."""
        _, roots, counts = alterations(self.roots(), self.counts)[ALTERATIONS.index(name)]
        return range_verdicts(*self.range_queries(), self.range_expected(), roots, counts)

    def share(self, t):
        """The rows of both tables that name tree t: (absence rows, range rows)."""
        return np.nonzero(self.absence_queries()[0] == t)[0], np.nonzero(self.range_queries()[0] == t)[0]


@functools.lru_cache(maxsize=None)
def every():
    return Every()


# ---- the circuit and the configs ------------------------------------------------------------------------------------------------------

CIRCUIT_SEED = 2


def sequence_of(circuit_seed):
    circuit = tuple(KINDS[v] for v in eulerian_circuit(len(KINDS), circuit_seed))
    return circuit, circuit + circuit[:1]


CIRCUIT, SEQUENCE = sequence_of(CIRCUIT_SEED)          # 37 steps: the closing pair is performed too


def pairs_of(sequence):
    return set(zip(sequence, sequence[1:]))


Config = collections.namedtuple("Config", "name trees aim")
CONFIGS = {"roomy": Config("roomy", 12, 70), "tight": Config("tight", 3, 9)}
SEEDS = {"roomy": (2, 3, 4), "tight": (3, 13, 14)}       # walks that meet the conditions of tests/test_sorted_set_model.py

EVENTS = ("a tree emptied by remove", "a tree emptied by common", "an insert into an empty tree", "every tree empty after a step",
          "a merge step from a source whose every tree is empty", "an empty batch", "an empty batch into a forest with leaves", "a batch whose every digest was a leaf already",
          "a batch with repeats", "a count crossing a power of two upwards", "a count crossing a power of two downwards", "levels changed",
          "an insert below a tree's first leaf", "an insert above a tree's last leaf", "the first leaf removed", "the last leaf removed",
          "a batch row equal to a leaf in words 0..6", "two batch rows equal in words 0 and 1", "the all-zero digest as a leaf",
          "the all-ones digest as a leaf", "reserve_trees > 0 and mutated=True", "an explicit max_count equal to the largest count of the result",
          "a one-leaf stored tree")


def crossed(c, c2):
    """Does some power of two 2^k, k >= 2, lie in [min, max) of the two counts?"""
    lo, hi = min(c, c2), max(c, c2)
    return any(lo <= (1 << k) < hi for k in range(2, 62))


def between(lo, hi, rng):
    """An integer strictly between lo and hi drawn from rng, or None where there is none."""
    if hi - lo < 2:
        return None
    return lo + 1 + int.from_bytes(rng.bytes(32), "big") % (hi - lo - 1)


class SetLife:
    """One walk: the model of the forest under test (`m`), of the stored tree (`tree`, a list of word tuples that is never
    empty), and the counters the CPU test asserts over.  steps() yields (number, kind, parameters) with the models as they are
    BEFORE the step; the caller performs the step and then calls apply(), which moves the models and returns what the Python layer
    is to return.  A disorder step is performed in its four parts by the caller, between bend() and mend()."""

    def __init__(self, seed, config, sequence=SEQUENCE):
        self.seed, self.config, self.sequence = seed, config, tuple(sequence)
        self.rng = np.random.default_rng([seed, config.aim])
        self.ask = np.random.default_rng([seed, config.aim, 1])               # the questions asked after a step: another stream
        counts = [int(c) for c in self.rng.integers(0, config.aim // 2 + 1, size=config.trees)]
        counts[0] = max(counts[0], 3)
        counts[-1] = 0                                                        # an empty tree from the start
        self.m = ModelSet([sorted(mc.words(r) for r in self.fresh(c)) for c in counts])
        self.tree = list(self.m.trees[0])
        self.events, self.done, self.degenerate, self.pairs = set(), collections.Counter(), collections.Counter(), set()
        self.last, self.disorders = None, 0
        # which occurrence of a merge kind asks for which capacity, and which brings the special batch: drawn once, from the seed
        self.plans = {kind: [str(x) for x in self.rng.permutation(["plain", "plain", "exact", "roomy", "plain", "roomy", "exact"])] for kind in MERGES}
        self.special = {kind: int(self.rng.integers(0, 6)) for kind in MERGES}
        self.hollow = (self.special["insert"] + 1 + int(self.rng.integers(0, 5))) % 6     # the insert that brings no row: another occurrence

    def fresh(self, n):
        """n random digests with room below the lowest and above the highest there can be: word 0 in [0x30000000, 0xB0000000)."""
        out = random_leaves(self.rng, n)
        out[:, 0] = (out[:, 0] >> np.uint32(1)) + np.uint32(0x30000000)
        return out

    # -- the steps --------------------------------------------------------------------------------------------------------------
    def steps(self):
        for number, kind in enumerate(self.sequence):
            assert sum(self.done.values()) == number, "apply() the step before asking for the next"
            self.next_kind = self.sequence[number + 1] if number + 1 < len(self.sequence) else None
            yield number, kind, getattr(self, "_draw_" + ("merge" if kind in MERGES else kind))(*([kind] if kind in MERGES else []))

    def _capacity(self, plan, largest):
        """The keywords of a build: plain (none), exact (max_count = the largest count of the result), roomy (room behind)."""
        if plan == "exact" and largest >= 1:
            return {"max_count": largest}
        if plan == "roomy":
            return {"max_count": max(1, largest) + int(self.rng.integers(0, 4)), "reserve_trees": int(self.rng.integers(1, 3)),
                    "reserve_leaves": int(self.rng.integers(0, 6)), "mutated": bool(self.rng.integers(0, 2))}
        return {}

    def _draw_sort_build(self):
        m = self.m
        shuffled = [rows_of([t[int(j)] for j in self.rng.permutation(len(t))]) for t in m.trees]
        plan = ("plain", "exact", "roomy")[int(self.rng.integers(0, 3))]
        return {"leaves": np.concatenate(shuffled + [rows_of([])]), "counts": m.counts[: m.used_trees],
                "build": self._capacity(plan, max(m.counts)), "degenerate": m.live == 0}

    def _near(self, leaf):
        """The leaf but for word 7."""
        return leaf[:7] + ((leaf[7] + 1 + int(self.rng.integers(0, 1000))) & 0xFFFFFFFF,)

    def _some(self, pool, k):
        """Up to k rows of `pool`, each once."""
        return [pool[int(j)] for j in self.rng.choice(len(pool), size=min(len(pool), k), replace=False)] if pool else []

    def _strays(self, rows, leaves):
        """What a remove and a common batch hold besides leaves: at times a digest that is no leaf, a row equal to a leaf but for
        word 7, and a row twice."""
        rng = self.rng
        rows = rows + [mc.words(r) for r in self.fresh(int(rng.integers(0, 2)))]
        if leaves and rng.integers(0, 4) == 0:
            rows.append(self._near(leaves[int(rng.integers(0, len(leaves)))]))
        if rows and rng.integers(0, 3) == 0:
            rows += rows[:1]
        return rows

    def _insert_rows(self, leaves, special):
        """Tree `leaves` gets: on the special occurrence up to three of its own leaves and nothing else; otherwise new digests
        towards the config's aim, at times with some leaves it has, a row equal to a leaf but for word 7, a row below its first
        or above its last leaf, the all-zero or the all-ones digest, two rows equal in words 0 and 1, and repeats."""
        rng, aim, c = self.rng, self.config.aim, len(leaves)
        if special:
            return self._some(leaves, 3)
        room = max(aim - c, 0)
        if rng.integers(0, 6) == 0:
            n = 0
        elif rng.integers(0, 2):
            n = int(rng.integers(0, room + 1))
        else:
            n = min(room, int(rng.integers(1, aim // 6 + 3)))
        rows = [mc.words(r) for r in self.fresh(n)] + self._some(leaves, int(rng.integers(0, 3)))
        if c and room - n >= 2:
            pick = int(rng.integers(0, 6))
            if pick == 0:
                rows.append(self._near(leaves[int(rng.integers(0, c))]))
            elif pick == 1:
                rows.append(mc.from_int(mc.as_int(leaves[0]) - 1 - int(rng.integers(0, 1000))) if mc.as_int(leaves[0]) > 2000 else ZERO)
            elif pick == 2:
                rows.append(mc.from_int(mc.as_int(leaves[-1]) + 1 + int(rng.integers(0, 1000))) if mc.as_int(leaves[-1]) < (1 << 256) - 2000 else ONES)
            elif pick in (3, 4):
                rows += [ZERO, ONES][int(rng.integers(0, 2)):][: int(rng.integers(1, 3))]
        if len(rows) >= 2 and rng.integers(0, 3) == 0:
            rows.append(rows[0][:2] + tuple(int(w) for w in random_leaves(rng, 1)[0][2:]))           # the leaf sort's tie step
        if rows and rng.integers(0, 3) == 0:
            rows += rows[: int(rng.integers(1, 3))]                                                    # repeats
        return rows

    def _remove_rows(self, t, leaves, special, empties_all):
        """Tree t loses: every leaf where the step empties the forest; on the special occurrence tree 0's batch is the stored
        tree's leaves but its last, which leaves that one leaf; otherwise nothing, the whole tree (every third tree at most) or
        up to half of its leaves, the first and the last at times among them."""
        rng, c = self.rng, len(leaves)
        if empties_all:
            rows = list(leaves)
        elif special and t == 0:
            rows = list(self.tree[:-1])
        else:
            pick = int(rng.integers(0, 6))
            if pick == 0 or c == 0:
                rows = []
            elif pick == 1 and t % 3 == 1:
                rows = list(leaves)
            else:
                rows = self._some(leaves, max(1, int(rng.integers(1, c // 2 + 2))))
                if rng.integers(0, 3) == 0:
                    rows.append(leaves[0])
                if rng.integers(0, 3) == 0:
                    rows.append(leaves[-1])
        return self._strays(rows, leaves)

    def _common_rows(self, t, leaves):
        """Tree t keeps: nothing (every fourth tree -- of three trees the first --, at times: two digests that are no leaves),
        or two thirds of its leaves and more."""
        rng, c = self.rng, len(leaves)
        if c and t % 4 == 3 % self.m.used_trees and rng.integers(0, 2):
            return [mc.words(r) for r in self.fresh(2)]
        return self._strays(self._some(leaves, max(1, c - int(rng.integers(0, c // 3 + 2)))), leaves)

    def _draw_merge(self, kind):
        """A batch in no order for every tree in use, its rows by _insert_rows, _remove_rows and _common_rows.  Three draws keep
        the walk alive and take it through the empty forest once:
          - a remove or a common in front of an insert names every leaf (remove) or no row at all (common), and so does the first
            remove that stands in front of another remove or a common while no remove or common step has been degenerate: the
            merge steps behind it find a source whose every tree is empty -- a remove and a common among them, degenerate and
            counted -- until an insert refills it;
          - a step from such a source asks for no room, so that the new forest has no cell of level 0 at all, and a common from it
            brings no row either;
          - on the `hollow` occurrence an insert into a forest that has leaves brings no row: the empty batch from a source that
            is not empty."""
        m, rng = self.m, self.rng
        occurrence = self.done[kind]
        special = occurrence == self.special[kind]
        untried = self.degenerate["remove"] == 0 and self.degenerate["common"] == 0
        empties_all = kind != "insert" and m.live > 0 and (self.next_kind == "insert" or (kind == "remove" and self.next_kind in ("remove", "common") and untried))
        batch = []
        for t, leaves in enumerate(m.trees):
            if kind == "insert":
                rows = [] if occurrence == self.hollow and m.live else self._insert_rows(leaves, special)
            elif kind == "remove":
                rows = self._remove_rows(t, leaves, special, empties_all)
            else:
                rows = [] if empties_all or m.live == 0 else self._common_rows(t, leaves)
            batch.append([rows[int(j)] for j in rng.permutation(len(rows))])
        if kind == "insert" and special and m.live == 0:
            batch = [[mc.words(r) for r in self.fresh(2)] for _ in m.trees]       # nothing is a leaf yet: the step still inserts
        counts = [len(rows) for rows in batch]
        largest = max(len((set(a) | set(b), set(a) - set(b), set(a) & set(b))[MERGES[kind]]) for a, b in zip(m.trees, batch))
        build = self._capacity(self.plans[kind][occurrence % 7], largest) if kind == "insert" or m.live else {}
        if kind == "insert":
            degenerate = sum(counts) == 0
        else:
            degenerate = m.live == 0 or (kind == "remove" and sum(counts) == 0)
        return {"batch": rows_of([r for rows in batch for r in rows]), "counts": counts, "build": build, "degenerate": degenerate,
                "tree_batch": rows_of(batch[0])}

    def _draw_update_in_order(self):
        """Up to six leaves, each to a digest strictly between its neighbours as they are once the ones before it have moved."""
        m, rng = self.m, self.rng
        state = [list(t) for t in m.trees]
        live = [(t, i) for t, leaves in enumerate(state) for i in range(len(leaves))]
        picks = [live[int(j)] for j in rng.choice(len(live), size=min(len(live), int(rng.integers(1, 7))), replace=False)] if live else []
        trees, indices, values = [], [], []
        for t, i in picks:
            lo = mc.as_int(state[t][i - 1]) if i > 0 else -1
            hi = mc.as_int(state[t][i + 1]) if i + 1 < len(state[t]) else 1 << 256
            v = between(lo, hi, rng)
            if v is not None and mc.from_int(v) != state[t][i]:
                state[t][i] = mc.from_int(v)
                trees.append(t), indices.append(i), values.append(state[t][i])
        return {"trees": trees, "indices": indices, "values": rows_of(values), "degenerate": not trees}

    def _draw_disorder(self):
        """One leaf of a tree of two or more to a value out of order -- every third time to its neighbour's --, and the batch that
        the three merges are refused with."""
        m, rng = self.m, self.rng
        self.disorders += 1
        able = [t for t, leaves in enumerate(m.trees) if len(leaves) >= 2]
        p = {"counts": [1 if t % 2 == 0 else 0 for t in range(m.used_trees)], "degenerate": not able}
        p["batch"] = self.fresh(sum(p["counts"]))
        if not able:
            return p
        t = able[int(rng.integers(0, len(able)))]
        leaves = m.trees[t]
        i = int(rng.integers(0, len(leaves)))
        beyond = ([mc.as_int(leaves[i + 1]) + 1] if i + 1 < len(leaves) else []) + ([mc.as_int(leaves[i - 1]) - 1] if i > 0 else [])
        beyond = [v for v in beyond if 0 <= v < 1 << 256]                  # just above the leaf behind, just below the leaf in front
        equal = self.disorders % 3 == 0 or not beyond
        bad = (leaves[i + 1] if i + 1 < len(leaves) else leaves[i - 1]) if equal else mc.from_int(beyond[int(rng.integers(0, len(beyond)))])
        p.update(tree=t, index=i, bad=rows_of([bad]), good=rows_of([leaves[i]]), equal=equal)
        return p

    # -- the model moved ------------------------------------------------------------------------------------------------------------
    def bend(self, p):
        """The first part of a disorder step: the model with the leaf out of order; (first_bad, info) as the pass must name them."""
        self.m.trees[p["tree"]][p["index"]] = mc.words(p["bad"][0])
        want = self.m.first_bad()
        assert want[1][1] == 1 and want[1][2] == int(p["equal"])
        return want

    def mend(self, p):
        self.m.trees[p["tree"]][p["index"]] = mc.words(p["good"][0])
        assert self.m.is_sorted()

    def apply(self, kind, p):
        """The models after the step, the counters and events kept; what the Python layer is to return."""
        m, ev = self.m, self.events
        before = m.copy()
        out = {}
        if kind == "sort_build":
            self.m = ModelSet(m.trees, p["build"].get("reserve_trees", 0), m.live + p["build"].get("reserve_leaves", 0), p["build"].get("max_count"))
        elif kind in MERGES:
            op = MERGES[kind]
            off = np.concatenate([[0], np.cumsum(p["counts"])]).astype(np.uint64)
            b_sorted = [sorted(mc.words(r) for r in p["batch"][int(off[t]): int(off[t + 1])]) for t in range(m.used_trees)]
            case = mc.Case("", m.image(), m.offsets()[: m.used_trees + 1], rows_of([r for rows in b_sorted for r in rows]), off)
            rows, starts, _, info = mc.model_merge(case, op)
            assert int(info[0]) == 0
            new = [[mc.words(r) for r in rows[int(starts[t]): int(starts[t + 1])]] for t in range(m.used_trees)]
            na, nb, build = m.live, int(off[-1]), p["build"]
            max_count = build.get("max_count")
            if max_count is None:                              # the documented rule: the largest count the result can have; the source's otherwise
                max_count = max([1] + [len(a) + len(b) for a, b in zip(m.trees, b_sorted)]) if op == 0 else m.max_count
            self.m = ModelSet(new, build.get("reserve_trees", 0), (na + nb if op == 0 else na) + build.get("reserve_leaves", 0), max_count)
            out["info"], out["case"], out["b_sorted"] = [int(x) for x in info], case, b_sorted
            # the stored tree takes tree 0's share
            mine = sorted(mc.words(r) for r in p["tree_batch"])
            one = mc.Case("", rows_of(self.tree), np.array([0, len(self.tree)], np.uint64), rows_of(mine), np.array([0, len(mine)], np.uint64))
            t_rows, _, _, t_info = mc.model_merge(one, op)
            out["tree_info"] = [int(x) for x in t_info]
            out["tree_left"] = int(t_info[1])
            if out["tree_left"]:
                self.tree = [mc.words(r) for r in t_rows[: out["tree_left"]]]
            if len(self.tree) == 1:
                ev.add("a one-leaf stored tree")
            self._merge_events(kind, before, b_sorted, info, build)
        elif kind == "update_in_order":
            for t, i, v in zip(p["trees"], p["indices"], p["values"]):
                m.trees[t][i] = mc.words(v)
            assert m.is_sorted()
        elif kind == "disorder":
            assert m.is_sorted()
        else:
            raise ValueError(kind)
        m = self.m
        if m.live == 0 and before.live:
            ev.add("every tree empty after a step")
        held = {r for t in m.trees for r in t}
        if ZERO in held:
            ev.add("the all-zero digest as a leaf")
        if ONES in held:
            ev.add("the all-ones digest as a leaf")
        self.done[kind] += 1
        self.degenerate[kind] += bool(p["degenerate"])
        if self.last is not None:
            self.pairs.add((self.last, kind))
        self.last = kind
        return out

    def _merge_events(self, kind, before, b_sorted, info, build):
        ev, after = self.events, self.m
        if before.live == 0 and kind != "insert" and after.total == 0:       # cap == 0: the new forest has no level 0 either
            ev.add("a merge step from a source whose every tree is empty")
        if any(crossed(len(a), len(new)) for a, new in zip(before.trees, after.trees)) and after.levels != before.levels:
            ev.add("levels changed")
        if sum(len(b) for b in b_sorted) == 0:
            ev.add("an empty batch" if before.live == 0 else "an empty batch into a forest with leaves")
        elif kind == "insert" and all(r in set(a) for a, b in zip(before.trees, b_sorted) for r in b):
            ev.add("a batch whose every digest was a leaf already")
        if int(info[3]):
            ev.add("a batch with repeats")
        if build.get("reserve_trees") and build.get("mutated"):
            ev.add("reserve_trees > 0 and mutated=True")
        if "reserve_trees" not in build and build.get("max_count") == max(after.counts):
            ev.add("an explicit max_count equal to the largest count of the result")
        for a, b, new in zip(before.trees, b_sorted, after.trees):
            if crossed(len(a), len(new)):
                ev.add("a count crossing a power of two upwards" if len(new) > len(a) else "a count crossing a power of two downwards")
            if a and not new:
                ev.add(f"a tree emptied by {kind}")
            if kind == "insert" and b and not a:
                ev.add("an insert into an empty tree")
            if kind == "insert" and a and new[0] < a[0]:
                ev.add("an insert below a tree's first leaf")
            if kind == "insert" and a and new[-1] > a[-1]:
                ev.add("an insert above a tree's last leaf")
            if kind == "remove" and a and new and a[0] != new[0]:
                ev.add("the first leaf removed")
            if kind == "remove" and a and new and a[-1] != new[-1]:
                ev.add("the last leaf removed")
            if any(r[:7] == x[:7] and r != x for r in b for x in a):
                ev.add("a batch row equal to a leaf in words 0..6")
            if any(x[:2] == y[:2] and x != y for x, y in zip(b, b[1:])):
                ev.add("two batch rows equal in words 0 and 1")

    # -- the questions asked after every step ------------------------------------------------------------------------------------------
    def absence_queries(self, m=None):
        """(trees, digests, present): every leaf and every gap of every tree in use, and the all-zero digest in every tree behind."""
        m = self.m if m is None else m
        out = []
        for t in range(m.used_trees):
            rows = m.rows(t)
            out += [(t, rows[i], True) for i in range(len(rows))]
            out += [(t, x, False) for x in (m.gap(t, g) for g in range(len(rows) + 1)) if x is not None]
        out += [(t, np.zeros(8, np.uint32), False) for t in range(m.used_trees, m.ntrees)]
        return (np.array([o[0] for o in out], dtype=np.uint32), np.array([o[1] for o in out], dtype=np.uint32).reshape(-1, 8),
                np.array([o[2] for o in out], dtype=bool))

    def range_queries(self):
        """(trees, lo, hi): per tree, the unused ones included, the whole range and four drawn pairs of leaves and gaps; one
        hi < lo; one tree outside the forest."""
        m, ask = self.m, self.ask
        zero, ones = np.zeros(8, np.uint32), np.full(8, 0xFFFFFFFF, np.uint32)
        out = []
        for t in range(m.ntrees):
            rows = m.rows(t)
            out.append((t, zero, ones))
            marks = [x for g in range(len(rows) + 1) for x in (m.gap(t, g), rows[g] if g < len(rows) else None) if x is not None]
            for _ in range(4):
                i, j = sorted(int(x) for x in ask.integers(0, len(marks), size=2))
                out.append((t, marks[i], marks[j]))
        out.append((int(ask.integers(0, m.ntrees)), ones, zero))
        out.append((m.ntrees + int(ask.integers(0, 3)), zero, ones))
        return (np.array([o[0] for o in out], dtype=np.uint32), np.array([o[1] for o in out], dtype=np.uint32).reshape(-1, 8),
                np.array([o[2] for o in out], dtype=np.uint32).reshape(-1, 8))

    def answers(self):
        """Everything the model answers to the questions of this step, as a dict: the absence table (`trees`, `digests`, `present`),
        `lower_bound`, `absence` and its `verdicts` under the model's own roots and counts, `find`; the range table (`r_trees`, `lo`,
        `hi`), `ranges` and `r_verdicts`."""
        m = self.m
        roots, counts = m.roots(), m.counts
        trees, digests, present = self.absence_queries()
        out = {"trees": trees, "digests": digests, "present": present, "roots": roots, "counts": counts, "lower_bound": m.lower_bound(trees, digests),
               "absence": m.absence(trees, digests), "find": m.find(digests)}
        out["verdicts"] = absence_verdicts(trees, digests, out["absence"], roots, counts)
        assert (out["verdicts"] == np.where(present, PRESENT, ABSENT)).all() and (out["lower_bound"][1] == present).all()
        out["r_trees"], out["lo"], out["hi"] = self.range_queries()
        out["ranges"] = m.ranges(out["r_trees"], out["lo"], out["hi"])
        out["r_verdicts"] = range_verdicts(out["r_trees"], out["lo"], out["hi"], out["ranges"], roots, counts)
        return out
