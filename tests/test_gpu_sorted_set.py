"""Sorted trees on the GPU against ONE model (tests/sorted_set_cases.py).

Every shape: EVERY, the forest of 41 trees of 0 .. 40 leaves, stored once by build_forest at offset 0 and once through the raw calls
at offsets[0] == 37 with slack behind; every leaf and every gap of every tree through the lower bound and the absence gather, every
pair of gaps through the range gather (12 341 queries in one call, in its two-call form), cell for cell between guard cells; both
batches verified on the device under the true roots and counts, under counts + 1, counts - 1 and the roots rotated by one tree; the
one-tree twins for the trees of 1, 22 and 40 leaves.

The walk: every sorted operation directly after every other (sort_build, insert, remove, common, update_in_order, disorder), and
after EVERY step everything the forest answers compared with the model, never one device result with another: the handle's books,
the offsets, level 0, the roots, the sortedness pass, the audit, every leaf and every gap of every tree through lower_bound, absence
and find, ranges, both verifiers as a follower that holds only the model's roots and counts, the proofs of the step before under
the roots of now, and a stored MerkleTree that takes tree 0's share of every merge.  A failure prints (config, seed, step, kind, the
kind before): the walk can be replayed on the model alone."""
import numpy as np
import pytest

import absence_cases as ac
import forest_update_cases as fu
import range_cases as rc
import sorted_set_cases as sc
from merkle_model import At

pytestmark = pytest.mark.gpu

GUARD = 4                                                    # guard cells on either side of every output
WALKS = [(name, seed) for name in sorted(sc.CONFIGS) for seed in sc.SEEDS[name]]
PLACEMENTS = ("at 0", "at 37")


def guarded(tmp, n, fill, dtype, width=1):
    return tmp.upload(np.full((n + 2 * GUARD) * width, fill, dtype))


def inner(gpu, buf, n, fill, dtype, width=1):
    """The n items between the guards, which must still be the fill."""
    got = gpu.download(buf, (n + 2 * GUARD) * width * np.dtype(dtype).itemsize, dtype=dtype).reshape(n + 2 * GUARD, width)
    assert (got[:GUARD] == fill).all() and (got[-GUARD:] == fill).all()
    return got[GUARD:-GUARD]


def at(buf, dtype, width=1):
    return At(buf, GUARD * width * np.dtype(dtype).itemsize)


def device_sorted(gpu, forest):
    """(first_bad [ntrees], info [4]) of one raw call, between guards."""
    with gpu.scope() as tmp:
        d_bad, d_info = guarded(tmp, forest.ntrees, ac.INDEX_FILL, np.uint64), guarded(tmp, 4, ac.INDEX_FILL, np.uint64)
        gpu.forest_sorted_enqueue(forest.digests, forest.total, forest.offsets, forest.ntrees, at(d_bad, np.uint64), at(d_info, np.uint64))
        return inner(gpu, d_bad, forest.ntrees, ac.INDEX_FILL, np.uint64)[:, 0], inner(gpu, d_info, 4, ac.INDEX_FILL, np.uint64)[:, 0]


def device_lower_bound(gpu, forest, trees, digests):
    Q = len(trees)
    with gpu.scope() as tmp:
        d_idx, d_found = guarded(tmp, Q, ac.INDEX_FILL, np.uint64), guarded(tmp, Q, ac.CANARY, np.uint32)
        gpu.forest_lower_bound_enqueue(forest.digests, forest.total, forest.offsets, forest.ntrees, tmp.upload(trees), tmp.upload(digests), Q,
                                       at(d_idx, np.uint64), at(d_found, np.uint32))
        return inner(gpu, d_idx, Q, ac.INDEX_FILL, np.uint64)[:, 0], inner(gpu, d_found, Q, ac.CANARY, np.uint32)[:, 0]


def device_absence(gpu, forest, trees, digests, stride):
    """(indices, pred, succ, main, low, heights) of one raw call, every output between guards that start as the canary."""
    Q = len(trees)
    with gpu.scope() as tmp:
        d_idx, d_h = guarded(tmp, Q, ac.INDEX_FILL, np.uint64), guarded(tmp, Q, ac.CANARY, np.uint32)
        d_nb = guarded(tmp, 2 * Q, ac.CANARY, np.uint32, 8)
        d_main, d_low = guarded(tmp, Q * stride, ac.CANARY, np.uint32, 8), guarded(tmp, Q * stride, ac.CANARY, np.uint32, 8)
        gpu.forest_absence_enqueue(forest.digests, forest.forest, forest.total, forest.offsets, forest.ntrees, forest.max_count, tmp.upload(trees),
                                   tmp.upload(digests), Q, stride, at(d_idx, np.uint64), at(d_nb, np.uint32, 8), at(d_main, np.uint32, 8),
                                   at(d_low, np.uint32, 8), at(d_h, np.uint32))
        nb = inner(gpu, d_nb, 2 * Q, ac.CANARY, np.uint32, 8).reshape(Q, 2, 8)
        return (inner(gpu, d_idx, Q, ac.INDEX_FILL, np.uint64)[:, 0], nb[:, 0], nb[:, 1], inner(gpu, d_main, Q * stride, ac.CANARY, np.uint32, 8).reshape(Q, stride, 8),
                inner(gpu, d_low, Q * stride, ac.CANARY, np.uint32, 8).reshape(Q, stride, 8), inner(gpu, d_h, Q, ac.CANARY, np.uint32)[:, 0])


def device_verify_absence(gpu, digests, trees, indices, pred, succ, main, low, heights, roots, counts):
    """verdict [Q] of one raw call, between guards."""
    Q, stride = len(trees), int(main.shape[1])
    nb = np.ascontiguousarray(np.stack([pred, succ], axis=1))
    with gpu.scope() as tmp:
        d_verdict = guarded(tmp, Q, ac.CANARY, np.uint32)
        ups = [tmp.upload(np.ascontiguousarray(a, dtype=t)) for a, t in ((digests, np.uint32), (trees, np.uint32), (indices, np.uint64), (nb, np.uint32),
                                                                       (main, np.uint32), (low, np.uint32), (heights, np.uint32))]
        gpu.verify_forest_absence_enqueue(*ups, Q, stride, tmp.upload(np.ascontiguousarray(roots, dtype=np.uint32)),
                                          tmp.upload(np.ascontiguousarray(counts, dtype=np.uint64)), len(counts), at(d_verdict, np.uint32))
        return inner(gpu, d_verdict, Q, ac.CANARY, np.uint32)[:, 0]


def device_range(gpu, forest, trees, lo, hi, stride, capacity):
    """(firsts, leaf_starts, leaves [capacity, 8], left, right, heights, info) of one raw call, every output between guards that
    start as the canary, the leaves included: what the call does not write is still the canary."""
    Q = len(trees)
    with gpu.scope() as tmp:
        d_first, d_starts = guarded(tmp, Q, rc.INDEX_FILL, np.uint64), guarded(tmp, Q + 1, rc.INDEX_FILL, np.uint64)
        d_h, d_info = guarded(tmp, Q, rc.CANARY, np.uint32), guarded(tmp, 4, rc.INDEX_FILL, np.uint64)
        d_leaves = guarded(tmp, capacity, rc.CANARY, np.uint32, 8)
        d_left, d_right = guarded(tmp, Q * stride, rc.CANARY, np.uint32, 8), guarded(tmp, Q * stride, rc.CANARY, np.uint32, 8)
        forest.range_async(tmp.upload(trees), tmp.upload(lo), tmp.upload(hi), Q, stride, tmp.alloc(gpu.range_scratch_bytes(0, Q)), at(d_first, np.uint64),
                           at(d_starts, np.uint64), at(d_leaves, np.uint32, 8), capacity, at(d_left, np.uint32, 8), at(d_right, np.uint32, 8),
                           at(d_h, np.uint32), at(d_info, np.uint64))
        return (inner(gpu, d_first, Q, rc.INDEX_FILL, np.uint64)[:, 0], inner(gpu, d_starts, Q + 1, rc.INDEX_FILL, np.uint64)[:, 0],
                inner(gpu, d_leaves, capacity, rc.CANARY, np.uint32, 8), inner(gpu, d_left, Q * stride, rc.CANARY, np.uint32, 8).reshape(Q, stride, 8),
                inner(gpu, d_right, Q * stride, rc.CANARY, np.uint32, 8).reshape(Q, stride, 8), inner(gpu, d_h, Q, rc.CANARY, np.uint32)[:, 0],
                inner(gpu, d_info, 4, rc.INDEX_FILL, np.uint64)[:, 0])


def device_verify_range(gpu, trees, lo, hi, firsts, starts, leaves, left, right, heights, roots, counts):
    """(verdict, in_first, in_count) of one raw call, between guards."""
    Q, stride, n = len(trees), int(left.shape[1]), int(leaves.shape[0])
    with gpu.scope() as tmp:
        d_verdict, d_first, d_count = guarded(tmp, Q, rc.CANARY, np.uint32), guarded(tmp, Q, rc.INDEX_FILL, np.uint64), guarded(tmp, Q, rc.INDEX_FILL, np.uint64)
        up = lambda a, t: tmp.upload(np.ascontiguousarray(a, dtype=t))                               # noqa: E731
        gpu.verify_forest_range_enqueue(up(trees, np.uint32), up(lo, np.uint32), up(hi, np.uint32), up(firsts, np.uint64), up(starts, np.uint64),
                                        up(leaves, np.uint32) if n else None, n, up(left, np.uint32), up(right, np.uint32), up(heights, np.uint32), Q, stride,
                                        up(roots, np.uint32), up(counts, np.uint64), len(counts), tmp.alloc(gpu.range_scratch_bytes(n, Q)),
                                        at(d_verdict, np.uint32), at(d_first, np.uint64), at(d_count, np.uint64))
        return (inner(gpu, d_verdict, Q, rc.CANARY, np.uint32)[:, 0], inner(gpu, d_first, Q, rc.INDEX_FILL, np.uint64)[:, 0],
                inner(gpu, d_count, Q, rc.INDEX_FILL, np.uint64)[:, 0])


def same(got, want, names, note):
    """Array for array; a failure names the array and the first rows that differ -- with the query tables, the smallest (count,
    query)."""
    for what, a, b in zip(names, got, want):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape and (a == b).all(), (note, what, np.nonzero((a != b).reshape(a.shape[0], -1).any(axis=1))[0][:8])


ABSENCE = ("indices", "pred", "succ", "main", "low", "heights")
RANGES = ("firsts", "leaf_starts", "leaves", "left", "right", "heights", "info")
VERDICTS = ("verdict", "in_first", "in_count")


# ---- every shape ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def every():
    return sc.every()


@pytest.fixture(scope="module")
def stored(gpu, every):
    """EVERY on the device, built once: {"at 0": by build_forest, "at 37": through the raw calls with offsets[0] == 37 and 20
    cells behind}."""
    forest = gpu.build_forest(every.image(), every.counts)
    cells, offsets = every.placed(first=37, slack=20)
    raw = fu.RawForest(gpu, cells, every.counts, 40, first=37)
    assert int(offsets[0]) == 37 and raw.total == 877 and forest.levels == raw.handle.levels == sc.EVERY_STRIDE
    yield {"at 0": forest, "at 37": raw.handle}
    raw.free()
    forest.free()


@pytest.mark.parametrize("where", PLACEMENTS)
def test_every_leaf_and_every_gap_of_every_tree_through_the_lower_bound_and_the_absence_gather(gpu, every, stored, where):
    forest = stored[where]
    trees, digests, present = every.absence_queries()
    idx, found, *rest = every.absence_expected()
    same(device_lower_bound(gpu, forest, trees, digests), (idx, found), ("indices", "found"), where)
    same(device_absence(gpu, forest, trees, digests, sc.EVERY_STRIDE), [idx] + rest, ABSENCE, where)       # the cells the rule does not name are zero
    assert (forest.roots() == every.roots()).all() and forest.is_sorted()


@pytest.mark.parametrize("name", sc.ALTERATIONS)
def test_the_absence_batch_of_every_shape_verified_on_the_device(gpu, every, name):
    trees, digests, present = every.absence_queries()
    idx, found, *rest = every.absence_expected()
    _, roots, counts = sc.alterations(every.roots(), every.counts)[sc.ALTERATIONS.index(name)]
    got = device_verify_absence(gpu, digests, trees, idx, *rest, roots, counts)
    want = every.absence_verdicts_under(name)
    assert (got == want).all(), (name, [(int(trees[q]), q) for q in np.nonzero(got != want)[0][:8]])


@pytest.mark.parametrize("where", PLACEMENTS)
def test_every_pair_of_gaps_of_every_tree_through_the_range_gather_in_two_calls(gpu, every, stored, where):
    forest = stored[where]
    trees, lo, hi = every.range_queries()
    want = every.range_expected()
    counted = device_range(gpu, forest, trees, lo, hi, sc.EVERY_STRIDE, 0)                          # no leaf cell to write: bit 0 and the total
    assert counted[6].tolist() == [1, sc.EVERY_CARRIED, 0, sc.EVERY_IN_RANGE], where
    same(counted[:2] + counted[3:6], want[:2] + want[3:6], RANGES[:2] + RANGES[3:6], (where, "counted"))
    got = device_range(gpu, forest, trees, lo, hi, sc.EVERY_STRIDE, int(counted[6][1]))
    same(got, want, RANGES, where)


@pytest.mark.parametrize("name", sc.ALTERATIONS)
def test_the_range_batch_of_every_shape_verified_on_the_device(gpu, every, name):
    trees, lo, hi = every.range_queries()
    proofs = every.range_expected()
    _, roots, counts = sc.alterations(every.roots(), every.counts)[sc.ALTERATIONS.index(name)]
    got = device_verify_range(gpu, trees, lo, hi, *proofs[:6], roots, counts)
    want = every.range_verdicts_under(name)
    for what, a, b in zip(VERDICTS, got, want):
        bad = np.nonzero(a != b)[0]
        assert bad.size == 0, (name, what, [(int(trees[q]), int(proofs[0][q]), int(proofs[1][q + 1] - proofs[1][q])) for q in bad[:8]])     # (count, first, run)


@pytest.mark.parametrize("count", sc.EVERY_TRIPLES)
def test_the_one_tree_twins_of_every_shape(gpu, every, count):
    """Tree `count` of EVERY as a stored MerkleTree with its share of both tables: the same answers, the rows as long as the tree's
    own height."""
    import vk_merkle_roots_amd as vk
    t = count
    leaves, root = every.rows(t), every.roots()[t]
    mine, theirs = every.share(t)
    d_leaves = gpu.upload(leaves)
    tree = gpu.build_tree(d_leaves, count)
    try:
        h = tree.height
        assert h == ac.height(count) and tree.is_sorted() and (tree.root() == root).all()
        _, digests, present = (x[mine] for x in every.absence_queries())
        idx, found, pred, succ, main, low, heights = (x[mine] for x in every.absence_expected())
        got = tree.lower_bound(digests)
        assert (got[0] == idx).all() and (got[1] == present).all()
        proofs = tree.absence(digests)
        assert proofs.same_as(vk.AbsenceProofs(np.zeros(len(mine), np.uint32), digests, idx, pred, succ, main[:, :h], low[:, :h], heights))
        assert (proofs.verify(gpu, root[None], [count]) == every.absence_verdicts_under("true")[mine]).all()
        Q = len(mine)
        with gpu.scope() as tmp:                                                                     # the twin's own check: one root, one count
            d_verdict = guarded(tmp, Q, ac.CANARY, np.uint32)
            gpu.verify_absence_enqueue(tmp.upload(digests), tmp.upload(proofs.indices), tmp.upload(proofs.neighbours), tmp.upload(proofs.main),
                                       tmp.upload(proofs.low), Q, h, tmp.upload(tree.root()), count, at(d_verdict, np.uint32))
            assert (inner(gpu, d_verdict, Q, ac.CANARY, np.uint32)[:, 0] == np.where(present, sc.PRESENT, sc.ABSENT)).all()
        _, lo, hi = (x[theirs] for x in every.range_queries())
        e = every.range_expected()
        runs = [e[2][int(e[1][q]): int(e[1][q + 1])] for q in theirs]
        starts = np.concatenate([[0], np.cumsum([len(r) for r in runs])]).astype(np.uint64)
        Q = len(theirs)
        ranges = tree.range(lo, hi)
        assert ranges.same_as(vk.RangeProofs(np.zeros(Q, np.uint32), lo, hi, e[0][theirs], starts, np.concatenate(runs), e[3][theirs][:, :h], e[4][theirs][:, :h],
                                             np.full(Q, h, np.uint32)))
        want = [x[theirs] for x in every.range_verdicts_under("true")]
        same(ranges.verify(gpu, root[None], [count]), want, VERDICTS, count)
        n = int(starts[-1])
        with gpu.scope() as tmp:
            d_verdict, d_first, d_count = guarded(tmp, Q, rc.CANARY, np.uint32), guarded(tmp, Q, rc.INDEX_FILL, np.uint64), guarded(tmp, Q, rc.INDEX_FILL, np.uint64)
            gpu.verify_range_enqueue(tmp.upload(ranges.lo), tmp.upload(ranges.hi), tmp.upload(ranges.firsts), tmp.upload(ranges.leaf_starts),
                                     tmp.upload(ranges.leaves), n, tmp.upload(ranges.left), tmp.upload(ranges.right), Q, h, tmp.upload(tree.root()), count,
                                     tmp.alloc(gpu.range_scratch_bytes(n, Q)), at(d_verdict, np.uint32), at(d_first, np.uint64), at(d_count, np.uint64))
            same((inner(gpu, d_verdict, Q, rc.CANARY, np.uint32)[:, 0], inner(gpu, d_first, Q, rc.INDEX_FILL, np.uint64)[:, 0],
                  inner(gpu, d_count, Q, rc.INDEX_FILL, np.uint64)[:, 0]), want, VERDICTS, (count, "the twin's own check"))
    finally:
        tree.free()
        d_leaves.free()


# ---- the walk ---------------------------------------------------------------------------------------------------------------------------

def level_0(gpu, forest, n):
    return gpu.download(forest.digests, 32 * n).reshape(n, 8) if n else np.zeros((0, 8), np.uint32)


def state_equals_model(gpu, forest, m, note):
    """The handle's books, the offsets, the live cells of level 0 and the roots."""
    for name, want in m.books().items():
        got = getattr(forest, name)
        assert (got.tolist() if name == "counts" else got) == want, (note, name, got, want)
    assert (gpu.download(forest.offsets, 8 * (m.ntrees + 1), dtype=np.uint64) == m.offsets()).all(), (note, "offsets")
    assert (level_0(gpu, forest, m.live) == m.image()).all(), (note, "level 0")
    assert (forest.roots() == m.roots()).all(), (note, "roots")


def everything_equals_model(gpu, vk, forest, tree, life, previous, note):
    """Everything the forest and the stored tree answer after a step, against the model; the answers, for the step behind."""
    m, a = life.m, life.answers()
    roots, counts = a["roots"], a["counts"]                                                          # what the follower holds: the model's
    state_equals_model(gpu, forest, m, note)
    assert forest.is_sorted() and (forest.first_unsorted() == sc.NONE).all() and forest.audit().clean, note
    # every leaf and every gap of every tree in use, the all-zero digest in every tree behind
    idx, found = forest.lower_bound(a["trees"], a["digests"])
    assert (idx == a["lower_bound"][0]).all() and (found == a["present"]).all(), (note, "lower_bound")
    proofs = forest.absence(a["trees"], a["digests"])
    same([getattr(proofs, n) for n in ABSENCE], a["absence"], ABSENCE, note)
    absent = proofs.verify(gpu, roots, counts)
    assert (absent == a["verdicts"]).all(), (note, "the follower's verdicts")
    if previous is not None:                                                                         # the proofs of before under the roots of now
        old = vk.AbsenceProofs(previous["trees"], previous["digests"], *previous["absence"])
        want = sc.absence_verdicts(previous["trees"], previous["digests"], previous["absence"], roots, counts)
        assert (old.verify(gpu, roots, counts) == want).all(), (note, "the proofs of before")
    got = forest.find(a["digests"])
    assert (got[0] == a["find"][0]).all() and (got[1] == a["find"][1]).all(), (note, "find")
    # the ranges
    ranges = forest.ranges(a["r_trees"], a["lo"], a["hi"])
    same([getattr(ranges, n) for n in RANGES], a["ranges"], RANGES, note)
    verdict, in_first, in_count = ranges.verify(gpu, roots, counts)
    same((verdict, in_first, in_count), a["r_verdicts"], VERDICTS, note)
    for q, t in enumerate(a["r_trees"].tolist()):
        inside = ranges.in_range(q)
        assert inside.shape[0] == int(in_count[q]) and (verdict[q] == 0 or (inside == m.rows(t)[int(in_first[q]): int(in_first[q] + in_count[q])]).all()), (note, q)
    for t in range(m.used_trees, m.ntrees):                                                          # a tree behind the ones in use: nothing is in it
        mine, theirs = a["trees"] == t, (a["r_trees"] == t) & (a["ranges"][0] != sc.NONE)              # its one digest; its five ranges in order
        assert mine.sum() == 1 and (absent[mine] == sc.ABSENT).all(), (note, t, "what the device answered")
        assert theirs.sum() == 5 and (verdict[theirs] == 1).all() and not in_count[theirs].any() and not in_first[theirs].any(), (note, t)
    # the stored tree
    one = sc.ModelSet([life.tree])
    rows, c = one.rows(0), len(life.tree)
    assert tree.count == c and tree.height == one.levels and (tree.level(0) == rows).all() and (tree.root() == one.roots()[0]).all() and tree.is_sorted(), (note, "tree")
    trees, digests, present = life.absence_queries(one)
    got = tree.lower_bound(digests)
    want = one.lower_bound(trees, digests)
    assert (got[0] == want[0]).all() and (got[1] == present).all(), (note, "tree.lower_bound")
    proofs = tree.absence(digests)
    same([getattr(proofs, n) for n in ABSENCE], one.absence(trees, digests), ABSENCE, (note, "tree.absence"))
    assert (proofs.verify(gpu, one.roots(), [c]) == np.where(present, sc.PRESENT, sc.ABSENT)).all(), (note, "tree.absence verified")
    gaps = [one.gap(0, g) for g in range(c + 1)]
    pairs = [(gaps[g], gaps[min(g + 2, c)]) for g in range(c + 1) if gaps[g] is not None and gaps[min(g + 2, c)] is not None]
    lo = np.array([np.zeros(8, np.uint32)] + [p[0] for p in pairs], dtype=np.uint32)
    hi = np.array([np.full(8, 0xFFFFFFFF, np.uint32)] + [p[1] for p in pairs], dtype=np.uint32)
    trees = np.zeros(len(lo), np.uint32)
    ranges = tree.range(lo, hi)
    want = one.ranges(trees, lo, hi)
    same([getattr(ranges, n) for n in RANGES], want, RANGES, (note, "tree.range"))
    same(ranges.verify(gpu, one.roots(), [c]), sc.range_verdicts(trees, lo, hi, want, one.roots(), [c]), VERDICTS, (note, "tree.range verified"))
    return a


@pytest.mark.parametrize("name,seed", WALKS, ids=[f"{n}-{s}" for n, s in WALKS])
def test_every_sorted_operation_after_every_other_against_the_model(gpu, name, seed):
    import vk_merkle_roots_amd as vk
    life = sc.SetLife(seed, sc.CONFIGS[name])
    made = []                                                # every forest, tree and buffer this walk made
    try:
        forest, _ = gpu.build_sorted_forest(life.m.image(), life.m.counts)
        made.append(forest)
        d_first = gpu.upload(sc.rows_of(life.tree))
        made.append(d_first)
        tree = gpu.build_tree(d_first, len(life.tree))
        made.append(tree)
        previous = everything_equals_model(gpu, vk, forest, tree, life, None, (name, seed, "start"))
        for number, kind, p in life.steps():
            note = (name, seed, number, kind, life.last)
            merge = kind in sc.MERGES
            if kind == "sort_build":
                new, order = gpu.build_sorted_forest(p["leaves"], p["counts"], **p["build"])
                made.append(new)
                out = life.apply(kind, p)
                assert (p["leaves"][order.astype(np.int64)] == life.m.image()).all(), (note, "order")
            elif merge:
                was = life.m.copy()
                new, info = getattr(forest, sc.METHODS[kind])(p["batch"], p["counts"], **p["build"])
                made.append(new)
                state_equals_model(gpu, forest, was, (note, "the source"))                            # only read
                out = life.apply(kind, p)
                assert info.tolist() == out["info"], (note, info, out["info"])
                if p["build"].get("mutated"):
                    assert new.built_mutated.shape == (life.m.ntrees,) and not new.built_mutated.any(), note
                else:
                    assert new.built_mutated is None, note
                method = getattr(tree, sc.METHODS[kind])
                if out["tree_left"]:
                    other, info = method(p["tree_batch"])
                    made.append(other)
                    assert info.tolist() == out["tree_info"], (note, "tree", info, out["tree_info"])
                    tree.free()
                    tree = other
                else:
                    with pytest.raises(ValueError, match="no leaf is left"):
                        method(p["tree_batch"])
            elif kind == "update_in_order":
                forest.update(p["trees"], p["indices"], p["values"])
                life.apply(kind, p)
            else:
                if not p["degenerate"]:
                    forest.update([p["tree"]], [p["index"]], p["bad"])
                    want_bad, want_info = life.bend(p)
                    bad, info = device_sorted(gpu, forest)
                    assert (bad == want_bad).all() and info.tolist() == want_info and not forest.is_sorted(), (note, bad, info)
                    for method in sc.METHODS.values():
                        with pytest.raises(RuntimeError, match="bit 2: a tree of A is not strictly increasing"):
                            getattr(forest, method)(p["batch"], p["counts"])
                    state_equals_model(gpu, forest, life.m, (note, "refused three times"))
                    forest.update([p["tree"]], [p["index"]], p["good"])
                    life.mend(p)
                else:
                    assert forest.is_sorted(), note
                life.apply(kind, p)
            if kind == "sort_build" or merge:                # the new forest replaces the handle
                forest.free()
                forest = new
            previous = everything_equals_model(gpu, vk, forest, tree, life, previous if merge else None, note)
    finally:
        for x in made:
            x.free()
