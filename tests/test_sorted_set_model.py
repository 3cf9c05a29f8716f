"""tests/sorted_set_cases.py without a GPU: the circuit takes every ordered pair of the six kinds once and every walk performs them
all; no walk hides a kind behind degenerate steps; over the three seeds of a config every one of EVENTS occurs; after every step of
every walk the model is what the CPU twins of libvkmr_host.so compute -- the leaf sort, the merge with its offsets and info, the
sortedness pass, the lower bound, the absence and range gathers and their verifiers --; and for EVERY the model's proofs and
verdicts are the twins' for both tables, under the true roots and counts and under the three alterations, with the assertions that
keep the GPU comparisons from passing vacuously."""
import itertools

import numpy as np
import pytest

import absence_cases as ac
import leafsort_cases as lc
import merge_cases as mc
import range_cases as rc
import sorted_set_cases as sc

WALKS = [(name, seed) for name in sorted(sc.CONFIGS) for seed in sc.SEEDS[name]]


def offsets_of(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)


def model_walk(name, seed):
    """The walk on the model alone, finished."""
    life = sc.SetLife(seed, sc.CONFIGS[name])
    for _, kind, p in life.steps():
        if kind == "disorder" and not p["degenerate"]:
            life.bend(p)
            life.mend(p)
        life.apply(kind, p)
    return life


@pytest.fixture(scope="module")
def lives():
    return {(name, seed): model_walk(name, seed) for name, seed in WALKS}


def test_the_circuit_takes_every_ordered_pair_once_and_every_walk_performs_them_all(lives):
    every_pair = set(itertools.product(sc.KINDS, repeat=2))
    assert len(sc.CIRCUIT) == 36 and len(sc.SEQUENCE) == 37 and sc.SEQUENCE[-1] == sc.SEQUENCE[0]
    pairs = list(zip(sc.SEQUENCE, sc.SEQUENCE[1:]))
    assert len(pairs) == len(set(pairs)) == 36 and set(pairs) == every_pair == sc.pairs_of(sc.SEQUENCE)
    for walk, life in lives.items():
        assert life.pairs == every_pair and sum(life.done.values()) == 37, walk


def test_at_most_a_quarter_of_a_kinds_steps_are_degenerate(lives):
    for walk, life in lives.items():
        for kind in sc.KINDS:
            assert life.done[kind] >= 6 and 4 * life.degenerate[kind] <= life.done[kind], (walk, kind, life.degenerate[kind], life.done[kind])


@pytest.mark.parametrize("name", sorted(sc.CONFIGS))
def test_over_the_three_seeds_of_a_config_every_event_occurs(lives, name):
    seen = set().union(*(lives[name, seed].events for seed in sc.SEEDS[name]))
    assert len(sc.SEEDS[name]) == 3 and seen == set(sc.EVENTS), sorted(set(sc.EVENTS) - seen)


def same(got, want, note):
    for j, (a, b) in enumerate(zip(got, want)):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape and (a == b).all(), (note, j)


def twins_of_the_readers(life, note, previous):
    """The sortedness pass, the lower bound, both gathers and both verifiers of libvkmr_host.so over the model's level 0: what
    the model answers.  `previous`: the absence batch of the step before, verified once more under the roots as they are now."""
    m, a = life.m, life.answers()
    cells, offsets, stride = m.image(), m.offsets(), m.levels
    rc_, bad, info = ac.host_sorted(cells, offsets)
    want_bad, want_info = m.first_bad()
    assert rc_ == 0 and (bad == want_bad).all() and info.tolist() == want_info and m.is_sorted(), note
    same(ac.host_lower_bound(cells, offsets, a["trees"], a["digests"]), a["lower_bound"], (note, "lower_bound"))
    got = ac.host_absence(cells, offsets, a["trees"], a["digests"], stride)
    assert got[0] == 0
    same(got[1:], a["absence"], (note, "absence"))
    assert (ac.host_verify(a["digests"], a["trees"], *a["absence"], a["roots"], a["counts"]) == a["verdicts"]).all(), note
    n = int(a["ranges"][6][1])
    got = rc.host_range(cells, offsets, a["r_trees"], a["lo"], a["hi"], stride, capacity=n, guard=0)
    assert got[0] == 0
    same(got[1:], a["ranges"], (note, "ranges"))
    same(rc.host_verify(a["r_trees"], a["lo"], a["hi"], *a["ranges"][:6], a["roots"], a["counts"]), a["r_verdicts"], (note, "range verdicts"))
    assert (a["r_verdicts"][0] == (a["ranges"][0] != sc.NONE)).all(), note                          # whatever was gathered is proven
    # find against the lower bound: a digest found in its own tree stands at its lower bound; one that is no leaf of its tree is
    # found, if at all, in a tree in front of it
    trees, indices = a["find"]
    for q in range(len(a["trees"])):
        if a["present"][q]:
            assert trees[q] <= a["trees"][q] and (trees[q] != a["trees"][q] or indices[q] == a["lower_bound"][0][q]), (note, q)
        else:
            assert trees[q] == sc.NO_TREE or trees[q] != a["trees"][q], (note, q)
    if previous is not None:
        want = sc.absence_verdicts(previous["trees"], previous["digests"], previous["absence"], a["roots"], a["counts"])
        assert (ac.host_verify(previous["digests"], previous["trees"], *previous["absence"], a["roots"], a["counts"]) == want).all(), (note, "the proofs of before")
    return a


@pytest.mark.parametrize("name,seed", WALKS, ids=[f"{n}-{s}" for n, s in WALKS])
def test_after_every_step_the_model_is_what_the_cpu_twins_compute(native, name, seed):
    life = sc.SetLife(seed, sc.CONFIGS[name])
    previous = twins_of_the_readers(life, (name, seed, "start"), None)
    before_tree = list(life.tree)
    for number, kind, p in life.steps():
        note = (name, seed, number, kind, life.last)
        before = life.m.copy()
        if kind == "disorder" and not p["degenerate"]:
            want_bad, want_info = life.bend(p)
            rc_, bad, info = ac.host_sorted(life.m.image(), life.m.offsets())
            assert rc_ == 0 and (bad == want_bad).all() and info.tolist() == want_info and int(bad[p["tree"]]) != sc.NONE, note
            b_off = offsets_of(p["counts"])
            for op in mc.OPS:                                                                       # refused, and nothing written
                case = mc.Case("", life.m.image(), life.m.offsets()[: life.m.used_trees + 1], lc.host_sort(p["batch"], b_off, 1)[1], b_off)
                rc_, out, out_offsets, origin, info = mc.host_merge(case, op)
                assert rc_ == 0 and info.tolist() == [sc.A_NOT_INCREASING, 0, 0, 0] and (out == mc.CANARY).all() and (out_offsets == mc.OFFSET_FILL).all(), note
                same(mc.model_merge(case, op), (out, out_offsets, origin, info), note)
            life.mend(p)
        out = life.apply(kind, p)
        m = life.m
        if kind == "sort_build":
            cells, offsets = p["leaves"], offsets_of(p["counts"])
            max_count = p["build"].get("max_count", max([1] + p["counts"]))
            rc_, got, order, info = lc.host_sort(cells, offsets, max_count)
            want = lc.model_sort(cells, offsets, max_count)
            assert rc_ == 0 and (got == want[0]).all() and (order == want[1]).all() and info.tolist() == want[2].tolist(), note
            assert (got == m.image()).all() and info.tolist()[:2] == [0, m.live] and int(info[3]) == 0, note
        elif kind in sc.MERGES:
            op, b_off = sc.MERGES[kind], offsets_of(p["counts"])
            rc_, b_sorted, _, info = lc.host_sort(p["batch"], b_off, max([1] + p["counts"]))
            assert rc_ == 0 and int(info[0]) == 0 and (b_sorted == out["case"].b_cells).all(), note          # the batch as the merge takes it
            rc_, got, got_offsets, origin, info = mc.host_merge(out["case"], op)
            assert rc_ == 0, note
            same((got, got_offsets, origin, info), mc.model_merge(out["case"], op), note)
            n = int(info[1])
            assert info.tolist() == out["info"] and n == m.live and (got[:n] == m.image()).all() and (got_offsets == m.offsets()[: m.used_trees + 1]).all(), note
            one = mc.Case("", sc.rows_of(before_tree), offsets_of([len(before_tree)]), sc.rows_of(sorted(mc.words(r) for r in p["tree_batch"])),
                          offsets_of([len(p["tree_batch"])]))
            rc_, got, _, _, info = mc.host_merge(one, op, one_tree=True)
            assert rc_ == 0 and info.tolist() == out["tree_info"], note                              # the stored tree: the one-tree twin
            if out["tree_left"]:
                assert (got[: out["tree_left"]] == sc.rows_of(life.tree)).all(), note
            else:
                assert life.tree == before_tree, note
        previous = twins_of_the_readers(life, note, previous if kind in sc.MERGES else None)
        before_tree = list(life.tree)


# ---- EVERY ----------------------------------------------------------------------------------------------------------------------------

def test_every_shape_of_the_absence_table_is_the_cpu_twins(native):
    e = sc.every()
    trees, digests, present = e.absence_queries()
    idx, found, *rest = e.absence_expected()
    cells, offsets = e.placed(first=37, slack=20)
    same(ac.host_lower_bound(cells, offsets, trees, digests), (idx, found), "lower_bound")
    assert (found == present).all() and len(trees) == 1681 and (np.bincount(trees, minlength=41) == 2 * np.arange(41) + 1).all()
    got = ac.host_absence(cells, offsets, trees, digests, sc.EVERY_STRIDE)
    assert got[0] == 0
    same(got[1:], [idx] + rest, "absence")
    assert (rest[4] == [ac.height(c) for c in trees.tolist()]).all()                                # tree t holds t leaves


@pytest.mark.parametrize("name", sc.ALTERATIONS)
def test_every_absence_verdict_is_the_cpu_twins(native, name):
    e = sc.every()
    trees, digests, present = e.absence_queries()
    idx, found, *rest = e.absence_expected()
    _, roots, counts = sc.alterations(e.roots(), e.counts)[sc.ALTERATIONS.index(name)]
    want = e.absence_verdicts_under(name)
    assert (ac.host_verify(digests, trees, idx, *rest, roots, counts) == want).all()
    if name == "true":
        assert (want == np.where(present, sc.PRESENT, sc.ABSENT)).all()
    else:
        assert int((want == 0).sum()) >= 100, name


def test_every_shape_of_the_range_table_is_the_cpu_twins(native):
    e = sc.every()
    trees, lo, hi = e.range_queries()
    want = e.range_expected()
    cells, offsets = e.placed(first=37, slack=20)
    carried = sum(min(g2, c - 1) - max(g1 - 1, 0) + 1 for c in range(1, 41) for g1 in range(c + 1) for g2 in range(g1, c + 1))
    assert carried == sc.EVERY_CARRIED and want[6].tolist() == [0, carried, 0, sc.EVERY_IN_RANGE] and len(trees) == 12341
    got = rc.host_range(cells, offsets, trees, lo, hi, sc.EVERY_STRIDE, capacity=carried, guard=0)
    assert got[0] == 0
    same(got[1:], want, "ranges")
    counted = rc.host_range(cells, offsets, trees, lo, hi, sc.EVERY_STRIDE, capacity=0, guard=0)
    assert counted[0] == 0 and counted[7].tolist() == [1] + want[6].tolist()[1:]
    runs = {(int(t), int(a), int(a + n - 1)) for t, a, n in zip(trees, want[0], np.diff(want[1]).astype(np.int64)) if n}
    for c in range(1, 41):                                 # every run a tree of c leaves can carry: any a < b, and a fence alone at either end
        assert all((c, a, b) in runs for a in range(c) for b in range(a + 1, c)) and (c, 0, 0) in runs and (c, c - 1, c - 1) in runs, c


@pytest.mark.parametrize("name", sc.ALTERATIONS)
def test_every_range_verdict_is_the_cpu_twins(native, name):
    e = sc.every()
    trees, lo, hi = e.range_queries()
    proofs = e.range_expected()
    _, roots, counts = sc.alterations(e.roots(), e.counts)[sc.ALTERATIONS.index(name)]
    want = e.range_verdicts_under(name)
    same(rc.host_verify(trees, lo, hi, *proofs[:6], roots, counts), want, name)
    assert all(not a.any() and not n.any() for a, n in [(want[1][want[0] == 0], want[2][want[0] == 0])])       # nothing proven, nothing named
    if name == "true":
        assert (want[0] == 1).all() and int(want[2].sum()) == int(proofs[6][3])
    else:
        assert int((want[0] == 0).sum()) >= 100, name
    if name == "counts + 1":                               # a run that ends at the last leaf is bound by the count; one that does not, by the root
        ends = (proofs[0].astype(np.int64) + np.diff(proofs[1]).astype(np.int64) == trees) & (trees > 0)
        assert ends.sum() > 800 and not want[0][ends].any()
