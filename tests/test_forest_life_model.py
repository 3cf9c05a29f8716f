"""The model of a stored forest's life (tests/forest_life_cases.py) without a GPU: along every walk the model is compared with
the host library's CPU twins, so that it is known to be right before tests/test_gpu_forest_life.py spends GPU time on it; the
walks are shown to reach what they are meant to reach -- every ordered pair of kinds, few degenerate steps, every named event --
so that the GPU test cannot pass by doing nothing; and the two host-side rules a history exposed (the front in _same_shape, the
open tree behind a dropped front) are refused before any device call."""
import functools

import numpy as np
import pytest

import audit_cases
import find_cases as fd
import forest_cases as fc
import forest_life_cases as fl
import forest_multiproof_cases as fm
import forest_mutation_cases as fmu
import forest_proof_cases as fp
import frontier_cases as fr
import high_cases as hc
from merkle_model import fold, stored_level_base
from no_device import NoDevice, NoDeviceAt

WALKS = [(name, seed) for name in sorted(fl.CONFIGS) for seed in fl.SEEDS[name]]
ALL_PAIRS = {(a, b) for a in fl.KINDS for b in fl.KINDS}


@functools.lru_cache(maxsize=None)
def walked(name, seed):
    """The Life of one walk after its last step, the questions of every step asked on the way."""
    life = fl.Life(seed, fl.CONFIGS[name])
    for _, kind, p in life.steps():
        life.apply(kind, p)
        life.find_queries()
    return life


def test_the_circuit_takes_every_ordered_pair_once():
    assert len(fl.KINDS) == 11 and len(fl.CIRCUIT) == 121 and len(fl.SEQUENCE) == 122
    closed = fl.CIRCUIT + fl.CIRCUIT[:1]
    assert sorted(zip(closed, closed[1:])) == sorted(ALL_PAIRS)
    assert fl.pairs_of(fl.SEQUENCE) == ALL_PAIRS
    assert set(fl.STRUCTURAL) | {"update", "replace", "witness", "sync"} == set(fl.KINDS)


@pytest.mark.parametrize("name,seed", WALKS)
def test_every_ordered_pair_of_kinds_is_performed(name, seed):
    life = walked(name, seed)
    assert life.pairs == ALL_PAIRS and sum(life.done.values()) == 122


@pytest.mark.parametrize("name,seed", WALKS)
def test_at_most_a_quarter_of_a_kinds_steps_are_degenerate(name, seed):
    life = walked(name, seed)
    for kind in fl.KINDS:
        assert life.done[kind] >= 11 and 4 * life.degenerate[kind] <= life.done[kind], (kind, life.degenerate[kind], life.done[kind])


@pytest.mark.parametrize("name", sorted(fl.CONFIGS))
def test_every_named_event_occurs_over_the_seeds_of_a_config(name):
    seen = set().union(*(walked(name, seed).events for seed in fl.SEEDS[name]))
    assert [e for e in fl.EVENTS if e not in seen] == []
    assert len(fl.SEEDS[name]) == 3


def test_the_configs_are_the_two_small_ones():
    assert fl.CONFIGS["roomy"][1:] == (70, 12, 400) and fl.CONFIGS["tight"][1:] == (9, 12, 60)
    for name, config in fl.CONFIGS.items():
        first = fl.Life(1, config).a
        assert (first.ntrees, first.total, first.max_count) == (12, config.cells, config.max_count)
        assert first.levels == {"roomy": 7, "tight": 4}[name]


def brute_find(model, queries):
    """The rule in words: the first live leaf, in (tree, index) order, that equals the query."""
    trees, indices = [], []
    for q in queries:
        hit = next(((t, i) for t, i in model.entries() if (model.trees[t][i] == q).all()), (fl.NO_TREE, fl.NOT_FOUND))
        trees.append(hit[0])
        indices.append(hit[1])
    return np.array(trees, dtype=np.uint32), np.array(indices, dtype=np.uint64)


def against_the_cpu_twins(life, number):
    m = life.a
    off, roots = m.offsets(), m.roots()
    assert life.b.counts == m.counts and (life.b.offsets() == off).all() and life.b.books() == m.books()
    assert int(off[-1]) == m.used_leaves and (off[: m.dropped_trees + 1] == m.dropped_leaves).all() and (np.diff(off.astype(np.int64)) >= 0).all()
    rc, got = fc.host_cpu_roots(m.image, off)
    assert rc == 0 and (got == roots).all()
    rc, got_roots, got_masks = fmu.host_cpu_mutated(m.image, off)
    assert rc == 0 and (got_roots == roots).all() and (got_masks == m.masks()).all()
    counts, peaks = m.frontier()
    rc, got_counts, got_peaks = fr.host_forest_frontier(m.image[m.dropped_leaves:], m.counts, m.frontier_stride)
    assert rc == 0 and (got_counts == counts).all() and (got_peaks == peaks).all()
    for t in range(m.ntrees):
        assert (fr.model_root(int(counts[t]), peaks[t]) == roots[t]).all()
    # find: the model's answer is the rule in words, and the twin's
    case = fd.Case(m.image, off, life.find_queries())
    rc, trees, indices = fd.host_cpu_forest_find(case)
    want = m.find(case.queries)
    brute = brute_find(m, case.queries)
    assert rc == 0 and (trees == want[0]).all() and (indices == want[1]).all() and (brute[0] == want[0]).all() and (brute[1] == want[1]).all()
    # proofs of every live leaf and of three entries that name none
    live = m.entries()
    bad = [(0 if m.dropped_trees else m.ntrees + 1, 0), (m.used_trees - 1 if m.used_trees else 0, m.counts[max(m.used_trees - 1, 0)]), (m.ntrees, 0)]
    trees = np.array([t for t, _ in live + bad], dtype=np.uint32)
    indices = np.array([i for _, i in live + bad], dtype=np.uint64)
    sib, heights = m.proofs(trees, indices)
    rc, got_sib, got_h = fp.host_cpu_proofs(m.image, off, trees, indices, m.levels)
    assert rc == 0 and (got_sib == sib).all() and (got_h == heights).all()
    assert not heights[len(live):].any() and not sib[len(live):].any() and (heights[: len(live)] >= 1).all()
    for q in (0, len(live) // 2, len(live) - 1) if live else ():
        assert (fold(m.trees[live[q][0]][live[q][1]], live[q][1], sib[q], heights[q]) == roots[live[q][0]]).all()
    # one multiproof
    trees, indices = life.entry_set()
    if trees.shape[0]:
        nodes, heights, level_counts = m.multiproof(trees, indices)
        rc, got_nodes, got_h, info = fm.host_make(m.image, off, trees, indices, m.levels)
        assert rc == 0 and (got_nodes == nodes).all() and (got_h == heights).all() and [int(x) for x in info[2:]] == list(level_counts)
        assert fm.host_verify(m.leaves_at(trees, indices), trees, indices, heights, m.levels, nodes, roots)
    # every node has a cell of its own inside the level buffers; the audit's count is audit_cases' own
    cells, _ = m.nodes()
    assert cells.shape[0] == 0 or (0 <= cells.min() and cells.max() < stored_level_base(m.total, m.ntrees, m.levels + 1))
    if number % 16 == 0:
        shape = audit_cases.Forest(m.counts, first=m.dropped_leaves, slack=m.free_leaves, max_count=m.max_count)
        assert shape.audit().checked == m.checked() == cells.shape[0] + m.ntrees          # the inner nodes, and a root per tree


@pytest.mark.parametrize("name,seed", WALKS)
def test_the_model_is_what_the_cpu_twins_compute_after_every_step(native, name, seed):
    life = fl.Life(seed, fl.CONFIGS[name])
    against_the_cpu_twins(life, 0)
    for number, kind, p in life.steps():
        try:
            want = life.apply(kind, p)
            if kind == "sync":
                assert life.b.diff(life.a)[0].shape[0] == 0 and want["n"] == want["diff"][0].shape[0]
            against_the_cpu_twins(life, number)
        except Exception:
            print("failed at", (name, seed, number, kind, p))
            raise


def test_walk_yields_the_steps_of_a_life():
    config = fl.CONFIGS["tight"]
    kinds = [kind for kind, _ in fl.walk(1, config)]
    assert tuple(kinds) == fl.SEQUENCE
    a, b = [p for _, p in fl.walk(2, config)], [p for _, _, p in _steps(fl.Life(2, config))]
    assert repr(a) == repr(b)                                          # drawn from the seed and the model alone


def _steps(life):
    for number, kind, p in life.steps():
        yield number, kind, p
        life.apply(kind, p)


# ---- the two host-side rules: refused before any device call -----------------------------------------------------------------------

def handle(dev, counts, total, used_trees, dropped=(0, 0), max_count=9):
    import vk_merkle_roots_amd as vk
    f = vk.MerkleForest(dev, None, total, list(counts), None, max_count, None, None, used_trees=used_trees)
    f.dropped_trees, f.dropped_leaves = dropped
    return f


def test_forests_whose_trees_lie_at_other_offsets_are_not_the_same_shape(native):
    # A: built over [3, 4], the front dropped: offsets [3, 3, 7].  B: built over [0, 4] with three cells to spare: [0, 0, 4]
    a = handle(NoDeviceAt(0), [0, 4], 7, 2, dropped=(1, 3))
    b = handle(NoDeviceAt(0), [0, 4], 7, 2)
    assert (a.counts == b.counts).all() and (a.ntrees, a.total, a.max_count) == (b.ntrees, b.total, b.max_count)
    for first, second in ((a, b), (b, a)):
        for call in (lambda: first.diff(second), lambda: first.diff(second, capacity=4), lambda: first.sync_from(second),
                     lambda: first.diff_async(second, None, None, None, None, 0, None)):
            with pytest.raises(ValueError, match="dropped in front"):
                call()
    twin = handle(NoDeviceAt(0), [0, 4], 7, 2, dropped=(1, 3))           # the twin that dropped its front too passes the check
    assert a._same_shape(twin, "diff") is None
    with pytest.raises(AttributeError):                                  # and goes on to the device
        a.diff(twin)


def test_a_dropped_tree_is_never_the_open_tree(native):
    import vk_merkle_roots_amd as vk
    f = handle(NoDevice(), [0, 0, 0, 0], 20, 2, dropped=(2, 7))          # two trees in use, both dropped from the front
    assert f.open_tree is None and (f.used_leaves, f.free_leaves, f.free_trees) == (7, 13, 2)
    batch = vk.pack_lines(b"a\nb\n")
    for call in (lambda: f.extend(np.zeros((2, 8), np.uint32)), lambda: f.extend(np.zeros((0, 8), np.uint32)),
                 lambda: f.extend(np.zeros((1, 8), np.uint32), mutated=True), lambda: f.extend_packed(batch),
                 lambda: f.extend_async(None, 1, None), lambda: f.shrink(0), lambda: f.shrink(1, mutated=True),
                 lambda: f.shrink_async(1, None)):
        with pytest.raises(ValueError, match="no tree in use"):
            call()
    assert f.counts.tolist() == [0, 0, 0, 0]
    g = handle(NoDevice(), [0, 0, 5, 0], 20, 3, dropped=(2, 7))          # a tree appended behind the dropped ones is the open tree
    assert g.open_tree == 2 and g.used_leaves == 12
    assert g.extend(np.zeros((0, 8), np.uint32)) == 5 and g.shrink(0) == 5
    h = handle(NoDevice(), [0, 0, 0, 0], 20, 2, dropped=(1, 7))          # an empty tree in use that was not dropped still is
    assert h.open_tree == 1 and h.extend(np.zeros((0, 8), np.uint32)) == 0
    model = fl.ModelForest(4, 20, 9, [np.ones((3, 8), np.uint32), np.ones((4, 8), np.uint32)])
    model.drop_front(2)
    assert model.open_tree is None and model.books()["dropped_leaves"] == 7 and model.offsets().tolist() == [7, 7, 7, 7, 7]


# ---- the walks above 4 GiB (tests/high_cases.py): the placements do what they are for ---------------------------------------------

def test_the_walks_are_the_four_of_the_issue():
    assert hc.HIGH_WALKS == [(0, "roomy", 7), (0, "tight", 1), (1, "roomy", 7), (3, "roomy", 4)]


@pytest.mark.parametrize("level,name,seed", hc.HIGH_WALKS)
def test_the_high_walks_straddle_the_line_in_most_steps_and_in_every_kind(level, name, seed):
    steps, kinds = hc.straddling_steps(name, seed, level)
    print("straddling steps", (level, name, seed), steps)
    assert steps >= 60 and [k for k in fl.KINDS if k not in kinds] == []


def test_a_shift_is_the_smallest_that_puts_the_line_at_a_quarter_of_the_window():
    for name, config in fl.CONFIGS.items():
        total, ntrees = config.cells, config.trees
        assert hc.shift_for(0, total, ntrees) == 2**27 - total // 4
        for level in (1, 2, 3):
            D = hc.shift_for(level, total, ntrees)
            at = lambda d: stored_level_base(total + d, ntrees, level) + ((d + total // 4) >> level) + ntrees // 2
            assert at(D) >= 2**27 > at(D - 1), (name, level, D)
            assert D % (1 << (level + 4)), (name, level, D)          # not rounded to the levels above: (offset >> l) does not commute with it
            # the whole forest fits 72 GiB four times over: level 0 and the level buffers, 32 bytes a cell
            assert 4 * 32 * (D + total + stored_level_base(D + total, ntrees, 8)) <= 72 * 2**30


def test_a_view_at_shift_0_is_the_model_and_a_shifted_one_moves_the_cells_alone():
    life = fl.Life(7, fl.CONFIGS["roomy"])
    for number, kind, p in life.steps():
        life.apply(kind, p)
        m, same, high = life.a, hc.Shifted(life.a), hc.Shifted(life.a, 1)
        assert same.D == 0 and same.books() == m.books() and (same.offsets() == m.offsets()).all() and same.levels == m.levels
        assert all((x == y).all() for x, y in zip(same.nodes(), m.nodes())) and (same.live_cells() == m.live_cells()).all()
        D = high.D
        assert D == hc.shift_for(1, m.total, m.ntrees) and high.total == m.total + D and high.levels == 7
        books = high.books()
        assert (books["dropped_leaves"], books["used_leaves"], books["free_leaves"]) == (m.dropped_leaves + D, m.used_leaves + D, m.free_leaves)
        assert (high.offsets() == m.offsets() + np.uint64(D)).all() and (high.live_cells() == m.live_cells() + D).all()
        cells, digests, levels = high.nodes(with_levels=True)
        assert (digests == m.nodes()[1]).all() and cells.shape[0] == m.nodes()[0].shape[0]
        assert cells.shape[0] == 0 or cells.max() < stored_level_base(high.total, m.ntrees, high.levels + 1)
        if number % 16 == 0:
            trees, indices = life.entry_set()
            sib, heights = high.proofs(trees, indices)
            want = m.proofs(trees, indices)
            assert sib.shape[1] == high.levels and (sib[:, : m.levels] == want[0]).all() and not sib[:, m.levels:].any() and (heights == want[1]).all()


def test_a_handle_laid_into_a_larger_buffer_keeps_its_books_from_the_front(native):
    import vk_merkle_roots_amd as vk
    D = 2**27 - 15
    f = vk.MerkleForest(NoDevice(), None, D + 60, [4, 0, 9, 0, 0], None, 9, None, None, used_trees=3, front=D)
    assert (f.dropped_trees, f.dropped_leaves, f.used_leaves, f.live_leaves, f.free_leaves, f.free_trees) == (0, D, D + 13, 13, 47, 2)
    assert f.open_tree == 2 and f.levels == 4 and f.total == D + 60
    cells, counts = f._entry_cells(np.array([0, 2, 2], dtype=np.uint32), np.array([3, 0, 8], dtype=np.uint64))
    assert cells.tolist() == [D + 3, D + 4, D + 12] and counts.tolist() == [4, 9, 9]
    model = fl.ModelForest(5, 60, 9, [np.ones((4, 8), np.uint32), np.zeros((0, 8), np.uint32), np.ones((9, 8), np.uint32)])
    view = hc.Shifted(model, 0)
    assert view.D == D and all((getattr(f, k).tolist() if k == "counts" else getattr(f, k)) == v for k, v in view.books().items())
    high, low = (vk.MerkleForest(NoDeviceAt(0), None, D + 60, [4, 0, 9, 0, 0], None, 9, None, None, used_trees=3, front=d) for d in (D, 0))
    assert low.dropped_leaves == 0 and low.free_leaves == D + 47
    for call in (lambda: high.diff(low), lambda: low.sync_from(high)):   # the same counts at another place are another shape
        with pytest.raises(ValueError, match="dropped in front"):
            call()
    for front in (-1, D + 61):
        with pytest.raises(ValueError, match="in front of the first tree"):
            vk.MerkleForest(NoDevice(), None, D + 60, [4, 0, 9, 0, 0], None, 9, None, None, used_trees=3, front=front)
