"""The sort and dedup of leaf entries on the GPU (vkmr_hip_forest_sort_entries_async, vkmr_hip_tree_sort_entries_async,
vkmr_hip_gather_digests_async, raw and through MerkleForest / MerkleTree): cells [0, n) of every output and the four counters
exactly against the numpy model in tests/sort_cases.py, the words around the outputs, the inputs left alone, and the chains
find -> sort -> gather -> update and find -> sort -> multiproof -> verify against the host-ordered calls."""
import numpy as np
import pytest

import find_cases as fd
import forest_cases as fc
import merkle_model
import sort_cases as sc
from merkle_model import At

pytestmark = pytest.mark.gpu

PATTERN = 0xC3C3C3C3
PATTERN64 = PATTERN * 0x100000001
GUARD = 512                                   # words in front of and behind each output: more than one workgroup's lanes


class Outputs:
    """trees_out [k] uint32, indices_out [k] uint64, order_out [k] uint32 and info [4] uint64 on the device, each between
    GUARD words of a pattern."""

    def __init__(self, gpu, k):
        self.gpu, self.k = gpu, k
        self.bufs = [gpu.upload(np.full(2 * GUARD + n, PATTERN64 if dt == np.uint64 else PATTERN, dtype=dt))
                     for n, dt in ((k, np.uint32), (k, np.uint64), (k, np.uint32), (4, np.uint64))]
        self.trees, self.indices, self.order, self.info = (At(b, GUARD * np.dtype(dt).itemsize)
                                                           for b, dt in zip(self.bufs, (np.uint32, np.uint64, np.uint32, np.uint64)))

    def read(self):
        """(trees_out, indices_out, order_out, info), the guards checked."""
        out = []
        for b, n, dt in zip(self.bufs, (self.k, self.k, self.k, 4), (np.uint32, np.uint64, np.uint32, np.uint64)):
            a = self.gpu.download(b, np.dtype(dt).itemsize * (2 * GUARD + n), dtype=dt)
            pat = PATTERN64 if dt == np.uint64 else PATTERN
            assert (a[:GUARD] == pat).all() and (a[GUARD + n:] == pat).all()
            out.append(a[GUARD: GUARD + n])
        return tuple(out)

    def free(self):
        for b in self.bufs:
            b.free()


def forest_sort(gpu, case):
    """(trees_out, indices_out, order_out, info) of one raw vkmr_hip_forest_sort_entries_async over the case; the inputs are
    read back and must be as they were."""
    d_off = gpu.upload(case.offsets) if case.offsets.size else None
    d_trees, d_idx = gpu.upload(case.trees), gpu.upload(case.indices)
    d_scr = gpu.alloc(gpu.sort_entries_scratch_bytes(case.total, case.k))
    out = Outputs(gpu, case.k)
    gpu.forest_sort_entries_async(case.total, d_off, case.ntrees, d_trees, d_idx, case.k, d_scr, out.trees, out.indices, out.order, out.info)
    got = out.read()
    assert (gpu.download(d_trees, 4 * case.k) == case.trees).all() and (gpu.download(d_idx, 8 * case.k, dtype=np.uint64) == case.indices).all()
    for b in (d_trees, d_idx, d_scr, out) + ((d_off,) if d_off else ()):
        b.free()
    return got


def tree_sort(gpu, count, indices):
    k = int(indices.shape[0])
    d_idx, d_scr = gpu.upload(indices), gpu.alloc(gpu.sort_entries_scratch_bytes(count, k))
    out = Outputs(gpu, k)
    gpu.tree_sort_entries_async(count, d_idx, k, d_scr, out.indices, out.order, out.info)
    trees, io, oo, info = out.read()
    assert (trees == PATTERN).all()           # the tree call has no such output
    for b in (d_idx, d_scr, out):
        b.free()
    return io, oo, info


@pytest.mark.parametrize("shape", sc.SHAPES)
@pytest.mark.parametrize("name", sorted(sc.FORESTS))
def test_the_case_tables_give_the_models_answers(gpu, name, shape):
    """Every k of the table -- around a wavefront, around a tile, several tiles, the scan's second trip -- in every forest (one
    pass, a ragged last digit, three passes, the upper key word with an empty tree) and every shape."""
    for k in sc.k_values():
        case = sc.forest_case(name, shape, k)
        sc.assert_equals_the_model(case.want, forest_sort(gpu, case), (name, shape, k))


def test_one_pair_across_several_tiles_keeps_the_last_occurrence(gpu):
    k = 2 * sc.tile_keys() + 3
    for name in sorted(sc.FORESTS):
        case = sc.forest_case(name, "one_pair", k)
        to, io, oo, info = forest_sort(gpu, case)
        assert list(info) == [1, 0, 0, k - 1] and int(oo[0]) == k - 1          # stability across tiles
        assert int(to[0]) == int(case.trees[0]) and int(io[0]) == int(case.indices[0])


@pytest.mark.parametrize("count", sc.TREE_COUNTS)
def test_the_tree_form_gives_the_models_answers(gpu, count):
    for k in sc.k_values():
        idx, want = sc.tree_case(count, k)
        io, oo, info = tree_sort(gpu, count, idx)
        sc.assert_equals_the_model((None,) + want, (None, io, oo, info), (count, k))


def test_no_tree_and_no_leaf_count_every_entry_as_left_out(gpu):
    k = 300
    rng = np.random.default_rng(5)
    trees = np.where(rng.random(k) < 0.4, sc.NO_TREE, rng.integers(0, 4, size=k)).astype(np.uint32)
    idx = rng.integers(0, 3, size=k).astype(np.uint64)
    for total, offsets in ((0, []), (77, []), (0, [0, 0, 0]), (9, [4, 4])):
        case = sc.Case(total, offsets, trees, idx)
        got = forest_sort(gpu, case)
        assert case.want[3][0] == 0 and case.want[3][1] == int((trees == sc.NO_TREE).sum())
        sc.assert_equals_the_model(case.want, got, (total, offsets))
    marked = np.where(trees == sc.NO_TREE, np.uint64(sc.NOT_FOUND), idx)
    io, oo, info = tree_sort(gpu, 0, marked)
    sc.assert_equals_the_model((None,) + sc.tree_model(0, marked), (None, io, oo, info), "count 0")
    assert int(info[0]) == 0


def test_the_scratch_can_be_reused_and_the_answer_does_not_depend_on_what_it_held(gpu):
    case_a, case_b = sc.forest_case("total_2p40", "mixed", 2 * sc.tile_keys() + 3), sc.forest_case("total_300", "random", 65)
    d_scr = gpu.upload(np.full(gpu.sort_entries_scratch_bytes(case_a.total, case_a.k) // 4, 0xFFFFFFFF, dtype=np.uint32))
    for case in (case_a, case_b, case_a):
        d_off, d_trees, d_idx = gpu.upload(case.offsets), gpu.upload(case.trees), gpu.upload(case.indices)
        out = Outputs(gpu, case.k)
        gpu.forest_sort_entries_async(case.total, d_off, case.ntrees, d_trees, d_idx, case.k, d_scr, out.trees, out.indices, out.order, out.info)
        sc.assert_equals_the_model(case.want, out.read(), case.k)
        for b in (d_off, d_trees, d_idx, out):
            b.free()
    d_scr.free()


@pytest.mark.parametrize("n", [1, 65, None])
def test_gather_digests_is_numpy_indexing(gpu, n):
    n = n or 2 * sc.tile_keys() + 3
    rng = np.random.default_rng(n)
    src = merkle_model.random_leaves(rng, n + 40)
    order = rng.integers(0, n + 40, size=n).astype(np.uint32)
    d_src, d_order = gpu.upload(src), gpu.upload(order)
    d_dst = gpu.upload(np.full((n + 2, 8), PATTERN, dtype=np.uint32))
    gpu.gather_digests_async(d_src, d_order, n, At(d_dst, 32))
    got = gpu.download(d_dst, 32 * (n + 2)).reshape(n + 2, 8)
    assert (got[0] == PATTERN).all() and (got[-1] == PATTERN).all() and (got[1:-1] == src[order]).all()
    gpu.gather_digests_async(None, None, 0, None)                      # no cell: nothing to do
    for b in (d_src, d_order, d_dst):
        b.free()


# ---- end to end: find -> sort -> gather -> update, find -> sort -> multiproof --------------------------------------------------

def small_forest():
    """(cells, counts, offsets): about 40 trees of 0..300 leaves, one digest planted in two trees."""
    rng = np.random.default_rng(4242)
    counts = [0, 1, 2, 3, 300, 0, 0, 64, 65, 257] + [int(c) for c in rng.integers(0, 301, size=30)]
    off = fc.offsets_of(counts)
    cells = merkle_model.random_leaves(rng, int(off[-1]))
    cells[int(off[8]) + 9] = cells[int(off[4]) + 100]                  # tree 4 holds it at the lower position
    return cells, counts, off


def replace_batch(cells, off, rng):
    """(old, new): a shuffled batch of digests to replace -- leaves, the twice-planted one, repeats of some with other new
    values, digests that are no leaf, and two sibling leaves given one new value."""
    special = [int(off[4]) + 100, int(off[8]) + 9, int(off[7]) + 10, int(off[7]) + 11]       # named below, each once
    picks = rng.choice(np.setdiff1d(np.arange(int(off[-1])), special), size=120, replace=False)
    old = np.concatenate([cells[picks], cells[picks[:15]], cells[[int(off[4]) + 100]], merkle_model.random_leaves(rng, 12),
                          cells[[int(off[7]) + 10, int(off[7]) + 11]]])
    new = merkle_model.random_leaves(rng, old.shape[0])
    new[-1] = new[-2]                                                  # leaves 10 and 11 of tree 7 become equal siblings
    order = rng.permutation(old.shape[0])
    return old[order], new[order]


def replaced_cells(cells, off, old, new):
    """(cells after the replacement, replaced, missing) by the models: find's first occurrence, then last value wins."""
    trees, idx = fd.model(cells, off, old)
    st, si, order, info = sc.model(off, trees, idx)
    after = cells.copy()
    after[(off[st.astype(np.int64)] + si).astype(np.int64)] = new[order]
    return after, info[0], info[1]


def test_replace_in_a_forest_equals_a_fresh_build_over_the_replaced_leaves(gpu):
    cells, counts, off = small_forest()
    old, new = replace_batch(cells, off, np.random.default_rng(7))
    want_cells, want_replaced, want_missing = replaced_cells(cells, off, old, new)
    assert want_missing == 12 and 0 < want_replaced < old.shape[0] - 12 and (want_cells != cells).any()
    forest = gpu.build_forest(cells, counts)
    assert forest.replace(old, new) == (want_replaced, want_missing)
    fresh = gpu.build_forest(want_cells, counts)
    assert (gpu.download(forest.digests, 32 * forest.total).reshape(-1, 8) == want_cells).all()      # every level-0 cell
    assert (forest.roots() == fresh.roots()).all()
    assert (forest.mutated() == fresh.mutated()).all() and int(forest.mutated()[7]) & 1              # the equal siblings are seen
    assert (want_cells[int(off[8]) + 9] == cells[int(off[8]) + 9]).all()                             # the higher of two equal leaves stays
    forest.free()
    fresh.free()


def test_update_entries_refuses_an_entry_out_of_range_before_anything_changes(gpu):
    cells, counts, off = small_forest()
    forest = gpu.build_forest(cells, counts)
    roots = forest.roots()
    rng = np.random.default_rng(8)
    trees, idx = sc.entries_at(off, rng.integers(0, int(off[-1]), size=70, dtype=np.uint64))
    trees[3], idx[3] = sc.NO_TREE, sc.NOT_FOUND                        # a marker is fine
    leaves = merkle_model.random_leaves(rng, 70)
    for bad_tree, bad_idx in ((4, 300), (0, 0), (len(counts), 0)):     # just past a tree; an empty tree; past the forest
        t, i = trees.copy(), idx.copy()
        t[40], i[40] = bad_tree, bad_idx
        with gpu.scope() as tmp:
            with pytest.raises(IndexError):
                forest.update_entries(tmp.upload(t), tmp.upload(i), tmp.upload(leaves), 70)
        assert (forest.roots() == roots).all() and (gpu.download(forest.digests, 32 * forest.total).reshape(-1, 8) == cells).all()
    with gpu.scope() as tmp:                                           # and the same batch without the bad entry goes through
        got = forest.update_entries(tmp.upload(trees), tmp.upload(idx), tmp.upload(leaves), 70)
    st, si, order, info = sc.model(off, trees, idx)
    assert got == (info[0], info[1], info[3]) and info[1] == 1
    want = cells.copy()
    want[(off[st.astype(np.int64)] + si).astype(np.int64)] = leaves[order]
    fresh = gpu.build_forest(want, counts)
    assert (forest.roots() == fresh.roots()).all() and (gpu.download(forest.digests, 32 * forest.total).reshape(-1, 8) == want).all()
    forest.free()
    fresh.free()


def test_multiproof_of_equals_the_host_ordered_multiproof_and_verifies(gpu):
    cells, counts, off = small_forest()
    forest = gpu.build_forest(cells, counts)
    rng = np.random.default_rng(9)
    picks = rng.choice(int(off[-1]), size=90, replace=False)
    digests = np.concatenate([cells[picks], cells[picks[:10]], merkle_model.random_leaves(rng, 7), cells[[int(off[8]) + 9]]])
    digests = digests[rng.permutation(digests.shape[0])]
    mp, order = forest.multiproof_of(digests)
    trees, idx = fd.model(cells, off, digests)
    found = trees != fd.NO_TREE
    want = forest.multiproof(trees[found], idx[found])
    assert (mp.trees == want.trees).all() and (mp.indices == want.indices).all() and (mp.heights == want.heights).all()
    assert mp.nodes.shape == want.nodes.shape and (mp.nodes == want.nodes).all() and (mp.level_counts == want.level_counts).all()
    assert (order == sc.model(off, trees, idx)[2]).all()
    assert (digests[order] == cells[(off[mp.trees.astype(np.int64)] + mp.indices).astype(np.int64)]).all()
    assert gpu.verify_forest_multiproof(digests[order], mp.trees, mp.indices, mp.heights, mp.nodes, forest.roots())
    with pytest.raises(ValueError):
        forest.multiproof_of(merkle_model.random_leaves(rng, 5))       # none of them is a leaf
    forest.free()


def test_the_same_three_on_one_tree_of_1000_leaves(gpu):
    rng = np.random.default_rng(10)
    cells = merkle_model.random_leaves(rng, 1000)
    cells[700] = cells[30]
    off = np.array([0, 1000], dtype=np.uint64)
    d_cells = gpu.upload(cells)
    tree = gpu.build_tree(d_cells, 1000)
    # replace
    picks = rng.choice(1000, size=50, replace=False)
    old = np.concatenate([cells[picks], cells[picks[:8]], cells[[30]], merkle_model.random_leaves(rng, 6)])
    new = merkle_model.random_leaves(rng, old.shape[0])
    perm = rng.permutation(old.shape[0])
    old, new = old[perm], new[perm]
    want_cells, want_replaced, want_missing = replaced_cells(cells, off, old, new)
    assert tree.replace(old, new) == (want_replaced, want_missing) and want_missing == 6
    d_fresh = gpu.upload(want_cells)
    fresh = gpu.build_tree(d_fresh, 1000)
    assert (tree.level(0) == want_cells).all() and (tree.root() == fresh.root()).all()
    for l in range(1, tree.height + 1):
        assert (tree.level(l) == fresh.level(l)).all()
    assert (want_cells[700] == cells[30]).all()                        # the higher of two equal leaves stays
    # update_entries: an index out of range changes nothing
    idx = rng.integers(0, 1000, size=40, dtype=np.uint64)
    idx[5] = np.uint64(sc.NOT_FOUND)
    leaves = merkle_model.random_leaves(rng, 40)
    bad = idx.copy()
    bad[20] = 1000
    with gpu.scope() as tmp:
        with pytest.raises(IndexError):
            tree.update_entries(tmp.upload(bad), tmp.upload(leaves), 40)
    assert (tree.level(0) == want_cells).all() and (tree.root() == fresh.root()).all()
    with gpu.scope() as tmp:
        got = tree.update_entries(tmp.upload(idx), tmp.upload(leaves), 40)
    si, order, info = sc.tree_model(1000, idx)
    assert got == (info[0], info[1], info[3])
    now = want_cells.copy()
    now[si.astype(np.int64)] = leaves[order]
    assert (tree.level(0) == now).all() and (tree.root() == merkle_model.cpu_levels(now)[-1][0]).all()
    # multiproof_of
    digests = np.concatenate([now[rng.choice(1000, size=30, replace=False)], merkle_model.random_leaves(rng, 4)])
    digests = np.concatenate([digests, digests[:3]])[rng.permutation(37)]
    mp, order = tree.multiproof_of(digests)
    pos = fd.model(now, off, digests)[1]
    want = tree.multiproof(pos[pos != fd.NOT_FOUND])
    assert (mp.indices == want.indices).all() and (mp.nodes == want.nodes).all() and (mp.level_counts == want.level_counts).all()
    assert (digests[order] == now[mp.indices.astype(np.int64)]).all()
    assert gpu.verify_multiproof(digests[order], mp.indices, mp.nodes, tree.root(), tree.height)
    tree.free()
    fresh.free()
    d_cells.free()
    d_fresh.free()
