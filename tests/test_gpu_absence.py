"""Sorted trees and absence proofs on the GPU (vkmr_hip_forest_sorted_async, vkmr_hip_forest_lower_bound_async,
vkmr_hip_forest_absence_async, vkmr_hip_verify_forest_absence_async and their one-tree twins through HipDevice, MerkleForest and
MerkleTree): cell for cell what the CPU twins and the hashlib model of tests/absence_cases.py give for its one forest, between
guard words, at two placements; the sortedness cases; the verifier's negatives; a wide stride; no query; a forest without a
leaf; gather -> verify chained on one stream, the same behind an update on that stream, and an update that breaks the order; the
one-tree twins."""
import numpy as np
import pytest

import absence_cases as ac
import forest_update_cases as fu
from merkle_model import At, cpu_levels, random_leaves

pytestmark = pytest.mark.gpu

GUARD = 4                                                    # guard cells (indices, heights, verdicts) on either side of every output


def guarded(gpu, tmp, n, fill, dtype, width=1):
    """A device buffer of n items of `width` words of dtype with GUARD items of the fill on either side, all set to the fill."""
    return tmp.upload(np.full((n + 2 * GUARD) * width, fill, dtype))


def inner(gpu, buf, n, fill, dtype, width=1):
    """The n items between the guards, which must still be the fill."""
    got = gpu.download(buf, (n + 2 * GUARD) * width * np.dtype(dtype).itemsize, dtype=dtype).reshape(n + 2 * GUARD, width)
    assert (got[:GUARD] == fill).all() and (got[-GUARD:] == fill).all()
    return got[GUARD:-GUARD]


def at(buf, dtype, width=1):
    return At(buf, GUARD * width * np.dtype(dtype).itemsize)


def device_sorted(gpu, forest):
    """(first_bad [ntrees], info [4]) of one raw call on the MerkleForest `forest`, between guards."""
    with gpu.scope() as tmp:
        d_bad, d_info = guarded(gpu, tmp, forest.ntrees, ac.INDEX_FILL, np.uint64), guarded(gpu, tmp, 4, ac.INDEX_FILL, np.uint64)
        gpu.forest_sorted_enqueue(forest.digests, forest.total, forest.offsets, forest.ntrees, at(d_bad, np.uint64), at(d_info, np.uint64))
        return inner(gpu, d_bad, forest.ntrees, ac.INDEX_FILL, np.uint64)[:, 0], inner(gpu, d_info, 4, ac.INDEX_FILL, np.uint64)[:, 0]


def device_lower_bound(gpu, forest, trees, digests):
    Q = len(trees)
    with gpu.scope() as tmp:
        d_idx, d_found = guarded(gpu, tmp, Q, ac.INDEX_FILL, np.uint64), guarded(gpu, tmp, Q, ac.CANARY, np.uint32)
        gpu.forest_lower_bound_enqueue(forest.digests, forest.total, forest.offsets, forest.ntrees, tmp.upload(trees), tmp.upload(digests), Q,
                                       at(d_idx, np.uint64), at(d_found, np.uint32))
        return inner(gpu, d_idx, Q, ac.INDEX_FILL, np.uint64)[:, 0], inner(gpu, d_found, Q, ac.CANARY, np.uint32)[:, 0]


def device_absence(gpu, forest, trees, digests, stride):
    """(indices, pred, succ, main, low, heights) of one raw call, every output between guards."""
    Q = len(trees)
    with gpu.scope() as tmp:
        d_idx, d_h = guarded(gpu, tmp, Q, ac.INDEX_FILL, np.uint64), guarded(gpu, tmp, Q, ac.CANARY, np.uint32)
        d_nb = guarded(gpu, tmp, 2 * Q, ac.CANARY, np.uint32, 8)
        d_main, d_low = guarded(gpu, tmp, Q * stride, ac.CANARY, np.uint32, 8), guarded(gpu, tmp, Q * stride, ac.CANARY, np.uint32, 8)
        gpu.forest_absence_enqueue(forest.digests, forest.forest, forest.total, forest.offsets, forest.ntrees, forest.max_count, tmp.upload(trees),
                                   tmp.upload(digests), Q, stride, at(d_idx, np.uint64), at(d_nb, np.uint32, 8), at(d_main, np.uint32, 8),
                                   at(d_low, np.uint32, 8), at(d_h, np.uint32))
        nb = inner(gpu, d_nb, 2 * Q, ac.CANARY, np.uint32, 8).reshape(Q, 2, 8)
        return (inner(gpu, d_idx, Q, ac.INDEX_FILL, np.uint64)[:, 0], nb[:, 0], nb[:, 1], inner(gpu, d_main, Q * stride, ac.CANARY, np.uint32, 8).reshape(Q, stride, 8),
                inner(gpu, d_low, Q * stride, ac.CANARY, np.uint32, 8).reshape(Q, stride, 8), inner(gpu, d_h, Q, ac.CANARY, np.uint32)[:, 0])


def device_verify(gpu, digests, trees, indices, pred, succ, main, low, heights, roots, counts):
    """verdict [Q] of one raw call, between guards."""
    Q, stride = len(trees), int(main.shape[1])
    nb = np.ascontiguousarray(np.stack([pred, succ], axis=1))
    with gpu.scope() as tmp:
        d_verdict = guarded(gpu, tmp, Q, ac.CANARY, np.uint32)
        ups = [tmp.upload(np.ascontiguousarray(a, dtype=t)) for a, t in ((digests, np.uint32), (trees, np.uint32), (indices, np.uint64), (nb, np.uint32),
                                                                       (main, np.uint32), (low, np.uint32), (heights, np.uint32))]
        gpu.verify_forest_absence_enqueue(*ups, Q, stride, tmp.upload(np.ascontiguousarray(roots, dtype=np.uint32)),
                                          tmp.upload(np.ascontiguousarray(counts, dtype=np.uint64)), len(counts), at(d_verdict, np.uint32))
        return inner(gpu, d_verdict, Q, ac.CANARY, np.uint32)[:, 0]


def same(got, want, note):
    for what, a, b in zip(("indices", "pred", "succ", "main", "low", "heights"), got, want):
        assert a.shape == b.shape and (a == b).all(), (note, what, np.nonzero((a != b).reshape(a.shape[0], -1).any(axis=1))[0][:8])


@pytest.fixture(scope="module")
def cases():
    """The forest, its queries, what the model expects and what the CPU twin gives at the second placement, computed once."""
    f = ac.forest()
    trees, digests = f.queries()
    cells, offsets = f.placed(first=5, slack=7)
    twin = ac.host_absence(cells, offsets, trees, digests)
    assert twin[0] == 0
    return f, trees, digests, f.expected(), twin[1:], cells, offsets


@pytest.fixture(scope="module")
def placed(gpu, cases):
    """The forest stored on the device with offsets[0] > 0 and slack behind, and the same batch out of it in ONE call."""
    f, trees, digests, _, _, cells, offsets = cases
    raw = fu.RawForest(gpu, cells, f.counts, 130, first=5)
    assert int(offsets[0]) == 5 and raw.total == sum(f.counts) + 12
    got = device_absence(gpu, raw.handle, trees, digests, ac.STRIDE)
    yield raw, got
    raw.free()


def test_the_device_is_the_cpu_twin_and_the_model_cell_for_cell(gpu, cases, placed):
    f, trees, digests, expected, twin = cases[:5]
    raw, got = placed
    same(got, twin, "twin")
    same(got, expected[:1] + expected[2:7], "model")
    idx, found = device_lower_bound(gpu, raw.handle, trees, digests)
    assert (idx == expected[0]).all() and (found == expected[1]).all()
    assert (raw.handle.roots() == f.roots).all()
    bad, info = device_sorted(gpu, raw.handle)
    assert (bad == ac.NONE).all() and info.tolist() == [0, 0, 0, sum(f.counts) - 12]


def test_the_same_batch_verifies_on_the_device(gpu, cases, placed):
    f, trees, digests, expected = cases[:4]
    _, got = placed
    verdicts = device_verify(gpu, digests, trees, *got, f.roots, f.counts)
    assert (verdicts == expected[7]).all(), np.nonzero(verdicts != expected[7])[0][:8]
    assert (verdicts == ac.host_verify(digests, trees, *got, f.roots, f.counts)).all()
    other = np.roll(f.roots, 1, axis=0)                                                            # every tree under its neighbour's root
    wrong = device_verify(gpu, digests, trees, *got, other, f.counts)
    known = trees < f.ntrees
    assert not wrong[known & (np.array(f.counts + [0])[np.minimum(trees, f.ntrees)] > 0)].any()


def test_the_handles_at_the_first_placement_and_a_wide_stride(gpu, cases):
    import vk_merkle_roots_amd as vk
    f, trees, digests, expected = cases[:4]
    forest = gpu.build_forest(np.concatenate(f.trees), f.counts)
    assert forest.is_sorted() and (forest.first_unsorted() == ac.NONE).all()
    idx, found = forest.lower_bound(trees, digests)
    assert (idx == expected[0]).all() and (found == (expected[1] == 1)).all()
    proofs = forest.absence(trees, digests)
    assert proofs.stride == 8 and proofs.same_as(vk.AbsenceProofs(trees, digests, expected[0], *expected[2:7]))
    assert (proofs.verify(gpu, forest.roots(), forest.counts) == expected[7]).all()
    assert (gpu.verify_forest_absence(digests, trees, *expected[:1], *expected[2:7], f.roots, f.counts) == expected[7]).all()
    wide = forest.absence(trees, digests, stride=11)
    assert (wide.main[:, :8] == expected[4]).all() and not wide.main[:, 8:].any() and (wide.low[:, :8] == expected[5]).all() and not wide.low[:, 8:].any()
    assert (wide.verify(gpu, f.roots, f.counts) == expected[7]).all()
    with pytest.raises(vk.VkmrError):
        forest.absence(trees, digests, stride=7)                                                   # the forest's proofs have eight cells
    # range counts from two lower bounds: the leaves of the tree of 130 in [x, y)
    lo, hi = f.trees[13][17], f.trees[13][101]
    (a, b), _ = forest.lower_bound([13, 13], np.stack([lo, hi]))
    assert int(b) - int(a) == 84
    forest.free()


@pytest.mark.parametrize("case", ac.sortedness_cases(), ids=[c[0] for c in ac.sortedness_cases()])
def test_sortedness(gpu, case):
    what, trees, first_bad, unsorted, equal, pairs = case
    counts = [len(t) for t in trees]
    cells, offsets = ac.lay(trees, 4, 3)
    raw = fu.RawForest(gpu, cells, counts, max(counts), first=4)
    bad, info = device_sorted(gpu, raw.handle)
    assert (bad == first_bad).all() and info.tolist() == [0, unsorted, equal, pairs], (what, bad, info)
    assert raw.handle.is_sorted() == (unsorted == 0) and (raw.handle.first_unsorted() == first_bad).all()
    raw.free()


def test_the_verifiers_negatives(gpu):
    what, want, *batch = ac.negatives_batch()
    got = device_verify(gpu, *batch)
    assert got.tolist() == want.tolist(), [w for w, a, b in zip(what, got, want) if a != b]
    beyond = list(batch)
    beyond[1] = batch[1] + np.uint32(len(what))                                                     # every tree outside the table
    assert not device_verify(gpu, *beyond).any()


def test_no_query_and_a_forest_without_a_leaf(gpu):
    forest = gpu.build_forest(np.zeros((0, 8), np.uint32), [0, 0, 0])
    assert forest.is_sorted() and (forest.first_unsorted() == ac.NONE).all()
    trees, digests = np.array([0, 2, 3], np.uint32), np.stack([ac.ZERO, ac.ONES, ac.ONES])
    idx, found = forest.lower_bound(trees, digests)
    assert idx.tolist() == [0, 0, ac.NONE] and not found.any()
    got = device_absence(gpu, forest, trees, digests, 1)
    assert got[0].tolist() == [0, 0, ac.NONE] and got[5].tolist() == [0, 0, 0] and not any(a.any() for a in got[1:5])
    assert device_verify(gpu, digests, trees, *got, forest.roots(), forest.counts).tolist() == [ac.ABSENT, ac.ABSENT, ac.NOT_PROVEN]
    assert device_verify(gpu, digests, trees, *got, np.ones((3, 8), np.uint32), forest.counts).tolist() == [0, 0, 0]
    # Q == 0: nothing is done, no buffer is needed
    gpu.forest_lower_bound_enqueue(None, 0, None, 0, None, None, 0, None, None)
    gpu.forest_absence_enqueue(None, None, 0, None, 0, 0, None, None, 0, 0, None, None, None, None, None)
    gpu.verify_forest_absence_enqueue(None, None, None, None, None, None, None, 0, 0, None, None, 0, None)
    empty = forest.absence([], np.zeros((0, 8), np.uint32))
    assert empty.Q == 0 and empty.verify(gpu, forest.roots(), forest.counts).shape == (0,) and forest.lower_bound([], np.zeros((0, 8)))[0].shape == (0,)
    forest.free()


def test_gather_and_verify_chained_on_one_stream_also_behind_an_update(gpu, cases):
    f, trees, digests, expected = cases[:4]
    forest = gpu.build_forest(np.concatenate(f.trees), f.counts)
    stream = gpu.new_stream()
    Q, stride = len(trees), forest.levels
    # the update: leaf 40 of the tree of 130 moves to another digest between its neighbours; the order holds
    t, i = 13, 40
    old = f.trees[t][i].copy()
    new = ac.from_int(ac.as_int(f.trees[t][i - 1]) + (ac.as_int(f.trees[t][i + 1]) - ac.as_int(f.trees[t][i - 1])) // 3)
    assert ac.key(new) != ac.key(old) and ac.key(f.trees[t][i - 1]) < ac.key(new) < ac.key(f.trees[t][i + 1])
    after = f.trees[t].copy()
    after[i] = new
    levels = cpu_levels(after)
    more_t, more_x = np.full(4, t, np.uint32), np.stack([old, new, after[i - 1], ac.from_int(ac.as_int(new) + 1)])
    with gpu.scope() as tmp:
        d_trees, d_x = tmp.upload(trees), tmp.upload(digests)
        d_counts = tmp.upload(np.array(f.counts, dtype=np.uint64))
        d_idx, d_nb, d_main, d_low, d_h, d_verdict = (tmp.alloc(n) for n in (8 * Q, 64 * Q, 32 * Q * stride, 32 * Q * stride, 4 * Q, 4 * Q))
        forest.absence_async(d_trees, d_x, Q, stride, d_idx, d_nb, d_main, d_low, d_h, stream=stream)
        gpu.verify_forest_absence_enqueue(d_x, d_trees, d_idx, d_nb, d_main, d_low, d_h, Q, stride, forest.roots_buf, d_counts, forest.ntrees, d_verdict,
                                          stream=stream)                                          # nothing read in between
        # the update, the gather and the check behind it, still on that stream and still unread
        d_ut, d_ui, d_ul, d_status = tmp.upload(np.array([t], np.uint32)), tmp.upload(np.array([i], np.uint64)), tmp.upload(new.reshape(1, 8)), tmp.alloc(4)
        d_t2, d_x2 = tmp.upload(more_t), tmp.upload(more_x)
        d_idx2, d_nb2, d_main2, d_low2, d_h2, d_verdict2 = (tmp.alloc(n) for n in (8 * 4, 64 * 4, 32 * 4 * stride, 32 * 4 * stride, 4 * 4, 4 * 4))
        forest.update_async(d_ut, d_ui, d_ul, 1, d_status, stream=stream)
        forest.absence_async(d_t2, d_x2, 4, stride, d_idx2, d_nb2, d_main2, d_low2, d_h2, stream=stream)
        gpu.verify_forest_absence_enqueue(d_x2, d_t2, d_idx2, d_nb2, d_main2, d_low2, d_h2, 4, stride, forest.roots_buf, d_counts, forest.ntrees, d_verdict2,
                                          stream=stream)
        gpu.sync(stream)
        assert (gpu.download(d_verdict, 4 * Q) == expected[7]).all() and int(gpu.download(d_status, 4)[0]) == 0
        assert gpu.download(d_verdict2, 16).tolist() == [ac.ABSENT, ac.PRESENT, ac.PRESENT, ac.ABSENT]
        assert gpu.download(d_idx2, 32, dtype=np.uint64).tolist() == [i + (ac.key(old) > ac.key(new)), i, i - 1, i + 1]
        want = [ac.model_proof(after, levels, x, stride) for x in more_x]
        assert (gpu.download(d_main2, 32 * 4 * stride).reshape(4, stride, 8) == np.stack([w[3] for w in want])).all()
        assert (gpu.download(d_low2, 32 * 4 * stride).reshape(4, stride, 8) == np.stack([w[4] for w in want])).all()
    assert (forest.roots()[t] == levels[-1][0]).all() and forest.is_sorted()
    # an update that breaks the order: the proofs still fold, and the pass over the leaves is what catches it
    forest.update([10, t], [62, i], np.stack([f.trees[10][0], f.trees[t][i + 5]]))
    bad = forest.first_unsorted()
    assert not forest.is_sorted() and int(bad[t]) == i + 1 and int(bad[10]) == 62 and (np.delete(bad, [10, t]) == ac.NONE).all()
    forest.free()


def test_the_one_tree_twins(gpu):
    import vk_merkle_roots_amd as vk
    f = ac.forest()
    for t in (0, 2, 12, 13):
        leaves = f.trees[t]
        c = len(leaves)
        mine = np.nonzero(f.queries()[0] == t)[0]
        digests = f.queries()[1][mine]
        expected = [e[mine] for e in f.expected()]
        h = ac.height(c)
        d_leaves = gpu.upload(leaves)
        tree = gpu.build_tree(d_leaves, c)
        assert tree.height == h and tree.is_sorted() and tree.first_unsorted().tolist() == [ac.NONE]
        idx, found = tree.lower_bound(digests)
        assert (idx == expected[0]).all() and (found == (expected[1] == 1)).all()
        proofs = tree.absence(digests)
        want = vk.AbsenceProofs(np.zeros(len(mine), np.uint32), digests, expected[0], expected[2], expected[3], expected[4][:, :h], expected[5][:, :h], expected[6])
        assert proofs.same_as(want)
        assert (proofs.verify(gpu, f.roots[t: t + 1], [c]) == expected[7]).all()
        Q = len(mine)
        with gpu.scope() as tmp:                                                                     # the twin's own check: one root, one count
            d_verdict = guarded(gpu, tmp, Q, ac.CANARY, np.uint32)
            gpu.verify_absence_enqueue(tmp.upload(digests), tmp.upload(proofs.indices), tmp.upload(proofs.neighbours), tmp.upload(proofs.main),
                                       tmp.upload(proofs.low), Q, h, tmp.upload(tree.root()), c, at(d_verdict, np.uint32))
            assert (inner(gpu, d_verdict, Q, ac.CANARY, np.uint32)[:, 0] == expected[7]).all()
        tree.free()
        d_leaves.free()
    rng = np.random.default_rng(621)
    unsorted = random_leaves(rng, 300)
    d_leaves = gpu.upload(unsorted)
    tree = gpu.build_tree(d_leaves, 300)
    want = ac.model_first_bad(unsorted)[0]
    assert not tree.is_sorted() and tree.first_unsorted().tolist() == [want]
    idx, found = tree.lower_bound(unsorted[:50])
    assert idx.tolist() == [ac.model_lower_bound(unsorted, x)[0] for x in unsorted[:50]]
    tree.free()
    d_leaves.free()
