"""Stored forests that grow on the GPU (vkmr_hip_forest_append_async and vkmr_hip_forest_truncate_async through HipDevice and
MerkleForest): after every append the leaves, EVERY cell of the forest buffer, the roots and the offsets equal a fresh build over
the offsets as they now are, the cells nobody writes included; a refused append changes nothing; every reader takes the grown
forest; the append is ordered on its stream in front of a proof gather and a verify."""
import numpy as np
import pytest

import forest_append_cases as fa
import forest_cases as fc
import forest_proof_cases as fp
import merkle_model

pytestmark = pytest.mark.gpu


def grown_equals_fresh(gpu, leaves, counts, max_count, first=0, in_place=False, note=""):
    """From every split point: the rest appended in chunks of 1 tree, 2 trees and all that remain; after each chunk all four
    buffers equal a fresh build's."""
    for split in fa.split_points(len(counts)):
        forest = fa.Growing(gpu, leaves, counts, max_count, split, first=first)
        fa.assert_same(forest.state(), forest.fresh_state(), (note, split, "built"))
        for chunk in (1, 2, len(counts)):
            m = min(chunk, forest.ntrees - forest.used_trees)
            if m == 0:
                break
            assert forest.append_next(m, in_place=in_place) == 0, (note, split, chunk)
            fa.assert_same(forest.state(), forest.fresh_state(), (note, split, chunk))
        assert forest.used_trees == forest.ntrees
        forest.free()


@pytest.mark.parametrize("loose", [False, True], ids=["tight", "loose"])
@pytest.mark.parametrize("name", sorted(n for n in fc.CASES if n != "all_empty"))
def test_grown_forest_equals_a_fresh_build_in_every_cell(gpu, name, loose):
    counts = fc.CASES[name]
    leaves = fc.random_leaves(sum(counts), seed=len(name) * 7907 + sum(counts))
    grown_equals_fresh(gpu, leaves, counts, 2**63 if loose else max(counts), note=name)


def test_a_first_offset_above_zero_and_slack_behind_the_last_tree(gpu):
    counts = [4, 0, 0, 7, 0, 1, 130, 33, 0, 65, 64, 129]
    leaves = fc.random_leaves(5 + sum(counts) + 7, seed=56)          # total is the leaves buffer's size
    grown_equals_fresh(gpu, leaves, counts, max(counts), first=5)
    grown_equals_fresh(gpu, leaves, counts, 2**63, first=5, in_place=True)


@pytest.mark.parametrize("name", ["sizes_1_to_130", "power_of_two_edges", "empty_adjacent"])
def test_leaves_the_caller_put_in_place(gpu, name):
    counts = fc.CASES[name]
    leaves = fc.random_leaves(sum(counts), seed=len(name) * 7901 + 1)
    grown_equals_fresh(gpu, leaves, counts, max(counts), in_place=True, note=name)


def test_append_packed_from_strings_equals_the_forest_of_all_strings(gpu):
    import vk_merkle_roots_amd as vk
    counts = [3, 0, 65, 1, 130, 0, 2, 64, 7]
    n = sum(counts)
    batch = vk.pack_lines(b"".join(b"string %d of the forest\n" % i for i in range(n)))
    assert batch.count == n
    want = vk.merkle_forest_packed(gpu, batch, counts, max_count=130, reserve_trees=2, reserve_leaves=9)
    split, at = 3, sum(counts[:3])
    got = vk.merkle_forest_packed(gpu, batch.slice(0, at), counts[:split], max_count=130, reserve_trees=len(counts) - split + 2,
                                  reserve_leaves=n - at + 9)
    assert (got.used_trees, got.free_trees, got.used_leaves, got.free_leaves) == (split, len(counts) - split + 2, at, n - at + 9)
    mid = split + 2
    assert got.append_packed(batch.slice(at, sum(counts[:mid])), counts[split:mid]).tolist() == list(range(split, mid))
    assert got.append_packed(batch.slice(sum(counts[:mid]), n), counts[mid:]).tolist() == list(range(mid, len(counts)))
    assert (got.used_trees, got.free_trees, got.used_leaves, got.free_leaves) == (len(counts), 2, n, 9)
    assert (got.counts == want.counts).all() and (got.total, got.ntrees, got.levels) == (want.total, want.ntrees, want.levels)
    assert (got.roots() == want.roots()).all()
    assert (gpu.download(got.digests, 32 * n) == gpu.download(want.digests, 32 * n)).all()
    assert (gpu.download(got.offsets, 8 * (got.ntrees + 1), dtype=np.uint64) == gpu.download(want.offsets, 8 * (got.ntrees + 1), dtype=np.uint64)).all()
    trees, indices = got.diff(want)
    assert trees.shape == (0,) and indices.shape == (0,)
    assert got.audit().clean and want.audit().clean
    leaves = gpu.download(got.digests, 32 * n).reshape(n, 8)
    assert (got.roots()[: len(counts)] == gpu.forest_roots(leaves, counts)).all() and not got.roots()[len(counts):].any()
    got.free()
    want.free()


REFUSED = [  # (first_tree, used relative to the true one, new offsets, n_leaves, the status)
    (2, 0, [0, 3, 5], 5, 4),          # a first_tree whose tree is not empty: offsets[2] is not `used`
    (3, 1, [0, 3, 5], 5, 4),          # a wrong `used`: no offset from first_tree on equals it
    (3, -1, [0, 3, 5], 5, 4),
    (3, 0, [0, 5, 3, 8], 8, 1),       # the new offsets decrease
    (3, 0, [1, 3, 8], 8, 1),          # start above 0
    (3, 0, [0, 3, 7], 8, 1),          # end short
    (3, 0, [0, 3, 9], 8, 1),          # end past the leaves
    (3, 0, [0, 8, 9], 9, 2),          # a count above max_count
    (3, 0, [2, 10, 9], 9, 3),         # both
    (2, 1, [0, 9, 8], 9, 7),          # everything at once
]


@pytest.mark.parametrize("first_tree,used_off,new_offsets,n_leaves,want", REFUSED)
def test_a_refused_append_changes_nothing(gpu, first_tree, used_off, new_offsets, n_leaves, want):
    counts = [4, 0, 7, 3, 5, 1, 0, 6]                                # trees 0..2 resident, room for five more; max_count 7
    leaves = fc.random_leaves(sum(counts) + 11, seed=131)
    forest = fa.Growing(gpu, leaves, counts, 7, 3)
    before = forest.state()
    new = fc.random_leaves(n_leaves, seed=132)
    for mutated in (False, True):
        for in_place in (False,) if want & 4 else (False, True):
            used = forest.used + used_off
            got = forest.append_raw(first_tree, used, new, new_offsets, mutated=mutated, in_place=in_place)
            assert got == want                                       # the status word held 0xDEADBEEF
            after = forest.state()
            if in_place:                                             # the one exception: the leaves the caller put in place itself
                assert (after[0].reshape(-1, 8)[used: used + n_leaves] == new).all()
                after[0].reshape(-1, 8)[used: used + n_leaves] = fa.GUARD
                forest.put_leaves(used, np.full((n_leaves, 8), fa.GUARD, dtype=np.uint32))   # as they were, for the next round
            for what, a, b in zip(("leaves", "forest", "roots", "offsets", "masks"), after, before):
                assert (a == b).all(), (what, mutated, in_place)
    assert forest.append_next(2) == 0                                # and the forest still grows
    fa.assert_same(forest.state(), forest.fresh_state(), "after the refusals")
    forest.free()


def test_trailing_trees_that_are_not_empty_refuse_the_append(gpu):
    counts = [4, 0, 7, 3, 0]
    leaves = fc.random_leaves(sum(counts) + 20, seed=133)
    forest = fa.Growing(gpu, leaves, counts, 7, len(counts) - 1)     # tree 3 is resident, tree 4 the only free one
    before = forest.state()
    # the caller takes tree 2 for the first free one: offsets[2] = 4 is where it says, offsets[3] and later are not
    assert forest.append_raw(2, 4, fc.random_leaves(3, seed=134), [0, 3]) == 4
    assert all((a == b).all() for a, b in zip(forest.state(), before))
    forest.free()


def readers_case(gpu, seed):
    """(grown, fresh, leaves, counts): a forest grown in two appends (a zero-count tree and a tree of one leaf among the new)
    and a fresh build of the same capacity."""
    rng = np.random.default_rng(seed)
    counts = [int(c) for c in rng.integers(1, 131, size=40)] + [0, 1, 64, 65, 0, 129, 2, 3]
    leaves = merkle_model.random_leaves(rng, sum(counts))
    split, at = 30, sum(counts[:30])
    grown = gpu.build_forest(leaves[:at], counts[:split], max_count=130, reserve_trees=len(counts) - split + 3, reserve_leaves=sum(counts) - at + 50)
    mid, to = 41, sum(counts[:41])
    assert grown.append(leaves[at:to], counts[split:mid]).tolist() == list(range(split, mid))
    assert grown.append(leaves[to:], counts[mid:]).tolist() == list(range(mid, len(counts)))
    fresh = gpu.build_forest(leaves, counts, max_count=130, reserve_trees=3, reserve_leaves=50)
    return grown, fresh, leaves, counts


def test_every_reader_takes_the_grown_forest(gpu):
    grown, fresh, leaves, counts = readers_case(gpu, 141)
    rng = np.random.default_rng(142)
    n, ntrees = sum(counts), len(counts)
    off = fc.offsets_of(counts).astype(np.int64)
    assert (grown.ntrees, grown.total, grown.used_trees, grown.used_leaves) == (fresh.ntrees, fresh.total, ntrees, n) and (grown.counts == fresh.counts).all()
    assert (grown.roots() == fresh.roots()).all()
    assert (grown.roots()[:ntrees] == gpu.forest_roots(leaves, counts)).all() and not grown.roots()[ntrees:].any()
    # proofs: of random leaves, and of the first and the last leaf of every appended tree
    trees, indices = fp.random_queries(rng, counts, 300)
    new = [t for t in range(30, ntrees) if counts[t]]
    trees = np.concatenate([trees, np.array(new + new, dtype=np.uint32)])
    indices = np.concatenate([indices, np.array([0] * len(new) + [counts[t] - 1 for t in new], dtype=np.uint64)])
    at = off[trees.astype(np.int64)] + indices.astype(np.int64)
    sib, h = grown.proofs(trees, indices)
    sib_f, h_f = fresh.proofs(trees, indices)
    assert (sib == sib_f).all() and (h == h_f).all() and (h >= 1).all()
    assert gpu.verify_forest_proofs(leaves[at], trees, indices, sib, h, grown.roots()).all()
    # one multiproof over the same entries
    mp, mp_f = grown.multiproof(trees, indices), fresh.multiproof(trees, indices)
    assert (mp.trees == mp_f.trees).all() and (mp.indices == mp_f.indices).all() and (mp.heights == mp_f.heights).all() and (mp.nodes == mp_f.nodes).all()
    mp_at = off[mp.trees.astype(np.int64)] + mp.indices.astype(np.int64)
    assert gpu.verify_forest_multiproof(leaves[mp_at], mp.trees, mp.indices, mp.heights, mp.nodes, grown.roots())
    # find: leaves of old and new trees, and a digest that is no leaf
    queries = np.concatenate([leaves[at[:50]], leaves[at[-20:]], merkle_model.random_leaves(rng, 3)])
    found, found_f = grown.find(queries), fresh.find(queries)
    assert (found[0] == found_f[0]).all() and (found[1] == found_f[1]).all()
    assert (found[0][:70] == trees[np.r_[0:50, -20:0]]).all() and (found[0][70:] == 0xFFFFFFFF).all()
    assert (grown.mutated() == fresh.mutated()).all()
    assert grown.audit().clean and fresh.audit().clean
    d_trees, d_indices = grown.diff(fresh)
    assert d_trees.shape == (0,) and d_indices.shape == (0,)
    # update, entries into appended trees included; then the two still agree and still equal a forest of the edited leaves
    values = merkle_model.random_leaves(rng, trees.shape[0])
    grown.update(trees, indices, values)
    d_trees, d_indices = grown.diff(fresh)
    assert d_trees.shape[0] == np.unique(at).shape[0]
    fresh.update(trees, indices, values)
    edited = np.array(leaves, copy=True)
    edited[at] = values                                              # numpy keeps the last of repeated cells, as update does
    assert (grown.roots() == fresh.roots()).all() and (grown.roots()[:ntrees] == gpu.forest_roots(edited, counts)).all()
    assert grown.diff(fresh)[0].shape == (0,) and grown.audit().clean
    grown.free()
    fresh.free()


def test_append_proofs_and_verify_in_stream_order(gpu):
    rng = np.random.default_rng(151)
    counts = [int(c) for c in rng.integers(1, 131, size=60)]
    new_counts = [int(c) for c in rng.integers(1, 131, size=16)]
    leaves, new = merkle_model.random_leaves(rng, sum(counts)), merkle_model.random_leaves(rng, sum(new_counts))
    forest = gpu.build_forest(leaves, counts, max_count=130, reserve_trees=20, reserve_leaves=sum(new_counts) + 5)
    H, ntrees = forest.levels, forest.ntrees
    qt, qi = fp.random_queries(rng, new_counts, 200)                 # leaves of the new trees only
    q_leaves = new[fc.offsets_of(new_counts).astype(np.int64)[qt.astype(np.int64)] + qi.astype(np.int64)]
    qt = (qt + len(counts)).astype(np.uint32)
    d_new, d_off, d_qt, d_qi, d_ql = (gpu.upload(a) for a in (new, fc.offsets_of(new_counts), qt, qi, q_leaves))
    d_status = gpu.upload(np.full(1, 0xDEADBEEF, dtype=np.uint32))
    d_sib, d_h, d_ok = gpu.alloc(32 * 200 * H), gpu.alloc(4 * 200), gpu.alloc(4 * 200)
    s = gpu.new_stream()
    forest.append_async(d_new, new.shape[0], d_off, len(new_counts), d_status, stream=s)
    forest.proofs_async(d_qt, d_qi, 200, d_sib, d_h, stream=s)
    gpu.verify_forest_proofs_async(d_ql, d_qt, d_qi, d_sib, d_h, 200, H, forest.roots_buf, ntrees, d_ok, stream=s)
    gpu.sync(s)
    assert int(gpu.download(d_status, 4)[0]) == 0
    assert (gpu.download(d_ok, 4 * 200) == 1).all()                 # every proof of a new leaf verifies against the new roots in place
    assert (gpu.download(d_h, 4 * 200) >= 1).all()
    forest.appended(new_counts)
    assert forest.used_trees == 76 and forest.free_trees == 4 and forest.free_leaves == 5
    assert (forest.roots()[:76] == gpu.forest_roots(np.concatenate([leaves, new]), counts + new_counts)).all()
    gpu.lib.vkmr_hip_stream_destroy(gpu.index, s)
    for b in (d_new, d_off, d_qt, d_qi, d_ql, d_status, d_sib, d_h, d_ok):
        b.free()
    forest.free()


def test_truncate_then_append_others(gpu):
    counts = [5, 130, 0, 64, 3, 65, 1, 9]
    others = [2, 77]
    rng = np.random.default_rng(161)
    leaves = merkle_model.random_leaves(rng, sum(counts) + 40)
    forest = fa.Growing(gpu, leaves, counts, 130, len(counts))       # all eight resident, 40 spare cells, no spare tree
    forest.truncate(5)                                               # trees 5, 6, 7 go
    forest.counts[5:] = others + [0]
    kept = forest.used
    forest.leaves = np.concatenate([leaves[:kept], merkle_model.random_leaves(rng, sum(others)), leaves[kept + sum(others):]])
    got, want = forest.state(), forest.fresh_state()
    for what, a, b in zip(("roots", "offsets"), got[2:4], want[2:4]):    # the level cells of the dropped trees stay: no tree's any more
        assert (a == b).all(), what
    assert not got[2].reshape(-1, 8)[5:].any()                       # the roots of the dropped trees are zero
    assert forest.raw.handle.audit().clean
    assert forest.append_next(2) == 0
    got, want = forest.state(), forest.fresh_state()
    assert (got[2] == want[2]).all() and (got[3] == want[3]).all()
    assert not got[2].reshape(-1, 8)[7:].any()                       # tree 7 is unused now
    # every cell a build writes: the handle over the offsets as they are proves every leaf, and nothing is a bad node
    import vk_merkle_roots_amd as vk
    now = forest.counts_now()
    handle = vk.MerkleForest(gpu, forest.raw.d_leaves, forest.total, now, forest.raw.d_off, 130, forest.raw.d_forest, forest.raw.d_roots)
    fresh = gpu.build_forest(forest.leaves[: sum(now)], now, max_count=130, reserve_leaves=forest.total - sum(now))
    assert handle.audit().clean and handle.diff(fresh)[0].shape == (0,)
    trees, indices = fa.fu.every_leaf(now)
    sib, h = handle.proofs(trees, indices)
    sib_f, h_f = fresh.proofs(trees, indices)
    assert (sib == sib_f).all() and (h == h_f).all()
    assert gpu.verify_forest_proofs(forest.leaves[: sum(now)], trees, indices, sib, h, handle.roots()).all()
    fresh.free()
    forest.free()


def test_truncate_and_append_through_the_handle(gpu):
    rng = np.random.default_rng(171)
    counts = [5, 130, 0, 64, 3, 65, 1, 9]
    leaves = merkle_model.random_leaves(rng, sum(counts))
    forest = gpu.build_forest(leaves, counts, max_count=130, reserve_trees=1, reserve_leaves=30)
    forest.truncate(5)
    kept = sum(counts[:5])
    assert (forest.used_trees, forest.free_trees, forest.used_leaves, forest.free_leaves) == (5, 4, kept, forest.total - kept)
    assert not forest.roots()[5:].any() and forest.audit().clean
    others, other_leaves = [2, 77, 0], merkle_model.random_leaves(rng, 79)
    assert forest.append(other_leaves, others).tolist() == [5, 6, 7]
    now = counts[:5] + others
    assert forest.counts.tolist() == now + [0]
    assert (forest.roots()[:8] == gpu.forest_roots(np.concatenate([leaves[:kept], other_leaves]), now)).all() and not forest.roots()[8:].any()
    assert forest.audit().clean
    with pytest.raises(ValueError):
        forest.append(merkle_model.random_leaves(rng, 2), [1, 1])    # one free tree
    forest.free()


def test_masks_of_the_appended_trees(gpu):
    rng = np.random.default_rng(181)
    a, b, c = merkle_model.random_leaves(rng, 3)
    head = merkle_model.random_leaves(rng, 9)
    counts = [5, 4, 4, 3, 0, 2]                                      # trees 0, 1 resident; then [a, b, c, c], [a, b, c], none, [a, a]
    leaves = np.concatenate([head, [a, b, c, c], [a, b, c], [a, a]])
    want = gpu.forest_roots_mutated(leaves, counts)[1]
    assert want[2] != 0 and want[3] == 0 and want[5] != 0
    forest = fa.Growing(gpu, leaves, counts + [0], 5, 2)
    assert forest.append_next(4, mutated=True) == 0
    masks = forest.state()[4]
    assert (masks[2:6] == want[2:6]).all()
    assert (masks[[0, 1, 6]] == 0x5A5A5A5A5A5A5A5A).all()            # the other trees' masks in the caller's array are untouched
    fa.assert_same(forest.state(), forest.fresh_state(), "masks")
    forest.free()
    # and through the handle
    grown = gpu.build_forest(head, counts[:2], max_count=5, mutated=True, reserve_trees=5, reserve_leaves=9)
    built = np.array(grown.built_mutated, copy=True)
    trees, masks = grown.append(leaves[9:], counts[2:], mutated=True)
    assert trees.tolist() == [2, 3, 4, 5] and (masks == want[2:6]).all()
    assert (grown.built_mutated == built).all()                      # stays what it says: the masks of the build
    assert (grown.mutated()[:6] == want).all() and not grown.mutated()[6:].any()
    grown.free()


def test_a_forest_of_a_million_leaves_grows_by_64_trees(gpu):
    rng = np.random.default_rng(191)
    counts = []
    while sum(counts) < (1 << 20) - 4095:
        counts.append(int(rng.integers(1, 4096)))
    counts.append((1 << 20) - sum(counts))
    more = [int(c) for c in rng.integers(1, 4096, size=64)]
    leaves = merkle_model.random_leaves(rng, (1 << 20) + sum(more) + 100)
    forest = fa.Growing(gpu, leaves, counts + more, 4095, len(counts))
    assert forest.append_next(64) == 0
    fa.assert_same(forest.state(), forest.fresh_state(), "2^20 leaves and 64 trees")
    forest.free()
