"""Forests that slide on the GPU (vkmr_hip_forest_drop_front_async and vkmr_hip_forest_copy_trees_async through HipDevice and
MerkleForest): a drop moves nothing and leaves what a fresh build over the new offsets writes; after every copy the leaves,
EVERY cell of the forest buffer, the roots, the offsets and the masks equal a fresh build over the destination's offsets, the
cells nobody writes included; a refused copy changes nothing; the copy is ordered on its stream in front of a proof gather and
a verify; and the slide itself -- drop, repack with a new reserve, append -- through the handles."""
import numpy as np
import pytest

import forest_append_cases as fa
import forest_cases as fc
import forest_proof_cases as fp
import forest_repack_cases as fr
import forest_update_cases as fu
import merkle_model

pytestmark = pytest.mark.gpu

NAMES = sorted(n for n in fc.CASES if n != "all_empty")


def with_equal_siblings(leaves, counts, first):
    """`leaves` with the first two leaves of every third tree of two or more made equal: masks that are not all zero."""
    leaves = np.array(leaves, copy=True)
    off = fc.offsets_of(counts).astype(np.int64) + first
    for t in range(0, len(counts), 3):
        if counts[t] >= 2:
            leaves[off[t] + 1] = leaves[off[t]]
    return leaves


def scan_masks(gpu, raw, d_mutated):
    gpu.forest_tree_mutated_async(raw.d_leaves, raw.d_forest, raw.total, raw.d_off, raw.ntrees, raw.max_count, d_mutated)
    return gpu.download(d_mutated, 8 * raw.ntrees, dtype=np.uint64)


def fresh_after_drop(gpu, leaves, used_end, now, max_count, first):
    """(leaves, forest buffer, roots, offsets, masks) of a fresh build between guard patterns over the counts `now`, the first
    tree at cell `first`."""
    fresh = fu.RawForest(gpu, fa.guarded(leaves, used_end), now, max_count, first=first)
    d_mut = gpu.alloc(8 * len(now))
    state = (*fresh.state(), gpu.download(fresh.d_off, 8 * (len(now) + 1), dtype=np.uint64), scan_masks(gpu, fresh, d_mut))
    d_mut.free()
    fresh.free()
    return state


def cells_where_written(fresh, otherwise):
    """The forest buffer a build leaves when it writes `fresh`'s cells over `otherwise`: a cell of 8 guard words was not written."""
    fresh, otherwise = fresh.reshape(-1, 8), otherwise.reshape(-1, 8)
    kept = (fresh == fa.GUARD).all(axis=1)
    return np.where(kept[:, None], otherwise, fresh).reshape(-1)


# ---- drop_front ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_a_drop_moves_nothing_and_leaves_a_fresh_builds_roots_offsets_and_masks(gpu, name):
    import vk_merkle_roots_amd as vk
    counts, first = fc.CASES[name], 5
    n, ntrees, max_count = sum(counts), len(counts), max(counts)
    leaves = with_equal_siblings(fc.random_leaves(first + n + 7, seed=len(name) * 7919 + n), counts, first)
    forest = fa.Growing(gpu, leaves, counts, max_count, ntrees, first=first)
    raw = forest.raw
    scan_masks(gpu, raw, forest.d_mutated)                           # the masks of the forest as built
    before = forest.state()
    off = fc.offsets_of(counts).astype(np.int64) + first
    for k in fr.drop_points(ntrees):
        gpu.forest_drop_front_enqueue(raw.d_off, ntrees, k, raw.d_roots, forest.d_mutated)
        gpu.sync()
        after = forest.state()
        assert (after[0] == before[0]).all() and (after[1] == before[1]).all(), k      # leaves and forest buffer: byte for byte
        now = [0] * k + counts[k:]
        want = fresh_after_drop(gpu, leaves, forest.used, now, max_count, int(off[k]))
        for what, a, b in zip(("roots", "offsets", "masks"), after[2:], want[2:]):
            assert a.shape == b.shape and (a == b).all(), (k, what)
        assert not after[2].reshape(-1, 8)[:k].any() and (after[3][: k + 1] == off[k]).all()
        handle = vk.MerkleForest(gpu, raw.d_leaves, forest.total, now, raw.d_off, max_count, raw.d_forest, raw.d_roots)
        assert handle.audit().clean, k
        if k and counts[0]:                                          # an update entry naming a dropped tree: refused on the device
            assert raw.update(np.array([0], dtype=np.uint32), np.array([0], dtype=np.uint64), fc.random_leaves(1, seed=k)) != 0
            fr.assert_unchanged(forest.state(), after, (k, "refused update"))
    forest.free()


@pytest.mark.parametrize("name", NAMES)
def test_the_kept_trees_keep_their_numbers_proofs_and_leaves(gpu, name):
    counts = fc.CASES[name]
    n, ntrees = sum(counts), len(counts)
    leaves = fc.random_leaves(n, seed=len(name) * 7927 + n)
    forest = gpu.build_forest(leaves, counts, max_count=max(counts))
    trees, indices = fu.every_leaf(counts)
    at = fu.cells_of(counts, trees, indices)
    sib, h = forest.proofs(trees, indices)
    pick = np.unique(np.concatenate([np.arange(min(n, 40)), np.arange(max(0, n - 40), n), np.linspace(0, n - 1, 40).astype(np.int64)]))
    found = forest.find(leaves[at[pick]])
    assert (found[0] == trees[pick]).all() and (found[1] == indices[pick]).all()
    for k in fr.drop_points(ntrees):
        forest.drop_front(k)
        cut = int(sum(counts[:k]))
        assert (forest.dropped_trees, forest.dropped_leaves, forest.live_leaves, forest.used_leaves, forest.free_leaves) == (k, cut, n - cut, n, 0)
        assert forest.counts.tolist() == [0] * k + counts[k:]
        roots = forest.roots()
        assert not roots[:k].any() and (k == ntrees or (roots[k:] == gpu.forest_roots(leaves[cut:], counts[k:])).all())
        assert forest.audit().clean
        keep = trees >= k
        if keep.any():
            sib_k, h_k = forest.proofs(trees[keep], indices[keep])
            assert (sib_k == sib[keep]).all() and (h_k == h[keep]).all()
            assert gpu.verify_forest_proofs(leaves[at[keep]], trees[keep], indices[keep], sib_k, h_k, roots).all()
        now = forest.find(leaves[at[pick]])
        gone = trees[pick] < k
        assert (now[0][gone] == 0xFFFFFFFF).all() and (now[1][gone] == 2**64 - 1).all()
        assert (now[0][~gone] == trees[pick][~gone]).all() and (now[1][~gone] == indices[pick][~gone]).all()
        if k and counts[0]:
            with pytest.raises(IndexError):
                forest.update([0], [0], fc.random_leaves(1, seed=3))
    forest.free()


def test_append_and_extend_go_on_behind_a_dropped_front(gpu):
    counts = [4, 0, 7, 130, 33, 0, 65, 64, 129, 3]                   # seven resident, three to append; then the last takes 3 more
    k, split, more = 3, 7, 3
    leaves = fc.random_leaves(sum(counts) + more + 6, seed=211)
    forest = fa.Growing(gpu, leaves, counts, 132, split)
    raw = forest.raw
    off = fc.offsets_of(counts).astype(np.int64)
    gpu.forest_drop_front_enqueue(raw.d_off, forest.ntrees, k, raw.d_roots, None)
    gpu.sync()
    before = forest.state()
    assert forest.append_next(3) == 0
    got = forest.state()
    want = fresh_after_drop(gpu, leaves, forest.used, [0] * k + counts[k:], 132, int(off[k]))
    assert (got[0] == want[0]).all() and (got[2] == want[2]).all() and (got[3] == want[3]).all()
    assert (got[1] == cells_where_written(want[1], before[1])).all()  # the dropped trees' cells stay, every other cell is the build's
    used, last = forest.used, forest.ntrees - 1
    d_new, d_status = gpu.upload(leaves[used: used + more]), gpu.upload(np.full(1, fa.STATUS_FILL, dtype=np.uint32))
    gpu.forest_extend_enqueue(raw.d_leaves, raw.d_forest, forest.total, raw.d_off, forest.ntrees, 132, last, counts[last], used, d_new, more,
                              raw.d_roots, None, d_status)
    assert int(gpu.download(d_status, 4)[0]) == 0
    got = forest.state()
    want = fresh_after_drop(gpu, leaves, used + more, [0] * k + counts[k:last] + [counts[last] + more], 132, int(off[k]))
    assert (got[0] == want[0]).all() and (got[2] == want[2]).all() and (got[3] == want[3]).all()
    assert (got[1] == cells_where_written(want[1], before[1])).all()
    d_new.free()
    d_status.free()
    forest.free()


# ---- copy ------------------------------------------------------------------------------------------------------------------

def copied_equals_fresh(gpu, src, tight_dst, flagged, note):
    """Every selection at every placement: all five arrays of the destination equal a fresh build's over the same guard-filled
    buffers, the masks those of the source trees (forest_roots_mutated's)."""
    for sel_name, sel in sorted(fr.selections(src.ntrees).items()):
        for first_tree, used in fr.PLACEMENTS:
            dst_max = fr.max_counts(src.counts, sel, used, first_tree, tight_dst)[1]
            dst = fr.Destination(gpu, src, sel, first_tree, used, dst_max)
            assert dst.copy_all(flagged=flagged) == 0, (note, sel_name, first_tree, used)
            got = dst.state()
            fa.assert_same(got, dst.fresh_state(), (note, sel_name, first_tree, used))
            masks = np.full(dst.ntrees, fr.MASK_FILL, dtype=np.uint64)
            if flagged:
                masks[first_tree: first_tree + len(sel)] = src.masks[np.asarray(sel, dtype=np.int64)]
            assert (got[4] == masks).all(), (note, sel_name, first_tree, used)
            dst.free()


@pytest.mark.parametrize("tight_dst,flagged", [(True, False), (False, True), (True, True), (False, False)],
                         ids=["tight", "loose-flagged", "tight-flagged", "loose"])
@pytest.mark.parametrize("name", sorted(fc.CASES))
def test_copied_trees_equal_a_fresh_build_in_every_cell(gpu, name, tight_dst, flagged):
    counts = fc.CASES[name]
    n = sum(counts)
    leaves = with_equal_siblings(fc.random_leaves(fr.SRC_FIRST + n + fr.SRC_SLACK, seed=len(name) * 7933 + n), counts, fr.SRC_FIRST)
    src_max = fr.max_counts(counts, [], 0, 0, tight_dst)[0]
    src = fr.Source(gpu, counts, src_max, 0, leaves=leaves)
    if n:                                                            # the source's masks are forest_roots_mutated's
        want = gpu.forest_roots_mutated(leaves[fr.SRC_FIRST: fr.SRC_FIRST + n], counts)
        assert (src.raw.state()[2].reshape(-1, 8) == want[0]).all() and (src.masks == want[1]).all()
    copied_equals_fresh(gpu, src, tight_dst, flagged, name)
    src.free()


def test_masks_are_zeroed_when_only_the_destination_has_them(gpu):
    counts = [5, 4, 4, 3, 0, 2]
    leaves = with_equal_siblings(fc.random_leaves(fr.SRC_FIRST + sum(counts) + fr.SRC_SLACK, seed=221), counts, fr.SRC_FIRST)
    src = fr.Source(gpu, counts, 5, 0, leaves=leaves)
    assert src.masks[0] != 0 and src.masks[3] != 0
    dst = fr.Destination(gpu, src, [3, 0, 4, 5], 3, 5, 5)
    assert dst.copy_all(flagged=True, src_masks=False) == 0
    got = dst.state()
    fa.assert_same(got, dst.fresh_state(), "no source masks")
    assert got[4].tolist() == [fr.MASK_FILL] * 3 + [0] * 4 + [fr.MASK_FILL] * fr.BEHIND
    dst.free()
    src.free()


SRC_COUNTS = [4, 0, 7, 3, 5, 1, 0, 6, 9]                             # nine trees; the destination allows 7 leaves a tree
REFUSED = [  # (sel, first_tree, used relative to the true one, new offsets, n_leaves, the status)
    ([3, 4], 3, 0, [1, 4, 9], 9, 1),             # the new offsets start above 0
    ([3, 4], 3, 0, [0, 3, 8], 9, 1),             # end short of n_leaves
    ([8], 3, 0, [0, 9], 9, 2),                   # a count above the destination's max_count
    ([3, 4], 3, 1, [0, 3, 8], 8, 4),             # a wrong `used`: no offset from first_tree on equals it
    ([3, 4], 3, -1, [0, 3, 8], 8, 4),
    ([3, 4], 0, 0, [0, 3, 8], 8, 4),             # a first_tree whose tree is not empty at `used`
    ([9], 3, 0, [0, 3], 3, 8),                   # a tree the source does not have
    ([2**32 - 1, 3], 3, 0, [0, 3, 6], 6, 8),
    ([3], 3, 0, [0, 4], 4, 8),                   # a new count that is not the source tree's
    ([5, 0], 3, 0, [0, 1, 2], 2, 8),
    ([9, 3], 3, 1, [2, 11, 9], 9, 15),           # everything at once
]


@pytest.mark.parametrize("sel,first_tree,used_off,new_offsets,n_leaves,want", REFUSED)
def test_a_refused_copy_changes_nothing(gpu, sel, first_tree, used_off, new_offsets, n_leaves, want):
    src = fr.Source(gpu, SRC_COUNTS, 9, seed=231)
    dst = fr.Destination(gpu, src, [3, 4, 5], 3, 5, 7)
    before = dst.state()
    for flagged in (False, True):
        got = dst.copy_raw(sel, first_tree, dst.used + used_off, new_offsets, n_leaves=n_leaves, flagged=flagged)
        assert got == want                                           # the status word held 0xDEADBEEF
        fr.assert_unchanged(dst.state(), before, flagged)
    assert dst.copy_all() == 0                                       # and the forest still takes a good copy
    fa.assert_same(dst.state(), dst.fresh_state(), "after the refusals")
    dst.free()
    src.free()


def test_copy_proofs_and_verify_in_stream_order(gpu):
    rng = np.random.default_rng(241)
    counts = [int(c) for c in rng.integers(1, 131, size=60)]
    src_counts = [int(c) for c in rng.integers(1, 131, size=30)] + [0, 1]
    leaves, src_leaves = merkle_model.random_leaves(rng, sum(counts)), merkle_model.random_leaves(rng, sum(src_counts))
    sel = [int(t) for t in rng.permutation(32)[:16]]
    new_counts = [src_counts[t] for t in sel]
    n = sum(new_counts)
    src = gpu.build_forest(src_leaves, src_counts, max_count=130)
    forest = gpu.build_forest(leaves, counts, max_count=130, reserve_trees=20, reserve_leaves=n + 5)
    H, ntrees = forest.levels, forest.ntrees
    src_off = fc.offsets_of(src_counts).astype(np.int64)
    new = np.concatenate([src_leaves[src_off[t]: src_off[t + 1]] for t in sel])
    qt, qi = fp.random_queries(rng, new_counts, 200)                 # leaves of the new trees only
    q_leaves = new[fc.offsets_of(new_counts).astype(np.int64)[qt.astype(np.int64)] + qi.astype(np.int64)]
    qt = (qt + len(counts)).astype(np.uint32)
    d_sel, d_off, d_qt, d_qi, d_ql = (gpu.upload(a) for a in (np.array(sel, dtype=np.uint32), fc.offsets_of(new_counts), qt, qi, q_leaves))
    d_status = gpu.upload(np.full(1, fa.STATUS_FILL, dtype=np.uint32))
    d_sib, d_h, d_ok = gpu.alloc(32 * 200 * H), gpu.alloc(4 * 200), gpu.alloc(4 * 200)
    s = gpu.new_stream()
    forest.append_from_async(src, d_sel, len(sel), n, d_off, d_status, stream=s)
    forest.proofs_async(d_qt, d_qi, 200, d_sib, d_h, stream=s)
    gpu.verify_forest_proofs_async(d_ql, d_qt, d_qi, d_sib, d_h, 200, H, forest.roots_buf, ntrees, d_ok, stream=s)
    gpu.sync(s)
    assert int(gpu.download(d_status, 4)[0]) == 0
    assert (gpu.download(d_ok, 4 * 200) == 1).all()                 # every proof of a copied leaf verifies against the new roots in place
    assert (gpu.download(d_h, 4 * 200) >= 1).all()
    forest.appended(new_counts)
    assert forest.used_trees == 76 and forest.free_trees == 4 and forest.free_leaves == 5
    assert (forest.roots()[:76] == gpu.forest_roots(np.concatenate([leaves, new]), counts + new_counts)).all()
    assert forest.audit().clean
    gpu.lib.vkmr_hip_stream_destroy(gpu.index, s)
    for b in (d_sel, d_off, d_qt, d_qi, d_ql, d_status, d_sib, d_h, d_ok):
        b.free()
    forest.free()
    src.free()


# ---- through the handles ---------------------------------------------------------------------------------------------------

def same_forest(gpu, got, want, leaves, counts):
    """`got` is `want`, a build_forest of `counts` over `leaves`: roots, the proofs of every leaf, an empty diff, a clean audit."""
    assert (got.ntrees, got.total, got.max_count, got.levels) == (want.ntrees, want.total, want.max_count, want.levels)
    assert (got.counts == want.counts).all() and got.used_trees == want.used_trees and got.used_leaves == want.used_leaves
    assert (got.roots() == want.roots()).all()
    assert (got.roots()[: len(counts)] == gpu.forest_roots(leaves, counts)).all()
    trees, indices = fu.every_leaf(counts)
    sib, h = got.proofs(trees, indices)
    sib_w, h_w = want.proofs(trees, indices)
    assert (sib == sib_w).all() and (h == h_w).all()
    assert gpu.verify_forest_proofs(leaves[fu.cells_of(counts, trees, indices)], trees, indices, sib, h, got.roots()).all()
    d_trees, d_indices = got.diff(want)
    assert d_trees.shape == (0,) and d_indices.shape == (0,)
    assert got.audit().clean and want.audit().clean


def test_the_slide_drop_repack_append(gpu):
    rng = np.random.default_rng(251)
    counts = [5, 130, 0, 64, 3, 65, 1, 9, 2, 77, 33]
    leaves = merkle_model.random_leaves(rng, sum(counts))
    off = fc.offsets_of(counts).astype(np.int64)
    forest = gpu.build_forest(leaves[: off[8]], counts[:8], max_count=130)          # eight trees, no reserve
    forest.drop_front(3)
    assert (forest.free_trees, forest.free_leaves, forest.dropped_leaves) == (0, 0, 135)
    slid = forest.repacked(reserve_trees=3, reserve_leaves=sum(counts[8:]) + 4)
    assert (slid.ntrees, slid.used_trees, slid.free_trees, slid.dropped_trees, slid.used_leaves, slid.free_leaves) == (8, 5, 3, 0, int(off[8] - off[3]), 116)
    assert slid.append(leaves[off[8]:], counts[8:]).tolist() == [5, 6, 7]
    want = gpu.build_forest(leaves[off[3]:], counts[3:], max_count=130, reserve_leaves=4)
    same_forest(gpu, slid, want, leaves[off[3]:], counts[3:])
    assert forest.audit().clean and (forest.roots()[3:] == want.roots()[:5]).all()  # the old forest is as it was
    for f in (forest, slid, want):
        f.free()


def test_append_from_merges_two_forests(gpu):
    rng = np.random.default_rng(261)
    a_counts, b_counts = [7, 0, 130, 2, 64], [1, 65, 0, 4, 4, 129]
    a_leaves, b_leaves = merkle_model.random_leaves(rng, sum(a_counts)), merkle_model.random_leaves(rng, sum(b_counts))
    b_leaves[67] = b_leaves[66]                                      # tree 3 of b: [x, x, ., .]
    a, b = gpu.build_forest(a_leaves, a_counts, max_count=130), gpu.build_forest(b_leaves, b_counts, max_count=129)
    both = a.repacked(reserve_trees=b.ntrees, reserve_leaves=b.total)
    numbers, masks = both.append_from(b, np.arange(b.ntrees), mutated=True)
    assert numbers.tolist() == list(range(5, 11))
    leaves, counts = np.concatenate([a_leaves, b_leaves]), a_counts + b_counts
    assert (masks == gpu.forest_roots_mutated(leaves, counts)[1][5:]).all() and masks[3] != 0
    want = gpu.build_forest(leaves, counts, max_count=130)
    same_forest(gpu, both, want, leaves, counts)
    # the device's own refusal: a handle whose counts are not the forest's
    stale = a.repacked(reserve_trees=1, reserve_leaves=130)
    b.counts[[0, 3]] = b.counts[[3, 0]]
    with pytest.raises(RuntimeError, match="bit 3"):
        stale.append_from(b, [0])
    assert stale.used_trees == 5 and stale.audit().clean
    for f in (a, b, both, want, stale):
        f.free()


def test_repacked_deletes_from_the_middle_and_keeps_masks(gpu):
    rng = np.random.default_rng(271)
    counts = [5, 130, 0, 64, 3, 65, 1, 9]
    leaves = merkle_model.random_leaves(rng, sum(counts))
    leaves[6] = leaves[5]                                            # tree 1: equal leaves 0 and 1
    forest = gpu.build_forest(leaves, counts, max_count=130)
    keep = [0, 1, 4, 6, 7]
    off = fc.offsets_of(counts).astype(np.int64)
    kept_leaves = np.concatenate([leaves[off[t]: off[t + 1]] for t in keep])
    kept_counts = [counts[t] for t in keep]
    thin = forest.repacked(trees=keep, mutated=True)
    want = gpu.build_forest(kept_leaves, kept_counts, max_count=130, mutated=True)
    same_forest(gpu, thin, want, kept_leaves, kept_counts)
    assert (thin.built_mutated == want.built_mutated).all() and thin.built_mutated[1] != 0
    small = forest.repacked(trees=[4, 6], max_count=3)               # a tighter max_count: fewer levels than the source
    want_small = gpu.build_forest(np.concatenate([leaves[off[4]: off[5]], leaves[off[6]: off[7]]]), [3, 1], max_count=3)
    assert small.levels == 2 < forest.levels
    same_forest(gpu, small, want_small, np.concatenate([leaves[off[4]: off[5]], leaves[off[6]: off[7]]]), [3, 1])
    for f in (forest, thin, want, small, want_small):
        f.free()


def test_a_suffix_of_a_forest_of_a_million_leaves_copied(gpu):
    rng = np.random.default_rng(281)
    counts = []
    while sum(counts) < (1 << 20) - 4095:
        counts.append(int(rng.integers(1, 4096)))
    counts.append((1 << 20) - sum(counts))
    leaves = merkle_model.random_leaves(rng, fr.SRC_FIRST + (1 << 20) + fr.SRC_SLACK)
    src = fr.Source(gpu, counts, 4095, 0, leaves=leaves)
    sel = list(range(len(counts) // 2, len(counts)))
    dst = fr.Destination(gpu, src, sel, 3, 5, 2**63)
    assert dst.copy_all() == 0
    fa.assert_same(dst.state(), dst.fresh_state(), "a suffix of 2^20 leaves")
    dst.free()
    src.free()
