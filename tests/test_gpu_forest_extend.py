"""The open tree of a stored forest grown or shrunk by leaves on the GPU (vkmr_hip_forest_extend_async and
vkmr_hip_forest_shrink_async through HipDevice and MerkleForest): after every call the leaves, the offsets, the roots and every
cell of the forest buffer that a fresh build of the final counts writes equal that build, and every other cell -- the guard
pattern around the buffers, the cells of dropped nodes -- is what it was; a refused call changes nothing; every reader takes the
result; the call is ordered on its stream in front of a proof gather and a verify."""
import numpy as np
import pytest

import forest_cases as fc
import forest_extend_cases as fe
import merkle_model

pytestmark = pytest.mark.gpu


def one_call(gpu, front, behind, c, c2, slack=3, max_count=None, in_place=False, seed=0):
    """Built with c leaves in the open tree, taken to c2 in one call, compared; then back to c in one more, compared again."""
    o, top = sum(front), max(c, c2)
    leaves = fc.random_leaves(o + top + slack, seed=1000 * c + c2 + seed)
    forest = fe.Open(gpu, leaves, front, c, behind, max_count or max(top, 3))
    for to in (c2, c):
        before = forest.state()
        assert forest.go(to, in_place=in_place) == 0, (c, c2, to)
        fe.assert_as_fresh(forest.state(), before, forest.fresh_state(), forest.used, (c, c2, to))
    forest.free()


@pytest.mark.parametrize("c,c2", fe.PAIRS, ids=[f"{a}to{b}" for a, b in fe.PAIRS])
def test_the_open_tree_at_tree_3_offset_5_with_two_empty_trees_behind(gpu, c, c2):
    one_call(gpu, fe.FRONT, 2, c, c2)


@pytest.mark.parametrize("c,c2", fe.THREE, ids=[f"{a}to{b}" for a, b in fe.THREE])
def test_the_open_tree_as_tree_0(gpu, c, c2):
    one_call(gpu, [], 2, c, c2, seed=1)


@pytest.mark.parametrize("c,c2", fe.THREE, ids=[f"{a}to{b}" for a, b in fe.THREE])
def test_no_tree_behind_no_cell_to_spare_and_max_count_reached(gpu, c, c2):
    # ntrees == used_trees; the larger count fills the leaves buffer to its last cell and is max_count exactly
    one_call(gpu, fe.FRONT, 0, c, c2, slack=0, max_count=max(c, c2), seed=2)


@pytest.mark.parametrize("c,c2", [(2, 3), (4, 9), (63, 130), (0, 3)], ids=["2to3", "4to9", "63to130", "0to3"])
def test_leaves_the_caller_put_in_place(gpu, c, c2):
    one_call(gpu, fe.FRONT, 2, c, c2, in_place=True, seed=3)


@pytest.mark.parametrize("c,c2", [(2, 3), (3, 2), (5, 7), (64, 65), (7, 0)], ids=["2to3", "3to2", "5to7", "64to65", "7to0"])
def test_more_launches_than_the_open_tree_has_levels(gpu, c, c2):
    one_call(gpu, fe.FRONT, 2, c, c2, slack=5000, max_count=4096, seed=4)     # H = 12


def test_steps_one_after_another_each_against_a_fresh_build(gpu):
    leaves = fc.random_leaves(5 + 140 + 3, seed=77)
    forest = fe.Open(gpu, leaves, fe.FRONT, 1, 2, 140)
    for to in (2, 3, 4, 5, 9, 8, 16, 17, 33, 31, 64, 130, 129, 128, 65, 64, 63, 2, 3, 0, 140, 1):
        before = forest.state()
        assert forest.go(to) == 0, to
        fe.assert_as_fresh(forest.state(), before, forest.fresh_state(), forest.used, to)
    forest.free()


def test_extend_packed_from_strings_equals_the_forest_of_all_strings(gpu):
    import vk_merkle_roots_amd as vk
    counts, n = [3, 65, 7], 75
    batch = vk.pack_lines(b"".join(b"string %d of the forest\n" % i for i in range(n + 130)))
    want = vk.merkle_forest_packed(gpu, batch, counts[:2] + [7 + 130], max_count=200, reserve_trees=2, reserve_leaves=9)
    got = vk.merkle_forest_packed(gpu, batch.slice(0, n), counts, max_count=200, reserve_trees=2, reserve_leaves=139)
    assert (got.open_tree, got.used_leaves, got.free_leaves) == (2, n, 139)
    assert got.extend_packed(batch.slice(n, n + 1)) == 8
    assert got.extend_packed(batch.slice(n + 1, n + 130)) == 137
    assert (got.open_tree, got.used_trees, got.used_leaves, got.free_leaves) == (2, 3, n + 130, 9)
    assert (got.counts == want.counts).all() and (got.total, got.ntrees, got.levels) == (want.total, want.ntrees, want.levels)
    assert (got.roots() == want.roots()).all()
    assert (gpu.download(got.digests, 32 * (n + 130)) == gpu.download(want.digests, 32 * (n + 130))).all()
    assert (gpu.download(got.offsets, 8 * (got.ntrees + 1), dtype=np.uint64) == gpu.download(want.offsets, 8 * (got.ntrees + 1), dtype=np.uint64)).all()
    assert got.diff(want)[0].shape == (0,) and got.audit().clean
    got.free()
    want.free()


def test_extend_append_truncate_extend_through_the_handle(gpu):
    rng = np.random.default_rng(201)
    leaves = merkle_model.random_leaves(rng, 400)
    forest = gpu.build_forest(leaves[:70], [5, 65], max_count=130, reserve_trees=3, reserve_leaves=330)

    def same_as_fresh(counts, rows):
        fresh = gpu.build_forest(rows, counts, max_count=130, reserve_trees=5 - len(counts), reserve_leaves=400 - rows.shape[0])
        assert forest.counts.tolist() == fresh.counts.tolist() and forest.used_trees == len(counts) and forest.used_leaves == rows.shape[0]
        assert (forest.roots() == fresh.roots()).all() and forest.diff(fresh)[0].shape == (0,) and forest.audit().clean
        assert (gpu.download(forest.offsets, 8 * 6, dtype=np.uint64) == gpu.download(fresh.offsets, 8 * 6, dtype=np.uint64)).all()
        trees, indices = fe.fu.every_leaf(counts)
        sib, h = forest.proofs(trees, indices)
        sib_f, h_f = fresh.proofs(trees, indices)
        assert (sib == sib_f).all() and (h == h_f).all()
        fresh.free()

    assert forest.extend(leaves[70:135]) == 130                      # tree 1: 65 -> 130
    same_as_fresh([5, 130], leaves[:135])
    assert forest.append(leaves[135:145], [3, 7]).tolist() == [2, 3]
    assert forest.open_tree == 3
    same_as_fresh([5, 130, 3, 7], leaves[:145])
    assert forest.extend(leaves[145:147]) == 9                       # the open tree is now tree 3
    same_as_fresh([5, 130, 3, 9], leaves[:147])
    forest.truncate(2)
    assert forest.open_tree == 1 and forest.shrink(66) == 64         # tree 1 again: 130 -> 64
    same_as_fresh([5, 64], leaves[:69])
    other = merkle_model.random_leaves(rng, 3)
    assert forest.extend(other) == 67
    same_as_fresh([5, 67], np.concatenate([leaves[:69], other]))
    with pytest.raises(ValueError):
        forest.extend(merkle_model.random_leaves(rng, 64))           # 67 + 64 leaves, max_count 130
    forest.free()


REFUSED = [  # (tree, count and used relative to the true ones)
    (3, 1, 0), (3, -1, 0),            # a wrong count: the open tree does not begin at used - count
    (3, 0, 1), (3, 0, -1),            # a wrong used: no offset behind the open tree equals it
    (3, 1, 1),                        # both, consistent with offsets[3]: the offsets behind are not `used`
    (2, -4, -7),                      # tree 2 (3 leaves ending at cell 5) taken for the open tree: a tree with leaves behind it
    (4, 0, 0),                        # the first empty tree taken for the open tree, with the open tree's count
]


@pytest.mark.parametrize("tree,count_off,used_off", REFUSED)
def test_a_refused_call_changes_nothing(gpu, tree, count_off, used_off):
    leaves = fc.random_leaves(5 + 7 + 12, seed=211)
    forest = fe.Open(gpu, leaves, fe.FRONT, 7, 2, 16)
    before = forest.state()
    new = fc.random_leaves(4, seed=212)
    count, used = forest.c + count_off, forest.used + used_off
    for mutated in (False, True):
        assert forest.extend_raw(tree, count, used, new, mutated=mutated) == 4     # the status word held 0xDEADBEEF
        assert all((a == b).all() for a, b in zip(forest.state(), before)), ("extend", mutated)
        if count >= 2:
            assert forest.shrink_raw(tree, count, used, 2, mutated=mutated) == 4
            assert all((a == b).all() for a, b in zip(forest.state(), before)), ("shrink", mutated)
    # leaves put in place by the caller are the one exception
    assert forest.extend_raw(tree, count, used, new, in_place=True) == 4
    after = forest.state()
    assert (after[0].reshape(-1, 8)[used: used + 4] == new).all()
    forest.put_leaves(used, before[0].reshape(-1, 8)[used: used + 4])
    assert all((a == b).all() for a, b in zip(forest.state(), before))
    assert forest.go(11) == 0 and forest.go(6) == 0                  # and the forest still grows and shrinks
    fresh = forest.fresh_state()
    assert (forest.state()[2] == fresh[2]).all() and (forest.state()[3] == fresh[3]).all()
    forest.free()


def test_a_tree_with_leaves_behind_the_open_tree_refuses_the_call(gpu):
    import vk_merkle_roots_amd as vk
    leaves = fc.random_leaves(30, seed=221)
    forest = fe.Open(gpu, leaves, [1, 1, 3, 4], 2, 1, 16)            # tree 3 has four leaves and tree 4, with two, is the open tree
    before = forest.state()
    # tree 3 with its true count and the cell it ends at: offsets[3] + 4 == 9 == offsets[4], but offsets[5] is 11
    assert forest.extend_raw(3, 4, 9, fc.random_leaves(2, seed=222)) == 4
    assert forest.shrink_raw(3, 4, 9, 1) == 4
    assert all((a == b).all() for a, b in zip(forest.state(), before))
    forest.free()
    # and the handle reports the device's refusal: a host view that has lost two leaves of the open tree
    handle = gpu.build_forest(leaves[:11], [1, 1, 3, 4, 2], max_count=16, reserve_trees=1, reserve_leaves=8)
    handle.counts[4] = 0
    with pytest.raises(RuntimeError, match="bit 2"):
        handle.extend(leaves[11:13])
    assert vk.forest_append_status_text(4) in str(pytest.raises(RuntimeError, handle.extend, leaves[11:13]).value)
    handle.counts[4] = 2
    assert handle.extend(leaves[11:13]) == 4 and handle.audit().clean
    handle.free()


def readers(gpu, forest, fresh, leaves, counts, new_cells, rng):
    """Every reader over `forest` against `fresh`, a fresh build of the same counts and capacity; new_cells: leaves the call
    brought in, as cells of the open tree."""
    ntrees, open_tree = len(counts), len(counts) - 1
    off = fc.offsets_of(counts).astype(np.int64)
    assert (forest.counts == fresh.counts).all() and (forest.roots() == fresh.roots()).all()
    assert (forest.roots()[:ntrees] == gpu.forest_roots(leaves, counts)).all() and not forest.roots()[ntrees:].any()
    assert forest.audit().clean
    c = counts[open_tree]
    trees = np.array([0, 1, open_tree, open_tree, open_tree], dtype=np.uint32)
    indices = np.array([0, counts[1] - 1, 0, c // 2, c - 1], dtype=np.uint64)      # the first, a middle and the last leaf of the open tree
    at = off[trees.astype(np.int64)] + indices.astype(np.int64)
    sib, h = forest.proofs(trees, indices)
    sib_f, h_f = fresh.proofs(trees, indices)
    assert (sib == sib_f).all() and (h == h_f).all() and (h >= 1).all()
    assert gpu.verify_forest_proofs(leaves[at], trees, indices, sib, h, forest.roots()).all()
    mp, mp_f = forest.multiproof(trees, indices), fresh.multiproof(trees, indices)
    assert (mp.trees == mp_f.trees).all() and (mp.indices == mp_f.indices).all() and (mp.heights == mp_f.heights).all() and (mp.nodes == mp_f.nodes).all()
    mp_at = off[mp.trees.astype(np.int64)] + mp.indices.astype(np.int64)
    assert gpu.verify_forest_multiproof(leaves[mp_at], mp.trees, mp.indices, mp.heights, mp.nodes, forest.roots())
    d_trees, d_indices = forest.diff(fresh)
    assert d_trees.shape == (0,) and d_indices.shape == (0,)
    cells = np.array(new_cells + [c - 1], dtype=np.int64)
    found = forest.find(np.concatenate([leaves[off[open_tree] + cells], merkle_model.random_leaves(rng, 1)]))
    assert (found[0][:-1] == open_tree).all() and (found[1][:-1] == cells).all() and found[0][-1] == 0xFFFFFFFF
    # update of a leaf at the right edge, in both; they still agree and equal a forest of the edited leaves
    value = merkle_model.random_leaves(rng, 1)
    for f in (forest, fresh):
        f.update(np.array([open_tree], dtype=np.uint32), np.array([c - 1], dtype=np.uint64), value)
    edited = np.array(leaves, copy=True)
    edited[off[open_tree] + c - 1] = value[0]
    assert (forest.roots() == fresh.roots()).all() and (forest.roots()[:ntrees] == gpu.forest_roots(edited, counts)).all()
    assert forest.diff(fresh)[0].shape == (0,) and forest.audit().clean


def test_every_reader_takes_the_result(gpu):
    rng = np.random.default_rng(231)
    front = [int(x) for x in rng.integers(1, 131, size=20)] + [0, 64]
    o = sum(front)
    leaves = merkle_model.random_leaves(rng, o + 200)
    forest = gpu.build_forest(leaves[: o + 64], front + [64], max_count=200, reserve_trees=2, reserve_leaves=136 + 20)
    assert forest.extend(leaves[o + 64: o + 65]) == 65 and forest.extend(leaves[o + 65: o + 200]) == 200
    fresh = gpu.build_forest(leaves, front + [200], max_count=200, reserve_trees=2, reserve_leaves=20)
    readers(gpu, forest, fresh, leaves, front + [200], [64, 65, 199], rng)
    fresh.free()
    now = gpu.download(forest.digests, 32 * (o + 129)).reshape(-1, 8)           # the update above is in the last leaf, which goes
    assert forest.shrink(71) == 129
    fresh = gpu.build_forest(now, front + [129], max_count=200, reserve_trees=2, reserve_leaves=71 + 20)
    readers(gpu, forest, fresh, now, front + [129], [0, 128], rng)
    fresh.free()
    forest.free()


def test_extend_proofs_and_verify_in_stream_order(gpu):
    rng = np.random.default_rng(241)
    front = [int(x) for x in rng.integers(1, 131, size=30)]
    o = sum(front)
    leaves, new = merkle_model.random_leaves(rng, o + 63), merkle_model.random_leaves(rng, 67)
    forest = gpu.build_forest(leaves, front + [63], max_count=130, reserve_trees=1, reserve_leaves=70)
    H, ntrees, k = forest.levels, forest.ntrees, 67
    qt, qi = np.full(k, 30, dtype=np.uint32), np.arange(63, 130, dtype=np.uint64)    # the new leaves only
    d_new, d_qt, d_qi = (gpu.upload(a) for a in (new, qt, qi))
    d_status = gpu.upload(np.full(1, 0xDEADBEEF, dtype=np.uint32))
    d_sib, d_h, d_ok = gpu.alloc(32 * k * H), gpu.alloc(4 * k), gpu.alloc(4 * k)
    s = gpu.new_stream()
    forest.extend_async(d_new, k, d_status, stream=s)
    forest.proofs_async(d_qt, d_qi, k, d_sib, d_h, stream=s)
    gpu.verify_forest_proofs_async(d_new, d_qt, d_qi, d_sib, d_h, k, H, forest.roots_buf, ntrees, d_ok, stream=s)
    gpu.sync(s)
    assert int(gpu.download(d_status, 4)[0]) == 0
    assert (gpu.download(d_ok, 4 * k) == 1).all()                    # every proof of a new leaf verifies against the new root in place
    assert (gpu.download(d_h, 4 * k) == 8).all()                     # 130 leaves: eight levels
    forest.extended(k)
    assert forest.counts[30] == 130 and forest.free_leaves == 3
    assert (forest.roots()[:31] == gpu.forest_roots(np.concatenate([leaves, new]), front + [130])).all()
    # and a shrink in front of a gather: the proof of the new last leaf is that of the smaller tree
    d_status2 = gpu.upload(np.full(1, 0xDEADBEEF, dtype=np.uint32))
    forest.shrink_async(66, d_status2, stream=s)
    forest.proofs_async(d_qt, d_qi, 1, d_sib, d_h, stream=s)         # (30, 63): the last leaf of 64
    gpu.verify_forest_proofs_async(d_new, d_qt, d_qi, d_sib, d_h, 1, H, forest.roots_buf, ntrees, d_ok, stream=s)
    gpu.sync(s)
    assert int(gpu.download(d_status2, 4)[0]) == 0 and int(gpu.download(d_ok, 4)[0]) == 1 and int(gpu.download(d_h, 4)[0]) == 6
    forest.shrunk(66)
    assert forest.counts[30] == 64 and forest.audit().clean
    gpu.lib.vkmr_hip_stream_destroy(gpu.index, s)
    for b in (d_new, d_qt, d_qi, d_status, d_status2, d_sib, d_h, d_ok):
        b.free()
    forest.free()


def masks_case(gpu, front_leaves, front, before, after):
    """The open tree from the leaves `before` to `after` (one a prefix of the other), raw and through the handle: its mask is
    what the flagged reduction gives for the final leaves, and no other mask moves."""
    longest = before if len(before) > len(after) else after
    leaves = np.concatenate([front_leaves, longest, merkle_model.random_leaves(np.random.default_rng(5), 2)])
    counts = front + [len(after)]
    want = gpu.forest_roots_mutated(np.concatenate([front_leaves, after]), counts)[1]
    was = gpu.forest_roots_mutated(np.concatenate([front_leaves, before]), front + [len(before)])[1]
    forest = fe.Open(gpu, leaves, front, len(before), 2, 8)
    state = forest.state()
    assert forest.go(len(after), mutated=True) == 0
    masks = forest.state()[4]
    assert masks[len(front)] == want[len(front)]
    others = [t for t in range(forest.ntrees) if t != len(front)]
    assert (masks[others] == fe.MASK_FILL).all()                     # the other trees' masks in the caller's array are untouched
    fe.assert_as_fresh(forest.state()[:4], state[:4], forest.fresh_state(), forest.used, "masks")
    forest.free()
    handle = gpu.build_forest(np.concatenate([front_leaves, before]), front + [len(before)], max_count=8, mutated=True, reserve_trees=1, reserve_leaves=4)
    assert (handle.built_mutated[: len(front) + 1] == was).all()
    if len(after) > len(before):
        count, mask = handle.extend(after[len(before):], mutated=True)
    else:
        count, mask = handle.shrink(len(before) - len(after), mutated=True)
    assert count == len(after) and mask == want[len(front)]
    assert (handle.mutated()[: len(front) + 1] == want).all() and not handle.mutated()[len(front) + 1:].any()
    handle.free()
    return int(was[len(front)]), int(want[len(front)])


def test_masks_of_the_open_tree(gpu):
    rng = np.random.default_rng(251)
    a, b, c = merkle_model.random_leaves(rng, 3)
    front, front_leaves = [2, 3], np.stack([a, a, a, b, c])           # tree 0 = [a, a] carries a flag of its own
    # an extend that creates an equal pair: [a, b] + [c, c]
    assert masks_case(gpu, front_leaves, front, np.stack([a, b]), np.stack([a, b, c, c])) == (0, 1)
    # an extend that removes one: [a, a, a] has two equal level-1 nodes, hash(a, a) and the lone a hashed with itself; + [b] parts them
    assert masks_case(gpu, front_leaves, front, np.stack([a, a, a]), np.stack([a, a, a, b])) == (3, 1)
    # a shrink that removes one: [a, b, c, c] -> [a, b, c], the lone c is no pair
    assert masks_case(gpu, front_leaves, front, np.stack([a, b, c, c]), np.stack([a, b, c])) == (1, 0)
    # a shrink to nothing clears the mask
    assert masks_case(gpu, front_leaves, front, np.stack([a, a]), np.zeros((0, 8), np.uint32)) == (1, 0)


def test_a_forest_of_a_million_leaves_whose_open_tree_fills_up(gpu):
    rng = np.random.default_rng(261)
    counts = [2048] * 511 + [2000]
    n = sum(counts)
    leaves = merkle_model.random_leaves(rng, n + 48)
    forest = gpu.build_forest(leaves[:n], counts, max_count=2048, reserve_leaves=48)
    assert forest.open_tree == 511 and forest.free_trees == 0
    at = n
    for step in (1, 7, 40):
        assert forest.extend(leaves[at: at + step]) == at + step - (n - 2000)
        at += step
        want = gpu.forest_roots(leaves[:at], counts[:-1] + [at - (n - 2000)])
        assert (forest.roots() == want).all() and forest.audit().clean, step
    assert at == 1 << 20 and forest.free_leaves == 0
    assert forest.shrink(48) == 2000
    assert (forest.roots() == gpu.forest_roots(leaves[:n], counts)).all() and forest.audit().clean
    forest.free()
