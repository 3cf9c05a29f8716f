"""Leaf updates of a stored forest on the GPU (vkmr_hip_forest_update_async through HipDevice and MerkleForest): after an update
the leaves, EVERY cell of the forest buffer and the roots equal a fresh build over the edited leaves, the cells nobody writes
included; refused batches change nothing; the update is ordered on its stream in front of a proof gather and a verify."""
import numpy as np
import pytest

import forest_cases as fc
import forest_proof_cases as fp
import forest_update_cases as fu
import merkle_model

pytestmark = pytest.mark.gpu


def new_leaves(rng, k):
    return merkle_model.random_leaves(rng, k)


def updated_equals_fresh(gpu, leaves, counts, max_count, sets, rng, first=0):
    """Every entry set applied in turn to one stored forest: after each, all three buffers equal a fresh build's."""
    host = np.array(leaves, dtype=np.uint32, copy=True)
    forest = fu.RawForest(gpu, host, counts, max_count, first=first)
    for name, (trees, indices) in sets.items():
        new = new_leaves(rng, trees.shape[0])
        assert forest.update(trees, indices, new) == 0, name
        host[fu.cells_of(counts, trees, indices, first)] = new
        fresh = fu.RawForest(gpu, host, counts, max_count, first=first)
        got, want = forest.state(), fresh.state()
        fresh.free()
        assert (got[0] == host.reshape(-1)).all(), name
        for what, a, b in zip(("leaves", "forest", "roots"), got, want):
            assert a.shape == b.shape and (a == b).all(), (name, what, np.nonzero(a != b)[0][:8] // 8)
    forest.free()


@pytest.mark.parametrize("loose", [False, True], ids=["tight", "loose"])
@pytest.mark.parametrize("name", sorted(n for n in fc.CASES if n != "all_empty"))
def test_updated_forest_equals_a_fresh_build_in_every_cell(gpu, name, loose):
    counts = fc.CASES[name]
    rng = np.random.default_rng(len(name) * 31 + loose)
    leaves = fc.random_leaves(sum(counts), seed=len(name) * 7919 + sum(counts))
    updated_equals_fresh(gpu, leaves, counts, 2**63 if loose else max(counts), fu.update_sets(counts, rng), rng)


def test_a_first_offset_above_zero_and_slack_behind_the_last_tree(gpu):
    counts = [4, 0, 0, 7, 0, 1, 130, 33]
    rng = np.random.default_rng(5)
    leaves = fc.random_leaves(5 + sum(counts) + 7, seed=55)        # total is the leaves buffer's size
    updated_equals_fresh(gpu, leaves, counts, max(counts), fu.update_sets(counts, rng), rng, first=5)


def test_a_lone_leaf_and_the_last_leaf_of_two_to_the_k_plus_one(gpu):
    counts = fc.CASES["power_of_two_edges"]
    off = fc.offsets_of(counts).astype(np.int64)
    host = fc.random_leaves(sum(counts), seed=91)
    forest = gpu.build_forest(host, counts)
    lone = [t for t, c in enumerate(counts) if c == 1]
    odd = [t for t, c in enumerate(counts) if c > 2 and (c - 1) & (c - 2) == 0]      # 2^k + 1 for k >= 1: duplicate-last at every level
    assert len(lone) >= 14 and sorted({counts[t] for t in odd}) == [(1 << k) + 1 for k in range(1, 14)]
    trees = np.array(lone + odd, dtype=np.uint32)
    indices = np.array([0] * len(lone) + [counts[t] - 1 for t in odd], dtype=np.uint64)
    rng = np.random.default_rng(92)
    new = new_leaves(rng, trees.shape[0])
    before = forest.roots()
    forest.update(trees, indices, new)
    host[fu.cells_of(counts, trees, indices)] = new
    roots = forest.roots()
    for q, t in enumerate(trees.tolist()):
        levels = merkle_model.cpu_levels(host[off[t]: off[t + 1]])
        assert (roots[t] == levels[-1][0]).all(), (t, counts[t])
        if counts[t] == 1:
            assert (roots[t] == merkle_model.node(new[q], new[q])).all()            # root = H(leaf || leaf)
    untouched = np.setdiff1d(np.arange(len(counts)), trees)
    assert (roots[untouched] == before[untouched]).all()
    forest.free()


def test_eight_successive_rounds_with_repeated_pairs(gpu):
    counts = fc.CASES["sizes_1_to_130"] + fc.CASES["power_of_two_edges"]
    host = fc.random_leaves(sum(counts), seed=101)
    forest = fu.RawForest(gpu, host, counts, max(counts))
    rng = np.random.default_rng(102)
    for rnd in range(8):
        k = int(rng.integers(1, 3000))
        trees, indices = fp.random_queries(rng, counts, k)
        again = rng.integers(0, k, size=k // 4 + 1)                 # a quarter of the pairs once more, behind the others: the last value counts
        trees, indices = np.concatenate([trees, trees[again]]), np.concatenate([indices, indices[again]])
        new = new_leaves(rng, trees.shape[0])
        forest.handle.update(trees, indices, new)                   # MerkleForest.update: sorts, keeps the last of a repeated pair
        host[fu.cells_of(counts, trees, indices)] = new              # numpy keeps the last of repeated cells too
        fresh = fu.RawForest(gpu, host, counts, max(counts))
        got, want = forest.state(), fresh.state()
        fresh.free()
        assert (got[2] == want[2]).all(), rnd                       # every root
        assert (got[1] == want[1]).all() and (got[0] == want[0]).all(), rnd   # the whole forest buffer, and the leaves
    forest.free()


REFUSALS = [([8], [0], 1), ([0], [4], 1), ([1], [0], 1), ([3, 3], [2, 2], 2), ([3, 0], [1, 2], 2), ([3, 3], [5, 4], 2), ([3, 0], [6, 9], 3),
            ([0, 3], [3, 0], 0), ([0, 3, 7], [0, 6, 0], 0)]


@pytest.mark.parametrize("trees,indices,want", REFUSALS)
def test_a_refused_batch_changes_nothing(gpu, trees, indices, want):
    counts = fc.CASES["empty_adjacent"]
    assert counts == [4, 0, 0, 7, 0, 0, 0, 1]
    host = fc.random_leaves(sum(counts), seed=111)
    forest = fu.RawForest(gpu, host, counts, max(counts))
    before = forest.state()
    new = new_leaves(np.random.default_rng(112), len(trees))
    assert forest.update(trees, indices, new) == want               # the status word held 0xDEADBEEF
    if want:
        assert fu.same_state(forest.state(), before)
    else:
        host[fu.cells_of(counts, trees, indices)] = new
        fresh = fu.RawForest(gpu, host, counts, max(counts))
        assert fu.same_state(forest.state(), fresh.state())
        fresh.free()
    forest.free()


def test_an_index_of_two_to_the_64_minus_one_is_refused(gpu):
    counts = fc.CASES["sizes_1_to_130"]
    forest = fu.RawForest(gpu, fc.random_leaves(sum(counts), seed=113), counts, max(counts))
    before = forest.state()
    assert forest.update([129], [2**64 - 1], new_leaves(np.random.default_rng(114), 1)) == 1
    assert fu.same_state(forest.state(), before)
    forest.free()


def test_update_proofs_and_verify_in_stream_order(gpu):
    import vk_merkle_roots_amd as vk
    rng = np.random.default_rng(121)
    counts = [int(c) for c in rng.integers(1, 131, size=76)]        # about 5 000 leaves in trees of 1..130
    total, ntrees = sum(counts), len(counts)
    host = fc.random_leaves(total, seed=122)
    forest = gpu.build_forest(host, counts)
    H = forest.levels
    touched = rng.choice(ntrees, size=ntrees // 2, replace=False)   # half of the trees stay as they are
    t_all, i_all = fp.random_queries(rng, [c if t in touched else 0 for t, c in enumerate(counts)], 300)
    trees, indices = fu.sorted_entries(zip(t_all.tolist(), i_all.tolist()))
    k = trees.shape[0]
    new = new_leaves(rng, k)
    old = np.ascontiguousarray(host[fu.cells_of(counts, trees, indices)])
    others = np.setdiff1d(np.arange(ntrees), touched)
    q_trees, q_idx = fp.random_queries(rng, [c if t in others else 0 for t, c in enumerate(counts)], 200)
    q_leaves = np.ascontiguousarray(host[fu.cells_of(counts, q_trees, q_idx)])
    old_sib, old_h = forest.proofs(trees, indices)
    d_trees, d_idx, d_new, d_old = gpu.upload(trees), gpu.upload(indices), gpu.upload(new), gpu.upload(old)
    d_qt, d_qi, d_ql = gpu.upload(q_trees), gpu.upload(q_idx), gpu.upload(q_leaves)
    d_old_sib, d_old_h = gpu.upload(old_sib), gpu.upload(old_h)
    d_status = gpu.upload(np.full(1, 0xDEADBEEF, dtype=np.uint32))
    d_sib, d_h, d_qsib, d_qh = gpu.alloc(32 * k * H), gpu.alloc(4 * k), gpu.alloc(32 * 200 * H), gpu.alloc(4 * 200)
    d_ok_new, d_ok_old, d_ok_q = gpu.alloc(4 * k), gpu.alloc(4 * k), gpu.alloc(4 * 200)
    s = gpu.new_stream()
    forest.update_async(d_trees, d_idx, d_new, k, d_status, stream=s)
    forest.proofs_async(d_trees, d_idx, k, d_sib, d_h, stream=s)
    forest.proofs_async(d_qt, d_qi, 200, d_qsib, d_qh, stream=s)
    gpu.verify_forest_proofs_async(d_new, d_trees, d_idx, d_sib, d_h, k, H, forest.roots_buf, ntrees, d_ok_new, stream=s)
    gpu.verify_forest_proofs_async(d_old, d_trees, d_idx, d_old_sib, d_old_h, k, H, forest.roots_buf, ntrees, d_ok_old, stream=s)
    gpu.verify_forest_proofs_async(d_ql, d_qt, d_qi, d_qsib, d_qh, 200, H, forest.roots_buf, ntrees, d_ok_q, stream=s)
    gpu.sync(s)
    assert int(gpu.download(d_status, 4)[0]) == 0
    assert (gpu.download(d_ok_new, 4 * k) == 1).all()               # every new proof verifies against the new roots in place
    assert (gpu.download(d_ok_old, 4 * k) == 0).all()               # the old proofs of updated leaves all fail
    assert (gpu.download(d_ok_q, 4 * 200) == 1).all()               # untouched trees still prove their leaves
    host[fu.cells_of(counts, trees, indices)] = new
    assert (forest.roots() == gpu.forest_roots(host, counts)).all()
    gpu.lib.vkmr_hip_stream_destroy(gpu.index, s)
    for b in (d_trees, d_idx, d_new, d_old, d_qt, d_qi, d_ql, d_old_sib, d_old_h, d_status, d_sib, d_h, d_qsib, d_qh, d_ok_new, d_ok_old, d_ok_q):
        b.free()
    forest.free()
    assert vk.MerkleForest.update_async.__doc__


def lines_batch(vk, strings):
    return vk.pack_lines(b"".join(s + b"\n" for s in strings))


@pytest.mark.parametrize("counts", [[1], [6, 0, 3], None], ids=["one", "six_none_three", "forty_trees"])
def test_update_packed_equals_a_forest_over_the_edited_strings(gpu, counts):
    import vk_merkle_roots_amd as vk
    rng = np.random.default_rng(131)
    if counts is None:
        counts = [int(c) for c in rng.integers(0, 51, size=40)]     # about 1 000 strings in 40 trees
    total = sum(counts)
    strings = [b"s%d-%d" % (j, int(rng.integers(0, 10**9))) for j in range(total)]
    forest = vk.merkle_forest_packed(gpu, lines_batch(vk, strings), counts)
    k = max(1, total // 3)
    trees, indices = fp.random_queries(rng, counts, k)
    trees, indices = np.concatenate([trees, trees[:2]]), np.concatenate([indices, indices[:2]])   # repeated pairs: the last string counts
    fresh_strings = [b"new%d-%d" % (q, int(rng.integers(0, 10**9))) for q in range(trees.shape[0])]
    forest.update_packed(trees, indices, lines_batch(vk, fresh_strings))
    for q, cell in enumerate(fu.cells_of(counts, trees, indices).tolist()):
        strings[cell] = fresh_strings[q]
    want = vk.merkle_forest_packed(gpu, lines_batch(vk, strings), counts)
    assert (forest.roots() == want.roots()).all()
    assert (gpu.download(forest.digests, 32 * total) == gpu.download(want.digests, 32 * total)).all()
    sib, heights = forest.proofs(trees, indices)
    want_sib, want_heights = want.proofs(trees, indices)
    assert (sib == want_sib).all() and (heights == want_heights).all()
    forest.free()
    want.free()


def test_two_to_the_20_leaves_in_trees_of_1_to_4095(gpu):
    rng = np.random.default_rng(141)
    counts = []
    while sum(counts) < 1 << 20:
        counts.append(min(int(rng.integers(1, 4096)), (1 << 20) - sum(counts)))
    host = fc.random_leaves(1 << 20, seed=142)
    forest = fu.RawForest(gpu, host, counts, 4095)
    assert forest.H == 12
    t_all, i_all = fp.random_queries(rng, counts, 1 << 14)
    trees, indices = fu.sorted_entries(zip(t_all.tolist(), i_all.tolist()))
    new = new_leaves(rng, trees.shape[0])
    assert forest.update(trees, indices, new) == 0
    host[fu.cells_of(counts, trees, indices)] = new
    fresh = fu.RawForest(gpu, host, counts, 4095)
    assert fu.same_state(forest.state(), fresh.state())
    fresh.free()
    forest.free()
