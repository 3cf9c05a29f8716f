"""Partial Merkle trees in BIP37 order on the GPU (vkmr_hip_forest_merkleblocks_async, vkmr_hip_tree_merkleblock_async through
HipDevice, MerkleForest, MerkleTree and PartialMerkleTrees): the device against the CPU twin byte for byte -- all eight outputs,
info and the canaries behind them --, the edges of the prefix sums, flag words and bytes that blocks share, the three status
bits, stream order behind an update, forests that grew and slid, the find -> sort -> merkleblocks chain, the single tree's twin,
one placement above 4 GiB, and device output -> extract -> the forest's roots.  tests/test_merkleblock_abi.py checks the twin
against the recursive rule."""
import numpy as np
import pytest

import consistency_cases as cc
import forest_life_cases as fl
import high_cases as hc
import merkleblock_cases as mb

pytestmark = pytest.mark.gpu


def device_merkleblocks(gpu, forest, trees, idx, hash_capacity=None, flag_capacity=None, slack=5, stream_first=None):
    """The raw call over buffers that start as canaries: (the eight outputs whole, with `slack` cells of canary behind the
    capacities, as merkleblock_cases.host_merkleblocks gives them; the capacities used).  stream_first(tmp): enqueue something
    in front on the same stream, with no host synchronisation between it and the call."""
    trees, idx = np.ascontiguousarray(trees, dtype=np.uint32), np.ascontiguousarray(idx, dtype=np.uint64)
    k = int(trees.shape[0])
    cap_h, cap_b, scratch = forest._merkleblocks_sizes(k)
    hash_capacity = cap_h if hash_capacity is None else hash_capacity
    flag_capacity = cap_b if flag_capacity is None else flag_capacity
    out = mb.fresh_outputs(k, hash_capacity, flag_capacity, slack)
    with gpu.scope() as tmp:
        bufs = [tmp.upload(a) for a in out]
        d_trees, d_idx, d_scr = tmp.upload(trees), tmp.upload(idx), tmp.alloc(scratch)
        if stream_first is not None:
            stream_first(tmp)
        entries = (d_idx,) if len(forest._columns) == 1 else (d_trees, d_idx)          # a tree's entries are its indices alone
        forest.merkleblocks_async(*entries, k, d_scr, *bufs[:5], bufs[5], hash_capacity, bufs[6], flag_capacity, bufs[7])
        got = [gpu.download(b, a.nbytes, dtype=a.dtype).reshape(a.shape) for a, b in zip(out, bufs)]
    return got, (hash_capacity, flag_capacity)


def host_image(gpu, forest):
    """(leaves [total, 8], offsets [ntrees + 1]) of a MerkleForest as the device holds them now."""
    return (gpu.download(forest.digests, 32 * forest.total).reshape(-1, 8), gpu.download(forest.offsets, 8 * (forest.ntrees + 1), dtype=np.uint64))


def same_as_twin(gpu, forest, leaves, offsets, trees, idx, what, **caps):
    """The device's outputs, whole buffers with their canaries, equal the twin's over the same capacities.  The device's status."""
    got, (hc_, fc_) = device_merkleblocks(gpu, forest, trees, idx, **caps)
    rc, want = mb.host_merkleblocks(leaves, offsets, trees, idx, hash_capacity=hc_, flag_capacity=fc_)
    names = ("block_trees", "block_counts", "bit_counts", "hash_starts", "byte_starts", "hashes", "flags", "info")
    for name, a, b in zip(names, got, want):
        assert a.shape == b.shape and (a == b).all(), (what, name, np.nonzero((a != b).reshape(a.shape[0], -1).any(axis=1))[0][:8], a[:6], b[:6])
    assert rc == int(got[7][0])
    return rc, got


@pytest.fixture(scope="module")
def square(gpu):
    """The 0..130 forest: empty trees in between; its stored forest, and the leaves and offsets the twin takes."""
    model = mb.square()
    forest = gpu.build_forest(model.leaves[model.first:], model.counts)
    leaves, offsets = host_image(gpu, forest)
    assert (leaves == model.leaves[model.first:]).all()
    yield model, forest, leaves, offsets
    forest.free()


def test_every_single_leaf_all_leaves_and_random_subsets_against_the_twin(gpu, square):
    model, forest, leaves, offsets = square
    rng = np.random.default_rng(801)
    sets = {"every leaf": mb.every_leaf(model.counts), "one in ten": mb.random_entries(model.counts, rng, 0.1), "half": mb.random_entries(model.counts, rng, 0.5),
            "few": mb.random_entries(model.counts, rng, 0.004)}
    for j, e in enumerate(mb.single_leaf_batches(model.counts)):           # every single leaf: leaf j of every tree that has one, one call
        sets[f"leaf {j} of every tree"] = e
    for what, (trees, idx) in sets.items():
        rc, got = same_as_twin(gpu, forest, leaves, offsets, trees, idx, what)
        assert rc == 0 and int(got[7][1]) == len(set(trees.tolist()))
    assert int(got[7][2]) > 0


@pytest.mark.parametrize("k", [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025])
def test_the_edges_of_the_prefix_sums(gpu, square, k):
    """A wavefront, a workgroup of the prefix sums and four of them, each with its neighbours: a prefix of a fixed random entry
    set.  (More blocks than a workgroup has lanes: test_blocks_that_share_flag_words_and_bytes.)"""
    model, forest, leaves, offsets = square
    trees, idx = mb.random_entries(model.counts, np.random.default_rng(802), 0.2)
    assert trees.shape[0] > 1025
    assert same_as_twin(gpu, forest, leaves, offsets, trees[:k], idx[:k], k)[0] == 0


def test_blocks_that_share_flag_words_and_bytes(gpu):
    rng = np.random.default_rng(803)
    counts = [int(c) for c in rng.integers(1, 4, size=300)]                # 2..4 flags a block, a byte each: four blocks share a 32-bit word
    leaves = mb.Forest(counts, seed=804, first=0).leaves
    forest = gpu.build_forest(leaves, counts)
    trees, idx = mb.every_leaf(counts)
    rc, got = same_as_twin(gpu, forest, *host_image(gpu, forest), trees, idx, "300 small trees")
    assert rc == 0 and got[7][:4].tolist() == [0, 300, sum(counts), 300] and (got[4][:301] == np.arange(301)).all()
    forest.free()
    counts = [1, 1, 2049, 1, 1, 1]                                         # a tall tree beside lone leaves: a long run of flag words between shared ones
    leaves = mb.Forest(counts, seed=805, first=0).leaves
    forest = gpu.build_forest(leaves, counts)
    for what, (trees, idx) in {"all": mb.every_leaf(counts), "some": mb.random_entries(counts, rng, 0.3),
                               "edges": mb.sorted_entries([(0, 0), (1, 0), (2, 0), (2, 2047), (2, 2048), (3, 0), (5, 0)])}.items():
        assert same_as_twin(gpu, forest, *host_image(gpu, forest), trees, idx, what)[0] == 0
    forest.free()


@pytest.mark.parametrize("k", [255, 256, 257, 1024])
def test_as_many_blocks_as_entries_at_the_edge_of_a_workgroup(gpu, k):
    """B == k with k a multiple of 256: the lane behind the last block, which writes byte_starts[B], is the first lane of a
    workgroup one past those the per-workgroup sums have; its neighbours 255 and 257 beside it.  Lone leaves: every entry its own
    tree, two flags and a byte each."""
    counts = [1] * 1024
    leaves = mb.Forest(counts, seed=820, first=0).leaves
    forest = gpu.build_forest(leaves, counts)
    rc, got = same_as_twin(gpu, forest, *host_image(gpu, forest), np.arange(k, dtype=np.uint32), np.zeros(k, np.uint64), k)
    assert rc == 0 and got[7][:4].tolist() == [0, k, k, k] and int(got[4][k]) == k and (got[6][:k] == 3).all()
    forest.free()


@pytest.mark.parametrize("what", ["tree outside", "index outside", "empty tree", "out of order", "repeated", "both"])
def test_status_bits_0_and_1_with_nothing_written(gpu, what):
    model = mb.Forest([5, 0, 9, 129], seed=414, first=0)
    forest = gpu.build_forest(model.leaves, model.counts)
    trees, idx, status = {"tree outside": ([0, 4], [1, 0], 1), "index outside": ([0, 2], [1, 9], 1), "empty tree": ([0, 1], [1, 0], 1),
                          "out of order": ([2, 0], [1, 1], 2), "repeated": ([2, 2, 3], [4, 4, 0], 2), "both": ([3, 3], [500, 2], 3)}[what]
    rc, got = same_as_twin(gpu, forest, model.leaves, model.offsets, trees, idx, what)
    assert rc == status
    got[7][0] = mb.CANARY64
    mb.assert_untouched(got)
    forest.free()


def test_bit_2_gives_the_totals_and_the_second_call_succeeds(gpu):
    model = mb.Forest([5, 0, 9, 129, 1, 64], seed=415, first=0)
    forest = gpu.build_forest(model.leaves, model.counts)
    trees, idx = mb.sorted_entries([(0, 1), (2, 3), (2, 8), (3, 77), (3, 128), (4, 0), (5, 63)])
    want = mb.model(model, trees, idx)
    n, m = int(want[7][2]), int(want[7][3])
    for caps in ((n - 1, m), (n, m - 1), (0, 0)):                          # the hash capacity one short, the byte capacity one short, each alone; none at all
        rc, got = same_as_twin(gpu, forest, model.leaves, model.offsets, trees, idx, caps, hash_capacity=caps[0], flag_capacity=caps[1])
        assert rc == 4 and got[7][:4].tolist() == [4, 5, n, m]
        mb.assert_untouched(got, upto=(5, 6))                              # no hash, no flag
        for i in range(5):
            assert (got[i][: want[i].shape[0]] == want[i]).all(), i       # the per-block arrays are valid
        rc, got = same_as_twin(gpu, forest, model.leaves, model.offsets, trees, idx, "again", hash_capacity=int(got[7][2]), flag_capacity=int(got[7][3]))
        assert rc == 0
        mb.assert_outputs(got, want, caps)                                 # exact buffers: canaries right behind the used hashes and bytes
    forest.free()


def test_stream_order_behind_an_update(gpu):
    model = mb.Forest([40, 3, 0, 130, 17], seed=416, first=0)
    forest = gpu.build_forest(model.leaves, model.counts)
    trees, idx = mb.sorted_entries([(0, 3), (0, 39), (1, 2), (3, 64), (3, 65), (4, 16)])
    new = mb.Forest([len(idx)], seed=417, first=0).leaves
    after = model.leaves.copy()
    after[(model.offsets[trees.astype(np.int64)] + idx).astype(np.int64)] = new
    pending = {}

    def update_first(tmp):
        d_t, d_i, d_l, d_s = tmp.upload(trees), tmp.upload(idx), tmp.upload(new), tmp.upload(np.zeros(1, np.uint32))
        forest.update_async(d_t, d_i, d_l, len(idx), d_s)                  # enqueued; nothing waits for it
        pending["status"] = d_s

    ask_t, ask_i = mb.sorted_entries([(0, 3), (0, 4), (1, 0), (3, 65), (3, 129), (4, 0)])
    got, (hc_, fc_) = device_merkleblocks(gpu, forest, ask_t, ask_i, stream_first=update_first)
    rc, want = mb.host_merkleblocks(after, model.offsets, ask_t, ask_i, hash_capacity=hc_, flag_capacity=fc_)
    assert rc == 0 and all((a == b).all() for a, b in zip(got, want))
    rc, stale = mb.host_merkleblocks(model.leaves, model.offsets, ask_t, ask_i, hash_capacity=hc_, flag_capacity=fc_)
    assert not (stale[5] == got[5]).all()                                  # and not the forest as it was
    forest.free()


def test_forests_that_grew_and_slid(gpu):
    rng = np.random.default_rng(806)
    counts = [9, 0, 33, 5]
    first = mb.Forest(counts, seed=807, first=0).leaves
    forest = gpu.build_forest(first, counts, max_count=200, reserve_trees=3, reserve_leaves=300)
    forest.extend(mb.Forest([60], seed=808, first=0).leaves)               # the open tree: 5 -> 65 leaves
    forest.append(mb.Forest([1, 130], seed=809, first=0).leaves, [1, 130])
    forest.drop_front(1)
    leaves, offsets = host_image(gpu, forest)
    now = [int(b - a) for a, b in zip(offsets, offsets[1:])]
    assert now[:6] == [0, 0, 33, 65, 1, 130] and forest.levels == 8
    trees, idx = mb.random_entries(now, rng, 0.3)
    rc, got = same_as_twin(gpu, forest, leaves, offsets, trees, idx, "after extend, append, drop_front")
    assert rc == 0
    roots = forest.roots()
    for t, c, hashes, flags in blocks(got):
        code, root, found, _ = mb.host_extract(c, hashes, flags)
        assert code == 0 and (root == roots[t]).all() and found.tolist() == idx[trees == t].tolist()
    rc, got = same_as_twin(gpu, forest, leaves, offsets, [0, 2], [0, 0], "an entry in a dropped tree")
    assert rc == 1
    with pytest.raises(IndexError):
        forest.merkleblocks([0], [0])
    forest.free()


def blocks(out):
    for b in range(int(out[7][1])):
        yield int(out[0][b]), int(out[1][b]), out[5][int(out[3][b]): int(out[3][b + 1])], out[6][int(out[4][b]): int(out[4][b + 1])].tobytes()


def test_the_chain_from_digests_and_the_single_trees_twin(gpu, square):
    import vk_merkle_roots_amd as vk
    model, forest, leaves, offsets = square
    rng = np.random.default_rng(810)
    trees, idx = mb.random_entries(model.counts, rng, 0.05)
    cells = (offsets[trees.astype(np.int64)] + idx).astype(np.int64)
    asked = np.concatenate([leaves[cells], leaves[cells[:7]], mb.Forest([5], seed=811, first=0).leaves])   # repeated ones, unknown ones
    shuffle = rng.permutation(asked.shape[0])
    result, order = forest.merkleblocks_of(asked[shuffle])
    direct = forest.merkleblocks(trees[::-1], idx[::-1])                   # sorted on the host
    assert isinstance(result, vk.PartialMerkleTrees) and len(result) == len(direct) == len(set(trees.tolist()))
    for name in ("trees", "counts", "bit_counts", "hash_starts", "byte_starts", "hashes", "flags"):
        assert (getattr(result, name) == getattr(direct, name)).all(), name
    assert order.shape[0] == trees.shape[0] and (asked[shuffle][order] == leaves[cells]).all()
    with pytest.raises(ValueError):
        forest.merkleblocks_of(mb.Forest([3], seed=812, first=0).leaves)   # none is a leaf
    # the tree twin against the forest of one tree
    for c in (2, 3, 7, 64, 65, 130):
        tree_leaves = mb.Forest([c], seed=813 + c, first=0).leaves
        d_leaves = gpu.upload(tree_leaves)
        tree, alone = gpu.build_tree(d_leaves, c), gpu.build_forest(tree_leaves, [c])
        pick = sorted(set(rng.integers(0, c, size=max(1, c // 3)).tolist()))
        one, many = tree.merkleblock(pick), alone.merkleblocks([0] * len(pick), pick)
        assert len(many) == 1 and one.count == many[0].count == c and (one.hashes == many[0].hashes).all() and (one.flags == many[0].flags).all()
        got, (hc_, fc_) = device_merkleblocks(gpu, tree, np.zeros(len(pick), np.uint32), pick)   # the raw call: every output and the canaries
        rc, want = mb.host_merkleblocks(tree_leaves, [0, c], [0] * len(pick), pick, hash_capacity=hc_, flag_capacity=fc_)
        assert rc == 0 and all((a == b).all() for a, b in zip(got, want)), c
        found, order = tree.merkleblock_of(tree_leaves[pick][::-1])
        assert (found.hashes == one.hashes).all() and found.extract()[1].tolist() == pick
        root, matched, got_leaves = one.extract()
        assert (root == tree.root()).all() and matched.tolist() == pick and (got_leaves == tree_leaves[pick]).all()
        tree.free()
        alone.free()
        d_leaves.free()


def test_a_forest_across_the_4_gib_line(gpu):
    """Level 0 placed so that its cells straddle cell 2^27 (byte offset 2^32): the leaves the emit copies and the offsets it adds
    are up there; the buffers in front are allocated and never touched.  Skipped where the device has no such memory
    (high_cases.alloc)."""
    model = cc.Forest(cc.GPU_COUNTS, seed=421, first=3)
    shape = fl.ModelForest(model.ntrees, sum(model.counts), 2048, [model.tree(t) for t in range(model.ntrees)])
    view = hc.Shifted(shape, 0)
    assert hc.straddles(view) and view.D >= 2**27 - shape.total
    forest = hc.build(gpu, view)
    try:
        rng = np.random.default_rng(814)
        for what, (trees, idx) in {"every leaf": mb.every_leaf(model.counts), "one in seven": mb.random_entries(model.counts, rng, 0.14)}.items():
            got, (hc_, fc_) = device_merkleblocks(gpu, forest, trees, idx)
            rc, want = mb.host_merkleblocks(model.leaves, model.offsets, trees, idx, hash_capacity=hc_, flag_capacity=fc_)
            assert rc == 0 and all((a == b).all() for a, b in zip(got, want)), what
        assert hc.canaries_intact(gpu, forest.canaries)
    finally:
        forest.free()


def test_device_output_extracts_to_the_forests_roots(gpu, square):
    model, forest, _, _ = square
    trees, idx = mb.random_entries(model.counts, np.random.default_rng(815), 0.25)
    result = forest.merkleblocks(trees, idx)
    roots = forest.roots()
    assert (roots == model.roots()).all() and len(result) == len(set(trees.tolist()))
    for b in range(len(result)):
        t = int(result.trees[b])
        root, found, leaves = result[b].extract()
        assert (root == roots[t]).all() and found.tolist() == idx[trees == t].tolist() and (leaves == model.tree(t)[found.astype(np.int64)]).all(), t
        assert result[b].count == model.counts[t] and int(result.bit_counts[b]) == len(mb.walk(model.counts[t], found.tolist())[0])
