"""One stored tree and a stored forest that holds the same tree, side by side on the GPU: the kernels of the two share their
bodies (csrc/entries.hpp), so over the same leaves they must give the same proofs, the same tree after the same update, the
same untouched tree after a refused update, and the same multiproof.  The forest is that one tree alone, and that tree
between an empty tree and a 3-leaf tree, so that an entry's neighbour is in another tree or in none.  The counts reach the
ragged right edge, a lone node, the ballot-word edge (64 / 65) and, with 16385 consecutive entries of 16400 leaves, the
16384-entry block of the ranking's prefix sum.  tests/test_gpu_forest_multiproof.py already compares each tree's share of a
forest multiproof with the single tree's; this module does not repeat it."""
import functools

import numpy as np
import pytest

from merkle_model import At, cpu_levels, random_leaves, tree_height

pytestmark = pytest.mark.gpu

COUNTS = [1, 2, 3, 5, 64, 65, 127, 129, 16400]
BIG = 16400
BIG_RUN = np.arange(7, 7 + 16385, dtype=np.uint64)        # crosses one 16384-entry block and 256 ballot words
SHAPES = {"alone": (0, 0), "between an empty tree and a 3-leaf tree": (1, 3)}     # name: (the tree's number, leaves behind it)


@functools.lru_cache(maxsize=None)
def leaves_of(count):
    leaves = random_leaves(np.random.default_rng(7000 + count), count + 3)
    leaves.setflags(write=False)
    return leaves


@functools.lru_cache(maxsize=None)
def levels_of(count):
    return cpu_levels(leaves_of(count)[:count])


def entries(count):
    """Every leaf of a small tree; of the big one the first two, the two around the 16384th and the last."""
    return np.arange(count, dtype=np.uint64) if count <= 129 else np.array([0, 1, 16383, 16384, 16399], dtype=np.uint64)


def batches(count):
    """Sorted update batches: one leaf; the first and the last; every other leaf; of the big tree also 16385 in a row."""
    out = {"one leaf": [count // 2], "first and last": sorted({0, count - 1}), "every other leaf": list(range(0, count, 2))}
    if count == BIG:
        out["16385 consecutive leaves"] = BIG_RUN
    return {name: np.asarray(idx, dtype=np.uint64) for name, idx in out.items()}


class Pair:
    """A MerkleTree over `leaves` and a MerkleForest in which tree `t` holds the same leaves."""

    def __init__(self, gpu, leaves, shape):
        self.gpu, self.count = gpu, leaves.shape[0]
        self.t, behind = SHAPES[shape]
        self.counts = [0] * self.t + [self.count] + ([behind] if behind else [])
        self.d_in = gpu.upload(np.ascontiguousarray(leaves))
        self.tree = gpu.build_tree(self.d_in, self.count)
        self.forest = gpu.build_forest(np.concatenate([leaves, leaves_of(self.count)[self.count: self.count + behind]]), self.counts)

    def trees(self, idx):
        return np.full(len(idx), self.t, dtype=np.uint32)

    def assert_same_proofs(self, idx, what):
        """The forest's height is the tree's and the first `height` cells of each proof are the tree's, byte for byte."""
        h = self.tree.height
        mine = self.tree.proofs(idx)
        sib, heights = self.forest.proofs(self.trees(idx), idx)
        assert (heights == h).all(), what
        assert sib[:, :h].tobytes() == mine.tobytes(), what
        return mine, sib, heights

    def assert_root(self, want, what):
        assert (self.tree.root() == want).all(), what
        assert (self.forest.roots()[self.t] == want).all(), what

    def free(self):
        self.tree.free()
        self.forest.free()
        self.d_in.free()


@pytest.mark.parametrize("count", COUNTS)
def test_proofs_are_the_same_and_verify_against_the_model_s_root(gpu, count):
    leaves, want = leaves_of(count)[:count], levels_of(count)[-1][0]
    idx = entries(count)
    for shape in SHAPES:
        pair = Pair(gpu, leaves, shape)
        assert pair.tree.height == tree_height(count) == len(levels_of(count)) - 1
        mine, sib, heights = pair.assert_same_proofs(idx, (count, shape))
        pair.assert_root(want, (count, shape))
        roots = pair.forest.roots()
        roots[pair.t] = want
        assert gpu.verify_proofs(leaves[idx.astype(np.int64)], idx, mine, want).all(), (count, shape)
        assert gpu.verify_forest_proofs(leaves[idx.astype(np.int64)], pair.trees(idx), idx, sib, heights, roots).all(), (count, shape)
        pair.free()


def test_a_lone_leaf_has_height_0_in_the_tree_api_and_height_1_in_the_forest(gpu):
    """What each API documents: a tree built with height 0 is its leaf and has no sibling; the forest hashes it with itself."""
    leaves = leaves_of(1)[:1]
    d_in = gpu.upload(np.ascontiguousarray(leaves))
    tree = gpu.build_tree(d_in, 1, height=0)
    assert (tree.root() == leaves[0]).all() and tree.proofs([0]).shape == (1, 0, 8)
    forest = gpu.build_forest(leaves, [1])
    sib, heights = forest.proofs([0], [0])
    assert forest.levels == 1 and int(heights[0]) == 1 and (sib[0, 0] == leaves[0]).all()
    assert (forest.roots()[0] == levels_of(1)[1][0]).all()
    tree.free()
    forest.free()
    d_in.free()


@pytest.mark.parametrize("count", COUNTS)
def test_the_same_update_gives_the_same_tree(gpu, count):
    rng = np.random.default_rng(8000 + count)
    steps, leaves = [], leaves_of(count)[:count].copy()
    for name, idx in batches(count).items():               # the model, once for both shapes
        new = random_leaves(rng, len(idx))
        leaves[idx.astype(np.int64)] = new
        steps.append((name, idx, new, cpu_levels(leaves)[-1][0]))
    for shape in SHAPES:
        pair = Pair(gpu, leaves_of(count)[:count], shape)
        for name, idx, new, want in steps:
            pair.tree.update(idx, new)
            pair.forest.update(pair.trees(idx), idx, new)
            pair.assert_root(want, (count, shape, name))
            pair.assert_same_proofs(idx if count <= 129 else entries(count), (count, shape, name))
        pair.free()


@pytest.mark.parametrize("count", COUNTS)
def test_a_refused_batch_leaves_both_bit_identical(gpu, count):
    leaves = leaves_of(count)[:count]
    idx = np.array([count // 2, count // 2], dtype=np.uint64)              # a repeated index: status bit 1 in both
    new = random_leaves(np.random.default_rng(9000 + count), 2)
    for shape in SHAPES:
        pair = Pair(gpu, leaves, shape)
        root, roots = pair.tree.root(), pair.forest.roots()
        mine, sib, _ = pair.assert_same_proofs(entries(count), (count, shape))
        cells = gpu.download(pair.forest.digests, 32 * pair.forest.total)
        d_idx, d_trees, d_new = gpu.upload(idx), gpu.upload(pair.trees(idx)), gpu.upload(new)
        d_status = gpu.upload(np.array([0xDEADBEEF, 0xDEADBEEF], dtype=np.uint32))
        pair.tree.update_async(d_idx, d_new, 2, d_status)
        pair.forest.update_async(d_trees, d_idx, d_new, 2, At(d_status, 4))
        assert [int(x) for x in gpu.download(d_status, 8)] == [2, 2], (count, shape)
        assert (pair.tree.root() == root).all() and (pair.forest.roots() == roots).all(), (count, shape)
        assert (gpu.download(pair.d_in, 32 * count).reshape(count, 8) == leaves).all(), (count, shape)
        assert (gpu.download(pair.forest.digests, 32 * pair.forest.total) == cells).all(), (count, shape)
        mine2, sib2, _ = pair.assert_same_proofs(entries(count), (count, shape))
        assert mine2.tobytes() == mine.tobytes() and sib2.tobytes() == sib.tobytes(), (count, shape)
        for b in (d_idx, d_trees, d_new, d_status):
            b.free()
        pair.free()


def test_the_same_multiproof_of_16385_entries(gpu):
    leaves, want = leaves_of(BIG)[:BIG], levels_of(BIG)[-1][0]
    proved = leaves[BIG_RUN.astype(np.int64)]
    for shape in SHAPES:
        pair = Pair(gpu, leaves, shape)
        one = pair.tree.multiproof(BIG_RUN)
        many = pair.forest.multiproof(pair.trees(BIG_RUN), BIG_RUN)
        assert (many.heights == one.height).all() and many.stride == one.height, shape
        assert [int(x) for x in many.level_counts] == [int(x) for x in one.level_counts], shape
        assert many.nodes.tobytes() == one.nodes.tobytes(), shape
        assert gpu.verify_multiproof(proved, BIG_RUN, one.nodes, want, one.height), shape
        roots = pair.forest.roots()
        assert (roots[pair.t] == want).all(), shape
        assert gpu.verify_forest_multiproof(proved, many.trees, many.indices, many.heights, many.nodes, roots), shape
        pair.free()
