"""The model of tests/proofs_at_cases.py against trees built from the leaves, with hashlib alone: for every 1 <= c <= c2 <= 130
and every leaf i < c, the cells the rule takes out of the level lists of the tree of c2 leaves (and out of the old tree's right
edge, hashed once per epoch) are merkle_model.proof_path of the tree BUILT FROM the first c leaves, the old root is that tree's
root, and the hashes are the plan's count.  374 660 proofs.  No library, no GPU."""
import numpy as np
import pytest

import proofs_at_cases as pc
from merkle_model import cpu_levels, fold, proof_path, random_leaves, tree_height

TOP = 130


@pytest.fixture(scope="module")
def base():
    """The leaves and, for every n <= TOP, the level lists of the tree built from the first n of them: the tree as it was (n = c)
    and the tree as it is (n = c2)."""
    leaves = random_leaves(np.random.default_rng(500), TOP)
    return leaves, [None] + [cpu_levels(leaves[:n]) for n in range(1, TOP + 1)]


def test_every_leaf_of_every_pair_up_to_130_against_the_trees_built_from_the_leaves(base):
    _, built = base
    proofs = 0
    for c in range(1, TOP + 1):
        was, H = built[c], tree_height(c)
        every = np.arange(c)
        want = np.stack([proof_path(was, i, H) for i in every])                # [c, H, 8]: the old tree's own proofs
        for c2 in range(c, TOP + 1):
            stride = c2.bit_length()
            edge, old_root, n = pc.model_epoch(built[c2], c, stride)
            assert (old_root == was[-1][0]).all(), (c, c2)
            assert n == pc.hashes(c) <= H, (c, c2)
            assert [l for l in range(stride) if edge[l].any()] == pc.edge_levels(c), (c, c2)
            cells, heights = pc.model_proofs(built[c2], edge, c, every, stride)
            assert (heights == H).all() and (cells[:, :H] == want).all() and not cells[:, H:].any(), (c, c2)
            proofs += c
    assert proofs == 374660


def test_the_proofs_fold_to_the_old_root(base):
    leaves, built = base
    for c, c2 in ((1, 1), (1, 130), (2, 3), (3, 4), (5, 8), (7, 7), (64, 130), (65, 129), (96, 97), (127, 130), (129, 130), (130, 130)):
        edge, old_root, _ = pc.model_epoch(built[c2], c, 8)
        cells, heights = pc.model_proofs(built[c2], edge, c, np.arange(c), 8)
        for i in {0, c // 2, c - 1}:
            assert (fold(leaves[i], i, cells[i], heights[i]) == old_root).all(), (c, c2, i)
            assert c2 == c or (old_root != built[c2][-1][0]).any()              # which is not the root the tree has now


def test_the_degenerate_epochs_and_queries(base):
    _, built = base
    edge, root, n = pc.model_epoch(built[9], 0, 4)
    assert not edge.any() and not root.any() and n == 0
    cells, heights = pc.model_proofs(built[9], edge, 0, [0, 1], 4)
    assert not cells.any() and not heights.any()                               # an epoch not yet begun proves nothing
    edge, root, n = pc.model_epoch(built[9], 5, 4)
    cells, heights = pc.model_proofs(built[9], edge, 5, [4, 5, 6, 1 << 40], 4)
    assert heights.tolist() == [3, 0, 0, 0] and cells[0].any() and not cells[1:].any()
    for c in (2, 4, 8, 64, 128):                                               # a power of two: no hash, no edge cell
        edge, root, n = pc.model_epoch(built[130], c, 8)
        assert n == 0 and not edge.any() and (root == built[130][tree_height(c)][0]).all() and (root == built[c][-1][0]).all()
    assert pc.hashes(1) == 1 and pc.edge_levels(1) == [] and pc.hashes(6) == 2 and pc.edge_levels(6) == [2] and pc.hashes(0) == 0


def test_a_fork_is_caught_by_the_root():
    """Two trees that agree on fewer than c leaves: the proofs out of the second fold to ITS root as of c, not to the first's."""
    rng = np.random.default_rng(501)
    honest = random_leaves(rng, 40)
    for keep in (0, 1, 17, 23):
        forked = np.concatenate([honest[:keep], random_leaves(rng, 40 - keep)])
        levels = cpu_levels(forked)
        for c in (keep + 1, 24, 32, 40):
            edge, old_root, _ = pc.model_epoch(levels, c, 6)
            assert (old_root == cpu_levels(forked[:c])[-1][0]).all() and (old_root != cpu_levels(honest[:c])[-1][0]).any(), (keep, c)
