"""The model of tests/consistency_cases.py against trees built from the leaves, with hashlib alone: for every 1 <= c <= c2 <= 130
the proof gathered from the level lists of the tree of c2 leaves verifies under the root of the tree BUILT FROM the first c
leaves and the root of the whole tree, and under no other; c == 0 beside them.  No library, no GPU."""
import numpy as np
import pytest

import consistency_cases as cc
from merkle_model import cpu_levels, random_leaves

TOP = 130


@pytest.fixture(scope="module")
def base():
    leaves = random_leaves(np.random.default_rng(400), TOP)
    return leaves, cc.prefix_roots(leaves)


def test_the_prefix_roots_are_the_roots_of_the_trees_built_from_the_leaves(base):
    leaves, roots = base
    assert not roots[0].any()
    for c in (1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 127, 128, 129, 130):
        assert (roots[c] == cpu_levels(leaves[:c])[-1][0]).all(), c


def test_every_pair_up_to_130_against_the_trees_built_from_the_leaves(base):
    leaves, roots = base
    other = cc.prefix_roots(random_leaves(np.random.default_rng(399), 3))[3]
    for c2 in range(1, TOP + 1):
        levels = cpu_levels(leaves[:c2])
        stride = c2.bit_length()
        for c in range(1, c2 + 1):
            peaks, rights = cc.model_gather(levels, c, stride)
            reads = set()
            assert cc.model_check(c, c2, peaks, rights, roots[c], roots[c2], reads) == 1, (c, c2)
            assert reads == cc.read_set(c, c2), (c, c2)
            assert len(reads) <= 2 * stride and cc.hashes(c, c2) <= cc.tree_height(c) + cc.tree_height(c2)
            written = {("peaks", l) for l in range(stride) if peaks[l].any()} | {("rights", l) for l in range(stride) if rights[l].any()}
            assert written == reads, (c, c2)                                   # every other cell is zero
            if c2 % 9 == 0:                                                    # and under no other root, on either side
                assert cc.model_check(c, c2, peaks, rights, other, roots[c2]) == 0 and cc.model_check(c, c2, peaks, rights, roots[c], other) == 0
                if c != c2:
                    assert cc.model_check(c, c2, peaks, rights, roots[c2], roots[c]) == 0
        peaks, rights = cc.model_gather(levels, 0, stride)                     # c == 0: any tree extends one not yet begun
        assert not peaks.any() and not rights.any()
        assert cc.model_check(0, c2, peaks, rights, cc.ZERO, roots[c2]) == 1 and cc.model_check(0, c2, peaks, rights, roots[1], roots[c2]) == 0


def test_what_is_answered_without_reading_a_cell(base):
    leaves, roots = base
    peaks, rights = cc.model_gather(cpu_levels(leaves[:9]), 5, 8)
    reads = set()
    assert cc.model_check(5, 9, peaks, rights, roots[5], roots[9]) == 1
    assert cc.model_check(9, 5, peaks, rights, roots[5], roots[9], reads) == 0                         # c > c2
    assert cc.model_check(5, 9, peaks[:3], rights[:3], roots[5], roots[9], reads) == 0                 # nine leaves: four bits
    wide = np.zeros((64, 8), np.uint32)
    assert cc.model_check(5, (1 << 58) + 1, wide, wide, roots[5], roots[9], reads) == 0 and not reads


def test_a_fork_is_caught():
    """Two trees that agree on fewer than c leaves: the proof out of the second does not verify under the first's old root."""
    rng = np.random.default_rng(398)
    honest = random_leaves(rng, 40)
    for keep in (0, 1, 17, 23):
        forked = np.concatenate([honest[:keep], random_leaves(rng, 40 - keep)])
        levels = cpu_levels(forked)
        for c in (keep + 1, 24, 32, 40):
            peaks, rights = cc.model_gather(levels, c, 6)
            assert cc.model_check(c, 40, peaks, rights, cc.prefix_roots(honest[:c])[c], levels[-1][0]) == 0, (keep, c)
            assert cc.model_check(c, 40, peaks, rights, cc.prefix_roots(forked[:c])[c], levels[-1][0]) == 1, (keep, c)
