"""Above 4 GiB: what no other GPU test hands a kernel -- a cell index of 2^27 or more, a byte offset of 2^32 or more, a
packed-word index of 2^30 or more (tests/high_cases.py; the life of a stored forest up there is in
tests/test_gpu_forest_life.py).  Here: the two newest readers of a stored forest, consistency proofs and proofs as of an
earlier count, out of a forest whose level 0 or level 1 straddles cell 2^27; and the map kernel, in every shipped instantiation
that can get there, over strings that lie across word 2^30, 2^31 and 3 * 2^30 of the data buffer and at the end of a buffer
of 2^32 - 5 words.  The buffers are large and almost wholly untouched; what is uploaded, hashed and read back is small.

map_kernel<256, 2048, 64, 2, true, 0> (DIRECT256) has no case: vkmr_map::plan gives it batches of fewer than 2^20 strings
averaging fewer than 128 words, that is data buffers below 127 * 2^20 < 2^27 words, so no batch of its reaches word 2^30."""
import functools

import numpy as np
import pytest

import consistency_cases as cc
import forest_life_cases as fl
import high_cases as hc
import proofs_at_cases as pc
from test_gpu_consistency import device_gather
from test_gpu_consistency import same as same_consistency
from test_gpu_proofs_at import device_proofs_at, leaves_of
from test_gpu_proofs_at import same as same_proofs_at

pytestmark = pytest.mark.gpu


# ---- the two newest readers --------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def readers_case():
    """The forest of every walk length with the existing queries, epochs and what the CPU twins give for it where it lies
    (3 cells in front: shift 0, for this purpose), computed once for both placements."""
    model = cc.Forest(cc.GPU_COUNTS, seed=421, first=3)
    trees, old = cc.gpu_queries()
    gathered = cc.host_gather(model.leaves, model.offsets, trees, old, stride=12)
    epoch_trees, epoch_counts, epochs, indices = pc.gpu_epochs_and_queries()
    proved = pc.host_proofs_at(model.leaves, model.offsets, epoch_trees, epoch_counts, epochs, indices, stride=12)
    assert gathered[0] == 0 and proved[0] == 0
    shape = fl.ModelForest(model.ntrees, sum(model.counts), 2048, [model.tree(t) for t in range(model.ntrees)])
    return model, shape, (trees, old, gathered), (epoch_trees, epoch_counts, epochs, indices, proved)


@pytest.mark.parametrize("level", [0, 1])
def test_consistency_and_proofs_at_out_of_a_forest_across_the_line(gpu, level):
    import vk_merkle_roots_amd as vk
    model, shape, (trees, old, gathered), (epoch_trees, epoch_counts, epochs, indices, proved) = readers_case()
    view = hc.Shifted(shape, level)
    assert hc.straddles(view) and view.D >= 2**27 - shape.total
    forest = hc.build(gpu, view)
    try:
        assert hc.canaries_intact(gpu, forest.canaries)                  # the build's stores first: a narrowed one lands at cell 0
        assert (forest.roots() == model.roots()).all() and forest.dropped_leaves == view.D
        # consistency: peaks, neighbours and status, and the batch verified
        got = device_gather(gpu, forest, trees, old, 12)
        assert got[0] == 0
        same_consistency(got[1:], gathered[1:], ("consistency", level))
        proof = forest.consistency(old, trees=trees)
        assert proof.same_as(vk.ConsistencyProof(trees, old, *gathered[1:]))
        old_roots, new_roots = model.query_roots(trees, old)
        assert (proof.verify(gpu, old_roots, new_roots) == 1).all()
        # proofs_at: status, edges, old roots, siblings and heights, and the batch verified under the old roots
        got = device_proofs_at(gpu, forest, epoch_trees, epoch_counts, epochs, indices, 12)
        assert got[0] == 0
        same_proofs_at(got[1:], proved[1:], ("proofs_at", level))
        leaves, good = leaves_of(model, epoch_trees, epoch_counts, epochs, indices)
        ok = gpu.verify_forest_proofs(leaves, epochs, indices, got[3], got[4], got[2])
        assert ok[good].all() and not ok[~good].any()
        assert hc.canaries_intact(gpu, forest.canaries)
    finally:
        forest.free()


# ---- the map kernel ----------------------------------------------------------------------------------------------------------

SHORT = 2**31 + 2**14           # words: 8 GiB and a little
LONG = 2**32 - 5                # words: the last index a uint32 `start` can name is beyond the buffer
POSITIONS = {"2^30": 2**30, "2^31": 2**31, "3*2^30": 3 * 2**30, "end": None}


def mapped(gpu, oracle, data_words, mode, count, positions, together):
    """The clusters at `positions` uploaded into one untouched buffer of data_words words; one call over all of them
    (`together`) or one call each."""
    per_lane = mode != "STAGED"
    clusters = [hc.Cluster(oracle, 900 + n, data_words, POSITIONS[p], long_ones=per_lane) for n, p in enumerate(positions)]
    d_data = hc.alloc(gpu, 4 * data_words, "the packed strings")
    try:
        for c in clusters:
            hc.put(gpu, d_data, 4 * c.first, c.words)
        for group in [clusters] if together else [[c] for c in clusters]:
            hc.map_case(gpu, oracle, d_data, data_words, count, group, mode)
    finally:
        d_data.free()


@pytest.mark.parametrize("position", ["2^30", "2^31"])
def test_the_staged_map_kernel_at_high_word_indices(gpu, oracle, position):
    mapped(gpu, oracle, SHORT, "STAGED", SHORT // 31 + 1, [position], together=False)


def test_the_direct_map_kernel_at_high_word_indices(gpu, oracle):
    mapped(gpu, oracle, SHORT, "DIRECT512", SHORT // 127 + 1, ["2^30", "2^31"], together=True)


@pytest.mark.parametrize("mode,count", [("LONG256", 5000), ("LONG512", 2**20)])
def test_the_long_map_kernels_at_high_word_indices(gpu, oracle, mode, count):
    mapped(gpu, oracle, LONG, mode, count, ["2^30", "2^31", "3*2^30", "end"], together=True)
