"""The mutation flag of a forest on the GPU (vkmr_hip_reduce_forest_mutated_async, its stored twin and the scan
vkmr_hip_forest_tree_mutated_async, raw and through HipDevice / MerkleForest): every mask against the rule restated in
tests/forest_mutation_cases.py, the roots and the stored levels against the plain builds on the same buffers, a refused forest,
the scan behind updates, and the words around the masks."""
import numpy as np
import pytest

import forest_cases as fc
import forest_mutation_cases as fm
from merkle_model import At

pytestmark = pytest.mark.gpu

PATTERN = 0xC3C3C3C3
GUARD = 64                                    # uint64 words in front of and behind the masks


class Run:
    """One raw call of a build over leaves already on the device; every output buffer starts as PATTERN."""

    def __init__(self, gpu, d_leaves, total, offsets, max_count, stored, flagged):
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        ntrees = offsets.shape[0] - 1
        d_off = gpu.upload(offsets)
        nbytes = gpu.forest_tree_bytes(total, ntrees, max_count) if stored else gpu.lib.vkmr_hip_forest_scratch_bytes(total, ntrees)
        d_levels = gpu.upload(np.full(nbytes // 4, PATTERN, dtype=np.uint32))
        d_roots = gpu.upload(np.full((ntrees, 8), PATTERN, dtype=np.uint32))
        d_status = gpu.upload(np.array([0xFFFFFFFF], dtype=np.uint32))
        d_mut = gpu.upload(np.full(2 * (GUARD + ntrees + GUARD), PATTERN, dtype=np.uint32))
        masks_at = At(d_mut, 8 * GUARD)
        if flagged:
            call = gpu.reduce_forest_tree_mutated_async if stored else gpu.reduce_forest_mutated_async
            call(d_leaves, total, d_off, ntrees, max_count, d_levels, d_roots, masks_at, d_status)
        else:
            call = gpu.reduce_forest_tree_async if stored else gpu.reduce_forest_async
            call(d_leaves, total, d_off, ntrees, max_count, d_levels, d_roots, d_status)
        self.status = int(gpu.download(d_status, 4)[0])
        self.roots = gpu.download(d_roots, 32 * ntrees).reshape(ntrees, 8)
        self.levels = gpu.download(d_levels, nbytes) if stored else None
        words = gpu.download(d_mut, 8 * (2 * GUARD + ntrees), dtype=np.uint64)
        self.masks = words[GUARD: GUARD + ntrees]
        self.guards = np.concatenate([words[:GUARD], words[GUARD + ntrees:]])
        for b in (d_off, d_levels, d_roots, d_status, d_mut):
            b.free()

    def guards_untouched(self):
        return (self.guards == np.uint64(PATTERN * 0x100000001)).all()


def check_case(gpu, name, runs):
    counts = fm.CASES[name]
    total, off = sum(counts), fm.offsets_of(counts)
    for run in runs:
        leaves = fm.leaves_of(name, run)
        want_roots, want = fm.expected(name, run)
        d_leaves = gpu.upload(leaves) if total else None
        plain = Run(gpu, d_leaves, total, off, max(1, max(counts)), stored=False, flagged=False)
        stored = Run(gpu, d_leaves, total, off, max(1, max(counts)), stored=True, flagged=False)
        assert plain.status == 0 and stored.status == 0
        assert (plain.roots == want_roots).all(), run
        for twin, ref in ((False, plain), (True, stored)):
            got = Run(gpu, d_leaves, total, off, max(1, max(counts)), stored=twin, flagged=True)
            assert got.status == 0, (run, twin)
            assert (got.masks == want).all(), (run, twin, np.nonzero(got.masks != want)[0][:10])
            assert (got.roots == ref.roots).all(), (run, twin)
            assert got.guards_untouched(), (run, twin)
            if twin:                          # the same forest, cell for cell (the cells nobody writes keep the fill in both)
                assert (got.levels == ref.levels).all(), (run, np.nonzero(got.levels != ref.levels)[0][:8] // 8)
        if d_leaves:
            d_leaves.free()


@pytest.mark.parametrize("name", sorted(fm.CASES))
def test_random_and_planted_leaves_give_the_models_masks(gpu, name):
    """Random leaves (every mask 0, at every ragged edge) and the nine planted variants: first, last and middle pair at the
    lowest, highest and a middle level of every tree."""
    check_case(gpu, name, [r for r in fm.RUNS if r != "equal"])


@pytest.mark.parametrize("name", sorted(fm.CASES))
def test_all_equal_leaves_give_the_models_masks(gpu, name):
    """Every genuine pair of every level hits.  power_of_two_edges and sizes_1_to_130 put tree starts inside wavefronts (the
    per-lane search and the per-lane atomic); one_tree_of_5000 and one_big_among_small fill whole wavefronts with one tree (the
    ballot, one atomic per wavefront, skipped once the bit is there)."""
    check_case(gpu, name, ["equal"])
    for t, c in enumerate(fm.CASES[name]):
        assert int(fm.expected(name, "equal")[1][t]) == (0 if c < 2 else (1 << fc.ceil_log2(c)) - 1)


@pytest.mark.parametrize("stored", [False, True], ids=["roots", "stored"])
def test_a_refused_forest_leaves_the_masks_zero_and_writes_no_root(gpu, stored):
    counts = [5, 9, 130, 1, 64]
    total, off = sum(counts), fm.offsets_of(counts)
    leaves = np.tile(fc.random_leaves(1, seed=9), (total, 1))       # all equal: every tree but the lone leaf would be flagged
    d_leaves = gpu.upload(leaves)
    ok = Run(gpu, d_leaves, total, off, 130, stored, flagged=True)
    assert ok.status == 0 and (ok.masks == fm.model(leaves, counts)[1]).all() and ok.masks[0] == 7 and ok.masks[3] == 0
    bad = Run(gpu, d_leaves, total, off, 129, stored, flagged=True)                   # one tree of max_count + 1
    assert bad.status == 2
    assert not bad.masks.any()
    assert (bad.roots == PATTERN).all()
    assert bad.guards_untouched()
    decreasing = off.copy()
    decreasing[2], decreasing[3] = off[3], off[2]
    bad = Run(gpu, d_leaves, total, decreasing, total, stored, flagged=True)
    assert bad.status & 1 and not bad.masks.any() and (bad.roots == PATTERN).all() and bad.guards_untouched()
    d_leaves.free()


def test_python_layer_returns_roots_and_masks(gpu):
    import vk_merkle_roots_amd as vk
    name = "sizes_1_to_130"
    counts = fm.CASES[name]
    leaves = fm.leaves_of(name, "plant4")
    want_roots, want = fm.expected(name, "plant4")
    roots, masks = gpu.forest_roots_mutated(leaves, counts)
    assert roots.dtype == np.uint32 and masks.dtype == np.uint64 and masks.shape == (len(counts),)
    assert (roots == want_roots).all() and (masks == want).all()
    assert (roots == gpu.forest_roots(leaves, counts)).all()
    roots, masks = gpu.forest_roots_mutated(leaves, counts, max_count=2**63)
    assert (roots == want_roots).all() and (masks == want).all()
    roots, masks = gpu.forest_roots_mutated(np.zeros((0, 8), dtype=np.uint32), [])
    assert roots.shape == (0, 8) and masks.shape == (0,)
    with pytest.raises(ValueError, match="bit 1"):
        gpu.forest_roots_mutated(leaves, counts, max_count=129)
    # the strings-to-verdict path on CVE-2012-2459's two pairs: equal roots, and the padded list is told apart
    blocks = [[b"a", b"b", b"c"], [b"a", b"b", b"c", b"c"], [b"a", b"b", b"c", b"d", b"e", b"f"], [b"a", b"b", b"c", b"d", b"e", b"f", b"e", b"f"], [b"x"]]
    batch = vk.pack_lines(b"".join(s + b"\n" for blk in blocks for s in blk))
    roots, masks = vk.merkle_roots_packed_forest_mutated(gpu, batch, [len(b) for b in blocks])
    assert (roots == vk.merkle_roots_packed_forest(gpu, batch, [len(b) for b in blocks])).all()
    assert (roots[0] == roots[1]).all() and (roots[2] == roots[3]).all()
    assert list(masks) == [0, 1, 0, 2, 0]


def test_the_scan_follows_updates_of_a_stored_forest(gpu):
    import vk_merkle_roots_amd as vk
    counts = [77, 4096, 0, 5000, 1, 130, 64, 3]
    off = fm.offsets_of(counts).astype(np.int64)
    host = fc.random_leaves(sum(counts), seed=313)
    fm.plant(host, int(off[0]), 77, 0, 37)            # tree 0: the last genuine pair of level 0
    fm.plant(host, int(off[3]), 5000, 11, 0)          # tree 3: the highest level at which a block fits
    forest = gpu.build_forest(host, counts, mutated=True)
    want_roots, want = fm.model(host, counts)
    assert list(want[[0, 3]]) == [1, 1 << 11] and not want[[1, 2, 4, 5, 6, 7]].any()
    assert forest.built_mutated.dtype == np.uint64 and (forest.built_mutated == want).all()
    assert (forest.mutated() == want).all()
    assert (forest.roots() == want_roots).all()
    plain = gpu.build_forest(host, counts)            # the plain build keeps no masks; its scan gives the same
    assert plain.built_mutated is None and (plain.mutated() == want).all()
    plain.free()

    # one planted pair disappears, one appears at level 0, one at level 4 through the update of a whole block
    rng = np.random.default_rng(314)
    trees = [0, 1] + [5] * 16
    indices = [75, 2001] + list(range(48, 64))
    new = np.concatenate([fc.random_leaves(1, seed=315), host[off[1] + 2000: off[1] + 2001], host[off[5] + 32: off[5] + 48]])
    order = rng.permutation(len(trees))               # update() sorts
    forest.update(np.array(trees, dtype=np.uint32)[order], np.array(indices, dtype=np.uint64)[order], new[order])
    host[off[0] + 75] = new[0]
    host[off[1] + 2001] = new[1]
    host[off[5] + 48: off[5] + 64] = new[2:]
    want_roots, want = fm.model(host, counts)
    assert list(want[[0, 1, 3, 5]]) == [0, 1, 1 << 11, 1 << 4]
    assert (forest.mutated() == want).all()
    assert (forest.roots() == want_roots).all() and (forest.roots() == gpu.forest_roots(host, counts)).all()
    assert (forest.built_mutated != want).any()       # the build's masks are the build's

    # update_packed: two equal strings side by side are a level-0 hit; the leaves are read back for the model
    forest.update_packed([6, 6], [10, 11], vk.pack_lines(b"same\nsame\n"))
    host = gpu.download(forest.digests, 32 * sum(counts)).reshape(-1, 8)
    want_roots, want = fm.model(host, counts)
    assert int(want[6]) == 1
    assert (forest.mutated() == want).all() and (forest.roots() == want_roots).all()

    # update and scan on one stream with no synchronisation in between: the scan sees the new leaves
    s = gpu.new_stream()
    d_trees, d_idx = gpu.upload(np.array([7], dtype=np.uint32)), gpu.upload(np.array([1], dtype=np.uint64))
    d_new, d_status, d_mut = gpu.upload(host[off[7]: off[7] + 1]), gpu.alloc(4), gpu.alloc(8 * len(counts))
    forest.update_async(d_trees, d_idx, d_new, 1, d_status, stream=s)
    forest.mutated_async(d_mut, stream=s)
    masks = gpu.download(d_mut, 8 * len(counts), dtype=np.uint64, stream=s)
    assert int(gpu.download(d_status, 4, stream=s)[0]) == 0
    host[off[7] + 1] = host[off[7]]
    assert (masks == fm.model(host, counts)[1]).all() and int(masks[7]) == 1          # [a, a, c]: level 0 only
    gpu.lib.vkmr_hip_stream_destroy(gpu.index, s)
    for b in (d_trees, d_idx, d_new, d_status, d_mut):
        b.free()
    forest.free()


def test_the_scan_of_every_case_table_equals_the_builds_masks(gpu):
    for name in sorted(fm.CASES):
        counts = fm.CASES[name]
        for run in ("equal", "plant7"):
            want = fm.expected(name, run)[1]
            forest = gpu.build_forest(fm.leaves_of(name, run), counts, mutated=True)
            assert (forest.built_mutated == want).all(), (name, run)
            assert (forest.mutated() == want).all(), (name, run)
            forest.free()
