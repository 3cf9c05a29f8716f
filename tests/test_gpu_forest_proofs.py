"""Stored forests on the GPU (vkmr_hip_reduce_forest_tree_async, vkmr_hip_forest_proofs_async,
vkmr_hip_verify_forest_proofs_async through HipDevice and MerkleForest): the roots against the roots-only forest call, every
proof against the stored tree of that tree alone and against the host CPU counterpart, the verifier's acceptance rule one
corruption at a time, stream order and buffer bounds, and the full size."""
import numpy as np
import pytest

import forest_cases as fc
import forest_proof_cases as fp

pytestmark = pytest.mark.gpu

PATTERN = 0xC3C3C3C3


def leaves_at(leaves, counts, trees, indices):
    """[k, 8]: the leaf every (tree, index) query names; the queries all name one."""
    off = fc.offsets_of(counts).astype(np.int64)
    return np.ascontiguousarray(leaves[off[np.asarray(trees, dtype=np.int64)] + np.asarray(indices, dtype=np.int64)])


def seed_of(name, counts):
    return len(name) * 7919 + sum(counts)


@pytest.mark.parametrize("name", sorted(fc.CASES))
def test_roots_equal_the_roots_only_forest_call_for_tight_and_loose_max_count(gpu, name):
    counts = fc.CASES[name]
    total, largest = sum(counts), max(1, max(counts))
    leaves = fc.random_leaves(total, seed=seed_of(name, counts))
    want = gpu.forest_roots(leaves, counts)
    for max_count in (None, largest, 1 << fc.ceil_log2(largest), max(total, 1), 2**63):
        forest = gpu.build_forest(leaves, counts, max_count=max_count)
        assert forest.ntrees == len(counts) and [int(c) for c in forest.counts] == counts
        assert forest.levels == fp.stride_of(total, max_count or largest)
        roots = forest.roots()
        assert roots.shape == (len(counts), 8) and roots.dtype == np.uint32
        assert (roots == want).all(), (max_count, np.nonzero((roots != want).any(axis=1))[0][:10])
        forest.free()


@pytest.mark.parametrize("name", sorted(fc.CASES))
def test_every_tree_gives_the_proofs_of_its_own_stored_tree_and_of_the_host_cpu(gpu, name):
    import vk_merkle_roots_amd as vk
    counts = fc.CASES[name]
    total = sum(counts)
    leaves = fc.random_leaves(total, seed=seed_of(name, counts))
    off = fc.offsets_of(counts)
    trees, indices = fp.all_queries(counts)
    forest = gpu.build_forest(leaves, counts)
    H = forest.levels
    sib, heights = forest.proofs(trees, indices)
    assert sib.shape == (trees.shape[0], H, 8) and heights.shape == (trees.shape[0],) and heights.dtype == np.uint32
    rc, cpu_sib, cpu_heights = fp.host_cpu_proofs(leaves, off, trees, indices, H)
    assert rc == 0
    assert (heights == cpu_heights).all()
    assert (sib == cpu_sib).all(), np.nonzero((sib != cpu_sib).any(axis=(1, 2)))[0][:10]
    roots = forest.roots()
    for t, c in enumerate(counts):
        if c == 0:
            continue
        mine = np.nonzero(trees == t)[0]
        h = vk.tree_height(c)
        assert (heights[mine] == h).all(), t
        d_slice = gpu.upload(leaves[int(off[t]): int(off[t + 1])])
        tree = gpu.build_tree(d_slice, c)
        assert tree.height == h
        single = tree.proofs(indices[mine])
        assert (sib[mine, :h] == single).all(), t
        assert not sib[mine, h:].any(), t
        assert (roots[t] == tree.root()).all(), t
        tree.free()
        d_slice.free()
    forest.free()


def mixed_batch():
    """(leaves, counts, trees, indices): every leaf of sizes_1_to_130 and power_of_two_edges as ONE forest, shuffled, a tenth
    of the queries twice."""
    counts = fc.CASES["sizes_1_to_130"] + fc.CASES["power_of_two_edges"]
    leaves = fc.random_leaves(sum(counts), seed=77)
    trees, indices = fp.all_queries(counts, sample_above=1 << 30)
    rng = np.random.default_rng(78)
    again = rng.integers(0, trees.shape[0], size=trees.shape[0] // 10)
    order = rng.permutation(np.concatenate([np.arange(trees.shape[0]), again]))
    return leaves, counts, trees[order], indices[order]


def test_a_mixed_batch_verifies_and_each_single_corruption_turns_exactly_its_own_answer(gpu):
    leaves, counts, trees, indices = mixed_batch()
    k = trees.shape[0]
    forest = gpu.build_forest(leaves, counts)
    H, roots = forest.levels, forest.roots()
    sib, heights = forest.proofs(trees, indices)
    forest.free()
    assert H == 14 and int(heights.min()) == 1 and int(heights.max()) == 14
    lv = leaves_at(leaves, counts, trees, indices)
    ok = gpu.verify_forest_proofs(lv, trees, indices, sib, heights, roots)
    assert ok.shape == (k,) and ok.all(), np.nonzero(~ok)[0][:10]

    rng = np.random.default_rng(79)
    mid = np.nonzero((heights > 1) & (heights < H))[0]           # proofs whose height can move both ways inside the stride

    def only(q, lv=lv, trees=trees, indices=indices, sib=sib, heights=heights):
        got = gpu.verify_forest_proofs(lv, trees, indices, sib, heights, roots)
        want = np.ones(k, dtype=bool)
        want[q] = False
        assert (got == want).all(), (q, np.nonzero(got != want)[0][:10])

    def pick(count, index):
        """A query for leaf `index` of a tree of `count` leaves.  The victims below have a sibling other than themselves at
        every level: where a node is its own sibling (the duplicate-last rule), swapping the operands changes nothing, and the
        index bit of that level is not covered by the proof (the ambiguity stated at vkmr_hip_verify_proofs_async)."""
        c = np.asarray(counts, dtype=np.int64)[trees.astype(np.int64)]
        return int(np.nonzero((c == count) & (indices == np.uint64(index)))[0][0])

    for q in (pick(2, 1), pick(77, 13), pick(8192, 5000), pick(8193, 0)):      # heights 1, 7, 13 and 14
        h = int(heights[q])
        for l in sorted({0, h - 1, int(rng.integers(0, h))}):      # a sibling cell below the height: one bit of one word
            bad = sib.copy()
            bad[q, l, int(rng.integers(0, 8))] ^= np.uint32(1 << int(rng.integers(0, 32)))
            only(q, sib=bad)
        bad = lv.copy()                                            # the leaf
        bad[q, 7] ^= np.uint32(0x80000000)
        only(q, lv=bad)
        for bit in sorted({0, h - 1, h, 63}):                      # an index bit: below the height the fold changes, at or above it the index is outside
            bad = indices.copy()
            bad[q] ^= np.uint64(1 << bit)
            only(q, indices=bad)
        for t in ((int(trees[q]) + 1) % len(counts), len(counts), 2**32 - 1):   # the tree number: another root, then no root at all
            bad = trees.copy()
            bad[q] = t
            only(q, trees=bad)
    for q in (int(mid[0]), int(mid[-1]), int(mid[mid.shape[0] // 2])):
        h = int(heights[q])
        for wrong in (h - 1, h + 1, 0, H + 1, 2**32 - 1):          # the height
            bad = heights.copy()
            bad[q] = wrong
            only(q, heights=bad)
    q = int(np.argmin(heights))                                    # height 1: h - 1 is 0
    bad = heights.copy()
    bad[q] = 0
    only(q, heights=bad)

    # padding cells at l >= height are never read: garbage in all of them changes nothing
    noisy = sib.copy()
    pad = np.arange(H)[None, :] >= heights[:, None]
    noisy[pad] = rng.integers(0, 2**32, size=(int(pad.sum()), 8), dtype=np.uint32)
    assert pad.any() and gpu.verify_forest_proofs(lv, trees, indices, noisy, heights, roots).all()
    # a wider stride with the same cells in front
    wide = np.concatenate([noisy, rng.integers(0, 2**32, size=(k, 3, 8), dtype=np.uint32)], axis=1)
    assert gpu.verify_forest_proofs(lv, trees, indices, wide, heights, roots).all()


def test_a_uniform_forest_agrees_with_the_single_height_verifier(gpu):
    h, ntrees, k = 8, 96, 20000
    counts = [1 << h] * ntrees
    leaves = fc.random_leaves(sum(counts), seed=81)
    rng = np.random.default_rng(82)
    trees, indices = fp.random_queries(rng, counts, k)
    forest = gpu.build_forest(leaves, counts)
    assert forest.levels == h
    roots = forest.roots()
    sib, heights = forest.proofs(trees, indices)
    forest.free()
    assert (heights == h).all()
    lv = leaves_at(leaves, counts, trees, indices)
    per_proof_roots = np.ascontiguousarray(roots[trees])
    good = gpu.verify_forest_proofs(lv, trees, indices, sib, heights, roots)
    assert good.all() and (good == gpu.verify_proofs(lv, indices, sib, per_proof_roots)).all()
    # a tenth of the proofs corrupted: a sibling cell, the leaf or the index, the same change seen by both verifiers
    victims = rng.choice(k, size=k // 10, replace=False)
    bad_sib, bad_lv, bad_idx = sib.copy(), lv.copy(), indices.copy()
    for n, q in enumerate(victims):
        if n % 3 == 0:
            bad_sib[q, int(rng.integers(0, h)), int(rng.integers(0, 8))] ^= np.uint32(1 << int(rng.integers(0, 32)))
        elif n % 3 == 1:
            bad_lv[q, int(rng.integers(0, 8))] ^= np.uint32(1)
        else:
            bad_idx[q] ^= np.uint64(1 << int(rng.integers(0, h + 2)))
    got = gpu.verify_forest_proofs(bad_lv, trees, bad_idx, bad_sib, heights, roots)
    want = np.ones(k, dtype=bool)
    want[victims] = False
    assert (got == want).all()
    assert (got == gpu.verify_proofs(bad_lv, bad_idx, bad_sib, per_proof_roots)).all()


@pytest.mark.parametrize("seed", range(50))
def test_random_forests_gather_verify_and_fold_on_the_cpu_to_the_oracle_roots(gpu, oracle, seed):
    rng = np.random.default_rng(seed)
    counts = fp.random_counts(rng, 1 << 20)
    leaves = fc.random_leaves(sum(counts), seed=2000 + seed)
    want_roots = fc.oracle_roots(oracle, leaves, counts)
    if not counts:
        return                               # the budget cut every tree: nothing to build
    forest = gpu.build_forest(leaves, counts)
    roots = forest.roots()
    assert (roots == want_roots).all()
    if max(counts) == 0:                     # only empty trees: no leaf to prove
        forest.free()
        return
    k = 4096
    trees, indices = fp.random_queries(rng, counts, k)
    sib, heights = forest.proofs(trees, indices)
    forest.free()
    lv = leaves_at(leaves, counts, trees, indices)
    assert gpu.verify_forest_proofs(lv, trees, indices, sib, heights, roots).all()
    for q in range(k):
        assert heights[q] == fp.tree_height(counts[int(trees[q])])
        assert (fp.host_fold(lv[q], indices[q], sib[q], heights[q]) == want_roots[int(trees[q])]).all(), q


def test_invalid_queries_get_height_zero_zero_cells_and_a_refusal_and_leave_their_neighbours_alone(gpu):
    counts = [4, 0, 0, 7, 0, 1, 130]
    leaves = fc.random_leaves(sum(counts), seed=17)
    forest = gpu.build_forest(leaves, counts)
    H, roots = forest.levels, forest.roots()
    #        named, tree == ntrees, named, index == c_t, named, empty, named, empty, index far above, named, tree 2^32 - 1, named
    trees = np.array([0, 7, 3, 0, 6, 1, 5, 4, 3, 6, 2**32 - 1, 0], dtype=np.uint32)
    indices = np.array([3, 0, 6, 4, 129, 0, 0, 0, 2**63, 0, 0, 0], dtype=np.uint64)
    valid = np.array([1, 0, 1, 0, 1, 0, 1, 0, 0, 1, 0, 1], dtype=bool)
    sib, heights = forest.proofs(trees, indices)
    forest.free()
    assert H == 8 and list(heights) == [2, 0, 3, 0, 8, 0, 1, 0, 0, 8, 0, 2]
    assert not sib[~valid].any()
    want_sib, want_heights, _ = fp.gather(leaves, fc.offsets_of(counts), trees, indices, H)
    assert (sib == want_sib).all() and (heights == want_heights).all()
    lv = fc.random_leaves(trees.shape[0], seed=19)                 # any leaf for the invalid ones: they are refused before the fold
    lv[valid] = leaves_at(leaves, counts, trees[valid], indices[valid])
    ok = gpu.verify_forest_proofs(lv, trees, indices, sib, heights, roots)
    assert (ok == valid).all()
    # the same answer from the restated rule
    assert [fp.accepts(lv[q], trees[q], indices[q], sib[q], heights[q], H, roots) for q in range(trees.shape[0])] == list(valid)


def test_a_refused_forest_raises_with_the_status_text(gpu):
    leaves = fc.random_leaves(20, seed=3)
    with pytest.raises(ValueError, match="bit 1"):
        gpu.build_forest(leaves, [5, 9, 6], max_count=8)
    with pytest.raises(ValueError):
        gpu.build_forest(leaves, [5, 9, 5])
    with pytest.raises(ValueError):
        gpu.build_forest(leaves, [])


def test_stream_order_exact_buffers_and_canaries(gpu, oracle):
    """map -> build -> proofs -> verify -> download on one stream with no synchronisation in between.  forest_dev is exactly
    vkmr_hip_forest_tree_bytes between two canary pages; the siblings and the heights lie between canary pages too."""
    import vk_merkle_roots_amd as vk
    batch = vk.rndm_packed(7, 20000, 60)
    rng = np.random.default_rng(8)
    counts = []
    while sum(counts) < batch.count:
        counts.append(min(int(rng.integers(0, 700)), batch.count - sum(counts)))
    ntrees, total, max_count = len(counts), batch.count, max(counts)
    host_leaves = oracle.leaves_packed(batch.data, batch.meta)
    want_roots = fc.oracle_roots(oracle, host_leaves, counts)
    k = 5000
    trees, indices = fp.random_queries(rng, counts, k)
    H = fp.stride_of(total, max_count)
    forest_bytes = gpu.lib.vkmr_hip_forest_tree_bytes(total, ntrees, max_count)
    assert forest_bytes == 32 * fp.stored_cells(total, ntrees, max_count)
    guard = 4096
    sib_bytes, h_bytes = 32 * k * H, 4 * k
    d_forest = gpu.upload(np.full((guard + forest_bytes + guard) // 4, PATTERN, dtype=np.uint32))
    d_sib = gpu.upload(np.full((guard + sib_bytes + guard) // 4, PATTERN, dtype=np.uint32))
    d_h = gpu.upload(np.full((guard + h_bytes + guard) // 4, PATTERN, dtype=np.uint32))
    d_data, d_meta, d_off = gpu.upload(batch.data), gpu.upload(batch.meta), gpu.upload(fc.offsets_of(counts))
    d_trees, d_idx = gpu.upload(trees), gpu.upload(indices)
    d_lv = gpu.upload(leaves_at(host_leaves, counts, trees, indices))
    d_leaves, d_roots, d_status, d_ok = gpu.alloc(32 * total), gpu.alloc(32 * ntrees), gpu.alloc(4), gpu.alloc(4 * k)
    lib, s = gpu.lib, gpu.new_stream()
    roots = np.zeros((ntrees, 8), dtype=np.uint32)
    status = np.full(1, 0xFFFFFFFF, dtype=np.uint32)
    ok = np.zeros(k, dtype=np.uint32)
    gpu.map_async(d_data, batch.words, d_meta, total, d_leaves, stream=s)
    vk.check(lib.vkmr_hip_reduce_forest_tree_async(gpu.index, s, d_leaves.ptr, total, d_off.ptr, ntrees, max_count, d_forest.at(guard), d_roots.ptr,
                                                   d_status.ptr), "vkmr_hip_reduce_forest_tree_async")
    vk.check(lib.vkmr_hip_forest_proofs_async(gpu.index, s, d_leaves.ptr, d_forest.at(guard), total, d_off.ptr, ntrees, max_count, d_trees.ptr,
                                              d_idx.ptr, k, d_sib.at(guard), d_h.at(guard)), "vkmr_hip_forest_proofs_async")
    vk.check(lib.vkmr_hip_verify_forest_proofs_async(gpu.index, s, d_lv.ptr, d_trees.ptr, d_idx.ptr, d_sib.at(guard), d_h.at(guard), k, H,
                                                     d_roots.ptr, ntrees, d_ok.ptr), "vkmr_hip_verify_forest_proofs_async")
    for dst, src in ((roots, d_roots), (status, d_status), (ok, d_ok)):
        vk.check(lib.vkmr_hip_memcpy_d2h_async(gpu.index, s, dst.ctypes.data, src.ptr, dst.nbytes), "d2h")
    gpu.sync(s)
    assert status[0] == 0
    assert (roots == want_roots).all()
    assert (ok == 1).all()
    for buf, payload in ((d_forest, forest_bytes), (d_sib, sib_bytes), (d_h, h_bytes)):
        after = gpu.download(buf, guard + payload + guard)
        assert (after[: guard // 4] == PATTERN).all() and (after[-(guard // 4):] == PATTERN).all()
    sib = gpu.download(d_sib, sib_bytes, offset=guard).reshape(k, H, 8)
    heights = gpu.download(d_h, h_bytes, offset=guard)
    rc, cpu_sib, cpu_heights = fp.host_cpu_proofs(host_leaves, fc.offsets_of(counts), trees, indices, H)
    assert rc == 0 and (sib == cpu_sib).all() and (heights == cpu_heights).all()
    lib.vkmr_hip_stream_destroy(gpu.index, s)
    for b in (d_forest, d_sib, d_h, d_data, d_meta, d_off, d_trees, d_idx, d_lv, d_leaves, d_roots, d_status, d_ok):
        b.free()


def test_merkle_forest_packed_maps_once_and_proves_strings(gpu, oracle):
    import vk_merkle_roots_amd as vk
    batch = vk.rndm_packed(42, 30_000, 127)
    rng = np.random.default_rng(42)
    counts = []
    while sum(counts) < batch.count:
        counts.append(min(int(rng.integers(0, 3000)), batch.count - sum(counts)))
    forest = vk.merkle_forest_packed(gpu, batch, counts)
    host_leaves = oracle.leaves_packed(batch.data, batch.meta)
    roots = forest.roots()
    assert (roots == fc.oracle_roots(oracle, host_leaves, counts)).all()
    trees, indices = fp.random_queries(rng, counts, 1000)
    sib, heights = forest.proofs(trees, indices)
    forest.free()
    assert gpu.verify_forest_proofs(leaves_at(host_leaves, counts, trees, indices), trees, indices, sib, heights, roots).all()


class _Slice:
    """A tree's leaves inside a larger device buffer: what MerkleTree needs of a DeviceBuffer."""

    def __init__(self, buf, first_cell):
        self.ptr = buf.at(32 * first_cell)


def test_two_to_the_26_leaves_in_equal_trees_two_to_the_20_queries(gpu):
    import vk_merkle_roots_amd as vk
    cap, ntrees, k = 1 << 11, 1 << 15, 1 << 20
    total = cap * ntrees
    leaves = np.empty((total, 8), dtype=np.uint32)
    d_leaves = gpu.alloc(32 * total)
    rng = np.random.default_rng(26)
    chunk = 1 << 22
    for at in range(0, total, chunk):      # random digests, uploaded in pieces
        leaves[at: at + chunk] = rng.integers(0, 2**32, size=(chunk, 8), dtype=np.uint32)
        part = leaves[at: at + chunk]
        vk.check(gpu.lib.vkmr_hip_memcpy_h2d_async(gpu.index, gpu.stream, d_leaves.at(32 * at), part.ctypes.data, part.nbytes), "h2d")
        gpu.sync()
    counts = [cap] * ntrees
    forest = gpu._build_forest_of_buffer(d_leaves, total, counts, cap, "full size")
    assert forest.levels == 11
    trees = rng.integers(0, ntrees, size=k).astype(np.uint32)
    indices = rng.integers(0, cap, size=k).astype(np.uint64)
    d_trees, d_idx = gpu.upload(trees), gpu.upload(indices)
    d_lv = gpu.upload(np.ascontiguousarray(leaves[trees.astype(np.int64) * cap + indices.astype(np.int64)]))
    d_sib, d_h, d_ok = gpu.alloc(32 * k * 11), gpu.alloc(4 * k), gpu.alloc(4 * k)
    forest.proofs_async(d_trees, d_idx, k, d_sib, d_h)
    gpu.verify_forest_proofs_async(d_lv, d_trees, d_idx, d_sib, d_h, k, 11, forest.roots_buf, ntrees, d_ok)
    assert (gpu.download(d_ok, 4 * k) == 1).all()
    assert (gpu.download(d_h, 4 * k) == 11).all()
    sib = gpu.download(d_sib, 32 * k * 11).reshape(k, 11, 8)
    roots = forest.roots()
    for q in rng.choice(k, size=64, replace=False):
        t = int(trees[q])
        tree = gpu.build_tree(_Slice(d_leaves, t * cap), cap)
        assert (tree.proofs(indices[q: q + 1])[0] == sib[q]).all(), q
        assert (tree.root() == roots[t]).all()
        tree.free()
    forest.free()
    for b in (d_leaves, d_trees, d_idx, d_lv, d_sib, d_h, d_ok):
        b.free()
