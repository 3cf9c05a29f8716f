"""Range proofs on the GPU (vkmr_hip_forest_range_async, vkmr_hip_verify_forest_range_async and their one-tree twins through
HipDevice, MerkleForest, MerkleTree and vk.RangeProofs): cell for cell what the CPU twins and the hashlib model of
tests/range_cases.py give for its one forest, between guard cells, at two placements; status bit 0; the count of 2^32 + 2^20 leaves;
the verifier's negatives; sort -> ranges -> verify chained on one stream; behind inserted and removed; a set synced in four chunks;
the forest and the outputs above 4 GiB; the one-tree twins."""
import numpy as np
import pytest

import forest_update_cases as fu
import high_cases as hc
import range_cases as rc
from merkle_model import At, cpu_levels, random_leaves

pytestmark = pytest.mark.gpu

GUARD = 4                                                    # guard cells on either side of every output


def guarded(tmp, n, fill, dtype, width=1):
    return tmp.upload(np.full((n + 2 * GUARD) * width, fill, dtype))


def inner(gpu, buf, n, fill, dtype, width=1):
    """The n items between the guards, which must still be the fill."""
    got = gpu.download(buf, (n + 2 * GUARD) * width * np.dtype(dtype).itemsize, dtype=dtype).reshape(n + 2 * GUARD, width)
    assert (got[:GUARD] == fill).all() and (got[-GUARD:] == fill).all()
    return got[GUARD:-GUARD]


def at(buf, dtype, width=1):
    return At(buf, GUARD * width * np.dtype(dtype).itemsize)


def device_range(gpu, forest, trees, lo, hi, stride, capacity):
    """(firsts, leaf_starts, leaves [capacity, 8], left, right, heights, info) of one raw call, every output between guards that
    start as the canary, the leaves included: what the call does not write is still the canary."""
    Q = len(trees)
    with gpu.scope() as tmp:
        d_first, d_starts = guarded(tmp, Q, rc.INDEX_FILL, np.uint64), guarded(tmp, Q + 1, rc.INDEX_FILL, np.uint64)
        d_h, d_info = guarded(tmp, Q, rc.CANARY, np.uint32), guarded(tmp, 4, rc.INDEX_FILL, np.uint64)
        d_leaves = guarded(tmp, capacity, rc.CANARY, np.uint32, 8)
        d_left, d_right = guarded(tmp, Q * stride, rc.CANARY, np.uint32, 8), guarded(tmp, Q * stride, rc.CANARY, np.uint32, 8)
        forest.range_async(tmp.upload(trees), tmp.upload(lo), tmp.upload(hi), Q, stride, tmp.alloc(gpu.range_scratch_bytes(0, Q)), at(d_first, np.uint64),
                           at(d_starts, np.uint64), at(d_leaves, np.uint32, 8) if capacity else None, capacity, at(d_left, np.uint32, 8),
                           at(d_right, np.uint32, 8), at(d_h, np.uint32), at(d_info, np.uint64))
        return (inner(gpu, d_first, Q, rc.INDEX_FILL, np.uint64)[:, 0], inner(gpu, d_starts, Q + 1, rc.INDEX_FILL, np.uint64)[:, 0],
                inner(gpu, d_leaves, capacity, rc.CANARY, np.uint32, 8), inner(gpu, d_left, Q * stride, rc.CANARY, np.uint32, 8).reshape(Q, stride, 8),
                inner(gpu, d_right, Q * stride, rc.CANARY, np.uint32, 8).reshape(Q, stride, 8), inner(gpu, d_h, Q, rc.CANARY, np.uint32)[:, 0],
                inner(gpu, d_info, 4, rc.INDEX_FILL, np.uint64)[:, 0])


def device_verify(gpu, trees, lo, hi, firsts, starts, leaves, left, right, heights, roots, counts):
    """(verdict, in_first, in_count) of one raw call, between guards."""
    Q, stride, n = len(trees), int(left.shape[1]), int(leaves.shape[0])
    with gpu.scope() as tmp:
        d_verdict, d_first, d_count = guarded(tmp, Q, rc.CANARY, np.uint32), guarded(tmp, Q, rc.INDEX_FILL, np.uint64), guarded(tmp, Q, rc.INDEX_FILL, np.uint64)
        up = lambda a, t: tmp.upload(np.ascontiguousarray(a, dtype=t))
        gpu.verify_forest_range_enqueue(up(trees, np.uint32), up(lo, np.uint32), up(hi, np.uint32), up(firsts, np.uint64), up(starts, np.uint64),
                                        up(leaves, np.uint32) if n else None, n, up(left, np.uint32), up(right, np.uint32), up(heights, np.uint32), Q, stride,
                                        up(roots, np.uint32), up(counts, np.uint64), len(counts), tmp.alloc(gpu.range_scratch_bytes(n, Q)),
                                        at(d_verdict, np.uint32), at(d_first, np.uint64), at(d_count, np.uint64))
        return (inner(gpu, d_verdict, Q, rc.CANARY, np.uint32)[:, 0], inner(gpu, d_first, Q, rc.INDEX_FILL, np.uint64)[:, 0],
                inner(gpu, d_count, Q, rc.INDEX_FILL, np.uint64)[:, 0])


def same(got, want, note):
    for what, a, b in zip(("firsts", "leaf_starts", "leaves", "left", "right", "heights", "info"), got, want):
        assert a.shape == b.shape and (a == b).all(), (note, what, np.nonzero((a != b).reshape(a.shape[0], -1).any(axis=1))[0][:8])


@pytest.fixture(scope="module")
def cases():
    """The forest, its queries, what the model expects and what the CPU twin gives at the second placement, computed once."""
    f = rc.forest()
    what, trees, lo, hi = f.queries()
    cells, offsets = f.placed(first=37, slack=100)
    expected = f.expected()
    n = int(expected[6][1])
    twin = rc.host_range(cells, offsets, trees, lo, hi, capacity=n, guard=0)
    assert twin[0] == 0
    return f, trees, lo, hi, expected, twin[1:], cells, n


@pytest.fixture(scope="module")
def placed(gpu, cases):
    """The forest stored on the device with offsets[0] == 37 and 100 cells behind, and the whole batch out of it in ONE call."""
    f, trees, lo, hi, expected, twin, cells, n = cases
    raw = fu.RawForest(gpu, cells, f.counts, 2500, first=37)
    got = device_range(gpu, raw.handle, trees, lo, hi, rc.STRIDE, n)
    yield raw, got
    raw.free()


def test_the_device_is_the_cpu_twin_and_the_model_cell_for_cell(gpu, cases, placed):
    f, trees, lo, hi, expected, twin = cases[:6]
    raw, got = placed
    same(got, twin, "twin")
    same(got, expected[:7], "model")
    assert (raw.handle.roots() == f.roots).all()
    verdict, in_first, in_count = device_verify(gpu, trees, lo, hi, *got[:6], f.roots, f.counts)
    want = rc.host_verify(trees, lo, hi, *got[:6], f.roots, f.counts)
    for what, a, b, c in zip(("verdict", "in_first", "in_count"), (verdict, in_first, in_count), want, expected[7:]):
        assert (a == b).all() and (a == c).all(), (what, np.nonzero(a != c)[0][:8])
    other = np.roll(f.roots, 1, axis=0)                                                            # every tree under its neighbour's root
    wrong = device_verify(gpu, trees, lo, hi, *got[:6], other, f.counts)
    assert not wrong[0].any() and not wrong[1].any() and not wrong[2].any()


def test_the_handles_at_the_first_placement_and_a_wide_stride(gpu, cases):
    import vk_merkle_roots_amd as vk
    f, trees, lo, hi, expected = cases[:5]
    forest = gpu.build_forest(np.concatenate(f.trees), f.counts)
    assert forest.is_sorted()
    proofs = forest.ranges(trees, lo, hi)
    assert proofs.stride == 12 and proofs.same_as(vk.RangeProofs(trees, lo, hi, *expected[:6])) and proofs.info.tolist() == expected[6].tolist()
    verdict, in_first, in_count = proofs.verify(gpu, forest.roots(), forest.counts)
    assert (verdict == expected[7]).all() and (in_first == expected[8]).all() and (in_count == expected[9]).all()
    for q in range(0, proofs.Q, 9):
        assert proofs.in_range(q).shape[0] == int(in_count[q])
    wide = forest.ranges(trees, lo, hi, stride=15)
    assert (wide.left[:, :12] == expected[3]).all() and not wide.left[:, 12:].any() and (wide.right[:, :12] == expected[4]).all() and not wide.right[:, 12:].any()
    assert (wide.verify(gpu, f.roots, f.counts)[0] == expected[7]).all()
    with pytest.raises(vk.VkmrError):
        forest.ranges(trees, lo, hi, stride=11)                                                    # the forest's rows have twelve cells
    none = forest.ranges([], np.zeros((0, 8), np.uint32), np.zeros((0, 8), np.uint32))
    assert none.Q == 0 and [x.shape for x in none.verify(gpu, f.roots, f.counts)] == [(0,)] * 3
    gpu.forest_range_enqueue(*([None, None, 0, None, 0, 0, None, None, None, 0, 0] + [None] * 4 + [0] + [None] * 4))   # Q == 0: nothing is done
    gpu.verify_forest_range_enqueue(*([None] * 6 + [0, None, None, None, 0, 0, None, None, 0] + [None] * 4))
    forest.free()


def test_bit_0_leaves_every_leaf_cell_untouched_and_names_the_total(gpu, cases, placed):
    import vk_merkle_roots_amd as vk
    f, trees, lo, hi, expected, twin, cells, n = cases
    raw, full = placed
    for capacity in (0, 7, n - 1):
        got = device_range(gpu, raw.handle, trees, lo, hi, rc.STRIDE, capacity)
        assert got[6].tolist() == [1, n] + expected[6].tolist()[2:] and (got[2] == rc.CANARY).all()
        same(got[:2] + got[3:6], full[:2] + full[3:6], f"capacity {capacity}")
    assert "bit 0" in vk.range_status_text(1)
    roomy = device_range(gpu, raw.handle, trees, lo, hi, rc.STRIDE, n + 9)                         # nothing at or behind leaf_starts[Q]
    assert roomy[6].tolist() == expected[6].tolist() and (roomy[2][:n] == expected[2]).all() and (roomy[2][n:] == rc.CANARY).all()


def test_4097_whole_tree_ranges_of_2_pow_20_leaves_count_2_pow_32_plus_2_pow_20(gpu):
    """Count only, capacity 0: no leaf is copied, and the prefix over m is formed in 64 bits."""
    rng = np.random.default_rng(731)
    c, Q = 1 << 20, 4097
    forest, _ = gpu.build_sorted_forest(random_leaves(rng, c), [c])
    trees, lo, hi = np.zeros(Q, np.uint32), np.zeros((Q, 8), np.uint32), np.full((Q, 8), 0xFFFFFFFF, np.uint32)
    firsts, starts, leaves, left, right, heights, info = device_range(gpu, forest, trees, lo, hi, 20, 0)
    assert info.tolist() == [1, (1 << 32) + (1 << 20), 0, Q * c]
    assert not firsts.any() and (heights == 20).all() and (starts == np.arange(Q + 1, dtype=np.uint64) * np.uint64(c)).all()
    assert not left.any() and not right.any()                                                      # a whole tree has nothing beside it
    forest.free()


def test_the_verifiers_negatives(gpu):
    neg = rc.negatives()
    want = [w for _, w, _ in neg]
    batch = rc.batch([p for _, _, p in neg])
    got, in_first, in_count = device_verify(gpu, *batch)
    assert got.tolist() == want, [w for (w, _, _), a, b in zip(neg, got, want) if a != b]
    twin = rc.host_verify(*batch)
    assert (in_first == twin[1]).all() and (in_count == twin[2]).all() and all(v == 1 or (a == 0 and n == 0) for v, a, n in zip(got, in_first, in_count))
    beyond = list(batch)
    beyond[0] = batch[0] + np.uint32(len(neg))                                                      # every tree outside the table
    assert not device_verify(gpu, *beyond)[0].any()
    bent = list(batch)
    bent[4] = batch[4].copy()
    bent[4][3] = bent[4][4] + np.uint64(1)                                                          # leaf_starts that is no prefix: nothing is proven
    assert not device_verify(gpu, *bent)[0].any()


def test_sort_ranges_and_verify_chained_on_one_stream(gpu, cases):
    f, trees, lo, hi, expected = cases[:5]
    rng = np.random.default_rng(732)
    shuffled = np.concatenate([t[rng.permutation(len(t))] for t in f.trees])
    forest, _ = gpu.build_sorted_forest(shuffled, f.counts)
    assert (forest.roots() == f.roots).all()
    stream = gpu.new_stream()
    Q, stride, n = len(trees), forest.levels, int(expected[6][1])
    with gpu.scope() as tmp:
        d_trees, d_lo, d_hi, d_counts = tmp.upload(trees), tmp.upload(lo), tmp.upload(hi), tmp.upload(np.array(f.counts, dtype=np.uint64))
        d_first, d_starts, d_leaves, d_left, d_right, d_h, d_info = (tmp.alloc(b) for b in (8 * Q, 8 * (Q + 1), 32 * n, 32 * Q * stride, 32 * Q * stride, 4 * Q, 32))
        d_verdict, d_in_first, d_in_count = tmp.alloc(4 * Q), tmp.alloc(8 * Q), tmp.alloc(8 * Q)
        forest.range_async(d_trees, d_lo, d_hi, Q, stride, tmp.alloc(gpu.range_scratch_bytes(0, Q)), d_first, d_starts, d_leaves, n, d_left, d_right, d_h,
                           d_info, stream=stream)
        gpu.verify_forest_range_enqueue(d_trees, d_lo, d_hi, d_first, d_starts, d_leaves, n, d_left, d_right, d_h, Q, stride, forest.roots_buf, d_counts,
                                        forest.ntrees, tmp.alloc(gpu.range_scratch_bytes(n, Q)), d_verdict, d_in_first, d_in_count, stream=stream)
        gpu.sync(stream)                                                                           # nothing read in between
        assert gpu.download(d_info, 32, dtype=np.uint64).tolist() == expected[6].tolist()
        assert (gpu.download(d_verdict, 4 * Q) == expected[7]).all() and (gpu.download(d_in_count, 8 * Q, dtype=np.uint64) == expected[9]).all()
        assert (gpu.download(d_in_first, 8 * Q, dtype=np.uint64) == expected[8]).all() and (gpu.download(d_leaves, 32 * n).reshape(n, 8) == expected[2]).all()
    forest.free()


def test_behind_inserted_and_removed(gpu):
    f = rc.forest()
    rng = np.random.default_rng(733)
    forest = gpu.build_forest(np.concatenate(f.trees), f.counts)
    counts = [3 if c else 0 for c in f.counts]
    batch = random_leaves(rng, sum(counts))
    more, info = forest.inserted(batch, counts)
    at, grown = 0, []
    for t, n in enumerate(counts):
        grown.append(rc.sorted_rows(np.concatenate([f.trees[t], batch[at: at + n]])) if n else f.trees[t])
        at += n
    t, leaves = 11, grown[11]
    lo, hi = rc.from_int(rc.as_int(leaves[200]) - 1), rc.from_int(rc.as_int(leaves[700]) + 1)
    p = more.ranges([t, 9], np.stack([lo, rc.ZERO]), np.stack([hi, rc.ONES]))
    verdict, in_first, in_count = p.verify(gpu, more.roots(), more.counts)
    assert verdict.tolist() == [1, 1] and in_first.tolist() == [200, 0] and in_count.tolist() == [501, 260]
    assert (p.in_range(0) == leaves[200:701]).all() and (p.in_range(1) == grown[9]).all()
    assert p.verify(gpu, forest.roots(), forest.counts)[0].tolist() == [0, 0]                      # not under the roots from before
    gone = leaves[300:400]
    drop = [len(gone) if j == t else 0 for j in range(f.ntrees)]
    less, info = more.removed(gone, drop)
    q = less.ranges([t], lo.reshape(1, 8), hi.reshape(1, 8))
    verdict, in_first, in_count = q.verify(gpu, less.roots(), less.counts)
    assert verdict.tolist() == [1] and in_count.tolist() == [401] and (q.in_range(0) == np.concatenate([leaves[200:300], leaves[400:701]])).all()
    for x in (less, more, forest):
        x.free()


def test_a_set_synced_in_four_chunks_from_a_source_that_is_not_trusted(gpu):
    """The four quarters of the digest space by the top two bits of word 0, each proven complete; the leaves in range, put together,
    are the source's tree."""
    f = rc.forest()
    forest = gpu.build_forest(np.concatenate(f.trees), f.counts)
    roots, counts = forest.roots(), forest.counts                                                  # what the replica holds
    lo, hi = np.zeros((4, 8), np.uint32), np.full((4, 8), 0xFFFFFFFF, np.uint32)
    lo[:, 0] = [k << 30 for k in range(4)]
    hi[:, 0] = [((k + 1) << 30) - 1 for k in range(4)]
    proofs = forest.ranges([12] * 4, lo, hi)
    verdict, in_first, in_count = proofs.verify(gpu, roots, counts)
    assert verdict.tolist() == [1] * 4 and int(in_count.sum()) == 2500 and in_first.tolist() == [0] + np.cumsum(in_count)[:3].tolist()
    synced = np.concatenate([proofs.in_range(q) for q in range(4)])
    assert synced.shape == (2500, 8)
    replica = gpu.build_forest(synced, [2500])
    assert (replica.roots()[0] == roots[12]).all()
    replica.free()
    forest.free()


def test_the_one_tree_twins(gpu):
    import vk_merkle_roots_amd as vk
    f = rc.forest()
    what, trees, lo, hi = f.queries()
    expected = f.expected()
    for t in (1, 5, 8, 11):
        leaves, c, h = f.trees[t], f.counts[t], rc.height(f.counts[t])
        mine = np.nonzero(trees == t)[0]
        Q = len(mine)
        d_leaves = gpu.upload(leaves)
        tree = gpu.build_tree(d_leaves, c)
        proofs = tree.range(lo[mine], hi[mine])
        runs = np.concatenate([expected[2][int(expected[1][q]): int(expected[1][q + 1])] for q in mine])
        starts = np.concatenate([[0], np.cumsum([int(expected[1][q + 1] - expected[1][q]) for q in mine])]).astype(np.uint64)
        want = vk.RangeProofs(np.zeros(Q, np.uint32), lo[mine], hi[mine], expected[0][mine], starts, runs, expected[3][mine][:, :h], expected[4][mine][:, :h],
                              np.full(Q, h, np.uint32))
        assert proofs.same_as(want)
        got = proofs.verify(gpu, f.roots[t: t + 1], [c])
        assert (got[0] == expected[7][mine]).all() and (got[1] == expected[8][mine]).all() and (got[2] == expected[9][mine]).all()
        n = int(runs.shape[0])
        with gpu.scope() as tmp:                                                                     # the twin's own check: one root, one count
            d_verdict, d_first, d_count = guarded(tmp, Q, rc.CANARY, np.uint32), guarded(tmp, Q, rc.INDEX_FILL, np.uint64), guarded(tmp, Q, rc.INDEX_FILL, np.uint64)
            gpu.verify_range_enqueue(tmp.upload(proofs.lo), tmp.upload(proofs.hi), tmp.upload(proofs.firsts), tmp.upload(proofs.leaf_starts),
                                     tmp.upload(proofs.leaves), n, tmp.upload(proofs.left), tmp.upload(proofs.right), Q, h, tmp.upload(tree.root()), c,
                                     tmp.alloc(gpu.range_scratch_bytes(n, Q)), at(d_verdict, np.uint32), at(d_first, np.uint64), at(d_count, np.uint64))
            assert (inner(gpu, d_verdict, Q, rc.CANARY, np.uint32)[:, 0] == expected[7][mine]).all()
            assert (inner(gpu, d_count, Q, rc.INDEX_FILL, np.uint64)[:, 0] == expected[9][mine]).all()
        tree.free()
        d_leaves.free()


def test_the_forest_and_the_outputs_above_4_gib(gpu, native):
    """The forest's leaves and the carried leaves at cell 2^27 + 5 of large, untouched buffers: every cell index and byte offset of
    theirs needs more than 32 bits."""
    import vk_merkle_roots_amd as vk
    f = rc.forest()
    what, trees, lo, hi = f.queries()
    expected = f.expected()
    n, Q, ntrees = int(expected[6][1]), len(trees), f.ntrees
    D = hc.LINE + 5
    total = D + f.total + 20
    bufs = []
    try:
        d_digests = hc.alloc(gpu, 32 * (total + hc.FENCE), "the leaves")
        bufs.append(d_digests)
        d_forest = hc.alloc(gpu, gpu.forest_tree_bytes(total, ntrees, 2500), "the stored levels")
        bufs.append(d_forest)
        d_out = hc.alloc(gpu, 32 * (D + n + hc.FENCE), "the carried leaves")
        bufs.append(d_out)
        hc.put(gpu, d_digests, 32 * D, np.concatenate(f.trees))
        canaries = [hc.write_canary(gpu, d_out, 0, hc.HEAD), hc.write_canary(gpu, d_out, D - hc.FENCE, hc.FENCE), hc.write_canary(gpu, d_out, D + n, hc.FENCE),
                    hc.write_canary(gpu, d_digests, 0, hc.HEAD), hc.write_canary(gpu, d_digests, D - hc.FENCE, hc.FENCE)]
        d_off, d_roots, d_status = gpu.upload(f.offsets0 + np.uint64(D)), gpu.alloc(32 * ntrees), gpu.upload(np.zeros(1, np.uint32))
        bufs += [d_off, d_roots, d_status]
        gpu.reduce_forest_tree_async(d_digests, total, d_off, ntrees, 2500, d_forest, d_roots, d_status)
        assert int(gpu.download(d_status, 4)[0]) == 0
        forest = vk.MerkleForest(gpu, d_digests, total, f.counts, d_off, 2500, d_forest, d_roots)
        assert (forest.roots() == f.roots).all()
        with gpu.scope() as tmp:
            d_trees, d_lo, d_hi, d_counts = tmp.upload(trees), tmp.upload(lo), tmp.upload(hi), tmp.upload(np.array(f.counts, dtype=np.uint64))
            d_first, d_starts, d_left, d_right, d_h, d_info = (tmp.alloc(b) for b in (8 * Q, 8 * (Q + 1), 32 * Q * 12, 32 * Q * 12, 4 * Q, 32))
            d_verdict, d_in_first, d_in_count = tmp.alloc(4 * Q), tmp.alloc(8 * Q), tmp.alloc(8 * Q)
            forest.range_async(d_trees, d_lo, d_hi, Q, 12, tmp.alloc(gpu.range_scratch_bytes(0, Q)), d_first, d_starts, At(d_out, 32 * D), n, d_left, d_right, d_h,
                               d_info)
            gpu.verify_forest_range_enqueue(d_trees, d_lo, d_hi, d_first, d_starts, At(d_out, 32 * D), n, d_left, d_right, d_h, Q, 12, d_roots, d_counts, ntrees,
                                            tmp.alloc(gpu.range_scratch_bytes(n, Q)), d_verdict, d_in_first, d_in_count)
            assert gpu.download(d_info, 32, dtype=np.uint64).tolist() == expected[6].tolist()
            assert (gpu.download(d_first, 8 * Q, dtype=np.uint64) == expected[0]).all() and (gpu.download(d_starts, 8 * (Q + 1), dtype=np.uint64) == expected[1]).all()
            assert (gpu.download(d_left, 32 * Q * 12).reshape(Q, 12, 8) == expected[3]).all() and (gpu.download(d_right, 32 * Q * 12).reshape(Q, 12, 8) == expected[4]).all()
            assert (gpu.download(d_verdict, 4 * Q) == expected[7]).all() and (gpu.download(d_in_count, 8 * Q, dtype=np.uint64) == expected[9]).all()
        assert (hc.read_cells(gpu, d_out, D + np.arange(n)) == expected[2]).all()
        assert hc.canaries_intact(gpu, canaries)
    finally:
        for b in bufs:
            b.free()
