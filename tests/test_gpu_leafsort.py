"""The leaf sort on the GPU (vkmr_hip_forest_sort_leaves_async, vkmr_hip_tree_sort_leaves_async through HipDevice,
build_sorted_forest, vk.sorted_forest_packed): cell for cell what the CPU twins and the model of tests/leafsort_cases.py give on
every case, between guard words, the cells outside the trees untouched; the status refusals, which write nothing; the batch of
exactly MAX_TIES leaves in one run; sort -> build -> sortedness pass chained on one stream; the handles; a payload that follows
the leaves; and one placement above 4 GiB."""
import numpy as np
import pytest

import absence_cases as ac
import high_cases as hc
import leafsort_cases as lc
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


def device_sort(gpu, cells, offsets, max_count, with_order=True, one_tree=False):
    """(out [total, 8], order [total], info [4]) of one raw call, every output between guards and the canary before the call; the
    input must be what it was."""
    cells = np.ascontiguousarray(cells, dtype=np.uint32).reshape(-1, 8)
    total, ntrees = int(cells.shape[0]), len(offsets) - 1
    with gpu.scope() as tmp:
        d_in = tmp.upload(cells)
        d_out, d_order, d_info = guarded(tmp, total, lc.CANARY, np.uint32, 8), guarded(tmp, total, lc.CANARY, np.uint32), guarded(tmp, 4, lc.INFO_FILL, np.uint64)
        d_scratch = tmp.alloc(gpu.sort_leaves_scratch_bytes(total))
        order_at = at(d_order, np.uint32) if with_order else None
        if one_tree:
            gpu.tree_sort_leaves_enqueue(d_in, total, d_scratch, at(d_out, np.uint32, 8), order_at, at(d_info, np.uint64))
        else:
            gpu.forest_sort_leaves_enqueue(d_in, total, tmp.upload(np.ascontiguousarray(offsets, dtype=np.uint64)), ntrees, max_count, d_scratch,
                                           at(d_out, np.uint32, 8), order_at, at(d_info, np.uint64))
        gpu.sync()
        assert (gpu.download(d_in, 32 * total).reshape(total, 8) == cells).all()
        return (inner(gpu, d_out, total, lc.CANARY, np.uint32, 8), inner(gpu, d_order, total, lc.CANARY, np.uint32)[:, 0],
                inner(gpu, d_info, 4, lc.INFO_FILL, np.uint64)[:, 0])


def same(got, want, note):
    for what, a, b in zip(("leaves", "order", "info"), got, want):
        assert a.shape == b.shape and (a == b).all(), (note, what, np.nonzero((a != b).reshape(a.shape[0], -1).any(axis=1))[0][:8], a[:4] if what == "info" else "")


@pytest.fixture(scope="module")
def twins(native):
    """What the CPU twin gives for every case, computed once; the model agrees with it in tests/test_leafsort_abi.py."""
    out = {}
    for c in lc.all_cases():
        rc, *got = lc.host_sort(c.cells, c.offsets, c.max_count)
        assert rc == 0
        out[c.name] = got
    return out


@pytest.mark.parametrize("case", lc.all_cases(), ids=[c.name for c in lc.all_cases()])
def test_the_device_is_the_cpu_twin_cell_for_cell(gpu, twins, case):
    got = device_sort(gpu, case.cells, case.offsets, case.max_count)
    same(got, twins[case.name], case.name)                   # the cells outside [offsets[0], offsets[ntrees]) are the canary in both
    assert int(got[2][0]) == 0 and int(got[2][1]) == int(case.offsets[-1]) - int(case.offsets[0])


def test_the_exact_and_the_wide_max_count_and_no_order(gpu, twins):
    exact, wide = lc.forest_cases()[1], [c for c in lc.shape_cases() if c.name.startswith("max_count")][0]
    a, b = device_sort(gpu, exact.cells, exact.offsets, exact.max_count), device_sort(gpu, wide.cells, wide.offsets, wide.max_count)
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all() and a[2][[0, 1, 3]].tolist() == b[2][[0, 1, 3]].tolist() and b[2][2] <= a[2][2]
    out, order, info = device_sort(gpu, exact.cells, exact.offsets, exact.max_count, with_order=False)
    assert (out == a[0]).all() and (order == lc.CANARY).all() and (info == a[2]).all()


def test_the_one_tree_twin(gpu):
    rng = np.random.default_rng(711)
    for n in (1, 2, 1500):
        rows = random_leaves(rng, n)
        if n > 100:
            rows[100:140, :7] = rows[7, :7]                  # a run of 41 under one prefix, in no order below
            rows[1499] = rows[0]
        rc, *want = lc.host_tree_sort(rows)
        assert rc == 0
        same(device_sort(gpu, rows, [0, n], n, one_tree=True), want, ("one tree", n))
        same(device_sort(gpu, rows, [0, n], n), want, ("a forest of one tree", n))


def test_the_status_refusals_write_nothing(gpu):
    exact = lc.forest_cases()[1]
    down = exact.offsets.copy()
    down[5] = down[4] - 1
    behind = exact.offsets.copy()
    behind[-1] = exact.cells.shape[0] + 1
    for what, offsets, max_count, status, n in (("the offsets decrease", down, 2500, 1, 0), ("the offsets end behind the cells", behind, 5000, 1, 0),
                                                ("a tree above max_count", exact.offsets, 2499, 2, 5933), ("both", behind, 2500, 3, 0)):
        out, order, info = device_sort(gpu, exact.cells, offsets, max_count)
        assert info.tolist() == [status, n, 0, 0] and (out == lc.CANARY).all() and (order == lc.CANARY).all(), what
    c = lc.tie_batch(1)
    n = lc.max_ties() + 1
    for one_tree in (False, True):
        out, order, info = device_sort(gpu, c.cells, c.offsets, c.max_count, one_tree=one_tree)
        assert info.tolist() == [lc.TOO_MANY_TIES, n, n, 0] and (out == lc.CANARY).all() and (order == lc.CANARY).all()


def test_the_batch_of_max_ties_in_one_run_sorts(gpu, native):
    c = lc.tie_batch(0)
    rc, *want = lc.host_sort(c.cells, c.offsets, c.max_count)
    assert rc == 0 and want[2].tolist() == [0, lc.max_ties(), lc.max_ties(), 1]
    same(device_sort(gpu, c.cells, c.offsets, c.max_count), want, "MAX_TIES")


def test_no_tree_and_no_cell(gpu):
    gpu.forest_sort_leaves_enqueue(None, 0, None, 0, 0, None, None, None, None)                    # no tree: nothing is done, no buffer is needed
    with gpu.scope() as tmp:
        d_info = guarded(tmp, 4, lc.INFO_FILL, np.uint64)
        gpu.forest_sort_leaves_enqueue(None, 0, tmp.upload(np.zeros(4, np.uint64)), 3, 1, None, None, None, at(d_info, np.uint64))
        assert inner(gpu, d_info, 4, lc.INFO_FILL, np.uint64)[:, 0].tolist() == [0, 0, 0, 0]
        gpu.forest_sort_leaves_enqueue(None, 0, tmp.upload(np.array([0, 0, 2, 2], np.uint64)), 3, 5, None, None, None, at(d_info, np.uint64))
        assert inner(gpu, d_info, 4, lc.INFO_FILL, np.uint64)[:, 0].tolist() == [1, 0, 0, 0]          # leaves, and no cell to hold them
        gpu.tree_sort_leaves_enqueue(None, 0, None, None, None, at(d_info, np.uint64))
        assert inner(gpu, d_info, 4, lc.INFO_FILL, np.uint64)[:, 0].tolist() == [0, 0, 0, 0]


def test_sort_build_and_the_sortedness_pass_chained_on_one_stream(gpu):
    import vk_merkle_roots_amd as vk
    rng = np.random.default_rng(712)
    counts = [5, 0, 64, 1, 300, 1025]
    trees = [random_leaves(rng, c) for c in counts]
    cells, offsets = lc.lay(trees)
    total, ntrees, max_count = int(cells.shape[0]), len(counts), 1025
    stream = gpu.new_stream()
    d_in, d_off = gpu.upload(cells), gpu.upload(offsets)
    d_out, d_forest, d_roots = gpu.alloc(32 * total), gpu.alloc(gpu.forest_tree_bytes(total, ntrees, max_count)), gpu.alloc(32 * ntrees)
    with gpu.scope() as tmp:
        d_scratch, d_order, d_info, d_status = tmp.alloc(gpu.sort_leaves_scratch_bytes(total)), tmp.alloc(4 * total), tmp.alloc(32), tmp.alloc(4)
        d_bad, d_sorted = tmp.alloc(8 * ntrees), tmp.alloc(32)
        gpu.forest_sort_leaves_enqueue(d_in, total, d_off, ntrees, max_count, d_scratch, d_out, d_order, d_info, stream=stream)
        gpu.reduce_forest_tree_async(d_out, total, d_off, ntrees, max_count, d_forest, d_roots, d_status, stream=stream)     # nothing read in between
        gpu.forest_sorted_enqueue(d_out, total, d_off, ntrees, d_bad, d_sorted, stream=stream)
        gpu.sync(stream)
        assert gpu.download(d_info, 32, dtype=np.uint64).tolist()[:2] == [0, total] and int(gpu.download(d_status, 4)[0]) == 0
        assert gpu.download(d_sorted, 32, dtype=np.uint64).tolist() == [0, 0, 0, total - 5]
        assert (gpu.download(d_bad, 8 * ntrees, dtype=np.uint64) == ac.NONE).all()
        order = gpu.download(d_order, 4 * total)
    d_in.free()
    forest = vk.MerkleForest(gpu, d_out, total, counts, d_off, max_count, d_forest, d_roots, owned=[d_out])
    try:
        want = [ac.sorted_rows(t) if len(t) else t for t in trees]
        assert forest.is_sorted() and (gpu.download(d_out, 32 * total).reshape(total, 8) == np.concatenate(want)).all()
        assert (cells[order] == np.concatenate(want)).all()
        roots = np.stack([cpu_levels(t)[-1][0] if len(t) else ac.ZERO for t in want])
        assert (forest.roots() == roots).all()
        t = 4                                                # a digest between two leaves of the tree of 300, and one that is a leaf
        gap = ac.from_int((ac.as_int(want[t][100]) + ac.as_int(want[t][101])) // 2)
        proofs = forest.absence([t, t], np.stack([gap, want[t][200]]))
        assert proofs.indices.tolist() == [101, 200] and proofs.verify(gpu, roots, counts).tolist() == [ac.ABSENT, ac.PRESENT]
    finally:
        forest.free()


def test_build_sorted_forest(gpu, twins):
    import vk_merkle_roots_amd as vk
    case = lc.forest_cases()[0]
    counts = lc.COUNTS
    want_leaves, want_order, _ = twins[case.name]
    forest, order = gpu.build_sorted_forest(case.cells, counts)
    plain = gpu.build_forest(want_leaves, counts)
    try:
        assert forest.total == 5933 and forest.max_count == 2500 and (order == want_order).all()
        assert (gpu.download(forest.digests, 32 * 5933).reshape(-1, 8) == want_leaves).all() and (forest.roots() == plain.roots()).all()
        bad = forest.first_unsorted()                        # the three equal leaves and the two all-ones leaves: sorted, and not strictly
        assert not forest.is_sorted() and set(np.nonzero(bad != ac.NONE)[0].tolist()) == {13, 17} and int(bad[17]) == 2499
        assert forest.audit().n_bad == 0
    finally:
        forest.free()
        plain.free()
    # room to grow, and the sort's own answers through the host-array call
    roomy, order2 = gpu.build_sorted_forest(case.cells, counts, max_count=4096, reserve_trees=2, reserve_leaves=50)
    try:
        assert roomy.total == 5983 and roomy.ntrees == len(counts) + 2 and roomy.used_trees == len(counts) and (order2 == want_order).all()
        assert (roomy.roots()[: len(counts)] == plain_roots(gpu, want_leaves, counts)).all()
        more = random_leaves(np.random.default_rng(713), 50)
        roomy.append(more, [20, 30])
        assert (roomy.roots()[len(counts):] == plain_roots(gpu, more, [20, 30])).all()
    finally:
        roomy.free()
    got = gpu.sort_leaves(case.cells, counts)
    same(got, (want_leaves, want_order, twins[case.name][2]), "sort_leaves")
    c = lc.tie_batch(1)
    with pytest.raises(RuntimeError, match=rf"{lc.max_ties() + 1} leaves tie.*{lc.max_ties()}.*sort_digests"):
        gpu.sort_leaves(c.cells, [c.cells.shape[0]])
    with pytest.raises(RuntimeError, match="max_count"):
        gpu.sort_leaves(case.cells, counts, max_count=100)
    assert (vk.sort_digests(c.cells, [c.cells.shape[0]]) == lc.host_tree_sort(c.cells)[1]).all()       # where such a batch goes


def plain_roots(gpu, leaves, counts):
    return gpu.forest_roots(leaves, counts)


def test_sorted_forest_packed(gpu):
    import vk_merkle_roots_amd as vk
    batch = vk.rndm_packed(20261021, 300, 40)
    counts = [100, 0, 199, 1]
    digests = gpu.leaf_digests(batch)
    want = vk.sort_digests(digests, counts)
    forest, order = vk.sorted_forest_packed(gpu, batch, counts)
    try:
        assert (gpu.download(forest.digests, 32 * 300).reshape(-1, 8) == want).all() and (digests[order] == want).all()
        assert forest.is_sorted() and (forest.roots() == plain_roots(gpu, want, counts)).all()
        found = forest.find(digests[[7, 150]])
        assert found[0].tolist() == [0, 2] and (want[[int(found[1][0]), 100 + int(found[1][1])]] == digests[[7, 150]]).all()
    finally:
        forest.free()
    roomy, order2 = vk.sorted_forest_packed(gpu, batch, counts, max_count=256, reserve_trees=1, reserve_leaves=10)
    try:
        assert roomy.total == 310 and (order2 == order).all() and (roomy.roots()[:4] == plain_roots(gpu, want, counts)).all()
    finally:
        roomy.free()


def test_a_payload_follows_the_leaves(gpu, twins):
    case = lc.forest_cases()[1]
    lo, hi, total = int(case.offsets[0]), int(case.offsets[-1]), int(case.cells.shape[0])
    payload = random_leaves(np.random.default_rng(714), total)                                     # a value beside every cell of the input
    with gpu.scope() as tmp:
        d_out, d_order, d_info = tmp.alloc(32 * total), tmp.alloc(4 * total), tmp.alloc(32)
        gpu.forest_sort_leaves_enqueue(tmp.upload(case.cells), total, tmp.upload(case.offsets), len(case.offsets) - 1, case.max_count,
                                       tmp.alloc(gpu.sort_leaves_scratch_bytes(total)), d_out, d_order, d_info)
        d_dst = guarded(tmp, hi - lo, lc.CANARY, np.uint32, 8)
        gpu.gather_digests_async(tmp.upload(payload), At(d_order, 4 * lo), hi - lo, at(d_dst, np.uint32, 8))     # order_out + offsets[0], n cells
        got = inner(gpu, d_dst, hi - lo, lc.CANARY, np.uint32, 8)
    assert (got == payload[twins[case.name][1][lo: hi]]).all()


def test_a_forest_above_4_gib(gpu, native):
    """A small forest at offsets[0] = 2^27 + 5 of large, untouched buffers: every cell index and byte offset of the leaves needs
    more than 32 bits.  The sort runs over `total` elements, nearly all of them sentinels; that is the design."""
    rng = np.random.default_rng(715)
    trees = [random_leaves(rng, c) for c in (3, 0, 130, 1025)]
    trees[3][1000:1020, :7] = trees[3][5, :7]                # a run that the place step walks, up there
    local, local_offsets = lc.lay(trees, 0, 20)
    rc, want_out, want_order, want_info = lc.host_sort(local, local_offsets, 1025)
    assert rc == 0 and int(want_info[2]) >= 21
    n, D = int(local_offsets[-1]), hc.LINE + 5
    total = D + n + 20
    bufs = []
    try:
        d_in, d_out = hc.alloc(gpu, 32 * (total + hc.FENCE), "the leaves"), hc.alloc(gpu, 32 * (total + hc.FENCE), "the sorted leaves")
        bufs += [d_in, d_out]
        d_order, d_scratch = hc.alloc(gpu, 4 * (total + hc.FENCE), "the order"), hc.alloc(gpu, gpu.sort_leaves_scratch_bytes(total), "the scratch")
        bufs += [d_order, d_scratch]
        hc.put(gpu, d_in, 32 * D, local)
        # a store that lost its upper bits lands at cell (D + j) mod 2^27 = 5 + j of the same buffer
        canaries = [hc.write_canary(gpu, d_out, 0, hc.HEAD), hc.write_canary(gpu, d_out, D - hc.FENCE, hc.FENCE), hc.write_canary(gpu, d_out, D + n, 20 + hc.FENCE),
                    hc.write_canary(gpu, d_order, 0, hc.HEAD, 1), hc.write_canary(gpu, d_order, D - hc.FENCE, hc.FENCE, 1),
                    hc.write_canary(gpu, d_order, D + n, 20 + hc.FENCE, 1), hc.write_canary(gpu, d_in, 0, hc.HEAD)]
        with gpu.scope() as tmp:
            d_info = tmp.upload(np.full(4, lc.INFO_FILL, np.uint64))
            gpu.forest_sort_leaves_enqueue(d_in, total, tmp.upload(local_offsets + np.uint64(D)), 4, 1025, d_scratch, d_out, d_order, d_info)
            assert gpu.download(d_info, 32, dtype=np.uint64).tolist() == want_info.tolist()
        assert (hc.read_cells(gpu, d_out, D + np.arange(n)) == want_out[:n]).all()
        assert (hc.read_cells(gpu, d_order, D + np.arange(n), 1)[:, 0].astype(np.int64) == want_order[:n].astype(np.int64) + D).all()
        assert (hc.read_cells(gpu, d_in, D + np.arange(n + 20)) == local).all()
        assert hc.canaries_intact(gpu, canaries)
    finally:
        for b in bufs:
            b.free()
