"""The merge of sorted forests on the GPU (vkmr_hip_forest_merge_leaves_async, vkmr_hip_tree_merge_leaves_async through HipDevice,
MerkleForest / MerkleTree.inserted, removed, common): cell for cell what the CPU twins give on every case and op of
tests/merge_cases.py, between guard words, the cells behind n_out untouched; every status bit, which writes nothing, and a short
output that reports the true n_out; no origin wanted; sort -> merge -> build -> sortedness pass chained on one stream with no host
step; the stored forests and trees that come out; the dedup of a batch; and one placement above 4 GiB."""
import time

import numpy as np
import pytest

import absence_cases as ac
import high_cases as hc
import merge_cases as mc
from merkle_model import At, cpu_levels, random_leaves

pytestmark = pytest.mark.gpu

GUARD = 4                                                    # guard cells on either side of every output
CELLS = [(c, op) for c in mc.all_cases() for op in mc.OPS]
CELL_IDS = [f"{c.name}: {mc.OP_NAMES[op]}" for c, op in CELLS]


def guarded(tmp, n, fill, dtype, width=1):
    return tmp.upload(np.full((n + 2 * GUARD) * width, fill, dtype))


def inner(gpu, buf, n, fill, dtype, width=1):
    """The n items between the guards, which must still be the fill."""
    got = gpu.download(buf, (n + 2 * GUARD) * width * np.dtype(dtype).itemsize, dtype=dtype).reshape(n + 2 * GUARD, width)
    assert (got[:GUARD] == fill).all() and (got[-GUARD:] == fill).all()
    return got[GUARD:-GUARD]


def at(buf, dtype, width=1):
    return At(buf, GUARD * width * np.dtype(dtype).itemsize)


def device_merge(gpu, case, op, capacity=None, with_origin=True, one_tree=False):
    """(out [capacity, 8], out_offsets [ntrees + 1], origin [capacity], info [4]) of one raw call, every output between guards and
    the canary before the call; the inputs must be what they were."""
    a, b = np.ascontiguousarray(case.a_cells, dtype=np.uint32).reshape(-1, 8), np.ascontiguousarray(case.b_cells, dtype=np.uint32).reshape(-1, 8)
    na, nb, ntrees = int(a.shape[0]), int(b.shape[0]), len(case.a_offsets) - 1
    capacity = mc.default_capacity(case, op) if capacity is None else capacity
    with gpu.scope() as tmp:
        d_a, d_b = (tmp.upload(a) if na else None), (tmp.upload(b) if nb else None)
        d_out, d_origin = guarded(tmp, capacity, mc.CANARY, np.uint32, 8), guarded(tmp, capacity, mc.OFFSET_FILL, np.uint64)
        d_off, d_info = guarded(tmp, ntrees + 1, mc.OFFSET_FILL, np.uint64), guarded(tmp, 4, mc.INFO_FILL, np.uint64)
        d_scratch = tmp.alloc(gpu.merge_leaves_scratch_bytes(na, nb, ntrees))
        origin_at = at(d_origin, np.uint64) if with_origin else None
        if one_tree:
            gpu.tree_merge_leaves_enqueue(d_a, na, d_b, nb, op, d_scratch, at(d_out, np.uint32, 8), capacity, origin_at, at(d_info, np.uint64))
        else:
            gpu.forest_merge_leaves_enqueue(d_a, na, tmp.upload(np.ascontiguousarray(case.a_offsets, dtype=np.uint64)), d_b, nb,
                                            tmp.upload(np.ascontiguousarray(case.b_offsets, dtype=np.uint64)), ntrees, op, d_scratch, at(d_out, np.uint32, 8),
                                            capacity, at(d_off, np.uint64), origin_at, at(d_info, np.uint64))
        gpu.sync()
        assert (na == 0 or (gpu.download(d_a, 32 * na).reshape(na, 8) == a).all()) and (nb == 0 or (gpu.download(d_b, 32 * nb).reshape(nb, 8) == b).all())
        return (inner(gpu, d_out, capacity, mc.CANARY, np.uint32, 8), inner(gpu, d_off, ntrees + 1, mc.OFFSET_FILL, np.uint64)[:, 0],
                inner(gpu, d_origin, capacity, mc.OFFSET_FILL, np.uint64)[:, 0], inner(gpu, d_info, 4, mc.INFO_FILL, np.uint64)[:, 0])


def same(got, want, note):
    for what, a, b in zip(("leaves", "offsets", "origin", "info"), got, want):
        assert a.shape == b.shape and (a == b).all(), (note, what, np.nonzero((a != b).reshape(a.shape[0], -1).any(axis=1))[0][:8], a[:4] if what == "info" else "")


@pytest.fixture(scope="module")
def twins(native):
    """What the CPU twin gives for every case and op, computed once; the model agrees with it in tests/test_merge_abi.py."""
    out = {}
    for c, op in CELLS:
        rc, *got = mc.host_merge(c, op)
        assert rc == 0
        out[c.name, op] = got
    return out


@pytest.mark.parametrize("case,op", CELLS, ids=CELL_IDS)
def test_the_device_is_the_cpu_twin_cell_for_cell(gpu, twins, case, op):
    want = twins[case.name, op]
    got = device_merge(gpu, case, op)
    same(got, want, case.name)                               # the cells at and behind n_out hold the canary in both
    na, nb = int(case.a_offsets[-1] - case.a_offsets[0]), int(case.b_offsets[-1] - case.b_offsets[0])
    status, n_out, matches, repeats = (int(x) for x in got[3])
    assert status == 0 and n_out == mc.n_out_of_counts(op, na, nb, matches, repeats) and int(got[1][0]) == 0 and int(got[1][-1]) == n_out
    if mc.is_one_tree(case):
        out, offsets, origin, info = device_merge(gpu, case, op, one_tree=True)
        assert (offsets == mc.OFFSET_FILL).all()
        same((out, origin, info), (want[0], want[2], want[3]), ("the one-tree twin", case.name))


def test_no_origin_and_room_behind(gpu, twins):
    case = mc.forest_cases()[1]
    for op in mc.OPS:
        want = twins[case.name, op]
        n = int(want[3][1])
        out, offsets, origin, info = device_merge(gpu, case, op, capacity=n + 9, with_origin=False)
        assert (info == want[3]).all() and (offsets == want[1]).all() and (out[:n] == want[0][:n]).all() and (out[n:] == mc.CANARY).all()
        assert (origin == mc.OFFSET_FILL).all()


@pytest.mark.parametrize("name", mc.REFUSALS)
def test_every_status_bit_writes_nothing(gpu, native, name):
    case, capacity, status, n_out = mc.refusal(name)
    for op in mc.OPS:
        full = mc.host_merge(case, op)[1:]
        cap = mc.default_capacity(case, op) if capacity is None else capacity
        if capacity == -1:                                   # one cell short
            cap = int(full[3][1]) - 1
            if cap < 0:
                continue
        rc, *want = mc.host_merge(case, op, capacity=cap)
        got = device_merge(gpu, case, op, capacity=cap)
        assert rc == 0 and int(got[3][0]) == status
        same(got, want, (name, op))
        assert (got[0] == mc.CANARY).all() and (got[1] == mc.OFFSET_FILL).all() and (got[2] == mc.OFFSET_FILL).all()
        if n_out is None:                                    # bit 4 reports the true n_out; the second call at that capacity succeeds
            assert got[3].tolist() == [16] + full[3].tolist()[1:]
            again = device_merge(gpu, case, op, capacity=int(got[3][1]))
            same(again, mc.host_merge(case, op, capacity=int(got[3][1]))[1:], (name, op, "again"))
            assert int(again[3][0]) == 0


def test_no_tree_and_no_cell(gpu):
    gpu.forest_merge_leaves_enqueue(None, 0, None, None, 0, None, 0, 0, None, None, 0, None, None, None)      # no tree: nothing is done, no buffer is needed
    zeros = np.zeros(4, np.uint64)
    with gpu.scope() as tmp:
        d_info, d_off = guarded(tmp, 4, mc.INFO_FILL, np.uint64), guarded(tmp, 4, mc.OFFSET_FILL, np.uint64)
        d_scratch = tmp.alloc(gpu.merge_leaves_scratch_bytes(0, 0, 3))
        for op in mc.OPS:
            gpu.forest_merge_leaves_enqueue(None, 0, tmp.upload(zeros), None, 0, tmp.upload(zeros), 3, op, d_scratch, None, 0, at(d_off, np.uint64), None,
                                            at(d_info, np.uint64))
            assert inner(gpu, d_info, 4, mc.INFO_FILL, np.uint64)[:, 0].tolist() == [0, 0, 0, 0]
            assert inner(gpu, d_off, 4, mc.OFFSET_FILL, np.uint64)[:, 0].tolist() == [0, 0, 0, 0]
        gpu.forest_merge_leaves_enqueue(None, 0, tmp.upload(np.array([0, 0, 2, 2], np.uint64)), None, 0, tmp.upload(zeros), 3, 0, d_scratch, None, 0,
                                        at(d_off, np.uint64), None, at(d_info, np.uint64))
        assert inner(gpu, d_info, 4, mc.INFO_FILL, np.uint64)[:, 0].tolist() == [1, 0, 0, 0]                      # leaves of A, and no cell to hold them
        gpu.tree_merge_leaves_enqueue(None, 0, None, 0, 0, d_scratch, None, 0, None, at(d_info, np.uint64))
        assert inner(gpu, d_info, 4, mc.INFO_FILL, np.uint64)[:, 0].tolist() == [0, 0, 0, 0]


def sorted_trees(rng, counts):
    return [ac.sorted_rows(random_leaves(rng, c)) if c else random_leaves(rng, 0) for c in counts]


def model_trees(a_trees, b_trees, op):
    out = []
    for a, b in zip(a_trees, b_trees):
        sa, sb = [mc.words(r) for r in a], {mc.words(r) for r in b}
        rows = sorted(set(sa) | sb) if op == 0 else [d for d in sa if (d in sb) == (op == 2)]
        out.append(mc.rows_of(rows))
    return out


def roots_of(trees):
    return np.stack([cpu_levels(t)[-1][0] if len(t) else ac.ZERO for t in trees])


def test_sort_merge_build_and_the_sortedness_pass_chained_on_one_stream(gpu):
    import vk_merkle_roots_amd as vk
    rng = np.random.default_rng(811)
    a_counts, b_counts = [5, 0, 64, 1, 300, 1025], [3, 2, 0, 1, 70, 200]
    a_trees = sorted_trees(rng, a_counts)
    b_trees = [random_leaves(rng, c) for c in b_counts]      # in no order
    b_trees[4][:10], b_trees[4][10:12] = a_trees[4][20:30], b_trees[4][40:42]     # ten that are leaves already, two that come twice
    b_trees[3][0] = a_trees[3][0]
    a_cells, a_off = mc.lay(a_trees)
    b_cells, b_off = mc.lay(b_trees)
    na, nb, ntrees = int(a_cells.shape[0]), int(b_cells.shape[0]), len(a_counts)
    cap, max_count = na + nb, 1025 + 200
    stream = gpu.new_stream()
    d_a, d_aoff, d_bin, d_boff = gpu.upload(a_cells), gpu.upload(a_off), gpu.upload(b_cells), gpu.upload(b_off)
    d_out, d_off = gpu.alloc(32 * cap), gpu.alloc(8 * (ntrees + 1))
    d_forest, d_roots = gpu.alloc(gpu.forest_tree_bytes(cap, ntrees, max_count)), gpu.alloc(32 * ntrees)
    with gpu.scope() as tmp:
        d_b, d_sort_info, d_info, d_status = tmp.alloc(32 * nb), tmp.alloc(32), tmp.alloc(32), tmp.alloc(4)
        d_bad, d_sorted = tmp.alloc(8 * ntrees), tmp.alloc(32)
        d_sort_scratch, d_scratch = tmp.alloc(gpu.sort_leaves_scratch_bytes(nb)), tmp.alloc(gpu.merge_leaves_scratch_bytes(na, nb, ntrees))
        gpu.forest_sort_leaves_enqueue(d_bin, nb, d_boff, ntrees, max(b_counts), d_sort_scratch, d_b, None, d_sort_info, stream=stream)
        gpu.forest_merge_leaves_enqueue(d_a, na, d_aoff, d_b, nb, d_boff, ntrees, 0, d_scratch, d_out, cap, d_off, None, d_info, stream=stream)
        gpu.reduce_forest_tree_async(d_out, cap, d_off, ntrees, max_count, d_forest, d_roots, d_status, stream=stream)     # nothing read in between
        gpu.forest_sorted_enqueue(d_out, cap, d_off, ntrees, d_bad, d_sorted, stream=stream)
        gpu.sync(stream)
        info = gpu.download(d_info, 32, dtype=np.uint64).tolist()
        assert gpu.download(d_sort_info, 32, dtype=np.uint64).tolist()[:2] == [0, nb] and int(gpu.download(d_status, 4)[0]) == 0
        assert info == [0, na + nb - 11 - 2, 11, 2]
        assert gpu.download(d_sorted, 32, dtype=np.uint64).tolist()[:3] == [0, 0, 0] and (gpu.download(d_bad, 8 * ntrees, dtype=np.uint64) == ac.NONE).all()
        offsets = gpu.download(d_off, 8 * (ntrees + 1), dtype=np.uint64)
    for b in (d_a, d_aoff, d_bin, d_boff):
        b.free()
    want = model_trees(a_trees, b_trees, 0)
    counts = np.diff(offsets)
    assert counts.tolist() == [len(t) for t in want]
    forest = vk.MerkleForest(gpu, d_out, cap, counts, d_off, max_count, d_forest, d_roots, owned=[d_out])
    try:
        roots = roots_of(want)
        assert forest.is_sorted() and (forest.roots() == roots).all()
        assert (gpu.download(d_out, 32 * info[1]).reshape(-1, 8) == np.concatenate(want)).all()
        t = 4                                                # an inserted digest, and one between two leaves that never was there
        inserted = b_trees[t][50]
        at_ = [mc.words(r) for r in want[t]].index(mc.words(inserted))
        gap = ac.from_int((ac.as_int(want[t][100]) + ac.as_int(want[t][101])) // 2)
        proofs = forest.absence([t, t], np.stack([inserted, gap]))
        assert proofs.indices.tolist() == [at_, 101] and proofs.verify(gpu, roots, counts).tolist() == [ac.PRESENT, ac.ABSENT]
    finally:
        forest.free()


def test_inserted_removed_and_common(gpu):
    rng = np.random.default_rng(812)
    a_counts, b_counts = [40, 0, 300, 7], [6, 3, 50, 0]
    a_trees = sorted_trees(rng, a_counts)
    b_trees = [random_leaves(rng, c) for c in b_counts]
    b_trees[2][:20], b_trees[2][20:23], b_trees[0][0] = a_trees[2][100:120], b_trees[2][30:33], a_trees[0][39]
    source = gpu.build_forest(np.concatenate(a_trees), a_counts)
    batch = np.concatenate(b_trees)
    made = []
    try:
        before = source.roots().copy()
        for method, op in ((source.inserted, 0), (source.removed, 1), (source.common, 2)):
            forest, info = method(batch, b_counts)
            made.append(forest)
            want = model_trees(a_trees, b_trees, op)
            n = sum(len(t) for t in want)
            assert info.tolist() == [0, n, 21, 3] and forest.counts.tolist() == [len(t) for t in want] and forest.used_trees == 4
            assert (forest.roots() == roots_of(want)).all() and forest.is_sorted() and forest.audit().clean
            assert n == 0 or (gpu.download(forest.digests, 32 * n).reshape(-1, 8) == np.concatenate(want)).all()
        assert (source.roots() == before).all() and source.counts.tolist() == a_counts               # the source is untouched
        # removed and inserted again: the original roots
        back, info = made[1].inserted(batch, b_counts)
        made.append(back)
        want = model_trees(model_trees(a_trees, b_trees, 1), b_trees, 0)
        assert (back.roots() == roots_of(want)).all() and info.tolist()[:2] == [0, sum(len(t) for t in want)]
        only_mine = [np.concatenate([a[:0]] + [r[None] for r in b if mc.words(r) in {mc.words(x) for x in a}]) for a, b in zip(a_trees, b_trees)]
        again, info = made[1].inserted(np.concatenate(only_mine), [len(t) for t in only_mine])       # what was removed, put back
        made.append(again)
        assert (again.roots() == before).all() and again.counts.tolist() == a_counts and info.tolist() == [0, sum(a_counts), 0, 0]
        # room to grow, a flagged build, a max_count that is too small
        roomy, info = source.inserted(batch, b_counts, max_count=512, reserve_trees=2, reserve_leaves=30, mutated=True)
        made.append(roomy)
        want = model_trees(a_trees, b_trees, 0)
        assert roomy.ntrees == 6 and roomy.used_trees == 4 and roomy.total == sum(a_counts) + sum(b_counts) + 30 and roomy.built_mutated.shape == (6,)
        assert (roomy.roots()[:4] == roots_of(want)).all() and roomy.audit().clean
        more = random_leaves(rng, 20)
        roomy.append(more, [20])
        assert (roomy.roots()[4] == cpu_levels(more)[-1][0]).all()
        with pytest.raises(ValueError, match="max_count"):
            source.inserted(batch, b_counts, max_count=300)
        # a source with one leaf overwritten out of order is refused, not trusted
        source.update([2], [17], a_trees[2][200][None])
        for method in (source.inserted, source.removed, source.common):
            with pytest.raises(RuntimeError, match="bit 2: a tree of A is not strictly increasing"):
                method(batch, b_counts)
    finally:
        for f in made + [source]:
            f.free()


def test_merge_leaves_and_the_dedup_of_a_batch(gpu):
    rng = np.random.default_rng(813)
    rows = random_leaves(rng, 300)
    batch = np.concatenate([rows[:200], rows[:50], rows[190:300], rows[:1]])                       # 361 rows that repeat, in no order
    out, counts, origin, info = gpu.merge_leaves(rows[:0], [0, 0], batch, [300, 61])
    want = [ac.sorted_rows(np.unique(batch[:300], axis=0)), ac.sorted_rows(np.unique(batch[300:], axis=0))]
    assert info.tolist() == [0, len(want[0]) + len(want[1]), 0, 361 - len(want[0]) - len(want[1])] and counts.tolist() == [len(want[0]), len(want[1])]
    assert (out == np.concatenate(want)).all() and ((origin >> np.uint64(63)) == 1).all()
    a = ac.sorted_rows(rows[:100])
    for name, op in zip(mc.OP_NAMES, mc.OPS):
        out, counts, origin, info = gpu.merge_leaves(a, [100], batch[:250], [250], op=name)
        want = model_trees([a], [batch[:250]], op)[0]
        assert (out == want).all() and counts.tolist() == [len(want)] and info.tolist() == [0, len(want), 100, 50]
        from_a = (origin >> np.uint64(63)) == 0
        assert (a[origin[from_a].astype(np.int64)] == out[from_a]).all()
    with pytest.raises(RuntimeError, match="bit 3: a tree of B decreases"):
        gpu.merge_leaves(a, [100], batch[:250], [250], sort_b=False)
    with pytest.raises(RuntimeError, match="bit 2"):
        gpu.merge_leaves(a[::-1], [100], batch[:250], [250])


def test_the_stored_tree(gpu):
    rng = np.random.default_rng(814)
    a = ac.sorted_rows(random_leaves(rng, 700))
    batch = np.concatenate([random_leaves(rng, 90), a[5:15], a[5:6]])
    d_a = gpu.upload(a)
    tree = gpu.build_tree(d_a, 700)
    made = []
    try:
        for method, op in ((tree.inserted, 0), (tree.removed, 1), (tree.common, 2)):
            new, info = method(batch)
            made.append(new)
            want = model_trees([a], [batch], op)[0]
            assert info.tolist() == [0, len(want), 10, 1] and new.count == len(want) and (new.root() == cpu_levels(want)[-1][0]).all()
            assert (new.level(0) == want).all() and new.is_sorted()
        with pytest.raises(ValueError, match="no leaf is left"):
            tree.common(random_leaves(rng, 3))
    finally:
        for t in made + [tree]:
            t.free()
        d_a.free()


def test_a_forest_above_4_gib(gpu, native):
    """A and the output at cell 2^27 + 5 of large, untouched buffers: every cell index and byte offset of the leaves needs more
    than 32 bits.  The elements are numbered from offsets[0], so the call works on a few thousand leaves, and says so by its time."""
    case = mc.forest_cases()[0]
    na, nb, ntrees = int(case.a_cells.shape[0]), int(case.b_cells.shape[0]), len(case.a_offsets) - 1
    D = hc.LINE + 5
    a_total, cap = D + na + 20, na + nb
    bufs = []
    try:
        d_a, d_big = hc.alloc(gpu, 32 * (a_total + hc.FENCE), "the leaves of A"), hc.alloc(gpu, 32 * (D + cap + hc.FENCE), "the merged leaves")
        bufs += [d_a, d_big]
        d_origin, d_scratch = hc.alloc(gpu, 8 * (D + cap + hc.FENCE), "the origin"), hc.alloc(gpu, gpu.merge_leaves_scratch_bytes(a_total, nb, ntrees), "the scratch")
        bufs += [d_origin, d_scratch]
        hc.put(gpu, d_a, 32 * D, case.a_cells)
        for op in mc.OPS:
            rc, want_out, want_off, want_origin, want_info = mc.host_merge(case, op, capacity=cap)
            n = int(want_info[1])
            # a store that lost its upper bits lands at cell (D + j) mod 2^27 = 5 + j of the same buffer
            canaries = [hc.write_canary(gpu, d_big, 0, hc.HEAD), hc.write_canary(gpu, d_big, D - hc.FENCE, hc.FENCE), hc.write_canary(gpu, d_big, D, cap + hc.FENCE),
                        hc.write_canary(gpu, d_origin, 0, hc.HEAD, 2), hc.write_canary(gpu, d_origin, D - hc.FENCE, hc.FENCE, 2),
                        hc.write_canary(gpu, d_origin, D, cap + hc.FENCE, 2), hc.write_canary(gpu, d_a, 0, hc.HEAD)]
            with gpu.scope() as tmp:
                d_info, d_off = tmp.upload(np.full(4, mc.INFO_FILL, np.uint64)), tmp.alloc(8 * (ntrees + 1))
                d_b, d_aoff, d_boff = tmp.upload(case.b_cells), tmp.upload(case.a_offsets + np.uint64(D)), tmp.upload(case.b_offsets)
                gpu.sync()
                t0 = time.perf_counter()
                gpu.forest_merge_leaves_enqueue(d_a, a_total, d_aoff, d_b, nb, d_boff, ntrees, op, d_scratch, At(d_big, 32 * D), cap, d_off, At(d_origin, 8 * D),
                                                d_info)
                gpu.sync()
                seconds = time.perf_counter() - t0
                assert gpu.download(d_info, 32, dtype=np.uint64).tolist() == want_info.tolist() and rc == 0
                assert (gpu.download(d_off, 8 * (ntrees + 1), dtype=np.uint64) == want_off).all()
            assert seconds < 0.5, seconds                    # the work follows the totals; nothing walks the 4 GiB in front
            assert (hc.read_cells(gpu, d_big, D + np.arange(n)) == want_out[:n]).all()
            got_origin = hc.read_cells(gpu, d_origin, D + np.arange(n), 2).view(np.uint64)[:, 0]
            from_b = (want_origin[:n] >> np.uint64(63)) == 1
            assert (got_origin[from_b] == want_origin[:n][from_b]).all() and (got_origin[~from_b] == want_origin[:n][~from_b] + np.uint64(D)).all()
            assert (hc.read_cells(gpu, d_big, D + n + np.arange(cap - n + hc.FENCE)) == hc.CANARY).all()          # behind n_out: untouched
            assert (hc.read_cells(gpu, d_a, D + np.arange(na)) == case.a_cells).all()
            assert hc.canaries_intact(gpu, canaries[:2] + canaries[3:5] + canaries[6:])
    finally:
        for b in bufs:
            b.free()
