"""The forest reduction on the GPU (vkmr_hip_reduce_forest_async through HipDevice): every root bit-exact against the oracle,
against the host CPU counterpart and against the engine's own one-tree and equal-slices kernels; the device-side checks;
stream order and the scratch budget."""
import ctypes as C

import numpy as np
import pytest

import forest_cases as fc
from merkle_model import random_counts

pytestmark = pytest.mark.gpu

PATTERN = 0xC3C3C3C3


def run_forest(gpu, d_leaves, total, offsets, max_count, ntrees=None):
    """(status, roots [ntrees, 8]) of one raw call; roots_dev is pre-filled with PATTERN."""
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    ntrees = offsets.shape[0] - 1 if ntrees is None else ntrees
    d_off = gpu.upload(offsets)
    d_scr = gpu.alloc(gpu.lib.vkmr_hip_forest_scratch_bytes(total, ntrees))
    d_roots = gpu.upload(np.full((ntrees, 8), PATTERN, dtype=np.uint32))
    d_status = gpu.upload(np.array([0xFFFFFFFF], dtype=np.uint32))
    gpu.reduce_forest_async(d_leaves, total, d_off, ntrees, max_count, d_scr, d_roots, d_status)
    status = int(gpu.download(d_status, 4)[0])
    roots = gpu.download(d_roots, 32 * ntrees).reshape(ntrees, 8)
    for b in (d_off, d_scr, d_roots, d_status):
        b.free()
    return status, roots


@pytest.mark.parametrize("name", sorted(fc.CASES))
def test_case_tables_equal_the_oracle_and_the_host_cpu(gpu, oracle, name):
    counts = fc.CASES[name]
    leaves = fc.random_leaves(sum(counts), seed=len(name) * 7919 + sum(counts))
    roots = gpu.forest_roots(leaves, counts)
    assert roots.shape == (len(counts), 8) and roots.dtype == np.uint32
    want = fc.oracle_roots(oracle, leaves, counts)
    assert (roots == want).all(), np.nonzero((roots != want).any(axis=1))[0][:10]
    rc, cpu = fc.host_cpu_roots(leaves, fc.offsets_of(counts))
    assert rc == 0 and (roots == cpu).all()


def test_ten_reference_trees_as_one_forest(gpu, oracle, ref_checks):
    leaves, counts = fc.ref_check_forest(oracle)
    roots = gpu.forest_roots(leaves, counts)
    assert [oracle.hex(r) for r in roots] == [t["root"] for t in ref_checks["trees"]]


@pytest.mark.parametrize("name", ["sizes_1_to_130", "power_of_two_edges", "one_big_among_small", "empty_adjacent", "all_ones"])
def test_tight_and_loose_max_count_give_the_same_roots(gpu, oracle, name):
    counts = fc.CASES[name]
    total, largest = sum(counts), max(counts)
    leaves = fc.random_leaves(total, seed=5)
    want = fc.oracle_roots(oracle, leaves, counts)
    for max_count in (largest, 1 << fc.ceil_log2(largest), total, 2**63):
        roots = gpu.forest_roots(leaves, counts, max_count=max_count)
        assert (roots == want).all(), max_count


@pytest.mark.parametrize("k", [0, 1, 7, 8, 11])
def test_equal_trees_match_reduce_slices_and_a_ragged_last_tree(gpu, k):
    cap = 1 << k
    nslices = 300 if k < 8 else 40
    last = max(1, cap // 2 - 1) if k != 7 else 77
    total = (nslices - 1) * cap + last
    leaves = fc.random_leaves(total, seed=100 + k)
    d_leaves = gpu.upload(leaves)
    height = max(1, k)
    d_scr = gpu.alloc(gpu.lib.vkmr_hip_reduce_slices_scratch_bytes(cap, nslices))
    d_roots = gpu.alloc(32 * nslices)
    gpu.reduce_slices_async(d_leaves, nslices, cap, last, height, d_scr, d_roots)
    slices = gpu.download(d_roots, 32 * nslices).reshape(nslices, 8)
    counts = [cap] * (nslices - 1) + [last]
    status, roots = run_forest(gpu, d_leaves, total, fc.offsets_of(counts), cap)
    assert status == 0
    assert (roots[:-1] == slices[:-1]).all()
    assert (roots[-1] == gpu.reduce_digests(leaves[(nslices - 1) * cap:])).all()
    for b in (d_leaves, d_scr, d_roots):
        b.free()


@pytest.mark.parametrize("seed", range(50))
def test_random_forests_match_the_one_tree_reduction(gpu, seed):
    rng = np.random.default_rng(seed)
    counts = random_counts(rng, 1 << 20)
    leaves = fc.random_leaves(sum(counts), seed=1000 + seed)
    roots = gpu.forest_roots(leaves, counts)
    off = fc.offsets_of(counts)
    for t, c in enumerate(counts):
        if c == 0:
            assert not roots[t].any(), t
        else:
            assert (roots[t] == gpu.reduce_digests(leaves[int(off[t]): int(off[t + 1])])).all(), (t, c)


def test_large_mixed_forest_equals_the_oracle(gpu, oracle):
    total = 1 << 22
    rng = np.random.default_rng(42)
    sizes = rng.integers(1, 4096, size=total // 1024)        # uniform in [1, 4095]; far more than needed
    ends = np.cumsum(sizes)
    n = int(np.searchsorted(ends, total))
    counts = [int(c) for c in sizes[:n]] + ([total - int(ends[n - 1])] if int(ends[n - 1]) < total else [])
    assert sum(counts) == total and max(counts) <= 4095
    leaves = fc.random_leaves(total, seed=43)
    roots = gpu.forest_roots(leaves, counts, max_count=4095)
    want = fc.oracle_roots(oracle, leaves, counts)
    assert (roots == want).all(), np.nonzero((roots != want).any(axis=1))[0][:10]


def test_two_to_the_26_leaves_in_equal_trees_match_reduce_slices(gpu):
    cap, ntrees = 1 << 11, 1 << 15
    total = cap * ntrees
    d_leaves = gpu.alloc(32 * total)
    rng = np.random.default_rng(26)
    chunk = 1 << 22
    for at in range(0, total, chunk):      # random digests, uploaded in pieces
        part = rng.integers(0, 2**32, size=(chunk, 8), dtype=np.uint32)
        gpu.lib.vkmr_hip_memcpy_h2d_async(gpu.index, gpu.stream, d_leaves.at(32 * at), part.ctypes.data, part.nbytes)
        gpu.sync()
    d_scr = gpu.alloc(gpu.lib.vkmr_hip_reduce_slices_scratch_bytes(cap, ntrees))
    d_roots = gpu.alloc(32 * ntrees)
    gpu.reduce_slices_async(d_leaves, ntrees, cap, cap, 11, d_scr, d_roots)
    slices = gpu.download(d_roots, 32 * ntrees).reshape(ntrees, 8)
    status, roots = run_forest(gpu, d_leaves, total, np.arange(ntrees + 1, dtype=np.uint64) * np.uint64(cap), cap)
    assert status == 0
    assert (roots == slices).all(), np.nonzero((roots != slices).any(axis=1))[0][:10]
    for b in (d_leaves, d_scr, d_roots):
        b.free()


def test_the_device_refuses_bad_offsets_and_writes_no_root(gpu, oracle):
    counts = [5, 9, 130, 1, 64]
    total, max_count = sum(counts), 130
    leaves = fc.random_leaves(total, seed=9)
    d_leaves = gpu.upload(leaves)
    good = fc.offsets_of(counts)
    want = fc.oracle_roots(oracle, leaves, counts)
    pattern = np.full((len(counts), 8), PATTERN, dtype=np.uint32)

    decreasing = good.copy()
    decreasing[2], decreasing[3] = good[3], good[2]           # offsets[3] < offsets[2]: decreasing in the middle
    status, roots = run_forest(gpu, d_leaves, total, decreasing, total)
    assert status & 1 and (roots == pattern).all()

    past = good.copy()
    past[-1] = total + 1                                      # the last tree (65 <= max_count) ends behind the leaves
    status, roots = run_forest(gpu, d_leaves, total, past, max_count)
    assert status == 1 and (roots == pattern).all()

    status, roots = run_forest(gpu, d_leaves, total, good, max_count - 1)      # one tree of max_count + 1
    assert status == 2 and (roots == pattern).all()

    with pytest.raises(ValueError, match="bit 1"):
        gpu.forest_roots(leaves, counts, max_count=129)

    # a following correct call on the same stream and buffers succeeds: bad, then good, no sync in between
    d_off_bad, d_off_good = gpu.upload(decreasing), gpu.upload(good)
    d_scr = gpu.alloc(gpu.lib.vkmr_hip_forest_scratch_bytes(total, len(counts)))
    d_roots = gpu.upload(pattern)
    d_status = gpu.alloc(4)
    gpu.reduce_forest_async(d_leaves, total, d_off_bad, len(counts), max_count, d_scr, d_roots, d_status)
    gpu.reduce_forest_async(d_leaves, total, d_off_good, len(counts), max_count, d_scr, d_roots, d_status)
    assert int(gpu.download(d_status, 4)[0]) == 0
    assert (gpu.download(d_roots, 32 * len(counts)).reshape(-1, 8) == want).all()
    for b in (d_leaves, d_off_bad, d_off_good, d_scr, d_roots, d_status):
        b.free()


def test_all_trees_empty_with_no_leaves_at_all(gpu):
    status, roots = run_forest(gpu, None, 0, np.zeros(6, dtype=np.uint64), 1)
    assert status == 0 and not roots.any()


def test_stream_order_exact_scratch_and_canaries(gpu, oracle):
    """map -> forest -> download on one stream with no synchronisation in between; one allocation laid out as
    canary | scratch of exactly vkmr_hip_forest_scratch_bytes | roots | canary."""
    import vk_merkle_roots_amd as vk
    batch = vk.rndm_packed(7, 20000, 60)
    rng = np.random.default_rng(8)
    counts = []
    while sum(counts) < batch.count:
        counts.append(min(int(rng.integers(0, 700)), batch.count - sum(counts)))
    ntrees, total = len(counts), batch.count
    want = fc.oracle_roots(oracle, oracle.leaves_packed(batch.data, batch.meta), counts)
    scratch_bytes = gpu.lib.vkmr_hip_forest_scratch_bytes(total, ntrees)
    guard = 4096
    block = np.full((guard + scratch_bytes + 32 * ntrees + guard) // 4, PATTERN, dtype=np.uint32)
    d_block = gpu.upload(block)
    d_data, d_meta, d_off = gpu.upload(batch.data), gpu.upload(batch.meta), gpu.upload(fc.offsets_of(counts))
    d_leaves, d_status = gpu.alloc(32 * total), gpu.alloc(4)
    lib, s = gpu.lib, gpu.new_stream()
    roots = np.zeros((ntrees, 8), dtype=np.uint32)
    status = np.full(1, 0xFFFFFFFF, dtype=np.uint32)
    gpu.map_async(d_data, batch.words, d_meta, total, d_leaves, stream=s)
    vk.check(lib.vkmr_hip_reduce_forest_async(gpu.index, s, d_leaves.ptr, total, d_off.ptr, ntrees, max(counts), d_block.at(guard),
                                              d_block.at(guard + scratch_bytes), d_status.ptr), "vkmr_hip_reduce_forest_async")
    vk.check(lib.vkmr_hip_memcpy_d2h_async(gpu.index, s, roots.ctypes.data, d_block.at(guard + scratch_bytes), roots.nbytes), "d2h")
    vk.check(lib.vkmr_hip_memcpy_d2h_async(gpu.index, s, status.ctypes.data, d_status.ptr, 4), "d2h")
    gpu.sync(s)
    assert status[0] == 0
    assert (roots == want).all()
    after = gpu.download(d_block, block.nbytes)
    assert (after[: guard // 4] == PATTERN).all() and (after[-(guard // 4):] == PATTERN).all()
    assert (after[(guard + scratch_bytes) // 4: (guard + scratch_bytes) // 4 + 8 * ntrees].reshape(-1, 8) == want).all()
    lib.vkmr_hip_stream_destroy(gpu.index, s)
    for b in (d_block, d_data, d_meta, d_off, d_leaves, d_status):
        b.free()


def test_merkle_roots_packed_forest_equals_the_per_tree_oracle(gpu, oracle):
    import vk_merkle_roots_amd as vk
    batch = vk.rndm_packed(42, 100_000, 127)
    rng = np.random.default_rng(42)
    counts = []
    while sum(counts) < batch.count:
        counts.append(min(int(rng.integers(0, 3000)), batch.count - sum(counts)))
    roots = vk.merkle_roots_packed_forest(gpu, batch, counts)
    want = fc.oracle_roots(oracle, oracle.leaves_packed(batch.data, batch.meta), counts)
    assert (roots == want).all()
