"""Frontiers on the GPU (vkmr_hip_frontier_extend_async, vkmr_hip_frontier_roots_async, vkmr_hip_verify_frontier_async,
vkmr_hip_forest_frontier_async through HipDevice, vk.Frontier and MerkleForest.frontier): byte for byte what the CPU twins give
for the batches of tests/frontier_cases.py -- counts, peaks (zero cells included) and roots --, in place as out of place, a chain of
extends as one, a follower beside a primary that appends and extends, the gather's edge cases, adoption, and the refusals."""
import numpy as np
import pytest

import frontier_cases as fr
from abi_support import assert_no_spills, isa_record
from merkle_model import random_leaves

pytestmark = pytest.mark.gpu

COUNT_FILL = 0xA5A5A5A5A5A5A5A5


def device_extend(gpu, counts, peaks, leaves, offsets, max_new, total_new=None, in_place=False):
    """One raw extend: (status, new counts, new peaks, roots); the status word starts as 0xDEADBEEF and every output as the
    canary (in place: the outputs are the inputs)."""
    counts, peaks = np.ascontiguousarray(counts, dtype=np.uint64), np.ascontiguousarray(peaks, dtype=np.uint32)
    leaves = np.ascontiguousarray(leaves, dtype=np.uint32).reshape(-1, 8)
    T, stride = int(counts.shape[0]), int(peaks.shape[1])
    total_new = int(leaves.shape[0]) if total_new is None else total_new
    with gpu.scope() as tmp:
        d_counts, d_peaks = tmp.upload(counts), tmp.upload(peaks)
        d_new_counts = d_counts if in_place else tmp.upload(np.full(T, COUNT_FILL, np.uint64))
        d_new_peaks = d_peaks if in_place else tmp.upload(np.full(peaks.shape, fr.CANARY, np.uint32))
        d_roots, d_status = tmp.upload(np.full((T, 8), fr.CANARY, np.uint32)), tmp.upload(np.full(1, 0xDEADBEEF, np.uint32))
        scratch = tmp.keep(gpu.frontier_extend_scratch(total_new, T))
        gpu.frontier_extend_enqueue(d_counts, d_peaks, stride, T, tmp.upload(leaves) if leaves.size else None, total_new,
                                    tmp.upload(np.ascontiguousarray(offsets, dtype=np.uint64)), max_new, scratch, d_new_counts, d_new_peaks, d_roots, d_status)
        return (int(gpu.download(d_status, 4)[0]), gpu.download(d_new_counts, 8 * T, dtype=np.uint64),
                gpu.download(d_new_peaks, 32 * T * stride).reshape(T, stride, 8), gpu.download(d_roots, 32 * T).reshape(T, 8))


@pytest.fixture(scope="module")
def twins():
    """What the CPU twin gives for every batch, computed once."""
    return {name: fr.host_extend(b.counts, b.peaks, b.leaves, b.offsets) for name, b in (("square", fr.square()), ("edges", fr.edges()), ("big", fr.big()))}


@pytest.mark.parametrize("name", ["square", "edges", "big"])
@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
def test_the_device_is_the_cpu_twin_byte_for_byte(gpu, twins, name, in_place):
    batch = getattr(fr, name)()
    want = twins[name]
    assert want[0] == 0 and (want[3] == batch.want_roots).all()           # the twin is the model (tests/test_frontier_abi.py)
    got = device_extend(gpu, batch.counts, batch.peaks, batch.leaves, batch.offsets, max(batch.new_counts), in_place=in_place)
    assert got[0] == 0
    for what, a, b in zip(("counts", "peaks", "roots"), got[1:], want[1:]):
        assert a.shape == b.shape and (a == b).all(), (name, what, np.nonzero((a != b).reshape(a.shape[0], -1).any(axis=1))[0][:8])
    import vk_merkle_roots_amd as vk
    after = vk.Frontier(got[1], got[2])
    assert (after.roots(gpu) == got[3]).all() and (after.verify(gpu, got[3]) == 1).all()


def test_a_tight_stride_and_trees_that_take_no_leaf(gpu):
    pairs = [(0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (5, 0), (64, 0), (100, 0), (127, 0), (128, 0)]
    batch = fr.Batch(pairs, seed=331, stride=8)
    want = fr.host_extend(batch.counts, batch.peaks, batch.leaves, batch.offsets)
    got = device_extend(gpu, batch.counts, batch.peaks, batch.leaves, batch.offsets, 0)          # no leaf at all: leaves_dev is NULL
    assert got[0] == 0 and want[0] == 0 and all((a == b).all() for a, b in zip(got[1:], want[1:]))
    assert (got[1] == batch.counts).all() and (got[2] == batch.peaks).all() and (got[3] == batch.want_roots).all()


def test_three_extends_equal_one_of_the_concatenation(gpu):
    import vk_merkle_roots_amd as vk
    rng = np.random.default_rng(341)
    steps = [[3, 0, 64, 1, 0], [0, 0, 1, 127, 5], [62, 0, 0, 1, 2100]]
    leaves = [random_leaves(rng, sum(s)) for s in steps]
    chain, once = vk.Frontier.empty(5, stride=13), vk.Frontier.empty(5, stride=13)
    for s, rows in zip(steps, leaves):
        roots = chain.extend(gpu, rows, s)
    per_tree = [[] for _ in range(5)]
    for s, rows in zip(steps, leaves):
        at = 0
        for q, n in enumerate(s):
            per_tree[q].append(rows[at: at + n])
            at += n
    all_rows = np.concatenate([np.concatenate(p) for p in per_tree])
    totals = [sum(s[q] for s in steps) for q in range(5)]
    assert (once.extend(gpu, all_rows, totals) == roots).all() and chain.same_as(once)
    assert chain.counts.tolist() == totals == [65, 0, 65, 129, 2105] and not roots[1].any()
    assert (roots == gpu.forest_roots(all_rows, totals)).all()                        # and what a holder of every leaf reduces
    assert (chain.extend(gpu, np.zeros((0, 8), np.uint32), [0] * 5) == roots).all() and chain.same_as(once)


def test_a_follower_beside_a_primary_that_appends_and_extends(gpu):
    rng = np.random.default_rng(351)
    leaves = random_leaves(rng, 400)
    forest = gpu.build_forest(leaves[:70], [5, 65], max_count=130, reserve_trees=3, reserve_leaves=330)
    follower = forest.frontier()
    assert follower.T == 5 and follower.stride == 8 and (follower.verify(gpu, forest.roots()) == 1).all()      # adopted under the roots
    assert forest.append(leaves[70:80], [3, 7]).tolist() == [2, 3]
    assert (follower.extend(gpu, leaves[70:80], [0, 0, 3, 7, 0]) == forest.roots()).all()
    assert forest.extend(leaves[80:200]) == 127                                       # the open tree, tree 3: 7 -> 127
    assert (follower.extend(gpu, leaves[80:200], [0, 0, 0, 120, 0]) == forest.roots()).all()
    assert forest.extend(leaves[200:201]) == 128                                      # a power of two: its peak lives in the roots
    assert (follower.extend(gpu, leaves[200:201], [0, 0, 0, 1, 0]) == forest.roots()).all()
    assert follower.same_as(forest.frontier()) and follower.counts.tolist() == forest.counts.tolist()
    assert (follower.roots(gpu) == forest.roots()).all()
    forest.free()


def test_extend_packed_maps_and_extends(gpu):
    import vk_merkle_roots_amd as vk
    batch = vk.pack_lines(b"".join(b"string %d of the follower\n" % i for i in range(75)))
    a, b = vk.Frontier.empty(3, stride=7), vk.Frontier.empty(3, stride=7)
    roots = a.extend_packed(gpu, batch, [3, 65, 7])
    assert (b.extend(gpu, gpu.leaf_digests(batch), [3, 65, 7]) == roots).all() and a.same_as(b)
    assert (roots == vk.merkle_roots_packed_forest(gpu, batch, [3, 65, 7])).all()


def test_the_gather_where_the_peak_lives_in_the_roots(gpu):
    counts = [0, 1, 2, 3, 4, 8, 16, 64, 128, 1024, 5, 0, 2048, 2047, 2]
    rng = np.random.default_rng(361)
    leaves = random_leaves(rng, sum(counts))
    forest = gpu.build_forest(leaves, counts)
    rc, want_counts, want_peaks = fr.host_forest_frontier(leaves, counts, stride=12)
    assert rc == 0
    got = forest.frontier()
    assert got.stride == 12 and (got.counts == want_counts).all() and (got.peaks == want_peaks).all()
    wide = forest.frontier(stride=64)
    assert (wide.peaks[:, :12] == want_peaks).all() and not wide.peaks[:, 12:].any()
    assert (got.roots(gpu) == forest.roots()).all()
    from vk_merkle_roots_amd._abi import VkmrError
    with pytest.raises(VkmrError):
        forest.frontier(stride=11)                                                    # a tree of 2 048 leaves has twelve bits
    forest.free()


def test_adoption_one_flipped_bit_and_one_changed_count(gpu):
    import vk_merkle_roots_amd as vk
    counts = [7, 64, 0, 100, 1, 6]
    leaves = random_leaves(np.random.default_rng(371), sum(counts))
    forest = gpu.build_forest(leaves, counts)
    roots, sent = forest.roots(), forest.frontier()
    assert (sent.verify(gpu, roots) == 1).all()
    flipped = vk.Frontier(sent.counts, sent.peaks)
    flipped.peaks[3, 5, 2] ^= 1 << 17                                                 # 100 = 0b1100100: bit 5 is set
    assert flipped.verify(gpu, roots).tolist() == [1, 1, 1, 0, 1, 1]
    recounted = vk.Frontier(sent.counts, sent.peaks)
    recounted.counts[0] = 5                                                           # 7 -> 5: both of height 3, both cells there
    assert recounted.verify(gpu, roots).tolist() == [0, 1, 1, 1, 1, 1]
    recounted.counts[0], recounted.counts[2] = 7, 1                                   # an empty tree claimed to hold a (zero) leaf
    assert recounted.verify(gpu, roots).tolist() == [1, 1, 0, 1, 1, 1]
    forest.free()


@pytest.mark.parametrize("what,status,counts,offsets,max_new,stride", fr.REFUSALS, ids=[r[0] for r in fr.REFUSALS])
def test_a_refused_extend_writes_nothing(gpu, what, status, counts, offsets, max_new, stride):
    import vk_merkle_roots_amd as vk
    old_counts, old_peaks, leaves = fr.refusal_frontier(counts, stride)
    assert fr.host_extend(old_counts, old_peaks, leaves, offsets, max_new=max_new, total_new=6)[0] == status
    got = device_extend(gpu, old_counts, old_peaks, leaves, offsets, max_new, total_new=6)
    assert got[0] == status, what
    assert (got[1] == COUNT_FILL).all() and (got[2] == fr.CANARY).all() and (got[3] == fr.CANARY).all()
    bit = status.bit_length() - 1
    assert f"bit {bit}:" in vk.frontier_status_text(got[0])
    in_place = device_extend(gpu, old_counts, old_peaks, leaves, offsets, max_new, total_new=6, in_place=True)
    assert in_place[0] == status and (in_place[1] == old_counts).all() and (in_place[2] == old_peaks).all() and (in_place[3] == fr.CANARY).all()


def test_the_handle_reports_the_devices_refusal(gpu):
    import vk_merkle_roots_amd as vk
    f = vk.Frontier.empty(2, stride=8)
    f.counts[1] = (1 << 58) - 1                                                       # a count no cell of this frontier stands for
    with pytest.raises(ValueError):
        f.extend(gpu, np.zeros((2, 8), np.uint32), [0, 2])                            # the host sees it first
    f._new_offsets = lambda counts, n, what: np.array([0, 0, 2], dtype=np.uint64)     # and behind a host that did not look, the device
    with pytest.raises(RuntimeError, match="bit 2"):
        f.extend(gpu, np.zeros((2, 8), np.uint32), [0, 2])
    assert f.counts.tolist() == [0, (1 << 58) - 1]


def test_the_level_kernels_listing(native):
    rec = isa_record(native)                                                          # the record the build writes beside the library
    assert rec is not None
    mine = {k: len(v) for k, v in rec["hash_blocks"].items() if "frontier_level_kernel" in k}
    assert list(mine.values()) == [1]
    assert rec["audit"]["block_count_errors"] == [] and {v for k, v in rec["audit"]["blocks"].items() if "frontier" in k} == {1}
    assert_no_spills(native, ["frontier_level_kernel"])                               # returns where the library came built, without its assembly
