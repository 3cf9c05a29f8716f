"""The diff of two stored forests or trees on the GPU (vkmr_hip_forest_diff_async and vkmr_hip_tree_diff_async, raw and through
MerkleForest / MerkleTree): every answer against the model in tests/diff_cases.py -- cells [0, n), the four counters, B's
leaves at the positions --, the words around the outputs, the inputs read back unchanged, the capacity's edge, and the chains
diff -> update (sync_from) and diff -> multiproof."""
import numpy as np
import pytest

import diff_cases as dc
import forest_cases as fc
from merkle_model import At

pytestmark = pytest.mark.gpu

PATTERN_A, PATTERN_B = 0xC3C3C3C3, 0x5A5A5A5A     # what the cells nobody writes hold in A and in B
PATTERN = 0xA5A5A5A5
PATTERN64 = PATTERN * 0x100000001
GUARD = 512                                       # words in front of and behind each output: more than one workgroup's lanes


class Outputs:
    """trees [cap] uint32, indices [cap] uint64, leaves [cap, 8] and info [4] on the device, each between GUARD words of PATTERN."""

    def __init__(self, gpu, cap):
        self.gpu, self.cap = gpu, cap
        self.d_trees = gpu.upload(np.full(2 * GUARD + cap, PATTERN, dtype=np.uint32))
        self.d_idx = gpu.upload(np.full(2 * GUARD + cap, PATTERN64, dtype=np.uint64))
        self.d_leaves = gpu.upload(np.full(2 * GUARD + 8 * cap, PATTERN, dtype=np.uint32))
        self.d_info = gpu.upload(np.full(2 * GUARD + 4, PATTERN64, dtype=np.uint64))
        self.trees_at, self.idx_at = At(self.d_trees, 4 * GUARD), At(self.d_idx, 8 * GUARD)
        self.leaves_at, self.info_at = At(self.d_leaves, 4 * GUARD), At(self.d_info, 8 * GUARD)

    def read(self, stream=None):
        """(trees, indices, leaves, info), the guards checked."""
        cap, gpu = self.cap, self.gpu
        t = gpu.download(self.d_trees, 4 * (2 * GUARD + cap), stream=stream)
        i = gpu.download(self.d_idx, 8 * (2 * GUARD + cap), dtype=np.uint64, stream=stream)
        lv = gpu.download(self.d_leaves, 4 * (2 * GUARD + 8 * cap), stream=stream)
        info = gpu.download(self.d_info, 8 * (2 * GUARD + 4), dtype=np.uint64, stream=stream)
        assert (t[:GUARD] == PATTERN).all() and (t[GUARD + cap:] == PATTERN).all()
        assert (i[:GUARD] == PATTERN64).all() and (i[GUARD + cap:] == PATTERN64).all()
        assert (lv[:GUARD] == PATTERN).all() and (lv[GUARD + 8 * cap:] == PATTERN).all()
        assert (info[:GUARD] == PATTERN64).all() and (info[GUARD + 4:] == PATTERN64).all()
        return t[GUARD: GUARD + cap], i[GUARD: GUARD + cap], lv[GUARD: GUARD + 8 * cap].reshape(cap, 8), tuple(int(x) for x in info[GUARD: GUARD + 4])

    def free(self):
        for b in (self.d_trees, self.d_idx, self.d_leaves, self.d_info):
            b.free()


def raw_pair(gpu, case):
    return (dc.RawForest(gpu, case.a, case.counts, case.max_count, case.first, PATTERN_A),
            dc.RawForest(gpu, case.b, case.counts, case.max_count, case.first, PATTERN_B))


def forest_diff(gpu, A, B, capacity, leaves=True, d_scr=None, stream=None):
    """(trees, indices, leaves, info) of one raw vkmr_hip_forest_diff_async between guards; capacity 0: NULL outputs."""
    mine = d_scr is None
    d_scr = gpu.upload(np.full(gpu.diff_scratch_bytes(capacity) // 4, PATTERN, dtype=np.uint32)) if mine else d_scr
    out = Outputs(gpu, capacity)
    A.handle.diff_async(B.handle, d_scr, out.trees_at if capacity else None, out.idx_at if capacity else None,
                        out.leaves_at if leaves and capacity else None, capacity, out.info_at, stream=stream)
    got = out.read(stream=stream)
    out.free()
    if mine:
        d_scr.free()
    return got


def assert_equals_the_model(case, got, what, leaves=True):
    trees, indices, lv, info = got
    n = case.n
    assert info == case.info, (what, info, case.info)
    assert (trees[:n] == case.trees).all() and (indices[:n] == case.indices).all(), what
    if leaves:
        assert (lv[:n] == case.leaves_b).all(), what
    else:
        assert (lv == PATTERN).all(), what


def assert_overflow(case, got, capacity, what):
    info = got[3]
    assert info[0] == dc.OVERFLOW and capacity < info[1] <= case.n and info[2] == case.info[2], (what, info)


@pytest.mark.parametrize("name,change", dc.PAIRS)
def test_every_table_through_the_raw_calls(gpu, name, change):
    case = dc.case(name, change)
    A, B = raw_pair(gpu, case)
    before = A.state(), B.state()
    n = case.n
    assert_equals_the_model(case, forest_diff(gpu, A, B, n), (name, change, "capacity n"))
    assert_equals_the_model(case, forest_diff(gpu, A, B, n + 300, leaves=False), (name, change, "room to spare, no leaves"), leaves=False)
    if n:
        assert_overflow(case, forest_diff(gpu, A, B, n - 1), n - 1, (name, change, "capacity n - 1"))
        swapped = forest_diff(gpu, B, A, n)                      # the other way round: the same positions, A's leaves
        assert (swapped[0] == case.trees).all() and (swapped[1] == case.indices).all() and swapped[3] == case.info
        assert (swapped[2] == case.a[case.flat + case.first]).all()
    after = A.state(), B.state()
    assert all(dc.fu.same_state(x, y) for x, y in zip(before, after))
    A.free()
    B.free()
    # the same cells as one tree
    count = sum(case.counts)
    if count == 0:
        return
    d_a, d_b = gpu.upload(case.window(case.a)), gpu.upload(case.window(case.b))
    ta, tb = gpu.build_tree(d_a, count), gpu.build_tree(d_b, count)
    want_info = dc.tree_counters(count, ta.height, case.flat)
    for capacity in sorted({n, n + 300, max(n - 1, 0)}):
        d_scr = gpu.upload(np.full(gpu.diff_scratch_bytes(capacity) // 4, PATTERN, dtype=np.uint32))
        out = Outputs(gpu, capacity)
        ta.diff_async(tb, d_scr, out.idx_at if capacity else None, out.leaves_at if capacity else None, capacity, out.info_at)
        trees, indices, lv, info = out.read()
        assert (trees == PATTERN).all()                          # the tree call has no such output
        if capacity >= n:
            assert info == want_info, (name, change, capacity, info, want_info)
            assert (indices[:n] == case.flat).all() and (lv[:n] == case.leaves_b).all()
        else:
            assert info[0] == dc.OVERFLOW and capacity < info[1] <= n and info[2] == 1
        out.free()
        d_scr.free()
    assert (gpu.download(d_a, 32 * count).reshape(-1, 8) == case.window(case.a)).all()
    assert (gpu.download(d_b, 32 * count).reshape(-1, 8) == case.window(case.b)).all()
    for x in (ta, tb, d_a, d_b):
        x.free()


@pytest.mark.parametrize("name,change", [(n, c) for n, c in dc.PAIRS if dc.FORESTS[n][0] == 0 and dc.FORESTS[n][1] == 0 and sum(dc.FORESTS[n][3])])
def test_every_table_through_the_python_layer(gpu, name, change):
    import vk_merkle_roots_amd as vk
    case = dc.case(name, change)
    fa, fb = gpu.build_forest(case.a, case.counts, case.max_count), gpu.build_forest(case.b, case.counts, case.max_count)
    trees, indices = fa.diff(fb)
    assert trees.dtype == np.uint32 and indices.dtype == np.uint64
    assert (trees == case.trees).all() and (indices == case.indices).all()
    trees, indices = fa.diff(fb, capacity=case.n)
    assert (trees == case.trees).all() and (indices == case.indices).all()
    if case.n:
        with pytest.raises(vk.DiffOverflow):
            fa.diff(fb, capacity=case.n - 1)
    fa.free()
    fb.free()
    d_a, d_b = gpu.upload(case.a), gpu.upload(case.b)
    ta, tb = gpu.build_tree(d_a, case.total), gpu.build_tree(d_b, case.total)
    got = ta.diff(tb)
    assert got.dtype == np.uint64 and (got == case.flat).all()
    if case.n:
        with pytest.raises(vk.DiffOverflow):
            ta.diff(tb, capacity=case.n - 1)
    for x in (ta, tb, d_a, d_b):
        x.free()


def test_capacity_zero_on_equal_forests_with_null_outputs(gpu):
    case = dc.case("window", "none")
    A, B = raw_pair(gpu, case)
    got = forest_diff(gpu, A, B, 0)
    assert got[3] == (0, 0, 0, 0)
    changed = case.a.copy()
    changed[case.first + 3, 2] ^= 1                              # leaf 3 of tree 0
    C = dc.RawForest(gpu, changed, case.counts, case.max_count, case.first, PATTERN_B)
    assert forest_diff(gpu, A, C, 0)[3] == (dc.OVERFLOW, 1, 1, 0)       # one root differs: a frontier of 1 is more than 0
    for x in (A, B, C):
        x.free()


def test_diff_without_a_capacity_grows_to_the_answer(gpu, monkeypatch):
    """The growth of diff(capacity=None) -- 16-fold while bit 2 is set -- from a small first capacity: 4, 64, 1024, 16384 for
    8193 differing leaves; and from the shipped 65536 on the same forests."""
    from vk_merkle_roots_amd import engine
    case = dc.case("twenty_thousand", "run_of_8193")
    fa, fb = gpu.build_forest(case.a, case.counts), gpu.build_forest(case.b, case.counts)
    seen = []
    real = engine.HipDevice.diff_scratch_bytes
    monkeypatch.setattr(engine.HipDevice, "diff_scratch_bytes", lambda self, cap: (seen.append(cap), real(self, cap))[1])
    monkeypatch.setattr(engine, "DIFF_FIRST_CAPACITY", 4)
    trees, indices = fa.diff(fb)
    assert seen == [4, 64, 1024, 16384]
    assert (trees == case.trees).all() and (indices == case.indices).all()
    assert fa.sync_from(fb) == case.n and fa.diff(fb)[0].shape == (0,)
    monkeypatch.undo()
    fa.free()
    fb.free()


@pytest.mark.parametrize("name,change", [("window", "random_third"), ("empty_adjacent", "every_leaf"), ("power_of_two_edges", "odd_last"),
                                         ("max_count_below_total", "first_and_last"), ("twenty_thousand", "run_of_8193")])
def test_sync_from_makes_a_equal_to_b(gpu, name, change):
    case = dc.case(name, change)
    A, B = raw_pair(gpu, case)
    fresh = dc.RawForest(gpu, case.b, case.counts, case.max_count, case.first, PATTERN_A)      # a build over B's leaves, A's prefill
    assert A.handle.sync_from(B.handle) == case.n
    assert (A.handle.roots() == B.handle.roots()).all()
    leaves, forest, roots = A.state()
    assert (case.window(leaves.reshape(-1, 8)) == case.window(case.b)).all()
    if case.first:                                               # cells outside the trees are no leaves: A keeps its own
        assert (leaves.reshape(-1, 8)[: case.first] == case.a[: case.first]).all()
        assert (leaves.reshape(-1, 8)[-case.slack:] == case.a[-case.slack:]).all()
    want = fresh.state()
    assert (forest == want[1]).all() and (roots == want[2]).all()
    assert (A.handle.mutated() == B.handle.mutated()).all()
    assert forest_diff(gpu, A, B, 0)[3] == (0, 0, 0, 0)
    trees, indices = A.handle.diff(B.handle)
    assert trees.shape == (0,) and indices.shape == (0,)
    for x in (A, B, fresh):
        x.free()


def test_sync_from_of_a_tree(gpu):
    case = dc.case("one_tree_of_5000", "random_third")
    d_a, d_b = gpu.upload(case.a), gpu.upload(case.b)
    ta, tb = gpu.build_tree(d_a, case.total), gpu.build_tree(d_b, case.total)
    assert ta.sync_from(tb) == case.n
    assert (ta.root() == tb.root()).all() and (gpu.download(d_a, 32 * case.total).reshape(-1, 8) == case.b).all()
    for l in range(1, ta.height + 1):
        assert (ta.level(l) == tb.level(l)).all()
    assert ta.diff(tb).shape == (0,) and ta.sync_from(tb) == 0
    for x in (ta, tb, d_a, d_b):
        x.free()


def test_a_tree_of_one_leaf_and_a_tree_above_its_own_height(gpu):
    rng = np.random.default_rng(dc.seed_of("tree edges"))
    one, other = dc.random_leaves(rng, 1), dc.random_leaves(rng, 1)
    for height in (0, 1, 3):
        d_a, d_b = gpu.upload(one), gpu.upload(other)
        ta, tb = gpu.build_tree(d_a, 1, height), gpu.build_tree(d_b, 1, height)
        d_scr = gpu.alloc(gpu.diff_scratch_bytes(4))
        out = Outputs(gpu, 4)
        ta.diff_async(tb, d_scr, out.idx_at, out.leaves_at, 4, out.info_at)
        _, indices, lv, info = out.read()
        assert info == dc.tree_counters(1, height, [0]) and int(indices[0]) == 0 and (lv[0] == other[0]).all(), height
        ta.diff_async(ta, d_scr, out.idx_at, out.leaves_at, 4, out.info_at)
        assert out.read()[3] == (0, 0, 0, 0)
        ta.diff_async(tb, d_scr, None, None, 0, out.info_at)
        assert out.read()[3] == (dc.OVERFLOW, 1, 1, 0)
        assert ta.sync_from(tb) == 1 and (ta.root() == tb.root()).all()
        for x in (ta, tb, d_a, d_b, d_scr, out):
            x.free()
    a = dc.random_leaves(rng, 77)
    b = a.copy()
    b[[3, 76]] ^= 1
    d_a, d_b = gpu.upload(a), gpu.upload(b)
    ta, tb = gpu.build_tree(d_a, 77, 9), gpu.build_tree(d_b, 77, 9)           # two levels above the 7 the count needs
    d_scr, out = gpu.alloc(gpu.diff_scratch_bytes(2)), Outputs(gpu, 2)
    ta.diff_async(tb, d_scr, out.idx_at, out.leaves_at, 2, out.info_at)
    _, indices, lv, info = out.read()
    assert info == dc.tree_counters(77, 9, [3, 76]) and list(indices) == [3, 76] and (lv == b[[3, 76]]).all()
    for x in (ta, tb, d_a, d_b, d_scr, out):
        x.free()


def test_a_diff_behind_an_update_on_one_stream_gives_the_updates_entries_back(gpu):
    case = dc.case("window", "none")
    A, B = raw_pair(gpu, case)
    trees, indices = dc.fu.sorted_entries([(0, 8), (2, 0), (2, 32), (5, 99)])
    new = fc.random_leaves(4, seed=31337)
    s = gpu.new_stream()
    d_t, d_i, d_new, d_status = gpu.upload(trees), gpu.upload(indices), gpu.upload(new), gpu.alloc(4)
    d_scr, out = gpu.alloc(gpu.diff_scratch_bytes(16)), Outputs(gpu, 16)
    B.handle.update_async(d_t, d_i, d_new, 4, d_status, stream=s)
    A.handle.diff_async(B.handle, d_scr, out.trees_at, out.idx_at, out.leaves_at, 16, out.info_at, stream=s)
    got_t, got_i, got_lv, info = out.read(stream=s)
    assert int(gpu.download(d_status, 4, stream=s)[0]) == 0
    assert info == dc.counters(case.counts, trees, indices)
    assert (got_t[:4] == trees).all() and (got_i[:4] == indices).all() and (got_lv[:4] == new).all()
    gpu.lib.vkmr_hip_stream_destroy(gpu.index, s)
    for x in (d_t, d_i, d_new, d_status, d_scr, out, A, B):
        x.free()


def test_diff_then_multiproof_on_b_proves_exactly_what_changed(gpu):
    case = dc.case("empty_both_ends", "random_third")
    fa, fb = gpu.build_forest(case.a, case.counts), gpu.build_forest(case.b, case.counts)
    n, H = case.n, fb.levels
    cap = gpu.lib.vkmr_hip_forest_multiproof_max_nodes(fb.total, fb.ntrees, fb.max_count, n)
    d_scr, d_trees, d_idx, d_lv, d_info = gpu.alloc(gpu.diff_scratch_bytes(n)), gpu.alloc(4 * n), gpu.alloc(8 * n), gpu.alloc(32 * n), gpu.alloc(32)
    d_mp = gpu.alloc(gpu.lib.vkmr_hip_forest_multiproof_scratch_bytes(n, H))
    d_nodes, d_h, d_mpinfo = gpu.alloc(32 * cap), gpu.alloc(4 * n), gpu.alloc(8 * (2 + H))
    s = gpu.new_stream()
    fa.diff_async(fb, d_scr, d_trees, d_idx, d_lv, n, d_info, stream=s)
    info = tuple(int(x) for x in gpu.download(d_info, 32, dtype=np.uint64, stream=s))      # the 32 bytes that cross: k for the next call
    assert info == case.info
    fb.multiproof_async(d_trees, d_idx, info[1], d_mp, d_nodes, cap, d_h, d_mpinfo, stream=s)
    mp = gpu.download(d_mpinfo, 8 * (2 + H), dtype=np.uint64, stream=s)
    assert int(mp[0]) == 0
    m = int(mp[1])
    nodes = gpu.download(d_nodes, 32 * m, stream=s).reshape(m, 8)
    leaves, heights = gpu.download(d_lv, 32 * n, stream=s).reshape(n, 8), gpu.download(d_h, 4 * n, stream=s)
    assert (leaves == case.leaves_b).all()
    assert gpu.verify_forest_multiproof(leaves, case.trees, case.indices, heights, nodes, fb.roots())
    assert not gpu.verify_forest_multiproof(leaves, case.trees, case.indices, heights, nodes, fa.roots())
    gpu.lib.vkmr_hip_stream_destroy(gpu.index, s)
    for x in (d_scr, d_trees, d_idx, d_lv, d_info, d_mp, d_nodes, d_h, d_mpinfo, fa, fb):
        x.free()


def test_two_calls_on_one_scratch_back_to_back(gpu):
    """The second call's answer, whatever the first left in the scratch: the larger call first."""
    big, small = dc.case("twenty_thousand", "run_of_8193"), dc.case("side_by_side", "run_of_33")
    A, B = raw_pair(gpu, big)
    C, D = raw_pair(gpu, small)
    d_scr = gpu.alloc(gpu.diff_scratch_bytes(big.n))
    s = gpu.new_stream()
    first = forest_diff(gpu, A, B, big.n, d_scr=d_scr, stream=s)
    out1, out2 = Outputs(gpu, big.n), Outputs(gpu, big.n)
    A.handle.diff_async(B.handle, d_scr, out1.trees_at, out1.idx_at, out1.leaves_at, big.n, out1.info_at, stream=s)
    C.handle.diff_async(D.handle, d_scr, out2.trees_at, out2.idx_at, out2.leaves_at, big.n, out2.info_at, stream=s)
    assert_equals_the_model(big, first, "first call")
    assert_equals_the_model(big, out1.read(stream=s), "the larger call")
    assert_equals_the_model(small, out2.read(stream=s), "the smaller call behind it, same scratch and capacity")
    gpu.lib.vkmr_hip_stream_destroy(gpu.index, s)
    for x in (A, B, C, D, d_scr, out1, out2):
        x.free()
