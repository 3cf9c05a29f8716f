"""The diff of two stored forests or trees without a GPU: the C ABI's declarations, the scratch layout and the argument checks,
the Python layer's argument errors, and tests/c/diff_plan_test.cpp -- whole descents replayed through csrc/diff_plan.hpp's own
functions, plain and under ASan/UBSan -- against the model in tests/diff_cases.py."""
import ctypes as C

import numpy as np
import pytest

import diff_cases as dc
import merkle_model
from abi_support import Refusals, assert_bound, assert_exported
from no_device import NoDeviceAt as NoDevice

NEW = {"vkmr_hip_diff_scratch_bytes": 1, "vkmr_hip_forest_diff_async": 18, "vkmr_hip_tree_diff_async": 13}


def test_library_exports_the_symbols_and_the_stub_binds_them(native):
    assert_exported(native.HIP_LIB, NEW)
    for name, nargs in NEW.items():
        assert_bound(name, nparams=nargs)


def test_the_model_itself():
    """A self-check of the fixture (no product code): cells outside the trees are never compared, an empty tree is never
    named, any one of the 32 bytes makes a leaf differ, and the counters are those of the changed paths."""
    a = np.arange(8 * 12, dtype=np.uint32).reshape(12, 8)
    b = a.copy()
    b[0, 0] ^= 1                               # in front of tree 0
    b[11, 7] ^= 1                              # behind the last tree
    b[1, 0] ^= 1                               # tree 1, leaf 0
    b[5, 7] ^= 1 << 31                         # tree 1, leaf 4 of 5: the last byte
    b[6, 3] ^= 2                               # tree 4, leaf 0
    off = [1, 1, 6, 6, 6, 10]                  # trees: empty, [1, 6), empty, empty, [6, 10); cells 0, 10 and 11 belong to none
    trees, idx = dc.model(a, b, off)
    assert list(trees) == [1, 1, 4] and list(idx) == [0, 4, 0]
    # tree 1 (5 leaves, height 3): leaf 0 -> (1,0) (2,0) (3,0); leaf 4 -> (1,2) (2,1) (3,0): 5 nodes; tree 4 (4 leaves): 2 nodes
    assert dc.counters([0, 5, 0, 0, 4], trees, idx) == (0, 3, 2, 7)
    assert dc.model(a, a, off)[0].shape == (0,) and dc.model(a, b, [])[0].shape == (0,)
    assert dc.tree_counters(5, 3, [0, 4]) == (0, 2, 1, 5) and dc.tree_counters(5, 4, [4]) == (0, 1, 1, 4) and dc.tree_counters(1, 0, [0]) == (0, 1, 1, 0)


@pytest.mark.parametrize("name,change", dc.SMALL_PAIRS)
def test_the_change_sets_hold_what_they_promise(name, change):
    case = dc.case(name, change)
    want = dc.entries_of(name, change)
    assert (case.trees == want[0]).all() and (case.indices == want[1]).all() and case.info[1] == case.n
    assert (case.window(case.a) != case.window(case.b)).any(axis=1).sum() == case.n
    if case.first:
        assert (case.a[: case.first] != case.b[: case.first]).any() and (case.a[-case.slack:] != case.b[-case.slack:]).any()
    if change == "odd_last" and name == "tiny_trees":
        assert list(zip(case.trees, case.indices)) == [(0, 0), (2, 2), (3, 4)]          # leaf 4 of 5 among them
    if change.startswith("run_of_"):
        assert case.n == int(change[7:]) and len(set(case.trees)) == 1 and (np.diff(case.indices.astype(np.int64)) == 1).all()


@pytest.mark.parametrize("capacity", [0, 1, 31, 32, 33, 8191, 8192, 8193, 2**32 - 1])
def test_scratch_bytes_is_the_layout(native, capacity):
    from vk_merkle_roots_amd import _abi
    c = dc.plan_constants()
    assert c == {"VKMR_DIFF_THREADS": 256, "VKMR_DIFF_WORD_ENTRIES": 32, "VKMR_DIFF_RANK_BLOCK_WORDS": 256, "VKMR_DIFF_ROOT_GROUPS": 1024,
                 "VKMR_DIFF_HEADER_WORDS": 6}
    want = dc.scratch_bytes(capacity)
    assert want % 16 == 0 and want >= 24 * capacity + capacity // 2 + 8 * 1024 + 48
    assert _abi.lib().vkmr_hip_diff_scratch_bytes(capacity) == want
    if capacity == 33:                         # written out once by hand: 2 * 272 + 2 * 144 + 2 * 16 + 8192 + 48
        assert want == 544 + 288 + 32 + 8192 + 48


def test_the_forest_call_refuses_bad_arguments_before_any_hip_call(native):
    from vk_merkle_roots_amd import _abi
    lib = _abi.lib()
    d = C.c_void_p(0x1000)                     # never dereferenced: every call below returns before launching anything
    # digests_a, forest_a, roots_a, digests_b, forest_b, roots_b, total, offsets, ntrees, max_count, scratch, trees_out, indices_out, leaves_b_out, capacity, info
    diff = Refusals(lib.vkmr_hip_forest_diff_async, "vkmr_hip_forest_diff_async", good=[d, d, d, d, d, d, 100, d, 4, 50, d, d, d, None, 8, d])
    diff.null(0, 1, 2, 3, 4, 5, 7, 10, 11, 12, 15)      # each pointer NULL where it is needed; B's leaves are optional
    diff.changed({9: 0}, {6: (1 << 58) + 1}, {10: C.c_void_p(0x1008)})         # no max_count, too many leaves, scratch off the 16-byte grid
    # capacity 0: the outputs may be missing -- the scratch and the counters may not
    diff.changed(*({11: None, 12: None, 14: 0, i: None} for i in (10, 15)))
    # no tree: nothing to do, whatever the rest
    diff.ok((None, None, None, None, None, None, 1 << 60, None, 0, 0, None, None, None, None, 7, None))


def test_the_tree_call_refuses_bad_arguments_before_any_hip_call(native):
    from vk_merkle_roots_amd import _abi
    lib = _abi.lib()
    d = C.c_void_p(0x1000)
    # digests_a, tree_a, digests_b, tree_b, count, height, scratch, indices_out, leaves_b_out, capacity, info
    diff = Refusals(lib.vkmr_hip_tree_diff_async, "vkmr_hip_tree_diff_async", good=[d, d, d, d, 100, 7, d, d, None, 8, d])
    diff.null(0, 1, 2, 3, 6, 7, 10)
    for count, height in ((100, 6), (100, 64), (1 << 59, 59)):                 # as vkmr_hip_tree_proofs_async refuses a height; too many leaves
        diff.changed({4: count, 5: height})
        assert lib.vkmr_hip_tree_proofs_async(0, None, d, d, count, height, d, 1, d) == _abi.ERR_INVALID or count > (1 << 58)
    diff.changed({6: C.c_void_p(0x1004)})
    # one leaf and no level: the tree buffers may be missing, the rest may not
    diff.changed(*({1: None, 3: None, 4: 1, 5: 0, i: None} for i in (0, 2, 6, 10)))
    # no leaf: nothing to do, whatever the rest
    diff.ok((None, None, None, None, 0, 99, None, None, None, 7, None))


def test_the_python_layer_refuses_other_shapes_before_any_device_call():
    import vk_merkle_roots_amd as vk
    forest = lambda dev, counts, max_count: vk.MerkleForest(NoDevice(dev), None, sum(counts), counts, None, max_count, None, None)      # noqa: E731
    a = forest(0, [5, 0, 9], 9)
    for other in (forest(1, [5, 0, 9], 9), forest(0, [5, 1, 8], 9), forest(0, [5, 0, 9, 0], 9), forest(0, [5, 0, 9], 10), None,
                  vk.MerkleTree(NoDevice(0), None, 14, 4, None)):
        for call in (lambda: a.diff(other), lambda: a.sync_from(other), lambda: a.diff_async(other, None, None, None, None, 4, None)):
            with pytest.raises(ValueError):
                call()
    same = forest(0, [5, 0, 9], 9)
    for capacity in (-1, 2**32):
        with pytest.raises(ValueError):
            a.diff(same, capacity=capacity)
    tree = lambda dev, count, height: vk.MerkleTree(NoDevice(dev), None, count, height, None)      # noqa: E731
    t = tree(0, 14, 4)
    for other in (tree(1, 14, 4), tree(0, 15, 4), tree(0, 14, 5), None, a):
        for call in (lambda: t.diff(other), lambda: t.sync_from(other), lambda: t.diff_async(other, None, None, None, 4, None)):
            with pytest.raises(ValueError):
                call()
    with pytest.raises(ValueError):
        t.diff(tree(0, 14, 4), capacity=2**32)
    assert issubclass(vk.DiffOverflow, RuntimeError)


# ---- the plan header replayed ---------------------------------------------------------------------------------------------------

def capacities(case, few):
    n = case.n
    return sorted({n, max(n - 1, 0)} if few else {n, max(n - 1, 0), 0, n // 2, n + 7})


def assert_replay_equals_the_model(rows, lines, cases):
    for row, line, case in zip(rows, lines, cases):
        status, n, roots, compared, H = row
        capacity = line[3]
        if capacity >= case.n:
            assert (status, n, roots, compared) == case.info, (case.name, case.change, capacity, row)
        else:
            assert status == dc.OVERFLOW and n > capacity and roots == case.info[2], (case.name, case.change, capacity, row)
        assert H == merkle_model.tree_height(min(case.max_count, case.total)) if case.total else H == 1


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_the_descent_replayed_through_the_plan_equals_the_model_on_every_table(tmp_path, sanitize):
    exe = dc.build_diff_plan_exe(tmp_path, sanitize)
    lines, cases = [], []
    for name, change in dc.PAIRS:
        case = dc.case(name, change)
        for capacity in capacities(case, few=case.total > 6000):
            lines.append(case.plan_line(capacity))
            cases.append(case)
    assert_replay_equals_the_model(dc.plan_replay(exe, tmp_path, lines), lines, cases)


class RandomCase:
    def __init__(self, rng):
        self.counts = []
        while not self.counts:                 # a first tree above the budget leaves no tree at all: the call then does nothing
            self.counts = merkle_model.random_counts(rng, 3000)
        self.first, self.slack = (int(x) for x in rng.integers(0, 9, size=2))
        self.max_count = max(max(self.counts, default=0), 1) + int(rng.integers(0, 3)) * 100
        self.total = self.first + sum(self.counts) + self.slack
        self.name, self.change = "random", tuple(self.counts)
        every = [(t, i) for t, c in enumerate(self.counts) for i in range(c)]
        kind = int(rng.integers(0, 4))
        k = 0 if not every else [0, 1, max(1, len(every) // 50), max(1, len(every) // 3)][kind]
        pick = rng.choice(len(every), size=min(k, len(every)), replace=False) if k else []
        self.trees, self.indices = dc.fu.sorted_entries([every[int(j)] for j in pick])
        self.n = int(self.trees.shape[0])
        self.info = dc.counters(self.counts, self.trees, self.indices)
        self.capacity = [self.n, max(self.n - 1, 0), self.n + 1, self.n // 3][int(rng.integers(0, 4))]


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_the_descent_replayed_through_the_plan_equals_the_model_on_1000_random_forests(tmp_path, sanitize):
    exe = dc.build_diff_plan_exe(tmp_path, sanitize)
    rng = np.random.default_rng(dc.seed_of("random forests"))
    cases = [RandomCase(rng) for _ in range(1000)]
    lines = [(c.first, c.slack, c.max_count, c.capacity, c.counts, c.trees, c.indices) for c in cases]
    assert sum(1 for c in cases if c.capacity < c.n) > 100 and sum(1 for c in cases if c.n == 0) > 100
    assert_replay_equals_the_model(dc.plan_replay(exe, tmp_path, lines, "random_diffs.txt"), lines, cases)
