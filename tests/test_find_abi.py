"""The lookup by digest without a GPU: the C ABI's declarations, sizes and argument checks, and the host counterparts
vkmr_host_cpu_forest_find / vkmr_host_cpu_tree_find against the rule restated in tests/find_cases.py."""
import ctypes as C

import numpy as np
import pytest

import find_cases as fd
from abi_support import Refusals, assert_bound, assert_exported

NEW = {"vkmr_hip_find_scratch_bytes": 1, "vkmr_hip_forest_find_async": 11, "vkmr_hip_tree_find_async": 8}


def assert_equals_the_model(case, trees, indices, what):
    assert (indices == case.indices).all(), (what, np.nonzero(indices != case.indices)[0][:10])
    if trees is not None:
        assert (trees == case.trees).all(), (what, np.nonzero(trees != case.trees)[0][:10])


def test_library_exports_the_symbols_and_the_stub_binds_them(native):
    from vk_merkle_roots_amd import _abi
    assert_exported(native.HIP_LIB, NEW)
    for name, nargs in NEW.items():
        assert_bound(name, nparams=nargs)
    assert_exported(native.HOST_LIB, ["vkmr_host_cpu_forest_find", "vkmr_host_cpu_tree_find"])
    assert_bound("vkmr_host_cpu_forest_find", nparams=8, table=_abi.HOST_SIGNATURES, header="vkmr_host.h")
    assert_bound("vkmr_host_cpu_tree_find", nparams=5, table=_abi.HOST_SIGNATURES, header="vkmr_host.h")


def test_the_model_itself():
    """A self-check of the fixture (no product code): lowest position, empty trees never named, cells outside never found."""
    cells = np.arange(8 * 10, dtype=np.uint32).reshape(10, 8)
    cells[6] = cells[2]
    cells[9] = cells[0]
    off = [1, 1, 4, 4, 4, 8]                   # trees: empty, [1, 4), empty, empty, [4, 8); cells 0, 8 and 9 belong to none
    trees, idx = fd.model(cells, off, cells[[2, 6, 1, 7, 0, 9, 4]])
    assert list(trees) == [1, 1, 1, 4, fd.NO_TREE, fd.NO_TREE, 4]
    assert list(idx) == [1, 1, 0, 3, fd.NOT_FOUND, fd.NOT_FOUND, 0]
    for off in ([], [3]):
        trees, idx = fd.model(cells, off, cells[:2])
        assert list(trees) == [fd.NO_TREE] * 2 and list(idx) == [fd.NOT_FOUND] * 2


@pytest.mark.parametrize("k", [0, 1, 32, 33, 1 << 20, 1 << 31])
def test_scratch_bytes_is_the_formula(native, k):
    from vk_merkle_roots_amd import _abi
    t = max(64, 1 << (2 * k - 1).bit_length()) if k else 64       # the smallest power of two >= max(64, 2k), written another way
    assert t == fd.table_slots(k) and t >= 2 * k and (t == 64 or t < 4 * k)
    want = (8 * t + 8 * k + 4 * k + 15) & ~15
    assert fd.scratch_bytes(k) == want
    assert _abi.lib().vkmr_hip_find_scratch_bytes(k) == want


def test_the_table_doubles_between_32_and_33():
    assert fd.table_slots(32) == 64 and fd.table_slots(33) == 128 and fd.table_slots(1000) == 2048


def test_the_plan_constants_can_be_read():
    c = fd.plan_constants()
    assert c["VKMR_FIND_MIN_SLOTS"] == 64 and c["VKMR_FIND_THREADS"] % 64 == 0
    assert fd.second_trip_total(256) == 256 * c["VKMR_FIND_GROUPS_PER_CU"] * c["VKMR_FIND_THREADS"] * c["VKMR_FIND_LEAVES_PER_LANE"] + 1


def test_the_forest_call_refuses_bad_arguments_before_any_hip_call(native):
    from vk_merkle_roots_amd import _abi
    d = C.c_void_p(0x1000)                     # never dereferenced: every call below returns before launching anything
    # digests, total, offsets, ntrees, queries, k, scratch, trees, indices
    find = Refusals(_abi.lib().vkmr_hip_forest_find_async, "vkmr_hip_forest_find_async", good=[d, 100, d, 4, d, 5, d, d, d])
    find.null(0, 2, 4, 6, 7, 8)                # each pointer NULL where it is needed
    find.changed({1: (1 << 58) + 1}, {6: C.c_void_p(0x1004)})      # more leaves than a forest takes; the slots are 8-byte words
    for total, ntrees in ((0, 4), (100, 0)):   # without a leaf the queries, the scratch and the outputs are still needed
        find.changed(*({0: None, 1: total, 2: d if ntrees else None, 3: ntrees, i: None} for i in (4, 6, 7, 8)))
    # k == 0 does nothing whatever the rest
    find.ok((None, 0, None, 0, None, 0, None, None, None), (None, (1 << 60), None, 7, None, 0, None, None, None))


def test_the_tree_call_refuses_bad_arguments_before_any_hip_call(native):
    from vk_merkle_roots_amd import _abi
    d = C.c_void_p(0x1000)
    # digests, count, queries, k, scratch, indices
    find = Refusals(_abi.lib().vkmr_hip_tree_find_async, "vkmr_hip_tree_find_async", good=[d, 100, d, 5, d, d])
    find.null(0, 2, 4, 5)
    find.changed({1: (1 << 58) + 1})
    find.changed(*({0: None, 1: 0, i: None} for i in (2, 4, 5)))   # count == 0: the leaves alone may be missing
    find.ok((None, 0, None, 0, None, None), (None, (1 << 60), None, 0, None, None))


@pytest.mark.parametrize("variant", fd.VARIANTS)
@pytest.mark.parametrize("name", sorted(fd.FORESTS))
def test_host_cpu_forest_find_equals_the_model_on_the_query_sets(native, name, variant):
    case = fd.forest_case(name, variant)
    rc, trees, indices = fd.host_cpu_forest_find(case)
    assert rc == 0
    assert_equals_the_model(case, trees, indices, (name, variant))


@pytest.mark.parametrize("variant", fd.VARIANTS)
@pytest.mark.parametrize("name", sorted(fd.FORESTS))
def test_the_query_sets_hold_what_they_promise(name, variant):
    """A self-check of the fixtures against the model (no product code): each kind of query is there and has the fate it was
    planted for."""
    case = fd.forest_case(name, variant)
    notes, found = case.notes, case.found()
    off = [int(x) for x in case.offsets]
    flat = lambda q: off[int(case.trees[q])] + int(case.indices[q])       # noqa: E731
    for what in ("first_of_forest", "last_of_forest", "first_of_a_tree", "last_of_a_tree", "three_times", "twice_in_one_tree"):
        assert all(found[q] for q in notes[what]), what
    for what in ("absent", "absent_but_for_word_7", "absent_but_for_word_0", "a_root", "a_level_1_node"):
        assert not any(found[q] for q in notes[what]), what
    assert flat(notes["first_of_forest"][0]) == off[0] and flat(notes["last_of_forest"][0]) == off[-1] - 1
    assert len(notes["three_times"]) == 3 and len({flat(q) for q in notes["three_times"]}) == 1
    assert found[notes["zero"][0]] == (variant == "zero_is_a_leaf") and found[notes["ones"][0]] == (variant == "ones_is_a_leaf")
    assert flat(notes["twice_in_one_tree"][0]) == case.inside[0] and int(case.trees[notes["twice_in_one_tree"][0]]) == case.big
    if case.others:
        assert int(case.trees[notes["in_two_trees"][0]]) == min(case.others)
    if any(c == 0 for c in case.counts):
        assert notes["beside_an_empty_tree"] and all(found[q] for q in notes["beside_an_empty_tree"])
    if "outside_the_window" in notes:
        assert off[0] > 0 and off[-1] < case.total and not found[notes["outside_the_window"][0]]
    for t in set(int(t) for t in case.trees[found]):
        assert case.counts[t] > 0                  # an empty tree is never named


@pytest.mark.parametrize("k", fd.CHAIN_K)
def test_host_cpu_forest_find_equals_the_model_on_the_chains(native, k):
    for wrap in (False, True):
        for parity in (0, 1):
            case = fd.chain_case(k, wrap, parity)
            assert len(set(case.queries[:, 0])) == 1
            if wrap:
                assert int(case.queries[0, 0]) & (fd.table_slots(k) - 1) == fd.table_slots(k) - 1
            rc, trees, indices = fd.host_cpu_forest_find(case)
            assert rc == 0
            assert_equals_the_model(case, trees, indices, (k, wrap, parity))
            if k < 500:                            # every plant has a cell of its own
                assert [q for q in range(k) if case.found()[q]] == case.notes["present"]
                assert case.found()[k - 1] == ((k - 1) % 2 == parity)


def test_host_cpu_finds_the_first_of_all_equal_leaves(native):
    case = fd.all_equal_case()
    assert list(case.trees) == [2, fd.NO_TREE, 2] and list(case.indices) == [0, fd.NOT_FOUND, 0]
    rc, trees, indices = fd.host_cpu_forest_find(case)
    assert rc == 0
    assert_equals_the_model(case, trees, indices, "all equal")


@pytest.mark.parametrize("total", fd.TOTALS)
def test_host_cpu_twins_equal_the_model_at_every_size(native, total):
    for k in fd.KS:
        case = fd.size_case(total, k)
        rc, trees, indices = fd.host_cpu_forest_find(case)
        assert rc == 0
        assert_equals_the_model(case, trees, indices, (total, k))
        rc, flat = fd.host_cpu_tree_find(case.cells, case.queries)      # the same cells as one tree: the flat positions
        want = fd.model(case.cells, [0, total], case.queries)[1]
        assert rc == 0 and (flat == want).all()
        assert case.found().sum() >= (k + 1) // 2 > 0


def test_host_cpu_twins_without_a_leaf_and_with_bad_arguments(native):
    import vk_merkle_roots_amd as vk
    queries = fd.size_case(65, 63).queries
    for offsets in ([0, 0, 0], [0, 0], [0]):                   # every tree empty; no tree at all
        case = fd.Case(np.zeros((0, 8), np.uint32), offsets, queries)
        rc, trees, indices = fd.host_cpu_forest_find(case)
        assert rc == 0 and (trees == fd.NO_TREE).all() and (indices == fd.NOT_FOUND).all()
    rc, indices = fd.host_cpu_tree_find(np.zeros((0, 8), np.uint32), queries)
    assert rc == 0 and (indices == fd.NOT_FOUND).all()
    f = vk.host_lib().vkmr_host_cpu_forest_find
    cells = fd.size_case(65, 63).cells
    out_t, out_i = np.full(63, 0xA5A5A5A5, dtype=np.uint32), np.full(63, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    for off in ([0, 40, 30, 65], [0, 66]):                     # decreasing; past the cells
        o = np.array(off, dtype=np.uint64)
        assert f(cells.ctypes.data, 65, o.ctypes.data, len(off) - 1, queries.ctypes.data, 63, out_t.ctypes.data, out_i.ctypes.data) == 1
        assert (out_t == 0xA5A5A5A5).all() and (out_i == 0xA5A5A5A5A5A5A5A5).all()      # nothing written
    o = np.array([0, 65], dtype=np.uint64)
    assert f(None, 65, o.ctypes.data, 1, queries.ctypes.data, 63, out_t.ctypes.data, out_i.ctypes.data) != 0      # leaves missing
    assert f(cells.ctypes.data, 65, o.ctypes.data, 1, None, 63, out_t.ctypes.data, out_i.ctypes.data) != 0
    assert f(None, 0, None, 0, None, 0, None, None) == 0                                # no query: nothing to do
    assert vk.host_lib().vkmr_host_cpu_tree_find(None, 0, None, 0, None) == 0


def test_python_layer_exports_the_sentinels():
    import vk_merkle_roots_amd as vk
    assert vk.NO_TREE == fd.NO_TREE and vk.NOT_FOUND == fd.NOT_FOUND
