"""The sort and dedup of leaf entries without a GPU: the C ABI's declarations, sizes and argument checks, the host counterparts
vkmr_host_cpu_forest_sort_entries / vkmr_host_cpu_tree_sort_entries against the rule restated in tests/sort_cases.py, the
plan's replay (tests/c/sort_plan_test.cpp, also under the sanitizers) and the Python layer's argument errors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import merkle_model
import sort_cases as sc
from abi_support import Refusals, assert_bound, assert_exported

NEW = {"vkmr_hip_sort_entries_scratch_bytes": 2, "vkmr_hip_forest_sort_entries_async": 13, "vkmr_hip_tree_sort_entries_async": 9,
       "vkmr_hip_gather_digests_async": 6}


def test_library_exports_the_symbols_and_the_stub_binds_them(native):
    from vk_merkle_roots_amd import _abi
    assert_exported(native.HIP_LIB, NEW)
    for name, nargs in NEW.items():
        assert_bound(name, nparams=nargs)
    assert_exported(native.HOST_LIB, ["vkmr_host_cpu_forest_sort_entries", "vkmr_host_cpu_tree_sort_entries"])
    assert_bound("vkmr_host_cpu_forest_sort_entries", nparams=10, table=_abi.HOST_SIGNATURES, header="vkmr_host.h")
    assert_bound("vkmr_host_cpu_tree_sort_entries", nparams=6, table=_abi.HOST_SIGNATURES, header="vkmr_host.h")


def test_the_model_itself():
    """A self-check of the fixture (no product code): the order, the last occurrence, every kind of entry that is left out."""
    off = [2, 2, 5, 5, 9]                      # trees: empty, [2, 5), empty, [5, 9)
    trees = [3, 1, sc.NO_TREE, 3, 1, 0, 4, 1, 3, sc.NO_TREE, 1]
    idx = [1, 2, 0, 1, 0, 0, 0, 3, 0, sc.NOT_FOUND, 2]
    t, i, o, info = sc.model(off, trees, idx)
    assert list(t) == [1, 1, 3, 3] and list(i) == [0, 2, 0, 1] and list(o) == [4, 10, 8, 3]
    assert info == [4, 2, 3, 2] and sum(info) == len(trees)
    assert list(sc.flat_keys(20, off, trees, idx)) == [6, 4, 20, 6, 2, 20, 20, 20, 5, 20, 4]
    for off in ([], [3]):                      # no tree: markers and out of range alone
        assert sc.model(off, [0, sc.NO_TREE], [0, 0])[3] == [0, 1, 1, 0]
    i, o, info = sc.tree_model(5, [4, sc.NOT_FOUND, 5, 4, 0])
    assert list(i) == [0, 4] and list(o) == [4, 3] and info == [2, 1, 1, 1]


def test_the_plan_constants_can_be_read_and_the_tables_follow_them():
    c = sc.plan_constants()
    assert c["VKMR_SORT_BINS"] == 1 << c["VKMR_SORT_RADIX_BITS"] == c["VKMR_SORT_THREADS"] and c["VKMR_SORT_THREADS"] % 64 == 0
    t = sc.tile_keys()
    assert t == c["VKMR_SORT_THREADS"] * c["VKMR_SORT_KEYS_PER_LANE"]
    ks = sc.k_values()
    assert ks[:4] == (1, 63, 64, 65) and ks[4:8] == (t - 1, t, t + 1, 2 * t + 3)
    assert sc.groups(ks[8] - 1) == c["VKMR_SORT_SCAN_SPAN"] and sc.groups(ks[8]) == c["VKMR_SORT_SCAN_SPAN"] + 1      # the scan's second trip
    assert [sc.passes(total) for total, _ in sc.FORESTS.values()] == [1, 2, 3, 6]
    assert sc.passes(0) == 0 and sc.passes(255) == 1 and sc.passes(256) == 2 and sc.passes(1 << 58) == 8


@pytest.mark.parametrize("k", [0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 16384, 16385, 262145, 1 << 20, (1 << 32) - 1])
def test_scratch_bytes_is_the_layout(native, k):
    from vk_merkle_roots_amd import _abi
    want = sc.scratch_bytes(k)
    assert want % 16 == 0 and want >= 24 * k
    for total in (0, 200, 1 << 40, 1 << 58):
        assert _abi.lib().vkmr_hip_sort_entries_scratch_bytes(total, k) == want, (total, k)


def test_the_forest_call_refuses_bad_arguments_before_any_hip_call(native):
    from vk_merkle_roots_amd import _abi
    d = C.c_void_p(0x1000)                     # never dereferenced: every call below returns before launching anything
    # total, offsets, ntrees, trees, indices, k, scratch, trees_out, indices_out, order_out, info
    sort = Refusals(_abi.lib().vkmr_hip_forest_sort_entries_async, "vkmr_hip_forest_sort_entries_async", good=[100, d, 4, d, d, 5, d, d, d, d, d])
    sort.null(1, 3, 4, 6, 7, 8, 9, 10)         # each pointer NULL
    sort.changed({0: (1 << 58) + 1})           # more leaves than a forest takes
    for bad in (0x1004, 0x1008):               # the scratch is laid out in 16-byte units
        sort.changed({6: C.c_void_p(bad)})
        assert b"16-byte" in _abi.lib().vkmr_hip_last_error()
    sort.changed(*({1: None, 2: 0, i: None} for i in (3, 4, 6, 7, 8, 9, 10)))      # no tree: the offsets alone may be missing
    # k == 0 does nothing whatever the rest
    sort.ok((0, None, 0, None, None, 0, None, None, None, None, None), (1 << 60, None, 7, None, None, 0, C.c_void_p(0x1004), None, None, None, None))


def test_the_tree_call_refuses_bad_arguments_before_any_hip_call(native):
    from vk_merkle_roots_amd import _abi
    d = C.c_void_p(0x1000)
    # count, indices, k, scratch, indices_out, order_out, info
    sort = Refusals(_abi.lib().vkmr_hip_tree_sort_entries_async, "vkmr_hip_tree_sort_entries_async", good=[100, d, 5, d, d, d, d])
    sort.null(1, 3, 4, 5, 6)
    sort.changed({0: (1 << 58) + 1}, {3: C.c_void_p(0x1008)})
    sort.ok((0, None, 0, None, None, None, None), (1 << 60, None, 0, None, None, None, None))


def test_the_gather_refuses_bad_arguments_before_any_hip_call(native):
    from vk_merkle_roots_amd import _abi
    d = C.c_void_p(0x1000)
    gather = Refusals(_abi.lib().vkmr_hip_gather_digests_async, "vkmr_hip_gather_digests_async", good=[d, d, 5, d])      # src, order, n, dst
    gather.null(0, 1, 3)
    gather.ok((None, None, 0, None))


@pytest.mark.parametrize("shape", sc.SHAPES)
@pytest.mark.parametrize("name", sorted(sc.FORESTS))
def test_host_cpu_forest_sort_equals_the_model_on_the_case_tables(native, name, shape):
    for k in sc.k_values():
        case = sc.forest_case(name, shape, k)
        rc, to, io, oo, info = sc.host_cpu_forest_sort(case)
        assert rc == 0
        sc.assert_equals_the_model(case.want, (to, io, oo, info), (name, shape, k))
        n = case.want[3][0]
        assert (to[n:] == sc.PATTERN32).all() and (io[n:] == sc.PATTERN64).all() and (oo[n:] == sc.PATTERN32).all()      # the CPU's writes end at n


@pytest.mark.parametrize("shape", sc.SHAPES)
@pytest.mark.parametrize("name", sorted(sc.FORESTS))
def test_the_case_tables_hold_what_they_promise(name, shape):
    """A self-check of the fixtures against the model (no product code)."""
    t = sc.tile_keys()
    for k in (65, 2 * t + 3):
        case = sc.forest_case(name, shape, k)
        n, markers, outside, repeats = case.want[3]
        keys = sc.flat_keys(case.total, case.offsets, case.trees, case.indices)
        if shape in ("random", "sorted", "reversed", "one_pair", "one_bin"):
            assert markers == outside == 0 and (keys < case.total).all()
        if shape == "sorted":
            assert (np.diff(keys.astype(np.int64)) >= 0).all()
        if shape == "reversed":
            assert (np.diff(keys.astype(np.int64)) <= 0).all() and (name == "total_200" or keys[0] > keys[-1])
        if shape == "one_pair":
            assert n == 1 and repeats == k - 1 and int(case.want[2][0]) == k - 1
        if shape == "one_bin":
            assert len(set(int(x) & 255 for x in keys)) == 1
        if shape == "all_invalid":
            assert n == 0 and markers > 0 and outside > 0 and (keys == case.total).all()
        if shape == "mixed":
            assert n > 0 and markers > 0 and outside > 0
        if shape == "random":
            assert repeats > 0
    if name == "total_2p40":
        case = sc.forest_case(name, "random", 2 * t + 3)
        assert (case.want[0] != 1).all() and set(int(x) for x in case.want[0]) == {0, 2}      # the empty tree is never named
        assert int(sc.flat_keys(case.total, case.offsets, case.trees, case.indices).max()) >> 32 > 0      # the upper key word


@pytest.mark.parametrize("count", sc.TREE_COUNTS)
def test_host_cpu_tree_sort_equals_the_model(native, count):
    for k in sc.k_values():
        idx, want = sc.tree_case(count, k)
        rc, io, oo, info = sc.host_cpu_tree_sort(count, idx)
        assert rc == 0
        sc.assert_equals_the_model((None,) + want, (None, io, oo, info), (count, k))
    idx, want = sc.tree_case(count, 2 * sc.tile_keys() + 3)
    assert min(want[2]) > 0                        # markers, indices past the count and repeats are all there


def test_host_cpu_forest_sort_equals_the_model_on_1000_random_forests(native):
    rng = np.random.default_rng(20240611)
    seen = {"no_tree": 0, "empty_tree": 0, "first_offset": 0, "slack": 0}
    for _ in range(1000):
        case = sc.random_forest_case(rng)
        rc, to, io, oo, info = sc.host_cpu_forest_sort(case)
        assert rc == 0
        if case.k:
            sc.assert_equals_the_model(case.want, (to, io, oo, info), [int(x) for x in case.offsets])
        else:
            assert (info == sc.PATTERN64).all()                        # k == 0 touches nothing
        seen["no_tree"] += case.ntrees == 0
        seen["empty_tree"] += case.ntrees > 0 and bool((np.diff(case.offsets.astype(np.int64)) == 0).any())
        seen["first_offset"] += case.ntrees > 0 and int(case.offsets[0]) > 0
        seen["slack"] += case.ntrees > 0 and case.total > int(case.offsets[-1])
    assert all(v > 50 for v in seen.values()), seen


def test_host_cpu_twins_refuse_bad_offsets_and_missing_pointers(native):
    import vk_merkle_roots_amd as vk
    f = vk.host_lib().vkmr_host_cpu_forest_sort_entries
    trees, idx = np.zeros(5, dtype=np.uint32), np.zeros(5, dtype=np.uint64)
    to, io, oo = np.full(5, sc.PATTERN32, dtype=np.uint32), np.full(5, sc.PATTERN64, dtype=np.uint64), np.full(5, sc.PATTERN32, dtype=np.uint32)
    info = np.full(4, sc.PATTERN64, dtype=np.uint64)
    outs = (to.ctypes.data, io.ctypes.data, oo.ctypes.data, info.ctypes.data)
    for off in ([0, 40, 30, 65], [0, 66]):                     # decreasing; past the total
        o = np.array(off, dtype=np.uint64)
        assert f(65, o.ctypes.data, len(off) - 1, trees.ctypes.data, idx.ctypes.data, 5, *outs) == 1
        assert (to == sc.PATTERN32).all() and (io == sc.PATTERN64).all() and (oo == sc.PATTERN32).all() and (info == sc.PATTERN64).all()
    o = np.array([0, 65], dtype=np.uint64)
    good = [65, o.ctypes.data, 1, trees.ctypes.data, idx.ctypes.data, 5, *outs]
    assert f(*good) == 0 and list(info) == [1, 0, 0, 4]
    for i in (1, 3, 4, 6, 7, 8, 9):
        args = good[:i] + [None] + good[i + 1:]
        assert f(*args) != 0, i
    assert f(0, None, 0, None, None, 0, None, None, None, None) == 0       # no entry: nothing to do
    g = vk.host_lib().vkmr_host_cpu_tree_sort_entries
    assert g(0, None, 0, None, None, None) == 0
    assert g(5, None, 3, io.ctypes.data, oo.ctypes.data, info.ctypes.data) != 0


# ---- the plan's replay: a stand-alone program, compiled here, plain and under the sanitizers ---------------------------------

def write_plan_cases(path):
    """One line per case of the tables: total, k, then the k flat keys (the sentinel for an entry that is left out)."""
    lines = []
    t = sc.tile_keys()
    for name in sorted(sc.FORESTS):
        for shape in sc.SHAPES:
            for k in (1, 63, 64, 65, t - 1, t, t + 1, 2 * t + 3):
                case = sc.forest_case(name, shape, k)
                keys = sc.flat_keys(case.total, case.offsets, case.trees, case.indices)
                lines.append(" ".join([str(case.total), str(k)] + [str(int(x)) for x in keys]))
    case = sc.forest_case("total_65537", "mixed", sc.second_trip_k())      # the scan's second trip, once
    keys = sc.flat_keys(case.total, case.offsets, case.trees, case.indices)
    lines.append(" ".join([str(case.total), str(case.k)] + [str(int(x)) for x in keys]))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return len(lines)


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")], ids=["plain", "asan_ubsan"])
def test_the_plan_replays_every_pass_as_a_stable_permutation(tmp_path, flags):
    exe = str(tmp_path / "sort_plan_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(merkle_model.ROOT, "vk_merkle_roots_amd", "csrc"),
                           os.path.join(merkle_model.ROOT, "tests", "c", "sort_plan_test.cpp"), "-o", exe])
    cases = str(tmp_path / "cases.txt")
    n = write_plan_cases(cases)
    r = subprocess.run([exe, cases], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = r.stdout.decode()
    assert r.returncode == 0 and "FAIL" not in text and f"ok: {n} cases from the tables" in text, text[-2000:]


# ---- the Python layer's argument errors: before any device call ---------------------------------------------------------------

def test_python_layer_refuses_bad_arguments_without_a_device():
    import vk_merkle_roots_amd as vk
    forest = vk.MerkleForest(None, None, 10, [4, 6], None, 6, None, None)      # no device: nothing below may reach one
    tree = vk.MerkleTree(None, None, 10, 4, None)
    d = np.zeros((3, 8), dtype=np.uint32)
    for obj in (forest, tree):
        with pytest.raises(ValueError):
            obj.replace(d, d[:2])                  # one new digest per old digest
        with pytest.raises(ValueError):
            obj.replace(np.zeros((3, 7), dtype=np.uint32), d)
        assert obj.replace(d[:0], d[:0]) == (0, 0)
        with pytest.raises(ValueError):
            obj.multiproof_of(d[:0])
        with pytest.raises(ValueError):
            obj.multiproof_of(np.zeros((2, 5), dtype=np.uint32))
    assert forest.update_entries(None, None, None, 0) == (0, 0, 0)
    assert tree.update_entries(None, None, 0) == (0, 0, 0)
    for name in ("sort_entries_scratch_bytes", "forest_sort_entries_async", "tree_sort_entries_async", "gather_digests_async"):
        assert callable(getattr(vk.HipDevice, name))
    for cls in (vk.MerkleForest, vk.MerkleTree):
        for name in ("sort_entries_async", "update_entries", "replace", "multiproof_of"):
            assert callable(getattr(cls, name))
        assert "LOWEST" in cls.replace.__doc__     # find's rule for a digest held by several leaves is stated
