"""Stored forests that grow, without a GPU: the C ABI's declarations and argument checks (vkmr_hip_forest_append_async,
vkmr_hip_forest_truncate_async), the host-side checks of MerkleForest.append, append_packed and truncate and of the builds
that reserve room, and the range rule of csrc/forest_plan.hpp replayed on the CPU with forest_append_level_kernel's own tests
(tests/c/forest_append_plan_test.cpp).  No compute calls here: every case returns before the library or the Python layer
touches HIP."""
import ctypes as C

import numpy as np
import pytest

import forest_append_cases as fa
import forest_cases as fc
from abi_support import Refusals, assert_bound, assert_exported, assert_key_resolves, assert_no_spills, isa_record
from merkle_model import random_counts
from no_device import NoDevice

APPEND, TRUNCATE = "vkmr_hip_forest_append_async", "vkmr_hip_forest_truncate_async"
LEVEL_KERNELS = ("forest_append_level_kernel", "forest_append_level_flagged_kernel")


def test_header_declares_both_and_the_stub_binds_every_argument():
    # dev, stream, digests, forest, total, offsets, ntrees, max_count, first_tree, used, leaves, n_leaves, new_offsets, m, roots,
    # mutated, status: seventeen; dev, stream, offsets, ntrees, keep_trees, roots: six
    for name, nparams, scalars in ((APPEND, 17, [C.c_int, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32]),
                                   (TRUNCATE, 6, [C.c_int, C.c_uint32, C.c_uint32])):
        assert_bound(name, nparams=nparams, scalars=scalars, restype=C.c_int)


def test_library_exports_both(native):
    assert_exported(native.HIP_LIB, [APPEND, TRUNCATE])


def test_bad_arguments_are_refused_before_any_hip_call(native):
    from vk_merkle_roots_amd import _abi
    lib = _abi.lib()
    d = C.c_void_p(0x1000)                 # never dereferenced: every call below returns before launching anything
    # digests, forest, total, offsets, ntrees, max_count, first_tree, used, leaves, n_leaves, new_offsets, m, roots, mutated, status
    append = Refusals(lib.vkmr_hip_forest_append_async, APPEND, good=[d, d, 100, d, 8, 50, 4, 60, d, 30, d, 3, d, None, d])
    append.null(0, 1, 3, 8, 10, 12, 14)    # each needed pointer NULL with m > 0 (mutated, 13, is NULL in `good` already)
    # first_tree + m > ntrees (also past 2^32), used + n_leaves > total (also past 2^64), max_count == 0, too many leaves
    append.changed({6: 6}, {11: 5}, {6: 9}, {6: 2**32 - 1, 11: 2}, {9: 41}, {7: 71}, {7: 101, 9: 0}, {7: 2**64 - 1, 9: 2}, {5: 0},
                   {2: (1 << 58) + 1})
    # m == 0 is a no-op whatever the rest
    append.ok((None, None, 100, None, 8, 50, 4, 60, None, 0, None, 0, None, None, None), (None, None, 0, None, 0, 0, 9, 9, None, 9, None, 0, None, None, None),
              (d, d, (1 << 58) + 1, d, 4, 0, 9, 0, d, 5, d, 0, d, d, d))

    truncate = Refusals(lib.vkmr_hip_forest_truncate_async, TRUNCATE, good=[d, 8, 3, d])              # offsets, ntrees, keep_trees, roots
    truncate.null(0, 3)
    truncate.changed({2: 9}, {0: None, 2: 9, 3: None}, {1: 0, 2: 1})                                  # keep_trees > ntrees
    truncate.ok((None, 8, 8, None), (None, 0, 0, None))                                               # keep_trees == ntrees: nothing to do


def host_forest(counts=(4, 0, 7, 0, 0, 0), total=20, max_count=8, used_trees=3):
    import vk_merkle_roots_amd as vk
    return vk.MerkleForest(NoDevice(), None, total, list(counts), None, max_count, None, None, used_trees=used_trees)


def test_the_handle_knows_its_room(native):
    f = host_forest()
    assert (f.ntrees, f.used_trees, f.free_trees, f.total, f.used_leaves, f.free_leaves) == (6, 3, 3, 20, 11, 9)
    import vk_merkle_roots_amd as vk
    full = vk.MerkleForest(NoDevice(), None, 11, [4, 0, 7], None, 7, None, None)       # as every build without a reserve makes it
    assert (full.used_trees, full.free_trees, full.used_leaves, full.free_leaves) == (3, 0, 11, 0)


@pytest.mark.parametrize("n,counts", [(9, [3, 3, 2, 1]),        # four trees, room for three
                                      (10, [5, 5]),             # ten leaves, room for nine
                                      (9, [9]),                 # a count above max_count
                                      (6, [3, 2]), (5, [3, 3]), (0, [1]), (3, []),   # counts that do not add up to the digests
                                      (3, [4, -1])])
def test_append_refuses_on_the_host(native, n, counts):
    with pytest.raises(ValueError):
        host_forest().append(np.zeros((n, 8), np.uint32), counts)
    with pytest.raises(ValueError):
        host_forest().append(np.zeros((n, 8), np.uint32), counts, mutated=True)


def test_append_of_no_tree_touches_no_device(native):
    f = host_forest()
    assert f.append(np.zeros((0, 8), np.uint32), []).shape == (0,)
    trees, masks = f.append(np.zeros((0, 8), np.uint32), [], mutated=True)
    assert trees.shape == (0,) and masks.shape == (0,) and f.used_trees == 3


def test_append_packed_refuses_before_any_device_call(native):
    import vk_merkle_roots_amd as vk
    batch = vk.pack_lines(b"a\nb\nc\n")
    assert batch.count == 3
    for counts in ([2], [2, 2], [1, 1, 1, 0], [3, 0, 0, 0]):   # do not add up; more trees than there is room for
        with pytest.raises(ValueError):
            host_forest().append_packed(batch, counts)
    with pytest.raises(ValueError):
        host_forest(max_count=2).append_packed(batch, [3])
    with pytest.raises(ValueError):
        host_forest(total=13).append_packed(batch, [3])         # two free cells


def test_truncate_refuses_trees_that_are_not_in_use(native):
    for keep in (4, 6, 7, -1):
        with pytest.raises(ValueError):
            host_forest().truncate(keep)


def test_a_reserve_needs_an_explicit_max_count(native):
    import vk_merkle_roots_amd as vk
    from vk_merkle_roots_amd import engine
    batch = vk.pack_lines(b"a\nb\nc\n")
    dev = object.__new__(vk.HipDevice)                          # never initialised: any device call is an AttributeError
    for reserve in ({"reserve_trees": 2}, {"reserve_leaves": 5}, {"reserve_trees": 1, "reserve_leaves": 1}):
        with pytest.raises(ValueError, match="max_count"):
            dev.build_forest(np.zeros((3, 8), np.uint32), [3], **reserve)
        with pytest.raises(ValueError, match="max_count"):
            vk.merkle_forest_packed(dev, batch, [3], **reserve)
    with pytest.raises(ValueError):
        dev.build_forest(np.zeros((3, 8), np.uint32), [3], max_count=4, reserve_trees=-1)
    # the counts are those of the leaves at hand, the slack apart
    assert engine._checked_offsets([4, 0, 7], 20, "t", slack=9)[1] == 3
    with pytest.raises(ValueError):
        engine._checked_offsets([4, 0, 7], 20, "t", slack=8)
    with pytest.raises(ValueError):
        engine._checked_offsets([4, 0, 7], 20, "t")


def test_diff_needs_equal_counts_and_equal_capacity(native):
    a = host_forest()
    for other in (host_forest(total=21), host_forest(counts=(4, 0, 7, 0, 0)), host_forest(counts=(4, 0, 7, 1, 0, 0), used_trees=4),
                  host_forest(max_count=9)):
        other.dev = a.dev = type("D", (), {"index": 0})()
        with pytest.raises(ValueError):
            a._same_shape(other, "diff")
    same = host_forest()
    same.dev = a.dev
    a._same_shape(same, "diff")
    cells, of = a._entry_cells(np.array([0, 2, 2], dtype=np.uint32), np.array([3, 0, 6], dtype=np.uint64))
    assert cells.tolist() == [3, 4, 10] and of.tolist() == [4, 7, 7]


def test_status_text_names_the_bits(native):
    import vk_merkle_roots_amd as vk
    text = vk.forest_append_status_text
    assert text(0) == "ok"
    for bit in range(3):
        assert [f"bit {b}" in text(1 << bit) for b in range(3)] == [b == bit for b in range(3)]
    assert all(f"bit {b}" in text(7) for b in range(3)) and "unknown" not in text(7)
    assert "unknown" in text(8)


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    return fa.build_append_plan_exe(tmp_path_factory.mktemp("forest_append_plan"))


def check_replay(plan_exe, directory, cases):
    got = fa.plan_replay(plan_exe, directory, cases)
    for (first, slack, max_count, split, counts), (H, cells, roots, lanes) in zip(cases, got):
        total = first + sum(counts) + slack
        assert H == fa.fu.fp.stride_of(total, max_count or max(1, max(counts)))
        assert (cells, roots) == fa.written(counts, split), (first, slack, max_count, split, counts[:10])
        # the range restriction: a launch covers the new trees' cells and under one wavefront more, never the whole level
        new_leaves, m = sum(counts[split:]), len(counts) - split
        assert lanes <= sum((new_leaves >> l) + m + 1 + 63 for l in range(1, H + 1)), (split, counts[:10])


def test_the_level_ranges_replayed_over_every_case_table(native, plan_exe, tmp_path):
    cases = []
    for name, counts in sorted(fc.CASES.items()):
        largest = max(1, max(counts))
        for first, slack in ((0, 0), (5, 7)):
            for split in fa.split_points(len(counts)):
                for max_count in (0, 1 << fc.ceil_log2(largest), 2**63):
                    cases.append((first, slack, max_count, split, counts))
    check_replay(plan_exe, tmp_path, cases)


def test_the_level_ranges_replayed_over_a_thousand_random_forests(native, plan_exe, tmp_path):
    rng = np.random.default_rng(20261)
    cases = []
    while len(cases) < 1000:
        counts = random_counts(rng, 1 << 13)
        if not counts:
            continue
        first, slack = (int(rng.integers(1, 1000)), int(rng.integers(1, 1000))) if rng.integers(0, 2) else (0, 0)
        max_count = (0, max(counts) + int(rng.integers(0, 5000)), 2**64 - 1)[len(cases) % 3]
        cases.append((first, slack, max_count, int(rng.integers(0, len(counts))), counts))
    check_replay(plan_exe, tmp_path, cases)


def test_the_append_level_kernels_hold_one_hash_block_and_the_build_lists_them(native):
    from vk_merkle_roots_amd import isa_prio_pass
    keys = isa_prio_pass.EXPECTED_HASH_BLOCKS
    for mine in LEVEL_KERNELS:
        assert keys[mine] == 1
        assert_key_resolves(mine)
    rec = isa_record(native)
    if rec is not None:                    # written by a build that ran the issue pass (tests/test_isa_prio_pass.py covers its absence)
        assert rec["audit"]["block_count_errors"] == [] and rec["audit"]["unclassified"] == []
        mine = {k: v for k, v in rec["audit"]["blocks"].items() if "forest_append" in k or "forest_truncate" in k}
        assert sorted(mine.values()) == [1, 1] and all(any(n in k for n in LEVEL_KERNELS) for k in mine)   # the check, leaves, offsets, truncate: none
    assert_no_spills(native, LEVEL_KERNELS, max_vgprs=64)  # 512 registers a lane, 8 wavefronts per SIMD
