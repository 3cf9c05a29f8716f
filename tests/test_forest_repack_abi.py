"""Forests that slide, without a GPU: the C ABI's declarations and argument checks (vkmr_hip_forest_drop_front_async,
vkmr_hip_forest_copy_trees_async), the host-side checks of MerkleForest.drop_front, append_from and repacked, and the copy and
drop rules of csrc/forest_plan.hpp replayed on the CPU with values (tests/c/forest_copy_plan_test.cpp).  No compute calls here:
every case returns before the library or the Python layer touches HIP."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import forest_cases as fc
import forest_repack_cases as fr
from abi_support import Refusals, assert_bound, assert_exported, isa_record
from conftest import ROOT
from no_device import NoDevice

DROP, COPY = "vkmr_hip_forest_drop_front_async", "vkmr_hip_forest_copy_trees_async"
KERNELS = ("forest_drop_front_kernel", "forest_copy_check_kernel", "forest_copy_level_kernel")


def test_header_declares_both_and_the_stub_binds_every_argument():
    u32, u64 = C.c_uint32, C.c_uint64
    # dev, stream, offsets, ntrees, drop_trees, roots, mutated: seven; the copy: dev, stream, eight of the source, sel, m, n_leaves,
    # new_offsets, ten of the destination, status: twenty-five
    for name, nparams, scalars in ((DROP, 7, [C.c_int, u32, u32]), (COPY, 25, [C.c_int, u64, u32, u64, u32, u64, u64, u32, u64, u32, u64])):
        assert_bound(name, nparams=nparams, scalars=scalars, restype=C.c_int)      # pointer for pointer, scalar for scalar, in the header's order


def test_library_exports_both(native):
    assert_exported(native.HIP_LIB, [DROP, COPY])


def good_copy():
    """Arguments every host check accepts (the pointers are never dereferenced: the tests below return before any launch).
    0 src_digests, 1 src_forest, 2 src_total, 3 src_offsets, 4 src_ntrees, 5 src_max_count, 6 src_roots, 7 src_mutated, 8 sel, 9 m,
    10 n_leaves, 11 new_offsets, 12 dst_digests, 13 dst_forest, 14 dst_total, 15 dst_offsets, 16 dst_ntrees, 17 dst_max_count,
    18 first_tree, 19 used, 20 dst_roots, 21 dst_mutated, 22 status"""
    p = [C.c_void_p(0x1000 * (i + 1)) for i in range(12)]
    return [p[0], p[1], 200, p[2], 9, 50, p[3], None, p[4], 3, 30, p[5], p[6], p[7], 100, p[8], 8, 50, 4, 60, p[9], None, p[10]]


def test_bad_copy_arguments_are_refused_before_any_hip_call(native):
    from vk_merkle_roots_amd import _abi
    lib = _abi.lib()
    g = good_copy()
    copy = Refusals(lib.vkmr_hip_forest_copy_trees_async, COPY, good=g)
    copy.null(0, 1, 3, 6, 8, 11, 12, 13, 15, 20, 22)        # each needed pointer NULL with m > 0 (the masks, 7 and 21, are NULL already)
    # first_tree + m > dst_ntrees (also past 2^32), used + n_leaves > dst_total (also past 2^64), either max_count == 0, either
    # total above 2^58, and the four pairs of buffers that may not be the same
    copy.changed({18: 6}, {9: 5}, {18: 9}, {18: 2**32 - 1, 9: 2}, {10: 41}, {19: 71}, {19: 101, 10: 0}, {19: 2**64 - 1, 10: 2}, {5: 0}, {17: 0},
                 {2: (1 << 58) + 1}, {14: (1 << 58) + 1}, {12: g[0]}, {13: g[1]}, {15: g[3]}, {20: g[6]})
    # m == 0 is a no-op whatever the rest
    copy.ok(*([changes.get(i, a) for i, a in enumerate(g)]
              for changes in ({9: 0}, {9: 0, 0: None, 12: None, 22: None}, {9: 0, 14: (1 << 58) + 1, 5: 0, 18: 99}, {9: 0, 12: g[0], 13: g[1]})))


def test_bad_drop_arguments_are_refused_before_any_hip_call(native):
    from vk_merkle_roots_amd import _abi
    lib = _abi.lib()
    d = C.c_void_p(0x1000)
    drop = Refusals(lib.vkmr_hip_forest_drop_front_async, DROP, good=[d, 8, 3, d, None])         # offsets, ntrees, drop_trees, roots, mutated
    drop.null(0, 3)
    drop.changed({2: 9, 4: d}, {0: None, 2: 9, 3: None}, {1: 0, 2: 1})                           # drop_trees > ntrees
    drop.ok((None, 8, 0, None, None), (None, 0, 0, None, None))                                  # drop_trees == 0: nothing to do


def host_forest(counts=(4, 0, 7, 0, 0, 0), total=20, max_count=8, used_trees=3):
    import vk_merkle_roots_amd as vk
    return vk.MerkleForest(NoDevice(), None, total, list(counts), None, max_count, None, None, used_trees=used_trees)


class Recorder:
    """Stands where a HipDevice would for the calls that only enqueue: records them."""

    def __init__(self):
        self.calls = []

    def forest_drop_front_enqueue(self, *args, **kw):
        self.calls.append(("drop", args))

    def forest_truncate_enqueue(self, *args, **kw):
        self.calls.append(("truncate", args))

    def sync(self, stream=None):
        self.calls.append(("sync", ()))


def test_a_fresh_handle_has_dropped_nothing(native):
    f = host_forest()
    assert (f.dropped_trees, f.dropped_leaves, f.used_leaves, f.live_leaves, f.free_leaves) == (0, 0, 11, 11, 9)


def test_drop_front_refuses_on_the_host_and_keeps_the_books(native):
    for k in (4, 6, 7, -1):
        with pytest.raises(ValueError):
            host_forest().drop_front(k)
    f = host_forest(counts=(4, 2, 7, 0, 0, 0))
    f.dev = Recorder()
    f.drop_front(0)                                          # nothing to drop: no device call
    assert f.dev.calls == [("sync", ())]
    f.drop_front(2)
    assert f.dev.calls[1] == ("drop", (None, 6, 2, None, None))
    assert (f.dropped_trees, f.dropped_leaves, f.used_leaves, f.live_leaves, f.free_leaves, f.used_trees, f.free_trees) == (2, 6, 13, 7, 7, 3, 3)
    assert f.counts.tolist() == [0, 0, 7, 0, 0, 0]
    cells, of = f._entry_cells(np.array([2, 2], dtype=np.uint32), np.array([0, 6], dtype=np.uint64))
    assert cells.tolist() == [6, 12] and of.tolist() == [7, 7]  # the kept tree's leaves lie where they lay
    with pytest.raises(IndexError):
        f._update_order([1], [0])                            # a dropped tree has no leaf to update
    n = len(f.dev.calls)
    f.drop_front(1)                                          # already dropped: absolute tree numbers
    assert [c for c in f.dev.calls[n:] if c[0] == "drop"] == [] and f.dropped_trees == 2
    f.drop_front(3)
    assert (f.dropped_trees, f.dropped_leaves, f.used_leaves, f.live_leaves, f.free_leaves) == (3, 13, 13, 0, 7)
    with pytest.raises(ValueError):
        f.truncate(2)                                        # in front of the dropped trees
    f.truncate(3)
    assert f.used_trees == 3


def test_append_from_refuses_on_the_host(native):
    src = host_forest(counts=(4, 9, 7, 1, 0, 3), total=24, max_count=9, used_trees=6)
    for trees, exc in (([0, 2, 3, 4], ValueError),           # four trees, room for three
                       ([0, 2], ValueError),                 # eleven leaves, room for nine
                       ([1], ValueError),                    # a count above max_count
                       ([6], IndexError), ([-1], IndexError), ([0.5], ValueError)):
        with pytest.raises(exc):
            host_forest().append_from(src, trees)
        with pytest.raises(exc):
            host_forest().append_from(src, trees, mutated=True)
    f = host_forest()
    with pytest.raises(ValueError):
        f.append_from(f, [0])                                # a copy inside one forest is not offered
    with pytest.raises(ValueError):
        f.append_from("no forest", [0])
    assert f.append_from(src, []).shape == (0,)              # no tree: no device call
    numbers, masks = f.append_from(src, [], mutated=True)
    assert numbers.shape == (0,) and masks.shape == (0,) and f.used_trees == 3


def test_repacked_refuses_on_the_host(native):
    f = host_forest()
    for kw in ({"trees": [6]}, {"trees": [-1]}):
        with pytest.raises(IndexError):
            f.repacked(**kw)
    for kw in ({"trees": []}, {"trees": [2], "max_count": 6}, {"max_count": 0}, {"reserve_trees": -1}, {"reserve_leaves": -1}):
        with pytest.raises(ValueError):
            f.repacked(**kw)


def test_status_text_names_the_bits(native):
    import vk_merkle_roots_amd as vk
    text = vk.forest_copy_status_text
    assert text(0) == "ok"
    for bit in range(4):
        assert [f"bit {b}" in text(1 << bit) for b in range(4)] == [b == bit for b in range(4)]
    assert all(f"bit {b}" in text(15) for b in range(4)) and "unknown" not in text(15)
    assert "unknown" in text(16)
    assert "unknown" in vk.forest_append_status_text(8)      # append's own text stays as it was


def test_the_kernel_names_match_no_hash_block_key(native):
    from vk_merkle_roots_amd import isa_prio_pass
    for name in KERNELS:
        for key in isa_prio_pass.EXPECTED_HASH_BLOCKS:
            assert key not in name, (key, name)
    text = open(os.path.join(ROOT, "vk_merkle_roots_amd", "csrc", "forest_copy_kernels.hpp")).read()
    assert set(re.findall(r"__global__ __launch_bounds__\(\d+\) void (\w+)\(", text)) == set(KERNELS)
    assert "hash_pair" not in text and "sha256" not in text.lower()
    rec = isa_record(native)
    if rec is not None:                    # written by a build that ran the issue pass
        assert rec["audit"]["block_count_errors"] == [] and rec["audit"]["unclassified"] == []
        assert not [k for k in rec["audit"]["blocks"] if "forest_copy" in k or "forest_drop_front" in k]


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    return fr.build_copy_plan_exe(tmp_path_factory.mktemp("forest_copy_plan"))


def test_the_copy_replayed_with_values_over_every_case_table(native, plan_exe, tmp_path):
    cases, heights = [], set()
    for name, counts in sorted(fc.CASES.items()):
        for sel_name, sel in sorted(fr.selections(len(counts)).items()):
            for i, (first_tree, used) in enumerate(fr.PLACEMENTS):
                for tight_dst in (False, True):
                    src_max, dst_max = fr.max_counts(counts, sel, used, first_tree, tight_dst)
                    cases.append((fr.SRC_FIRST, fr.SRC_SLACK, src_max, first_tree, used, fr.DST_SLACK, dst_max, fr.BEHIND, sel, counts))
    got = fr.copy_replay(plan_exe, tmp_path, cases)
    for (_, _, _, first_tree, used, _, _, _, sel, counts), (H_s, H_d, leaves, cells, roots, lanes) in zip(cases, got):
        assert (leaves, cells, roots) == fr.written(counts, sel), (first_tree, used, sel[:8], counts[:8])
        heights.add((H_d > H_s) - (H_d < H_s))
        # the range restriction: a launch covers the new trees' cells and under one wavefront more, never the whole level
        assert lanes <= sum((leaves >> l) + len(sel) + 1 + 63 for l in range(0, H_d + 1)), (sel[:8], counts[:8])
    assert {-1, 1} <= heights              # destinations with fewer and with more levels than their source


def test_drop_front_replayed_for_every_k_over_every_case_table(native, plan_exe, tmp_path):
    cases = []
    for name, counts in sorted(fc.CASES.items()):
        for first, slack in ((0, 0), (5, 7)):
            for max_count in (0, 2**63):
                cases.append((first, slack, max_count, counts))
    got = fr.drop_replay(plan_exe, tmp_path, cases)
    assert [n for _, n in got] == [len(c[3]) for c in cases]
