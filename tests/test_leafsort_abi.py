"""The leaf sort without a GPU: the C ABI's declarations and argument checks (vkmr_hip_forest_sort_leaves_async,
vkmr_hip_tree_sort_leaves_async, vkmr_hip_sort_leaves_scratch_bytes), the rules of csrc/leafsort_plan.hpp replayed
(tests/c/leafsort_plan_test.cpp, its own program under AddressSanitizer and UBSan), the CPU twins
(vkmr_host_cpu_forest_sort_leaves, vkmr_host_cpu_tree_sort_leaves) against the model of tests/leafsort_cases.py on every case,
vk.sort_digests beside them, and the host side of HipDevice.sort_leaves / build_sorted_forest and vk.sorted_forest_packed.  No
compute call on a device here."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import leafsort_cases as lc
from abi_support import Refusals, assert_bound, assert_exported, assert_no_spills, isa_record
from merkle_model import random_leaves
from no_device import NoDevice

ENTRY_POINTS = {"vkmr_hip_forest_sort_leaves_async": 11, "vkmr_hip_tree_sort_leaves_async": 8}
HOST_ENTRY_POINTS = {"vkmr_host_cpu_forest_sort_leaves": 8, "vkmr_host_cpu_tree_sort_leaves": 5}
KERNELS = tuple(f"{whose}_leafsort_{step}_kernel" for whose in ("forest", "tree") for step in ("keys", "ties", "place", "emit"))


def test_header_declares_them_and_the_stub_binds_every_argument():
    from vk_merkle_roots_amd import _abi
    for name, nparams in ENTRY_POINTS.items():
        assert_bound(name, nparams=nparams, restype=C.c_int)
    assert_bound("vkmr_hip_sort_leaves_scratch_bytes", nparams=1, scalars=[C.c_uint64], restype=C.c_size_t)
    for name, nparams in HOST_ENTRY_POINTS.items():
        assert_bound(name, nparams=nparams, restype=C.c_int, table=_abi.HOST_SIGNATURES, header="vkmr_host.h")


def test_libraries_export_them(native):
    assert_exported(native.HIP_LIB, list(ENTRY_POINTS) + ["vkmr_hip_sort_leaves_scratch_bytes"])
    assert_exported(native.HOST_LIB, HOST_ENTRY_POINTS)


def test_bad_arguments_are_refused_before_any_hip_call(native):
    from vk_merkle_roots_amd import _abi
    lib = _abi.lib()
    # never dereferenced: every call below returns before launching anything.  The three buffers lie a megabyte apart.
    d_in, d_out, d_scr, d = C.c_void_p(0x100000), C.c_void_p(0x200000), C.c_void_p(0x300000), C.c_void_p(0x1000)
    # digests_in, total, offsets, ntrees, max_count, scratch, digests_out, order_out, info
    r = Refusals(lib.vkmr_hip_forest_sort_leaves_async, "vkmr_hip_forest_sort_leaves_async", good=[d_in, 100, d, 8, 50, d_scr, d_out, d, d])
    r.null(0, 2, 5, 6, 8)
    r.changed({1: 1 << 32}, {1: (1 << 58) + 1}, {5: C.c_void_p(0x300008)}, {6: d_in}, {6: C.c_void_p(0x100000 + 32 * 99)}, {6: C.c_void_p(0x100000 - 32 * 99)},
              {6: C.c_void_p(0x300010)}, {6: C.c_void_p(0x300000 + lc.scratch_bytes(100) - 32)}, {5: C.c_void_p(0x200000 + 32 * 99 + 16)})
    r.ok([None, 0, None, 0, 0, None, None, None, None], [d_in, 1 << 40, None, 0, 50, None, None, None, None])     # no tree: nothing to do
    # digests_in, count, scratch, digests_out, order_out, info
    r = Refusals(lib.vkmr_hip_tree_sort_leaves_async, "vkmr_hip_tree_sort_leaves_async", good=[d_in, 100, d_scr, d_out, d, d])
    r.null(0, 2, 3, 5)
    r.changed({1: 1 << 32}, {2: C.c_void_p(0x300004)}, {3: d_in}, {3: C.c_void_p(0x300020)})
    # and the twins
    import vk_merkle_roots_amd as vk
    host = vk.host_lib()
    z = np.zeros(64, np.uint64)
    p = z.ctypes.data
    assert host.vkmr_host_cpu_forest_sort_leaves(p, 0, None, 1, 1, p, p, p) == -1 and host.vkmr_host_cpu_forest_sort_leaves(p, 0, p, 1, 1, p, p, None) == -1
    assert host.vkmr_host_cpu_forest_sort_leaves(p, 1 << 32, p, 1, 1, p, p, p) == -1
    assert host.vkmr_host_cpu_forest_sort_leaves(None, 0, None, 0, 0, None, None, None) == 0
    one = np.array([0, 1], dtype=np.uint64)
    assert host.vkmr_host_cpu_forest_sort_leaves(None, 1, one.ctypes.data, 1, 1, p, p, p) == -1     # a leaf, and nowhere to read it
    assert host.vkmr_host_cpu_tree_sort_leaves(p, 0, None, None, None) == -1


def test_the_scratch_size_is_the_plans(native):
    from vk_merkle_roots_amd import _abi
    lib = _abi.lib()
    for total in (0, 1, 2, 100, 1023, 1024, 1025, 5933, 1 << 20, (1 << 26) + 3, (1 << 32) - 1, 1 << 32, 1 << 40):
        got = lib.vkmr_hip_sort_leaves_scratch_bytes(total)
        assert got == lc.scratch_bytes(total) and got % 16 == 0, total
    assert 29 * (1 << 26) < lib.vkmr_hip_sort_leaves_scratch_bytes(1 << 26) < 30 * (1 << 26)     # 28 bytes a cell, one for the histograms, the ranking words


# ---- the replay of the plan ------------------------------------------------------------------------------------------------------------
def test_the_plan_replayed_under_the_sanitizers(tmp_path):
    exe = lc.build_leafsort_plan_exe(tmp_path)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    text = r.stdout.decode()
    assert r.returncode == 0 and "FAIL" not in text and "ok: 5808000 pairs of leaves, 15 forests" in text, text[-2000:]


# ---- the model and the cases ------------------------------------------------------------------------------------------------------------
def test_the_plan_restated_in_python():
    assert lc.max_ties() == 1 << 14 and lc.tile_keys() == 1024
    assert lc.shape(1, 5) == (0, 14, 2) and lc.shape(1 << 15, 2048) == (15, 32, 6) and lc.shape(1, 1 << 26) == (0, 62, 8)
    assert lc.shape(18, 2500)[:2] == (5, 32) and lc.shape(257, 3)[:2] == (9, 12) and lc.shape(2, 1 << 40) == (1, 63, 8)
    assert lc.key_of(1, lc.ONES, 63) == lc.key_of(0, lc.ONES, 64) == (1 << 64) - 1                 # the sentinel's bits
    assert lc.key_of(3, [0x80000000, 0, 0, 0, 0, 0, 0, 0], 8) == 0x380


def test_the_forest_holds_what_the_cases_promise():
    trees = lc.forest_trees()
    assert [len(t) for t in trees] == lc.COUNTS and sum(lc.COUNTS) == 5933
    (_, cells, offsets, max_count), (_, cells1, offsets1, _) = lc.forest_cases()
    assert int(offsets[0]) == 0 and cells.shape[0] == 5933 and int(offsets1[0]) == 37 and cells1.shape[0] == 37 + 5933 + 100 and max_count == 2500
    tile = lc.tile_keys()
    ends = [int(o) for o in offsets[1:]]
    assert {1384 - 1023, 1384, 1384 + 1024, 1384 + 1024 + 1025} <= set(ends)                       # 1 023, 1 024 and 1 025 leaves behind one another
    out, order, info = lc.model_sort(cells, offsets, max_count)
    # the run: 40 leaves equal in words 0..6 at input cells 1 004 .. 1 043, descending there; sorted they lie at the same cells, reversed
    run_in = cells[1004: 1004 + lc.RUN]
    assert (run_in[:, :7] == run_in[0, :7]).all() and (np.diff(run_in[:, 7].astype(np.int64)) == -1).all()
    assert order[1004: 1004 + lc.RUN].tolist() == list(range(1043, 1003, -1)) and 1004 < tile < 1043
    # the same prefix on both sides of a tree boundary: three leaves each, which stay on their side
    edge = int(offsets[16])
    assert all(lc.words(r)[:2] == (0x13572468, 0x9ABCDEF0) for r in cells[edge - 3: edge + 3])
    mine = [j for j in range(5933) if lc.words(out[j])[:2] == (0x13572468, 0x9ABCDEF0)]
    assert len(mine) == 6 and sum(j < edge for j in mine) == 3 and sorted(order[mine].tolist()) == list(range(edge - 3, edge + 3))
    seven = [lc.words(r) for r in out[int(offsets[6]): int(offsets[7])]]
    at = seven.index((0x7FFFFFFF,) + (0xFFFFFFFF,) * 7)
    assert seven[at + 1] == (0x80000000,) + (0,) * 7                                               # a signed compare would put them the other way
    last = out[int(offsets[17]): int(offsets[18])]
    assert not last[0].any() and (last[-2:] == 0xFFFFFFFF).all() and order[int(offsets[18]) - 2:].tolist() == [int(offsets[17]) + 100, int(offsets[17]) + 2499]
    three = [j for j in range(int(offsets[13]), int(offsets[14])) if (out[j] == cells[int(offsets[13]) + 60]).all()]
    assert len(three) == 3 and three == list(range(three[0], three[0] + 3)) and order[three].tolist() == [int(offsets[13]) + a for a in (5, 60, 129)]
    assert info.tolist() == [0, 5933, info[2], 3] and info[2] >= lc.RUN + 1 + 6 + 3 + 2             # the run and its pivot, the edge, the three, the ones
    # the placement with cells around it: the same leaves 37 cells on, the cells outside as they were
    out1, order1, info1 = lc.model_sort(cells1, offsets1, max_count)
    assert (out1[37: 37 + 5933] == out).all() and (order1[37: 37 + 5933] == order + 37).all() and info1.tolist() == info.tolist()
    assert (out1[:37] == lc.CANARY).all() and (out1[37 + 5933:] == lc.CANARY).all() and (order1[:37] == lc.CANARY).all()


def test_the_shapes_hold_what_they_promise():
    cases = {c.name: c for c in lc.shape_cases()}
    assert len(cases) == 8
    for name, want_sentinels in (("keys that equal the sentinel: the last of two trees, P = 63", 3), ("keys that equal the sentinel: one tree, P = 64", 3)):
        c = cases[name]
        ntrees = len(c.offsets) - 1
        p = lc.shape(ntrees, c.max_count)[1]
        keys = [lc.key_of(ntrees - 1, c.cells[j], p) for j in range(int(c.offsets[-2]), int(c.offsets[-1]))]
        assert keys.count((1 << 64) - 1) == want_sentinels and c.cells.shape[0] > int(c.offsets[-1])     # and sentinels behind them
    many = cases["257 trees of 0 to 3 leaves"]
    assert len(many.offsets) == 258 and lc.shape(257, 3)[0] == 9 and int(many.offsets[257]) > int(many.offsets[256]) > int(many.offsets[255])
    assert int(cases["every tree empty"].offsets[-1]) == int(cases["every tree empty"].offsets[0])
    wide, exact = cases["max_count 1 000 times too large"], lc.forest_cases()[1]
    a, b = lc.model_sort(wide.cells, wide.offsets, wide.max_count), lc.model_sort(exact.cells, exact.offsets, exact.max_count)
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all() and a[2][[0, 1, 3]].tolist() == b[2][[0, 1, 3]].tolist() and a[2][2] <= b[2][2]
    assert lc.shape(18, wide.max_count)[1] > lc.shape(18, exact.max_count)[1]


def test_the_tie_batches():
    for extra in (0, 1):
        c = lc.tie_batch(extra)
        n = lc.max_ties() + extra
        assert c.cells.shape[0] == n and len({lc.words(r)[:2] for r in c.cells}) == 1
        out, order, info = lc.model_sort(c.cells, c.offsets, c.max_count, tie_limit=lc.max_ties())
        if extra:
            assert info.tolist() == [lc.TOO_MANY_TIES, n, n, 0] and (out == lc.CANARY).all() and (order == lc.CANARY).all()
        else:
            assert info.tolist() == [0, n, n, 1] and sorted(order.tolist()) == list(range(n))


# ---- the CPU twins against the model ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", lc.all_cases(), ids=[c.name for c in lc.all_cases()])
def test_the_twin_is_the_model(native, case):
    want = lc.model_sort(case.cells, case.offsets, case.max_count)
    rc, *got = lc.host_sort(case.cells, case.offsets, case.max_count)
    assert rc == 0
    for what, a, b in zip(("leaves", "order", "info"), got, want):
        assert a.shape == b.shape and (a == b).all(), what
    rc, out, order, info = lc.host_sort(case.cells, case.offsets, case.max_count, with_order=False)     # no order wanted
    assert rc == 0 and (out == want[0]).all() and (order == lc.CANARY).all() and (info == want[2]).all()


def test_the_twin_has_no_tie_limit_and_says_what_it_refuses(native):
    c = lc.tie_batch(1)
    n = lc.max_ties() + 1
    want = lc.model_sort(c.cells, c.offsets, c.max_count)
    rc, out, order, info = lc.host_sort(c.cells, c.offsets, c.max_count)
    assert rc == 0 and info.tolist() == [0, n, n, 1] == want[2].tolist() and (out == want[0]).all() and (order == want[1]).all()
    rc, out, order, info = lc.host_tree_sort(c.cells)
    assert rc == 0 and info.tolist() == [0, n, n, 1] and (out == want[0]).all() and (order == want[1]).all()
    exact = lc.forest_cases()[1]
    down = exact.offsets.copy()
    down[5] = down[4] - 1
    behind = exact.offsets.copy()
    behind[-1] = exact.cells.shape[0] + 1
    for offsets, max_count, status, n in ((down, 2500, 1, 0), (behind, 5000, 1, 0), (exact.offsets, 2499, 2, 5933), (behind, 2500, 3, 0)):
        want = lc.model_sort(exact.cells, offsets, max_count)
        rc, out, order, info = lc.host_sort(exact.cells, offsets, max_count)
        assert rc == 0 and info.tolist() == [status, n, 0, 0] == want[2].tolist() and (out == lc.CANARY).all() and (order == lc.CANARY).all()


def test_sort_digests_gives_the_same_leaves(native):
    import vk_merkle_roots_amd as vk
    for case in lc.all_cases():
        lo, hi = int(case.offsets[0]), int(case.offsets[-1])
        got = vk.sort_digests(case.cells[lo: hi], np.diff(case.offsets.astype(np.int64)))
        assert (got == lc.host_sort(case.cells, case.offsets, case.max_count)[1][lo: hi]).all(), case.name


# ---- the Python layer's host side ---------------------------------------------------------------------------------------------------------
def test_the_python_layer_checks_on_the_host_and_names_the_status():
    import vk_merkle_roots_amd as vk
    from vk_merkle_roots_amd import engine
    assert engine.LEAFSORT_MAX_TIES == lc.max_ties()
    assert vk.leafsort_status_text(0) == "ok" and "bit 2" in vk.leafsort_status_text(4) and "tie" in vk.leafsort_status_text(4)
    assert "bit 0" in vk.leafsort_status_text(3) and "bit 1" in vk.leafsort_status_text(3) and "unknown" in vk.leafsort_status_text(8)
    rows = random_leaves(np.random.default_rng(704), 10)
    dev = NoDevice()
    with pytest.raises(ValueError, match="add up"):
        vk.HipDevice.sort_leaves(dev, rows, [5, 4])
    got, order, info = vk.HipDevice.sort_leaves(dev, rows[:0], [0, 0])
    assert got.shape == (0, 8) and order.shape == (0,) and info.tolist() == [0, 0, 0, 0]
    with pytest.raises(ValueError, match="max_count"):
        vk.HipDevice.build_sorted_forest(dev, rows, [10], reserve_leaves=4)
    with pytest.raises(ValueError, match="negative"):
        vk.HipDevice.build_sorted_forest(dev, rows, [10], max_count=16, reserve_trees=-1)
    batch = vk.rndm_packed(5, 12, 20)
    with pytest.raises(ValueError, match="add up"):
        vk.sorted_forest_packed(dev, batch, [5, 5])
    assert {"sort_leaves", "build_sorted_forest", "forest_sort_leaves_enqueue", "tree_sort_leaves_enqueue", "sort_leaves_scratch_bytes"} <= set(dir(vk.HipDevice))
    assert vk.sort_digests(rows, [4, 6]).shape == (10, 8)                                          # the host helper stays what it was


def test_the_code_object(native):
    rec = isa_record(native)
    assert rec is not None
    assert rec["audit"]["unclassified"] == [] and rec["audit"]["block_count_errors"] == []
    assert not any("leafsort" in name for name in rec["hash_blocks"])                               # they hash nothing
    assert assert_no_spills(native, KERNELS, prefix=True)                                           # a tree's kernels begin with its count
