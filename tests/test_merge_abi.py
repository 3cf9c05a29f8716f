"""The merge of sorted forests without a GPU: the C ABI's declarations and argument checks (vkmr_hip_forest_merge_leaves_async,
vkmr_hip_tree_merge_leaves_async, vkmr_hip_merge_leaves_scratch_bytes), the rules of csrc/merge_plan.hpp replayed
(tests/c/merge_plan_test.cpp, its own program under AddressSanitizer and UBSan), the CPU twins (vkmr_host_cpu_forest_merge_leaves,
vkmr_host_cpu_tree_merge_leaves) against the model of tests/merge_cases.py on every case and op, merge_status_text, the host side
of HipDevice.merge_leaves and MerkleForest / MerkleTree.inserted, removed, common, and the new kernels' code-object metadata.  No
compute call on a device here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import merge_cases as mc
from abi_support import ROOT, Refusals, assert_bound, assert_exported, assert_no_spills, isa_record
from merkle_model import random_leaves
from no_device import NoDevice

ENTRY_POINTS = {"vkmr_hip_forest_merge_leaves_async": 16, "vkmr_hip_tree_merge_leaves_async": 12}
HOST_ENTRY_POINTS = {"vkmr_host_cpu_forest_merge_leaves": 13, "vkmr_host_cpu_tree_merge_leaves": 9}
KERNELS = tuple(f"{whose}_merge_{step}_kernel" for whose in ("forest", "tree") for step in ("order", "mark", "emit"))
CASES = mc.all_cases()
CELLS = [(c, op) for c in CASES for op in mc.OPS]
CELL_IDS = [f"{c.name}: {mc.OP_NAMES[op]}" for c, op in CELLS]


def test_header_declares_them_and_the_stub_binds_every_argument():
    from vk_merkle_roots_amd import _abi
    assert_bound("vkmr_hip_forest_merge_leaves_async", nparams=16, restype=C.c_int,
                 scalars=[C.c_int, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64])
    assert_bound("vkmr_hip_tree_merge_leaves_async", nparams=12, restype=C.c_int, scalars=[C.c_int, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64])
    assert_bound("vkmr_hip_merge_leaves_scratch_bytes", nparams=3, scalars=[C.c_uint64, C.c_uint64, C.c_uint32], restype=C.c_size_t)
    for name, nparams in HOST_ENTRY_POINTS.items():
        assert_bound(name, nparams=nparams, restype=C.c_int, table=_abi.HOST_SIGNATURES, header="vkmr_host.h")


def test_libraries_export_them(native):
    assert_exported(native.HIP_LIB, list(ENTRY_POINTS) + ["vkmr_hip_merge_leaves_scratch_bytes"])
    assert_exported(native.HOST_LIB, HOST_ENTRY_POINTS)


def test_bad_arguments_are_refused_before_any_hip_call(native):
    from vk_merkle_roots_amd import _abi
    lib = _abi.lib()
    # never dereferenced: every call below returns before launching anything.  The buffers lie a megabyte apart.
    d_a, d_b, d_out, d_scr, d = C.c_void_p(0x100000), C.c_void_p(0x200000), C.c_void_p(0x300000), C.c_void_p(0x400000), C.c_void_p(0x1000)
    scratch = mc.scratch_bytes(100, 50)
    # a, a_total, a_offsets, b, b_total, b_offsets, ntrees, op, scratch, out, out_capacity, out_offsets, origin, info
    r = Refusals(lib.vkmr_hip_forest_merge_leaves_async, "vkmr_hip_forest_merge_leaves_async", good=[d_a, 100, d, d_b, 50, d, 8, 0, d_scr, d_out, 150, d, d, d])
    r.null(0, 2, 3, 5, 8, 9, 11, 13)
    r.changed({7: 3}, {7: 0xFFFFFFFF}, {1: 1 << 32}, {4: 1 << 32}, {1: (1 << 32) - 52}, {10: 1 << 60},
              {0: C.c_void_p(0x100008)}, {3: C.c_void_p(0x200004)}, {9: C.c_void_p(0x300010 - 8)}, {8: C.c_void_p(0x400008)},       # digests and scratch: 16 bytes
              {2: C.c_void_p(0x1004)}, {5: C.c_void_p(0x1004)}, {11: C.c_void_p(0x1004)}, {12: C.c_void_p(0x1004)}, {13: C.c_void_p(0x1004)},   # uint64_t: 8 bytes
              {9: d_a}, {9: C.c_void_p(0x100000 + 32 * 99)}, {9: C.c_void_p(0x100000 - 32 * 149)},                                   # the output over A
              {9: d_b}, {9: C.c_void_p(0x200000 + 32 * 49)}, {9: C.c_void_p(0x200000 - 32 * 149)},                                   # over B
              {9: d_scr}, {9: C.c_void_p(0x400000 + scratch - 16)}, {8: C.c_void_p(0x300000 + 32 * 149 + 16)})                       # over the scratch
    r.ok([None, 0, None, None, 0, None, 0, 0, None, None, 0, None, None, None], [d_a, 1 << 40, None, None, 0, None, 0, 7, None, None, 0, None, None, None])
    # a, a_count, b, b_count, op, scratch, out, out_capacity, origin, info
    r = Refusals(lib.vkmr_hip_tree_merge_leaves_async, "vkmr_hip_tree_merge_leaves_async", good=[d_a, 100, d_b, 50, 2, d_scr, d_out, 100, None, d])
    r.null(0, 2, 5, 6, 9)
    r.changed({4: 3}, {1: 1 << 32}, {5: C.c_void_p(0x400004)}, {6: d_a}, {6: d_b}, {6: C.c_void_p(0x400020)}, {8: C.c_void_p(0x1004)}, {9: C.c_void_p(0x1002)})
    # and the twins
    import vk_merkle_roots_amd as vk
    host = vk.host_lib()
    z = np.zeros(64, np.uint64)
    p = z.ctypes.data
    assert host.vkmr_host_cpu_forest_merge_leaves(p, 0, None, p, 0, p, 1, 0, p, 0, p, p, p) == -1              # no offsets of A
    assert host.vkmr_host_cpu_forest_merge_leaves(p, 0, p, p, 0, None, 1, 0, p, 0, p, p, p) == -1              # of B
    assert host.vkmr_host_cpu_forest_merge_leaves(p, 0, p, p, 0, p, 1, 0, p, 0, None, p, p) == -1              # nowhere to write the offsets
    assert host.vkmr_host_cpu_forest_merge_leaves(p, 0, p, p, 0, p, 1, 0, p, 0, p, p, None) == -1              # no info
    assert host.vkmr_host_cpu_forest_merge_leaves(p, 0, p, p, 0, p, 1, 3, p, 0, p, p, p) == -1                 # op
    assert host.vkmr_host_cpu_forest_merge_leaves(None, 1, p, p, 0, p, 1, 0, p, 1, p, p, p) == -1              # a cell of A and nowhere to read it
    assert host.vkmr_host_cpu_forest_merge_leaves(None, 0, None, None, 0, None, 0, 0, None, 0, None, None, None) == 0
    assert host.vkmr_host_cpu_tree_merge_leaves(p, 0, p, 0, 0, p, 0, None, None) == -1 and host.vkmr_host_cpu_tree_merge_leaves(p, 0, p, 0, 5, p, 0, None, p) == -1


def test_the_scratch_size_is_the_plans(native):
    from vk_merkle_roots_amd import _abi
    lib = _abi.lib()
    text = open(os.path.join(ROOT, "vk_merkle_roots_amd", "csrc", "merge_plan.hpp")).read()
    consts = {name: int(value) for name, value in re.findall(r"#define\s+(VKMR_MERGE_\w+)\s+(\d+)u\b", text)}
    assert consts["VKMR_MERGE_SCAN_ROW"] == mc.SCAN_ROW and consts["VKMR_MERGE_HEADER_WORDS"] == mc.HEADER_WORDS
    assert (consts["VKMR_MERGE_UNION"], consts["VKMR_MERGE_DIFFERENCE"], consts["VKMR_MERGE_INTERSECTION"]) == mc.OPS
    for a in (0, 1, 100, 8190, 8191, 5933, 1 << 20, (1 << 26) + 3, (1 << 32) - 3, 1 << 32, 1 << 40):
        for b in (0, 1, 2, 50, 1 << 16, (1 << 32) - 1):
            got = lib.vkmr_hip_merge_leaves_scratch_bytes(a, b, 7)
            assert got == mc.scratch_bytes(a, b) and got % 16 == 0, (a, b)
    assert 4 * (1 << 26) < lib.vkmr_hip_merge_leaves_scratch_bytes(1 << 26, 1 << 16, 1 << 15) < 4.1 * (1 << 26)      # 4 bytes a cell of A, 8 a cell of B


# ---- the replay of the plan ------------------------------------------------------------------------------------------------------------
def test_the_plan_replayed_under_the_sanitizers(tmp_path):
    exe = mc.build_merge_plan_exe(tmp_path)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    text = r.stdout.decode()
    assert r.returncode == 0 and "FAIL" not in text and "ok: 299064 leaves merged three ways, 46 forests" in text, text[-2000:]


# ---- the model and the cases ------------------------------------------------------------------------------------------------------------
def test_the_forest_holds_what_the_cases_promise():
    A, B = mc.forest_sides()
    assert [len(t) for t in A] == mc.COUNTS == [1, 2, 3, 0, 4, 5, 7, 8, 9, 0, 63, 64, 65, 130, 1023, 1024, 1025, 2500]
    c0, c1 = mc.forest_cases()
    assert int(c0.a_offsets[0]) == 0 == int(c0.b_offsets[0]) and int(c1.a_offsets[0]) == 37 and c1.a_cells.shape[0] == 37 + 5933 + 100
    assert B[0] == [] and A[0] and B[9] == [] == A[9] and A[3] == [] and len(B[3]) == 5
    assert B[1][-1] < A[1][0] and B[2][0] > A[2][-1] and B[4] == A[4] and len(B[5]) > len(A[5])
    assert B[3][-1] == B[4][0]                                                                     # the same digest on both sides of a tree boundary of B

    def runs(t):
        """{slot: leaves of B_t that are no repeat, in no A_t, with that lower bound}"""
        import bisect
        out = {}
        for d in sorted(set(B[t]) - set(A[t])):
            lb = bisect.bisect_left(A[t], d)
            out[lb] = out.get(lb, 0) + 1
        return out
    assert runs(15)[0] == 257 and runs(16)[0] == 65 and runs(10)[0] == 64 and runs(12)[0] == 1 and runs(7)[0] == 2                             # at slot 0
    assert runs(14)[1023] == 257 and runs(11)[64] == 65 and runs(13)[130] == 64 and runs(7)[8] == 1 and runs(2)[3] == 2  # behind the last leaf
    assert runs(13)[61] == 257 and runs(12)[31] == 64 and runs(7)[4] == 65 and runs(17)[1201] == 65 and runs(15)[512] == 2       # in the middle
    # words 0 to 6 equal and word 7 deciding; word 0 on either side of its sign bit; the lowest and the highest digest
    assert all(d[:7] == B[15][0][:7] for d in B[15][:257]) and len({d[7] for d in B[15][:257]}) == 257
    assert mc.HALF_BELOW in B[6] and mc.HALF in B[6] and A[6][5][0] == 0x7FFFFFFF and A[6][6][0] == 0x80000000 and B[6].index(mc.HALF_BELOW) + 1 == B[6].index(mc.HALF)
    assert A[17][0] == mc.ZERO == B[17][0] and A[17][-1] == mc.ONES and B[16][-1] == mc.ONES and B[11][0] == mc.ZERO and mc.ZERO not in A[11]
    # the repeats: a pair, a run of 40, one that also matches A
    assert B[8].count(A[8][3]) == 2 and sum(x == y for x, y in zip(B[8], B[8][1:])) == 2 and max(B[13].count(d) for d in set(B[13])) == 40
    # matches and non-matches alternate across flat positions 64, 256 and 1 024 of both sides
    flat_a = [(t, d) for t in range(18) for d in A[t]]
    flat_b = [(t, d) for t in range(18) for d in B[t]]
    for p in (64, 256, 1024):
        assert len({d in set(B[t]) for t, d in flat_a[p - 1: p + 1]}) == 2, ("A", p)
        assert len({d in set(A[t]) for t, d in flat_b[p - 1: p + 1]}) == 2, ("B", p)
    info = [mc.model_merge(c0, op)[3].tolist() for op in mc.OPS]
    na, nb = 5933, len(flat_b)
    matches, repeats = info[0][2], info[0][3]
    assert repeats == 1 + 1 + 39 and matches > 2500 and [i[0] for i in info] == [0, 0, 0] and all(i[2:] == [matches, repeats] for i in info)
    assert [i[1] for i in info] == [na + nb - matches - repeats, na - matches, matches]
    # the placement with cells around it changes nothing but the origin
    for op in mc.OPS:
        a, b = mc.model_merge(c0, op), mc.model_merge(c1, op)
        assert (a[0] == b[0]).all() and (a[1] == b[1]).all() and (a[3] == b[3]).all()
        n = int(a[3][1])
        a, b = (a[0], a[1], a[2][:n], a[3]), (b[0], b[1], b[2][:n], b[3])
        from_b = (a[2] >> np.uint64(63)) == 1
        assert ((b[2] - a[2])[from_b] == 11).all() and ((b[2] - a[2])[~from_b] == 37).all() and (op != 0 or from_b.sum() == nb - matches - repeats)


def test_the_shapes_hold_what_they_promise():
    cases = {c.name: c for c in mc.shape_cases()}
    assert len(cases) == 8
    many = cases["257 trees of 0 to 3 leaves on each side"]
    assert len(many.a_offsets) == 258 == len(many.b_offsets)
    assert set(np.diff(many.a_offsets.astype(np.int64)).tolist()) == {0, 1, 2, 3} == set(np.diff(many.b_offsets.astype(np.int64)).tolist())
    assert mc.model_merge(many, 0)[3][3] > 0 and mc.model_merge(many, 0)[3][2] > 0
    dedup = cases["an empty A: the distinct leaves of a batch that repeats"]
    out, offsets, origin, info = mc.model_merge(dedup, 0)
    rows = [mc.words(r) for r in dedup.b_cells]
    assert info.tolist() == [0, 51, 0, 57] and [mc.words(r) for r in out[:51]] == sorted(set(rows[:105])) + [rows[105]] and offsets.tolist() == [0, 50, 51]
    assert sum(mc.is_one_tree(c) for c in mc.all_cases()) == 2 and mc.is_one_tree(cases["the tree of 2 500 alone"])
    assert mc.model_merge(cases["one leaf against the same leaf"], 1)[3].tolist() == [0, 0, 1, 0]
    assert mc.model_merge(cases["one leaf against another"], 0)[3].tolist() == [0, 2, 0, 0]


def test_the_model_refuses_what_the_rule_refuses():
    c = mc.forest_cases()[1]
    for change, status in ((dict(a_offsets=np.concatenate([c.a_offsets[:5], c.a_offsets[5:6] - 9, c.a_offsets[6:]])), 1),
                           (dict(b_offsets=np.concatenate([c.b_offsets[:-1], [c.b_cells.shape[0] + 1]]).astype(np.uint64)), 2)):
        for op in mc.OPS:
            out, offsets, origin, info = mc.model_merge(c._replace(**change), op, capacity=20)
            assert info.tolist() == [status, 0, 0, 0] and (out == mc.CANARY).all() and (offsets == mc.OFFSET_FILL).all() and (origin == mc.OFFSET_FILL).all()
    assert mc.model_merge(c, 0, capacity=10119)[3].tolist() == [16, 10120, 2919, 41] and mc.model_merge(c, 0, capacity=10120)[3][0] == 0


# ---- the CPU twins against the model ------------------------------------------------------------------------------------------------------
def same(got, want, note):
    for what, a, b in zip(("leaves", "offsets", "origin", "info"), got, want):
        assert a.shape == b.shape and (a == b).all(), (note, what, a[:4] if what == "info" else "")


@pytest.mark.parametrize("case,op", CELLS, ids=CELL_IDS)
def test_the_twin_is_the_model(native, case, op):
    want = mc.model_merge(case, op)
    rc, *got = mc.host_merge(case, op)
    assert rc == 0
    same(got, want, case.name)
    na, nb = int(case.a_offsets[-1] - case.a_offsets[0]), int(case.b_offsets[-1] - case.b_offsets[0])
    assert int(got[3][1]) == mc.n_out_of_counts(op, na, nb, int(got[3][2]), int(got[3][3]))
    rc, out, offsets, origin, info = mc.host_merge(case, op, capacity=mc.default_capacity(case, op) + 3, with_origin=False)     # room behind, no origin
    assert rc == 0 and (info == want[3]).all() and (out[: len(want[0])] == want[0]).all() and (out[len(want[0]):] == mc.CANARY).all()
    assert (origin == mc.OFFSET_FILL).all() and (offsets == want[1]).all()
    if mc.is_one_tree(case):
        rc, out, offsets, origin, info = mc.host_merge(case, op, one_tree=True)
        assert rc == 0 and (offsets == mc.OFFSET_FILL).all()
        same((out, origin, info), (want[0], want[2], want[3]), ("one tree", case.name))


@pytest.mark.parametrize("name", mc.REFUSALS)
def test_the_twin_refuses_what_the_model_refuses_and_writes_nothing(native, name):
    case, capacity, status, n_out = mc.refusal(name)
    for op in mc.OPS:
        cap = mc.default_capacity(case, op) if capacity is None else capacity
        if capacity == -1:
            cap = int(mc.model_merge(case, op)[3][1]) - 1
            if cap < 0:
                continue
        want = mc.model_merge(case, op, capacity=cap)
        rc, *got = mc.host_merge(case, op, capacity=cap)
        assert rc == 0 and int(want[3][0]) == status
        same(got, want, (name, op))
        assert (got[0] == mc.CANARY).all() and (got[1] == mc.OFFSET_FILL).all() and (got[2] == mc.OFFSET_FILL).all()
        if n_out is None:                                                                          # the short output reports the true n_out: call again
            full = mc.model_merge(case, op)
            assert got[3].tolist() == [16] + full[3].tolist()[1:]
            rc, *again = mc.host_merge(case, op, capacity=cap + 1)
            assert rc == 0 and int(again[3][0]) == 0 and (again[0] == full[0][: cap + 1]).all()


# ---- the Python layer's host side ---------------------------------------------------------------------------------------------------------
def test_the_status_text():
    import vk_merkle_roots_amd as vk
    assert vk.merge_status_text(0) == "ok"
    for bit, word in enumerate(("offsets of A", "offsets of B", "A is not strictly increasing", "B decreases", "more leaves than cells")):
        text = vk.merge_status_text(1 << bit)
        assert f"bit {bit}" in text and word in text and ";" not in text
    assert vk.merge_status_text(12).count(";") == 1 and "unknown" in vk.merge_status_text(32)


def test_the_python_layer_checks_on_the_host():
    import vk_merkle_roots_amd as vk
    rows = random_leaves(np.random.default_rng(804), 10)
    dev = NoDevice()
    with pytest.raises(ValueError, match="add up"):
        vk.HipDevice.merge_leaves(dev, rows, [5, 4], rows, [5, 5])
    with pytest.raises(ValueError, match="add up"):
        vk.HipDevice.merge_leaves(dev, rows, [5, 5], rows, [5, 4])
    with pytest.raises(ValueError, match="2 trees of a, 3 of b"):
        vk.HipDevice.merge_leaves(dev, rows, [5, 5], rows, [5, 4, 1])
    with pytest.raises(ValueError, match="op is one of union, difference, intersection"):
        vk.HipDevice.merge_leaves(dev, rows, [5, 5], rows, [5, 5], op="xor")
    with pytest.raises(ValueError, match="op"):
        vk.HipDevice.merge_leaves(dev, rows, [5, 5], rows, [5, 5], op=3)
    out, counts, origin, info = vk.HipDevice.merge_leaves(dev, rows[:0], [], rows[:0], [])
    assert out.shape == (0, 8) and counts.shape == (0,) and origin.shape == (0,) and info.tolist() == [0, 0, 0, 0]
    forest = vk.MerkleForest(dev, None, 10, [5, 5, 0], None, 8, None, None, used_trees=2)
    for method in (forest.inserted, forest.removed, forest.common):
        with pytest.raises(ValueError, match="add up"):
            method(rows, [5, 4])
        with pytest.raises(ValueError, match="3 counts for the 2 trees in use"):
            method(rows, [5, 4, 1])
        with pytest.raises(ValueError, match="max_count"):
            method(rows, [5, 5], reserve_leaves=4)
        with pytest.raises(ValueError, match="negative"):
            method(rows, [5, 5], max_count=16, reserve_trees=-1)
        with pytest.raises(TypeError):
            method(rows, [5, 5], sort_b=False)
    forest.forest = forest.roots_buf = forest.offsets = None
    assert {"merge_leaves", "forest_merge_leaves_enqueue", "tree_merge_leaves_enqueue", "merge_leaves_scratch_bytes"} <= set(dir(vk.HipDevice))
    assert {"inserted", "removed", "common"} <= set(dir(vk.MerkleForest)) and {"inserted", "removed", "common"} <= set(dir(vk.MerkleTree))


def test_the_code_object(native):
    rec = isa_record(native)
    assert rec is not None
    assert rec["audit"]["unclassified"] == [] and rec["audit"]["block_count_errors"] == []
    assert not any("merge" in name for name in rec["hash_blocks"])                                  # they hash nothing
    assert assert_no_spills(native, KERNELS, max_vgprs=64, prefix=True)                             # a tree's kernels begin with its counts
