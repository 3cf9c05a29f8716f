"""Range proofs without a GPU: the C ABI's declarations and argument checks (vkmr_hip_forest_range_async,
vkmr_hip_verify_forest_range_async, their one-tree twins and vkmr_hip_range_scratch_bytes), the rules of csrc/range_plan.hpp
replayed (tests/c/range_plan_test.cpp, its own program under AddressSanitizer and UBSan), the CPU twins
(vkmr_host_cpu_forest_range, _tree_range, vkmr_host_cpu_verify_range) against the hashlib model of tests/range_cases.py on every
case, and the host side of vk.RangeProofs.  No compute call on a device here."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import range_cases as rc
from abi_support import Refusals, assert_bound, assert_exported, assert_key_resolves, assert_no_spills, isa_record
from no_device import NoDevice

ENTRY_POINTS = {"vkmr_hip_forest_range_async": 22, "vkmr_hip_tree_range_async": 17, "vkmr_hip_verify_forest_range_async": 21,
                "vkmr_hip_verify_range_async": 18}
HOST_ENTRY_POINTS = {"vkmr_host_cpu_forest_range": 17, "vkmr_host_cpu_tree_range": 13, "vkmr_host_cpu_verify_range": 18}
FOLDS = ("forest_range_level_kernel", "tree_range_level_kernel")
POINTER_FIRST = ("forest_range_runs_kernel", "tree_range_runs_kernel", "range_starts_kernel", "range_places_kernel", "forest_range_leaves_kernel",
                 "tree_range_leaves_kernel", "forest_range_rows_kernel", "tree_range_rows_kernel", "forest_range_heads_kernel", "range_order_kernel",
                 "forest_range_level_kernel", "forest_range_verdict_kernel")
SCALAR_FIRST = ("tree_range_heads_kernel", "tree_range_level_kernel", "tree_range_verdict_kernel")


def test_header_declares_them_and_the_stub_binds_every_argument():
    from vk_merkle_roots_amd import _abi
    for name, nparams in ENTRY_POINTS.items():
        assert_bound(name, nparams=nparams, restype=C.c_int)
    assert_bound("vkmr_hip_range_scratch_bytes", nparams=2, scalars=[C.c_uint64, C.c_uint32], restype=C.c_size_t)
    for name, nparams in HOST_ENTRY_POINTS.items():
        assert_bound(name, nparams=nparams, restype=C.c_int, table=_abi.HOST_SIGNATURES, header="vkmr_host.h")


def test_libraries_export_them(native):
    assert_exported(native.HIP_LIB, list(ENTRY_POINTS) + ["vkmr_hip_range_scratch_bytes"])
    assert_exported(native.HOST_LIB, HOST_ENTRY_POINTS)


def test_bad_arguments_are_refused_before_any_hip_call(native):
    from vk_merkle_roots_amd import _abi
    lib = _abi.lib()
    d, odd = C.c_void_p(0x1000), C.c_void_p(0x1004)        # never dereferenced: every call below returns before launching anything
    big = (1 << 58) + 1
    # 0 digests, forest, total, offsets, ntrees, 5 max_count, trees, lo, hi, Q, 10 stride, scratch, firsts, leaf_starts, leaves, 15 capacity, left,
    # right, heights, info
    r = Refusals(lib.vkmr_hip_forest_range_async, "vkmr_hip_forest_range_async", good=[d, d, 100, d, 8, 50, d, d, d, 5, 6, d, d, d, d, 9, d, d, d, d])
    r.null(0, 1, 3, 6, 7, 8, 11, 12, 13, 14, 16, 17, 18, 19)
    r.changed({10: 0}, {10: 64}, {10: 5}, {5: 0}, {2: big}, {15: big}, {0: odd}, {1: odd}, {7: odd}, {8: odd}, {11: odd}, {12: odd}, {13: odd}, {14: odd},
              {16: odd}, {17: odd}, {19: odd})                 # stride 5: 50 leaves need 6
    r.ok([None] * 2 + [0, None, 0, 0, None, None, None, 0, 0] + [None] * 4 + [0] + [None] * 4)
    # 0 digests, tree, count, height, lo, 5 hi, Q, scratch, firsts, leaf_starts, 10 leaves, capacity, left, right, info
    r = Refusals(lib.vkmr_hip_tree_range_async, "vkmr_hip_tree_range_async", good=[d, d, 100, 7, d, d, 5, d, d, d, d, 9, d, d, d])
    r.null(0, 1, 4, 5, 7, 8, 9, 10, 12, 13, 14)
    r.changed({3: 6}, {3: 8}, {2: 0}, {2: big}, {0: odd}, {4: odd}, {7: odd}, {8: odd}, {12: odd}, {14: odd})
    r.ok([None, None, 0, 0, None, None, 0] + [None] * 4 + [0, None, None, None])
    # 0 trees, lo, hi, firsts, leaf_starts, 5 leaves, nleaves, left, right, heights, 10 Q, stride, roots, counts, ntrees, 15 scratch, verdict,
    # in_first, in_count
    r = Refusals(lib.vkmr_hip_verify_forest_range_async, "vkmr_hip_verify_forest_range_async", good=[d, d, d, d, d, d, 9, d, d, d, 5, 6, d, d, 8, d, d, d, d])
    r.null(0, 1, 2, 3, 4, 5, 7, 8, 9, 12, 13, 15, 16, 17, 18)
    r.changed({11: 0}, {11: 64}, {6: big}, {1: odd}, {3: odd}, {5: odd}, {7: odd}, {8: odd}, {12: odd}, {15: odd}, {17: odd})
    r.ok([None] * 6 + [0, None, None, None, 0, 0, None, None, 0] + [None] * 4)
    # 0 lo, hi, firsts, leaf_starts, leaves, 5 nleaves, left, right, Q, height, 10 root, count, scratch, verdict, in_first, in_count
    r = Refusals(lib.vkmr_hip_verify_range_async, "vkmr_hip_verify_range_async", good=[d, d, d, d, d, 9, d, d, 5, 7, d, 100, d, d, d, d])
    r.null(0, 1, 2, 3, 4, 6, 7, 10, 12, 13, 14, 15)
    r.changed({9: 6}, {9: 8}, {11: 0}, {0: odd}, {2: odd}, {4: odd}, {6: odd}, {10: odd}, {12: odd}, {14: odd})
    r.ok([None] * 5 + [0, None, None, 0, 0, None, 0] + [None] * 4)
    assert lib.vkmr_hip_range_scratch_bytes(0, 0) == 0 and lib.vkmr_hip_range_scratch_bytes(big, 5) == 0
    small, more = lib.vkmr_hip_range_scratch_bytes(0, 300), lib.vkmr_hip_range_scratch_bytes(1000, 300)
    assert small % 32 == 0 and more == small + 32 * (500 + 250)                                     # levels 1 and 2 of 1 000 leaves
    # and the twins
    import vk_merkle_roots_amd as vk
    host = vk.host_lib()
    z = np.zeros(64, np.uint64)
    p = z.ctypes.data
    assert host.vkmr_host_cpu_forest_range(p, 0, p, 1, p, p, None, 1, 4, p, p, p, 1, p, p, p, p) == -1
    assert host.vkmr_host_cpu_forest_range(*([None, 0, None, 0] + [None] * 3 + [0, 0] + [None] * 3 + [0] + [None] * 4)) == 0
    assert host.vkmr_host_cpu_verify_range(p, p, p, p, p, p, 1, p, p, p, 1, 64, p, p, 1, p, p, p) == -1
    assert host.vkmr_host_cpu_verify_range(*([None] * 6 + [0, None, None, None, 0, 0, None, None, 0, None, None, None])) == 0
    down = np.array([4, 2, 6], dtype=np.uint64)             # offsets that decrease
    assert host.vkmr_host_cpu_forest_range(p, 8, down.ctypes.data, 2, p, p, p, 1, 4, p, p, p, 1, p, p, p, p) == 1


# ---- the replay of the plan ------------------------------------------------------------------------------------------------------------
def test_the_plan_replayed_for_every_run_up_to_40_leaves_and_random_forests(tmp_path):
    exe = rc.build_range_plan_exe(tmp_path)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    text = r.stdout.decode()
    runs = sum(c * (c + 1) // 2 for c in range(1, 41))
    assert r.returncode == 0 and "FAIL" not in text and f"ok: {runs} runs" in text and "ok: prefix 4294967296 + 1048576" in text, text[-2000:]


# ---- the CPU twins against the model -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def placements():
    f = rc.forest()
    return [f.placed(), f.placed(first=37, slack=100)]


def test_the_forest_holds_what_the_cases_promise():
    f = rc.forest()
    what, trees, lo, hi = f.queries()
    firsts, starts, leaves, left, right, heights, info, verdict, in_first, in_count = f.expected()
    assert f.counts == [0, 1, 2, 3, 5, 8, 9, 64, 65, 257, 0, 1000, 2500] and info.tolist()[0] == 0 and int(info[2]) == 13 + 3
    assert int((verdict == 1).sum()) == len(trees) - 16 and int(starts[-1]) == leaves.shape[0] == int(info[1])
    sizes = {w: int(in_count[q]) for q, w in enumerate(what) if "leaves from" in w}
    assert sizes == {f"{n} leaves from {s}": n for n in (255, 256, 257, 1025) for s in (10, 11)}
    whole = [q for q, w in enumerate(what) if w == "whole" and trees[q] < 13]
    assert [int(in_count[q]) for q in whole] == [f.counts[int(trees[q])] for q in whole]
    empty = [q for q, w in enumerate(what) if w.startswith("empty ") and trees[q] not in (0, 10)]
    assert empty and all(int(in_count[q]) == 0 and int(starts[q + 1] - starts[q]) in (1, 2) for q in empty)
    a, b = (rc.key(x) for x in f.word7)
    assert a[:7] == b[:7] and a < b
    same = [q for q, w in enumerate(what) if w.startswith("same bounds")]
    assert len(same) == 3 and all((lo[q] == lo[same[0]]).all() and (hi[q] == hi[same[0]]).all() for q in same)


def test_the_twins_are_the_model_on_every_case(native, placements):
    f = rc.forest()
    what, trees, lo, hi = f.queries()
    *want, verdict, in_first, in_count = f.expected()
    n = int(want[6][1])
    for cells, offsets in placements:
        rc_, *got = rc.host_range(cells, offsets, trees, lo, hi)
        assert rc_ == 0
        assert (got[2][:n] == want[2]).all() and (got[2][n:] == rc.CANARY).all()                      # nothing at or behind leaf_starts[Q]
        for name, a, b in zip(("firsts", "leaf_starts", None, "left", "right", "heights", "info"), got, want):
            assert name is None or (a.shape == b.shape and (a == b).all()), (name, np.nonzero((a != b).reshape(a.shape[0], -1).any(axis=1))[0][:8])
        v = rc.host_verify(trees, lo, hi, got[0], got[1], got[2][:n], got[3], got[4], got[5], f.roots, f.counts)
        assert (v[0] == verdict).all() and (v[1] == in_first).all() and (v[2] == in_count).all()
    wide = rc.host_range(*placements[1], trees, lo, hi, stride=15)
    assert wide[0] == 0 and (wide[4][:, :12] == want[3]).all() and not wide[4][:, 12:].any() and not wide[5][:, 12:].any()
    assert rc.host_range(*placements[0], trees, lo, hi, stride=11)[0] == 2                          # the tree of 2 500 needs twelve cells


def test_the_one_tree_twin_is_the_forest_of_one(native):
    import vk_merkle_roots_amd as vk
    f = rc.forest()
    what, trees, lo, hi = f.queries()
    mine = trees == 11
    lo, hi = np.ascontiguousarray(lo[mine]), np.ascontiguousarray(hi[mine])
    Q, leaves = int(mine.sum()), np.ascontiguousarray(f.trees[11])
    want = rc.host_range(leaves, np.array([0, 1000], np.uint64), np.zeros(Q, np.uint32), lo, hi, stride=10)
    cap = int(want[7][1])
    firsts, starts, info = np.zeros(Q, np.uint64), np.zeros(Q + 1, np.uint64), np.zeros(4, np.uint64)
    out, left, right = np.zeros((cap, 8), np.uint32), np.zeros((Q, 10, 8), np.uint32), np.zeros((Q, 10, 8), np.uint32)
    assert vk.host_lib().vkmr_host_cpu_tree_range(leaves.ctypes.data, 1000, lo.ctypes.data, hi.ctypes.data, Q, 10, firsts.ctypes.data, starts.ctypes.data,
                                                  out.ctypes.data, cap, left.ctypes.data, right.ctypes.data, info.ctypes.data) == 0
    for a, b in zip((firsts, starts, out, left, right, info), (want[1], want[2], want[3][:cap], want[4], want[5], want[7])):
        assert (a == b).all()


def test_status_bit_0_names_the_total_and_a_second_call_succeeds(native, placements):
    import vk_merkle_roots_amd as vk
    f = rc.forest()
    what, trees, lo, hi = f.queries()
    want = f.expected()
    n = int(want[6][1])
    for capacity in (0, 1, n - 1):
        rc_, firsts, starts, leaves, left, right, heights, info = rc.host_range(*placements[0], trees, lo, hi, capacity=capacity)
        assert rc_ == 0 and info.tolist() == [1, n] + want[6].tolist()[2:] and (leaves == rc.CANARY).all()   # no leaf written
        assert (firsts == want[0]).all() and (starts == want[1]).all() and (heights == want[5]).all() and (left == want[3]).all()
    again = rc.host_range(*placements[0], trees, lo, hi, capacity=n)
    assert again[7].tolist() == want[6].tolist() and (again[3][:n] == want[2]).all()
    assert vk.range_status_text(0) == "ok" and "bit 0" in vk.range_status_text(1) and "unknown" in vk.range_status_text(6)


def test_the_read_set_of_the_check():
    f = rc.forest()
    what, trees, lo, hi = f.queries()
    firsts, starts, leaves, left, right, heights, *_ = f.expected()
    for q in np.nonzero(trees == 12)[0]:
        a, m = int(firsts[q]), int(starts[q + 1] - starts[q])
        if a == rc.NONE:
            continue
        reads, b = set(), a + m - 1
        assert rc.model_verdict(12, 13, lo[q], hi[q], a, leaves[int(starts[q]): int(starts[q + 1])], left[q], right[q], 12, f.roots[12], 2500, reads)[0] == 1
        want = {("left", l) for l in range(12) if (a >> l) & 1} | {("right", l) for l in range(12) if not (b >> l) & 1 and (b >> l) + 1 < ((2499 >> l) + 1)}
        assert reads == want, q
        assert all(left[q, l].any() == (("left", l) in want) and right[q, l].any() == (("right", l) in want) for l in range(12))


def test_the_verifiers_negatives(native):
    neg = rc.negatives()
    want = [w for _, w, _ in neg]
    assert want.count(1) >= 8 and want.count(0) >= 17
    batch = rc.batch([p for _, _, p in neg])
    got, in_first, in_count = rc.host_verify(*batch)
    assert got.tolist() == want, [w for (w, _, _), a, b in zip(neg, got, want) if a != b]
    assert all(v == 1 or (a == 0 and n == 0) for v, a, n in zip(got, in_first, in_count))
    model = [rc.model_verdict(0, 1, p["lo"], p["hi"], p["first"], p["leaves"], p["left"], p["right"], p["h"], p["root"], p["c"])[0] for _, _, p in neg]
    assert model == want
    beyond = list(batch)
    beyond[0] = batch[0] + np.uint32(len(neg))                                                      # every tree outside the table
    assert not rc.host_verify(*beyond)[0].any()
    bent = list(batch)
    bent[4] = batch[4].copy()
    bent[4][3] = bent[4][4] + np.uint64(1)                                                          # leaf_starts that is no prefix: nothing is proven
    assert not rc.host_verify(*bent)[0].any()


# ---- the Python layer's host side --------------------------------------------------------------------------------------------------------
def test_range_proofs_hold_their_shapes_and_refuse_others():
    import vk_merkle_roots_amd as vk
    f = rc.forest()
    what, trees, lo, hi = f.queries()
    firsts, starts, leaves, left, right, heights, info, verdict, in_first, in_count = f.expected()
    p = vk.RangeProofs(trees, lo, hi, firsts, starts, leaves, left, right, heights, info)
    assert p.Q == len(p) == len(trees) and p.stride == 12 and p.same_as(p)
    for q in range(0, p.Q, 5):
        inside = p.in_range(q)
        assert inside.shape[0] == int(in_count[q])
        if verdict[q] and in_count[q]:
            assert (inside == f.trees[int(trees[q])][int(in_first[q]): int(in_first[q] + in_count[q])]).all()
        one = p[q]
        assert one["tree"] == trees[q] and one["first"] == firsts[q] and one["leaves"].shape[0] == starts[q + 1] - starts[q] and one["left"].shape == (12, 8)
    with pytest.raises(IndexError):
        p[p.Q]
    with pytest.raises(ValueError):
        vk.RangeProofs(trees, lo, hi, firsts, starts[:-1], leaves, left, right, heights)
    with pytest.raises(ValueError):
        vk.RangeProofs(trees, lo, hi, firsts, starts, leaves, left, right[:, :7], heights)
    empty = vk.RangeProofs([], np.zeros((0, 8)), np.zeros((0, 8)), [], [0], np.zeros((0, 8)), np.zeros((0, 12, 8)), np.zeros((0, 12, 8)), [])
    assert [x.shape for x in empty.verify(NoDevice(), f.roots, f.counts)] == [(0,)] * 3
    tree = vk.MerkleTree(NoDevice(), None, 5, 4, None)                                              # stored taller than max(1, ceil(log2 5)): refused on the host
    with pytest.raises(ValueError, match="height"):
        tree.range(lo[:2], hi[:2])
    forest = vk.MerkleForest.__new__(vk.MerkleForest)
    with pytest.raises(ValueError, match="one upper bound"):
        vk.MerkleForest._ranges(forest, trees[:2], lo[:2], hi[:3], 12)
    with pytest.raises(ValueError, match="one tree"):
        vk.MerkleForest._ranges(forest, trees[:3], lo[:2], hi[:2], 12)


def test_the_code_object(native):
    from vk_merkle_roots_amd import isa_prio_pass
    for k in FOLDS:
        assert_key_resolves(k)
    rec = isa_record(native)
    assert rec is not None
    for k in FOLDS:
        mine = {name: len(v) for name, v in rec["hash_blocks"].items() if k in name}
        assert list(mine.values()) == [isa_prio_pass.EXPECTED_HASH_BLOCKS[k]] == [1], k
    assert rec["audit"]["block_count_errors"] == [] and {v for name, v in rec["audit"]["blocks"].items() if "range_level" in name} == {1}
    assert not any("_range_" in name and "range_level" not in name for name in rec["hash_blocks"])   # the others hash nothing
    assert_no_spills(native, POINTER_FIRST)
    assert_no_spills(native, SCALAR_FIRST, prefix=True)
