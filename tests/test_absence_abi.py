"""Sorted trees and absence proofs without a GPU: the C ABI's declarations and argument checks (vkmr_hip_forest_sorted_async,
vkmr_hip_forest_lower_bound_async, vkmr_hip_forest_absence_async, vkmr_hip_verify_forest_absence_async and their one-tree
twins), the rules of csrc/absence_plan.hpp replayed (tests/c/absence_plan_test.cpp, its own program under AddressSanitizer and
UBSan), the CPU twins (vkmr_host_cpu_forest_sorted, _lower_bound, _absence, vkmr_host_cpu_verify_absence) against the hashlib
model of tests/absence_cases.py on every case, and the host side of vk.AbsenceProofs and vk.sort_digests.  No compute call on a
device here."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import absence_cases as ac
from abi_support import Refusals, assert_bound, assert_exported, assert_key_resolves, assert_no_spills, isa_record
from merkle_model import random_leaves
from no_device import NoDevice

ENTRY_POINTS = {"vkmr_hip_forest_sorted_async": 8, "vkmr_hip_tree_sorted_async": 6, "vkmr_hip_forest_lower_bound_async": 11,
                "vkmr_hip_tree_lower_bound_async": 8, "vkmr_hip_forest_absence_async": 17, "vkmr_hip_tree_absence_async": 12,
                "vkmr_hip_verify_forest_absence_async": 15, "vkmr_hip_verify_absence_async": 12}
HOST_ENTRY_POINTS = {"vkmr_host_cpu_forest_sorted": 6, "vkmr_host_cpu_forest_lower_bound": 9, "vkmr_host_cpu_forest_absence": 13,
                     "vkmr_host_cpu_verify_absence": 13}
FOLDS = ("forest_absence_fold_kernel", "tree_absence_fold_kernel")
KERNELS = ("forest_sorted_scan_kernel", "tree_sorted_scan_kernel", "forest_sorted_finish_kernel", "tree_sorted_finish_kernel", "forest_lower_bound_kernel",
           "tree_lower_bound_kernel", "forest_absence_entries_kernel", "tree_absence_entries_kernel", "forest_absence_rows_kernel",
           "tree_absence_rows_kernel") + FOLDS


def test_header_declares_them_and_the_stub_binds_every_argument():
    from vk_merkle_roots_amd import _abi
    for name, nparams in ENTRY_POINTS.items():
        assert_bound(name, nparams=nparams, restype=C.c_int)
    for name, nparams in HOST_ENTRY_POINTS.items():
        assert_bound(name, nparams=nparams, restype=C.c_int, table=_abi.HOST_SIGNATURES, header="vkmr_host.h")


def test_libraries_export_them(native):
    assert_exported(native.HIP_LIB, ENTRY_POINTS)
    assert_exported(native.HOST_LIB, HOST_ENTRY_POINTS)


def test_bad_arguments_are_refused_before_any_hip_call(native):
    from vk_merkle_roots_amd import _abi
    lib = _abi.lib()
    d, odd = C.c_void_p(0x1000), C.c_void_p(0x1004)        # never dereferenced: every call below returns before launching anything
    big = (1 << 58) + 1
    # digests, total, offsets, ntrees, first_bad, info
    r = Refusals(lib.vkmr_hip_forest_sorted_async, "vkmr_hip_forest_sorted_async", good=[d, 100, d, 8, d, d])
    r.null(0, 2, 4, 5)
    r.changed({1: big}, {0: odd}, {2: odd}, {4: odd}, {5: odd})
    r.ok([None, 0, None, 0, None, None])
    # digests, count, first_bad, info
    r = Refusals(lib.vkmr_hip_tree_sorted_async, "vkmr_hip_tree_sorted_async", good=[d, 100, d, d])
    r.null(0, 2, 3)
    r.changed({1: big}, {0: odd}, {2: odd}, {3: odd})
    # digests, total, offsets, ntrees, trees, queries, Q, indices, found
    r = Refusals(lib.vkmr_hip_forest_lower_bound_async, "vkmr_hip_forest_lower_bound_async", good=[d, 100, d, 8, d, d, 5, d, d])
    r.null(0, 2, 4, 5, 7, 8)
    r.changed({1: big}, {0: odd}, {5: odd}, {7: odd}, {2: odd})
    r.ok([None, 0, None, 0, None, None, 0, None, None])
    # digests, count, queries, Q, indices, found
    r = Refusals(lib.vkmr_hip_tree_lower_bound_async, "vkmr_hip_tree_lower_bound_async", good=[d, 100, d, 5, d, d])
    r.null(0, 2, 4, 5)
    r.changed({1: big}, {0: odd}, {2: odd}, {4: odd})
    r.ok([None, 0, None, 0, None, None])
    # digests, forest, total, offsets, ntrees, max_count, trees, queries, Q, stride, indices, neighbours, main, low, heights
    r = Refusals(lib.vkmr_hip_forest_absence_async, "vkmr_hip_forest_absence_async", good=[d, d, 100, d, 8, 50, d, d, 5, 6, d, d, d, d, d])
    r.null(0, 1, 3, 6, 7, 10, 11, 12, 13, 14)
    r.changed({9: 0}, {9: 64}, {9: 5}, {5: 0}, {2: big}, {0: odd}, {1: odd}, {7: odd}, {10: odd}, {11: odd}, {12: odd}, {13: odd})   # stride 5: 50 leaves need 6
    r.ok([None, None, 0, None, 0, 0, None, None, 0, 0] + [None] * 5)
    # digests, tree, count, height, queries, Q, indices, neighbours, main, low
    r = Refusals(lib.vkmr_hip_tree_absence_async, "vkmr_hip_tree_absence_async", good=[d, d, 100, 7, d, 5, d, d, d, d])
    r.null(0, 1, 4, 6, 7, 8, 9)
    r.changed({3: 6}, {3: 8}, {2: 0}, {2: big}, {0: odd}, {4: odd}, {6: odd}, {8: odd})
    r.ok([None, None, 0, 0, None, 0, None, None, None, None])
    # queries, trees, indices, neighbours, main, low, heights, Q, stride, roots, counts, ntrees, verdict
    r = Refusals(lib.vkmr_hip_verify_forest_absence_async, "vkmr_hip_verify_forest_absence_async", good=[d, d, d, d, d, d, d, 5, 6, d, d, 8, d])
    r.null(0, 1, 2, 3, 4, 5, 6, 9, 10, 12)
    r.changed({8: 0}, {8: 64}, {0: odd}, {2: odd}, {3: odd}, {4: odd}, {5: odd}, {9: odd}, {10: odd})
    r.ok([None] * 7 + [0, 0, None, None, 0, None])
    # queries, indices, neighbours, main, low, Q, height, root, count, verdict
    r = Refusals(lib.vkmr_hip_verify_absence_async, "vkmr_hip_verify_absence_async", good=[d, d, d, d, d, 5, 7, d, 100, d])
    r.null(0, 1, 2, 3, 4, 7, 9)
    r.changed({6: 6}, {6: 8}, {8: 0}, {0: odd}, {1: odd}, {3: odd}, {7: odd})
    r.ok([None, None, None, None, None, 0, 0, None, 0, None])
    # and the twins
    import vk_merkle_roots_amd as vk
    host = vk.host_lib()
    z = np.zeros(64, np.uint64)
    p = z.ctypes.data
    assert host.vkmr_host_cpu_forest_sorted(p, 0, None, 1, p, p) == -1 and host.vkmr_host_cpu_forest_sorted(None, 0, None, 0, None, None) == 0
    assert host.vkmr_host_cpu_forest_lower_bound(p, 0, p, 1, None, p, 1, p, p) == -1 and host.vkmr_host_cpu_forest_lower_bound(p, 0, p, 1, p, p, 0, p, p) == 0
    assert host.vkmr_host_cpu_forest_absence(p, 0, p, 1, p, p, 1, 4, p, p, None, p, p) == -1 and host.vkmr_host_cpu_forest_absence(None, 0, None, 0, None, None, 0, 0, None, None, None, None, None) == 0
    assert host.vkmr_host_cpu_verify_absence(p, p, p, p, p, p, p, 1, 64, p, p, 1, p) == -1 and host.vkmr_host_cpu_verify_absence(None, None, None, None, None, None, None, 0, 0, None, None, 0, None) == 0
    down = np.array([4, 2, 6], dtype=np.uint64)             # offsets that decrease, and offsets that end behind the cells
    assert host.vkmr_host_cpu_forest_sorted(p, 8, down.ctypes.data, 2, p, p) == 1
    behind = np.array([0, 2, 6], dtype=np.uint64)
    assert host.vkmr_host_cpu_forest_sorted(p, 5, behind.ctypes.data, 2, p, p) == 1


# ---- the replay of the plan ------------------------------------------------------------------------------------------------------------
def test_the_plan_replayed_for_every_count_and_index_up_to_130(tmp_path):
    exe = ac.build_absence_plan_exe(tmp_path)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    text = r.stdout.decode()
    assert r.returncode == 0 and "FAIL" not in text and f"ok: {sum(c + 1 for c in range(1, 131))} cases" in text, text[-2000:]


# ---- the model itself ----------------------------------------------------------------------------------------------------------------
def test_the_order_is_that_of_the_digest_bytes_and_unsigned():
    rng = np.random.default_rng(611)
    rows = random_leaves(rng, 200)
    rows[:50, 0] = rows[50:100, 0]                                                                 # ties on word 0 ...
    rows[:20, :7] = rows[50:70, :7]                                                                # ... and down to word 7
    by_bytes = sorted(range(200), key=lambda j: rows[j].astype(">u4").tobytes())
    assert [ac.key(rows[j]) for j in by_bytes] == sorted(ac.key(r) for r in rows)
    assert ac.key([0x7FFFFFFF] + [0xFFFFFFFF] * 7) < ac.key([0x80000000] + [0] * 7)
    assert [ac.as_int(ac.from_int(n)) for n in (0, 1, (1 << 256) - 1, 1 << 200)] == [0, 1, (1 << 256) - 1, 1 << 200]


def test_sort_digests_is_the_models_order_per_tree():
    import vk_merkle_roots_amd as vk
    rng = np.random.default_rng(612)
    counts = [5, 0, 64, 1, 30]
    rows = random_leaves(rng, 100)
    rows[5:40, 0] = 0x80000000
    rows[40:69, 0] = 0x7FFFFFFF
    rows[10:20, 1:7] = 7
    got = vk.sort_digests(rows, counts)
    at = 0
    for c in counts:
        if c:
            assert (got[at: at + c] == ac.sorted_rows(rows[at: at + c])).all()
        at += c
    with pytest.raises(ValueError):
        vk.sort_digests(rows, [5, 5])


# ---- the CPU twins against the model -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def placements():
    f = ac.forest()
    return [f.placed(), f.placed(first=5, slack=7)]


def test_the_forest_holds_what_the_cases_promise():
    f = ac.forest()
    trees, digests = f.queries()
    idx, found, pred, succ, main, low, heights, verdicts = f.expected()
    assert f.counts == [1, 2, 3, 0, 4, 5, 7, 8, 9, 0, 63, 64, 65, 130] and 2500 < len(trees) < 4000
    assert int((verdicts == ac.PRESENT).sum()) >= sum(f.counts) and int((verdicts == ac.ABSENT).sum()) > 1000 and int((verdicts == 0).sum()) == 9
    run = [ac.key(r) for r in f.run]
    assert all(a[:7] == b[:7] for a, b in zip(run, run[1:])) and run == sorted(run)
    nine = [ac.key(r) for r in f.trees[8]]
    assert all(k in nine for k in run) and nine.index(run[2]) == nine.index(run[0]) + 2
    seven = [ac.key(r) for r in f.trees[6]]
    at = seven.index((0x7FFFFFFF,) + (0xFFFFFFFF,) * 7)
    assert seven[at + 1] == (0x80000000,) + (0,) * 7                                               # a signed compare would put them the other way
    zero_or_ones = (digests == 0).all(axis=1) | (digests == 0xFFFFFFFF).all(axis=1)
    assert (verdicts[zero_or_ones & (trees == 7)] == ac.PRESENT).all() and (verdicts[zero_or_ones & (trees < 14) & (trees != 7)] == ac.ABSENT).all()
    # every index 0..c of every tree is some absent query's -- but where no digest lies between: below zero, above all ones, and
    # between 0x7FFFFFFF FFFFFFFF.. and 0x80000000 00000000.., between word 7 = 5 and 6 of the run -- and every top from 0 to 7 occurs
    for t, c in enumerate(f.counts):
        mine = (trees == t) & (verdicts == ac.ABSENT)
        bounds = [-1] + [ac.as_int(r) for r in f.trees[t]] + [1 << 256]
        room = {i for i in range(c + 1) if bounds[i + 1] - bounds[i] >= 2}
        assert set(idx[mine].tolist()) == room and set(range(c + 1)) - room == ({0, c} if t == 7 else {at + 1} if t == 6 else {nine.index(run[1])} if t == 8 else set()), t
    assert {ac.ctz(int(i)) for i in idx[(trees == 13) & (verdicts == ac.ABSENT) & (idx > 0) & (idx < 130)]} == set(range(8))


def test_the_twins_are_the_model_on_every_case(native, placements):
    f = ac.forest()
    trees, digests = f.queries()
    idx, found, pred, succ, main, low, heights, verdicts = f.expected()
    for cells, offsets in placements:
        got_idx, got_found = ac.host_lower_bound(cells, offsets, trees, digests)
        assert (got_idx == idx).all() and (got_found == found).all()
        rc, *got = ac.host_absence(cells, offsets, trees, digests)
        assert rc == 0
        for what, a, b in zip(("indices", "pred", "succ", "main", "low", "heights"), got, (idx, pred, succ, main, low, heights)):
            assert a.shape == b.shape and (a == b).all(), (what, np.nonzero((a != b).reshape(a.shape[0], -1).any(axis=1))[0][:8])
        assert (ac.host_verify(digests, trees, *got, f.roots, f.counts) == verdicts).all()
    wide = ac.host_absence(*placements[1], trees, digests, stride=11)
    assert wide[0] == 0 and (wide[4][:, :8] == main).all() and not wide[4][:, 8:].any() and not wide[5][:, 8:].any()
    assert (ac.host_verify(digests, trees, *wide[1:], f.roots, f.counts) == verdicts).all()
    assert ac.host_absence(*placements[0], trees, digests, stride=7)[0] == 2                        # the tree of 130 needs eight cells


def test_the_read_set_of_the_check():
    f = ac.forest()
    trees, digests = f.queries()
    idx, found, pred, succ, main, low, heights, verdicts = f.expected()
    for q in np.nonzero(trees == 13)[0][::7]:
        reads, c, i = set(), 130, int(idx[q])
        assert ac.model_verdict(digests[q], 13, 14, i, pred[q], succ[q], main[q], low[q], heights[q], f.roots[13], c, reads) == verdicts[q]
        want = {("main", l) for l in range(8)} | ({("low", l) for l in range(ac.ctz(i))} if 0 < i < c and not found[q] else set())
        assert reads == want, q


def test_lower_bound_on_an_unsorted_tree_is_the_loop(native):
    rng = np.random.default_rng(613)
    trees = [random_leaves(rng, c) for c in (1, 2, 7, 64, 131)]
    for t in trees[2:]:
        t[: len(t) // 2, 0] = 5                                                                    # long ties on word 0, in no order below
    cells, offsets = ac.lay(trees, first=3, slack=2)
    which = np.concatenate([np.full(len(t) + 3, j, np.uint32) for j, t in enumerate(trees)])
    digests = np.concatenate([np.concatenate([t, random_leaves(rng, 3)]) for t in trees])
    got_idx, got_found = ac.host_lower_bound(cells, offsets, which, digests)
    want = [ac.model_lower_bound(trees[int(t)], x) for t, x in zip(which, digests)]
    assert got_idx.tolist() == [w[0] for w in want] and got_found.tolist() == [int(w[1]) for w in want]
    assert any(ac.model_first_bad(t)[0] != ac.NONE for t in trees) and not all(got_found[which == 4][:131])   # the loop misses leaves that are there


@pytest.mark.parametrize("case", ac.sortedness_cases(), ids=[c[0] for c in ac.sortedness_cases()])
def test_sortedness(native, case):
    what, trees, first_bad, unsorted, equal, pairs = case
    for first, slack in ((0, 0), (4, 3)):
        rc, bad, info = ac.host_sorted(*ac.lay(trees, first, slack))
        assert rc == 0 and (bad == first_bad).all() and info.tolist() == [0, unsorted, equal, pairs], (what, bad, info)
    if what == "clean":
        assert unsorted == 0 and pairs == sum(ac.COUNTS) - 12
    if what == "two offences in one tree":
        assert first_bad[13] == 41 and equal == 1
    if what == "a descent across a tree boundary only":
        assert unsorted == 0


def test_the_verifiers_negatives(native):
    what, want, *batch = ac.negatives_batch()
    assert sorted(set(want.tolist())) == [0, 1] and int((want == 1).sum()) == 4
    got = ac.host_verify(*batch)
    assert got.tolist() == want.tolist(), [w for w, a, b in zip(what, got, want) if a != b]
    model = [ac.model_verdict(batch[0][q], q, len(what), batch[2][q], batch[3][q], batch[4][q], batch[5][q], batch[6][q], batch[7][q], batch[8][q], batch[9][q])
             for q in range(len(what))]
    assert model == want.tolist()
    beyond = list(batch)
    beyond[1] = batch[1] + np.uint32(len(what))                                                     # every tree outside the table
    assert not ac.host_verify(*beyond).any()


# ---- the Python layer's host side --------------------------------------------------------------------------------------------------------
def test_absence_proofs_hold_their_shapes_and_refuse_others():
    import vk_merkle_roots_amd as vk
    f = ac.forest()
    trees, digests = f.queries()
    idx, found, pred, succ, main, low, heights, verdicts = f.expected()
    p = vk.AbsenceProofs(trees, digests, idx, pred, succ, main, low, heights)
    assert p.Q == len(trees) and p.stride == 8 and p.neighbours.shape == (p.Q, 2, 8) and (p.neighbours[:, 1] == succ).all() and p.same_as(p)
    with pytest.raises(ValueError):
        vk.AbsenceProofs(trees, digests, idx[:-1], pred, succ, main, low, heights)
    with pytest.raises(ValueError):
        vk.AbsenceProofs(trees, digests, idx, pred, succ, main, low[:, :7], heights)
    empty = vk.AbsenceProofs([], np.zeros((0, 8)), [], np.zeros((0, 8)), np.zeros((0, 8)), np.zeros((0, 8, 8)), np.zeros((0, 8, 8)), [])
    assert empty.verify(NoDevice(), f.roots, f.counts).shape == (0,)
    tree = vk.MerkleTree(NoDevice(), None, 5, 4, None)                                              # stored taller than max(1, ceil(log2 5)): refused on the host
    with pytest.raises(ValueError, match="height"):
        tree.absence(digests[:2])


def test_the_code_object(native):
    from vk_merkle_roots_amd import isa_prio_pass
    for k in FOLDS:
        assert_key_resolves(k)
    rec = isa_record(native)
    assert rec is not None
    for k in FOLDS:
        mine = {name: len(v) for name, v in rec["hash_blocks"].items() if k in name}
        assert list(mine.values()) == [isa_prio_pass.EXPECTED_HASH_BLOCKS[k]] == [1], k
    assert rec["audit"]["block_count_errors"] == [] and {v for name, v in rec["audit"]["blocks"].items() if "absence" in name} == {1}
    assert not any(part in name for name in rec["hash_blocks"] for part in ("sorted_", "lower_bound", "absence_entries", "absence_rows"))   # they hash nothing
    assert_no_spills(native, KERNELS)
