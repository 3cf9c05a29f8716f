"""Consistency proofs without a GPU: the C ABI's declarations and argument checks (vkmr_hip_forest_consistency_async,
vkmr_hip_verify_consistency_async), the rules of csrc/consistency_plan.hpp replayed with values (tests/c/consistency_plan_test.cpp,
its own program under AddressSanitizer and UBSan), the CPU twins (vkmr_host_cpu_forest_consistency, _verify_consistency) against
the hashlib model of tests/consistency_cases.py -- the read set cell by cell --, and the host side of vk.ConsistencyProof.  No
compute call on a device here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import consistency_cases as cc
from abi_support import Refusals, assert_bound, assert_exported, assert_key_resolves, assert_no_spills, isa_record
from conftest import ROOT
from merkle_model import random_counts, random_leaves
from no_device import NoDevice

ENTRY_POINTS = {"vkmr_hip_forest_consistency_async": 17, "vkmr_hip_verify_consistency_async": 11}
HOST_ENTRY_POINTS = {"vkmr_host_cpu_forest_consistency": 10, "vkmr_host_cpu_verify_consistency": 9}
FOLD = "consistency_fold_kernel"
KERNELS = ("consistency_check_kernel", "consistency_gather_kernel", FOLD)
NAMES_OTHER_TESTS_COUNT = ("frontier", "mutated", "apply_", "_audit_", "forest_multiproof", "forest_update", "forest_extend", "forest_append",
                           "forest_truncate", "forest_proofs_kernel")


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
    d = C.c_void_p(0x1000)                 # never dereferenced: every call below returns before launching anything
    # digests, forest, total, offsets, ntrees, max_count, roots, trees, old_counts, Q, stride, new_counts, peaks, rights, status
    gather = Refusals(lib.vkmr_hip_forest_consistency_async, "vkmr_hip_forest_consistency_async", good=[d, d, 100, d, 8, 50, d, d, d, 5, 6, d, d, d, d])
    gather.null(0, 1, 3, 6, 7, 8, 11, 12, 13, 14)
    # what vkmr_hip_forest_frontier_async refuses: stride 5 -- a tree of 50 leaves has six bits
    gather.changed({10: 0}, {10: 65}, {10: 5}, {5: 0}, {2: (1 << 58) + 1})
    gather.ok((None, None, 0, None, 0, 0, None, None, None, 0, 0, None, None, None, None))      # no query
    # the verifier: old counts, new counts, peaks, rights, stride, Q, old roots, new roots, ok
    verify = Refusals(lib.vkmr_hip_verify_consistency_async, "vkmr_hip_verify_consistency_async", good=[d, d, d, d, 8, 3, d, d, d])
    verify.null(0, 1, 2, 3, 6, 7, 8)
    verify.changed({4: 0}, {4: 65})        # the stride
    verify.ok((None, None, None, None, 0, 0, None, None, None))
    # and the twins
    import vk_merkle_roots_amd as vk
    host = vk.host_lib()
    z = np.zeros(64, np.uint64)
    p = z.ctypes.data
    assert host.vkmr_host_cpu_forest_consistency(p, p, 1, p, p, 1, 0, p, p, p) == -1 and host.vkmr_host_cpu_forest_consistency(p, p, 1, p, p, 1, 65, p, p, p) == -1
    assert host.vkmr_host_cpu_forest_consistency(p, p, 1, None, p, 1, 8, p, p, p) == -1 and host.vkmr_host_cpu_forest_consistency(p, None, 1, p, p, 0, 8, p, p, p) == 0
    assert host.vkmr_host_cpu_verify_consistency(p, p, p, p, 0, 1, p, p, p) == -1 and host.vkmr_host_cpu_verify_consistency(p, p, p, None, 8, 1, p, p, p) == -1
    assert host.vkmr_host_cpu_verify_consistency(None, None, None, None, 0, 0, None, None, None) == 0


# ---- the replay of the plan ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    return cc.build_consistency_plan_exe(tmp_path_factory.mktemp("consistency_plan"))


def test_every_pair_up_to_130_replayed(plan_exe, tmp_path):
    pairs = [(c, c2) for c2 in range(1, 131) for c in range(c2 + 1)]
    cases = [(c2 % 5, max(1, c2.bit_length()), [c2], [(0, c)]) for c, c2 in pairs]                 # each alone, the tightest stride
    counts = cc.square_counts(130)
    trees, old = cc.every_pair(counts)
    cases.append((7, 8, counts, list(zip(trees.tolist(), old.tolist()))))                          # and side by side in one forest
    got = cc.plan_replay(plan_exe, tmp_path, cases)
    for (c, c2), (cells, hashes, status) in zip(pairs, got):
        assert status == 0 and cells == len(cc.read_set(c, c2)) and hashes == cc.hashes(c, c2) <= cc.tree_height(max(c, 1)) + cc.tree_height(c2), (c, c2)
    assert got[-1] == (sum(g[0] for g in got[:-1]), sum(g[1] for g in got[:-1]), 0)


def test_a_thousand_random_forests_replayed(plan_exe, tmp_path):
    rng = np.random.default_rng(20264)
    cases = []
    while len(cases) < 1000:
        counts = random_counts(rng, 9000)
        if not counts:
            continue
        stride = int(rng.integers(max(max(counts).bit_length(), 1), 65))
        queries = []
        for _ in range(int(rng.integers(1, 40))):
            t = int(rng.integers(0, len(counts)))
            n = counts[t]
            kind = int(rng.integers(0, 4))
            c = n if kind == 0 else int(rng.integers(0, n + 1)) if kind == 1 else min(n, 1 << int(rng.integers(0, 14))) if kind == 2 else max(0, n - int(rng.integers(0, 3)))
            queries.append((t, c))
        cases.append((int(rng.integers(0, 70)) * int(rng.integers(0, 2)), stride, counts, queries))
    got = cc.plan_replay(plan_exe, tmp_path, cases)
    for (_, _, counts, queries), (cells, hashes, status) in zip(cases, got):
        assert status == 0
        assert cells == sum(len(cc.read_set(c, counts[t])) for t, c in queries) and hashes == sum(cc.hashes(c, counts[t]) for t, c in queries)


def test_the_replay_reports_the_refusals(plan_exe, tmp_path):
    cases = [(3, stride, cc.REFUSAL_COUNTS, list(zip(trees, old))) for _, _, trees, old, stride, _ in cc.REFUSALS]
    assert [g[2] for g in cc.plan_replay(plan_exe, tmp_path, cases)] == [r[1] for r in cc.REFUSALS]


# ---- the CPU twins against the model -------------------------------------------------------------------------------------------------
def test_every_pair_up_to_130_in_one_batched_call(native):
    forest = cc.square()
    assert int(forest.offsets[0]) > 0 and forest.counts.count(0) == 18
    trees, old = cc.every_pair(forest.counts)
    assert trees.shape[0] == sum(n + 1 for n in forest.counts) > 8600
    order = np.random.default_rng(411).permutation(trees.shape[0])                               # out of order
    trees, old = trees[order], old[order]
    status, new_counts, peaks, rights = cc.host_gather(forest.leaves, forest.offsets, trees, old, stride=9)
    want = forest.proofs(trees, old, stride=9)
    assert status == 0
    for what, a, b in zip(("new counts", "peaks", "rights"), (new_counts, peaks, rights), want):
        assert a.shape == b.shape and (a == b).all(), (what, np.nonzero((a != b).reshape(a.shape[0], -1).any(axis=1))[0][:8])
    old_roots, new_roots = forest.query_roots(trees, old)
    ok = cc.host_verify(old, new_counts, peaks, rights, old_roots, new_roots)
    assert (ok == 1).all(), np.nonzero(ok != 1)[0][:8]
    for q in range(0, trees.shape[0], 37):                                                       # the model's own check, on a sample
        assert cc.model_check(old[q], new_counts[q], peaks[q], rights[q], old_roots[q], new_roots[q]) == 1
    # swapped roots: 0, unless the two counts are one (and, for c == 0, unless the new root is the zero root)
    swapped = cc.host_verify(old, new_counts, peaks, rights, new_roots, old_roots)
    want_swapped = ((old == new_counts) | ((old == 0) & ~new_roots.any(axis=1))).astype(np.uint32)
    assert (swapped == want_swapped).all()


def test_queries_repeated_and_out_of_order(native):
    forest = cc.Forest([9, 0, 130, 64], seed=412, first=1)
    trees = [2, 0, 2, 3, 2, 0, 3, 1, 2]
    old = [130, 9, 64, 64, 64, 0, 1, 0, 130]
    status, new_counts, peaks, rights = cc.host_gather(forest.leaves, forest.offsets, trees, old, stride=8)
    want = forest.proofs(trees, old, stride=8)
    assert status == 0 and all((a == b).all() for a, b in zip((new_counts, peaks, rights), want))
    assert (peaks[2] == peaks[4]).all() and (rights[2] == rights[4]).all() and (peaks[0] == peaks[8]).all()
    old_roots, new_roots = forest.query_roots(trees, old)
    assert (cc.host_verify(old, new_counts, peaks, rights, old_roots, new_roots) == 1).all()


def test_a_tree_of_two_to_the_forty_leaves_whose_cells_are_random_digests(native):
    """No such tree can be built: the cells are random digests, the two roots what the model's walk makes of them."""
    rng = np.random.default_rng(413)
    pairs = [((1 << 40) + (1 << 33) + 7, (1 << 40) + (1 << 35)), (1 << 40, 1 << 40), (1 << 40, (1 << 40) + 1), ((1 << 39) + 1, 1 << 40), (1, (1 << 40) - 1),
             ((1 << 58) - 1, 1 << 58)]
    stride = 59
    peaks, rights = random_leaves(rng, len(pairs) * stride).reshape(-1, stride, 8), random_leaves(rng, len(pairs) * stride).reshape(-1, stride, 8)
    old_roots, new_roots = np.zeros((len(pairs), 8), np.uint32), np.zeros((len(pairs), 8), np.uint32)

    for q, (c, c2) in enumerate(pairs):
        old_roots[q], new_roots[q] = cc.model_walk(c, c2, peaks[q], rights[q])
        assert cc.model_check(c, c2, peaks[q], rights[q], old_roots[q], new_roots[q]) == 1
    old, new = [c for c, _ in pairs], [c2 for _, c2 in pairs]
    assert cc.host_verify(old, new, peaks, rights, old_roots, new_roots).tolist() == [1] * len(pairs)
    flipped = rights.copy()
    flipped[0, 33, 0] ^= 1                                  # c = 2^40 + 2^33 + 7: bit 33 is set, the walk takes P_33 there, not rights[33]
    flipped[2, 40, 7] ^= 1 << 31                            # c = 2^40 of 2^40 + 1: the seed's right neighbour at level 40
    assert cc.host_verify(old, new, peaks, flipped, old_roots, new_roots).tolist() == [1, 1, 0, 1, 1, 1]
    # above 2^58, or of more bits than the rows have cells: 0 and nothing read
    assert cc.host_verify([1], [(1 << 58) + 1], peaks[:1], rights[:1], old_roots[:1], new_roots[:1]).tolist() == [0]
    assert cc.host_verify(old[:1], new[:1], peaks[:1, :40], rights[:1, :40], old_roots[:1], new_roots[:1]).tolist() == [0]


@pytest.mark.parametrize("what,status,trees,old,stride,max_count", cc.REFUSALS, ids=[r[0] for r in cc.REFUSALS])
def test_every_status_bit_is_reported_and_nothing_written(native, what, status, trees, old, stride, max_count):
    import vk_merkle_roots_amd as vk
    forest = cc.Forest(cc.REFUSAL_COUNTS, seed=414)
    got = cc.host_gather(forest.leaves, forest.offsets, trees, old, stride=stride)
    assert got[0] == status, what
    assert (got[1] == cc.COUNT_FILL).all() and (got[2] == cc.CANARY).all() and (got[3] == cc.CANARY).all()
    for bit in range(3):
        assert (f"bit {bit}:" in vk.consistency_status_text(status)) == bool(status >> bit & 1)
    # and the same queries with the fault taken out go through
    fine = cc.host_gather(forest.leaves, forest.offsets, [0, 3, 2], [5, 100, 9], stride=8)
    assert fine[0] == 0 and fine[1].tolist() == [5, 129, 9]


def test_the_status_text_names_every_bit(native):
    import vk_merkle_roots_amd as vk
    assert vk.consistency_status_text(0) == "ok"
    for bit in range(3):
        assert f"bit {bit}:" in vk.consistency_status_text(1 << bit) and "unknown" not in vk.consistency_status_text(1 << bit)
    assert "unknown bits" in vk.consistency_status_text(8)


# ---- the read set, exactly -------------------------------------------------------------------------------------------------------------
def test_the_read_set_exactly_one_flipped_bit_per_cell(native):
    """Every pair up to 40, both rows: a flip in a cell the rule reads gives 0, a flip anywhere else leaves 1."""
    f = cc.flips(40)
    assert f.stride == 6 and len(f.rows) == 820 * 13
    ok = cc.host_verify(f.old_counts, f.new_counts, f.peaks, f.rights, f.old_roots, f.new_roots)
    wrong = np.nonzero(ok != f.want)[0]
    assert wrong.size == 0, [(f.rows[i][0], f.rows[i][1], f.rows[i][5], int(ok[i])) for i in wrong[:8]]
    assert 0 < int(f.want.sum()) < len(f.rows) and int((f.want == 0).sum()) == sum(len(cc.read_set(r[0], r[1])) for r in f.rows if r[5] is None)
    for i in range(0, len(f.rows), 11):                      # the model itself decides: a sample of every kind of row
        assert cc.model_check(f.old_counts[i], f.new_counts[i], f.peaks[i], f.rights[i], f.old_roots[i], f.new_roots[i]) == f.want[i], f.rows[i][:2]


def test_a_changed_count_on_either_side(native):
    """The honest proof of (c, c2) verified as (c', c2) and as (c, c2'): 0, except where the model itself walks the same way."""
    top, stride = 40, 7
    rng = np.random.default_rng(415)
    leaves = random_leaves(rng, top)
    roots = cc.prefix_roots(leaves)
    rows = []                                               # (claimed c, claimed c2, peaks, rights, old root, new root, the walk is the same)
    from merkle_model import cpu_levels
    for c2 in range(1, top + 1):
        levels = cpu_levels(leaves[:c2])
        for c in range(1, c2 + 1):
            peaks, rights = cc.model_gather(levels, c, stride)
            for other in {c - 1, c + 1, c ^ 2, 2 * c} - {c}:
                if other >= 0:
                    rows.append((other, c2, peaks, rights, roots[c], roots[c2], False))
            for other in {c2 - 1, c2 + 1, c2 + 2, 2 * c2, 64 + c2} - {c2}:
                same = other >= c and cc.walk(c, other) == cc.walk(c, c2)
                rows.append((c, other, peaks, rights, roots[c], roots[c2], same))
    ok = cc.host_verify([r[0] for r in rows], [r[1] for r in rows], np.stack([r[2] for r in rows]), np.stack([r[3] for r in rows]),
                        np.stack([r[4] for r in rows]), np.stack([r[5] for r in rows]))
    assert ok.tolist() == [int(r[6]) for r in rows]
    assert 0 < sum(r[6] for r in rows) < len(rows) // 2                                          # both kinds occur
    for i in range(0, len(rows), 23):                                                            # the model decides
        r = rows[i]
        assert cc.model_check(r[0], r[1], r[2], r[3], r[4], r[5]) == int(r[6]), r[:2]


# ---- the Python layer ------------------------------------------------------------------------------------------------------------------
def test_the_proof_is_host_arrays_and_its_peaks_are_a_frontier(native):
    import vk_merkle_roots_amd as vk
    forest = cc.Forest([9, 130], seed=416)
    trees, old = [1, 0, 1], [64, 5, 130]
    new_counts, peaks, rights = forest.proofs(trees, old, stride=8)
    proof = vk.ConsistencyProof(trees, old, new_counts, peaks, rights)
    assert proof.Q == 3 and proof.stride == 8 and proof.trees.dtype == np.uint32 and proof.old_counts.dtype == np.uint64
    assert proof.same_as(vk.ConsistencyProof(trees, old, new_counts, peaks, rights))
    other = vk.ConsistencyProof(trees, old, new_counts, peaks, rights)
    other.rights[2, 7, 0] ^= 1                               # a zero cell counts too
    assert not proof.same_as(other)
    f = proof.frontier()
    assert isinstance(f, vk.Frontier) and f.counts.tolist() == old and (f.peaks == peaks).all()
    import frontier_cases as fr
    old_roots, _ = forest.query_roots(trees, old)
    assert all((fr.model_root(c, f.peaks[q]) == old_roots[q]).all() for q, c in enumerate(old))  # the root each tree had at its old count
    for bad in (lambda: vk.ConsistencyProof(trees, old[:2], new_counts, peaks, rights), lambda: vk.ConsistencyProof(trees, old, new_counts, peaks, rights[:, :7]),
                lambda: vk.ConsistencyProof(trees, old, new_counts, peaks.reshape(3, -1), rights.reshape(3, -1))):
        with pytest.raises(ValueError):
            bad()
    empty = vk.ConsistencyProof([], [], [], np.zeros((0, 8, 8), np.uint32), np.zeros((0, 8, 8), np.uint32))
    assert empty.verify(NoDevice(), np.zeros((0, 8), np.uint32), np.zeros((0, 8), np.uint32)).shape == (0,)


def test_the_handle_refuses_on_the_host_and_answers_no_query_without_a_device(native):
    import vk_merkle_roots_amd as vk
    forest = vk.MerkleForest(NoDevice(), None, 16, [4, 5, 7], None, 7, None, None)
    with pytest.raises(ValueError):
        forest.consistency([4, 5])                           # one old count per tree
    with pytest.raises(ValueError):
        forest.consistency([4, 5, 7], trees=[0, 1])
    none = forest.consistency([], trees=[])
    assert none.Q == 0 and none.stride == 3 and none.peaks.shape == (0, 3, 8) and none.same_as(forest.consistency([], trees=[], stride=3))


def test_the_wrappers_on_raw_buffers_are_not_named_async(native):
    import vk_merkle_roots_amd as vk
    for name in ("forest_consistency_enqueue", "verify_consistency_enqueue"):
        assert callable(getattr(vk.HipDevice, name))
    assert not any("consistency" in n and n.endswith("_async") for n in dir(vk.HipDevice))
    assert callable(vk.MerkleForest.consistency)


def test_the_kernel_key_resolves_to_itself_and_the_build_lists_it(native):
    from vk_merkle_roots_amd import isa_prio_pass
    keys = isa_prio_pass.EXPECTED_HASH_BLOCKS
    assert keys[FOLD] == 1
    assert_key_resolves(FOLD)
    for name in KERNELS:
        assert name == FOLD or not any(k in name for k in keys), name                            # no hash expected in the others
        assert not any(s in name for s in NAMES_OTHER_TESTS_COUNT), name
    text = open(os.path.join(ROOT, "vk_merkle_roots_amd", "csrc", "consistency_kernels.hpp")).read()
    assert len(re.findall(r"\bhash_pair\(", text)) == 1 and sorted(re.findall(r"void (\w+_kernel)\(", text)) == sorted(KERNELS)
    rec = isa_record(native)
    if rec is not None:                    # written by a build that ran the issue pass (tests/test_isa_prio_pass.py covers its absence)
        assert rec["audit"]["block_count_errors"] == [] and rec["audit"]["unclassified"] == []
        mine = {k: v for k, v in rec["audit"]["blocks"].items() if "consistency" in k}
        assert list(mine.values()) == [1] and FOLD in next(iter(mine))
    assert_no_spills(native, KERNELS)
