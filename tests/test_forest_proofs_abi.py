"""Stored forests and proofs inside a forest without a GPU: the C ABI's declarations and argument checks, the stored layout of
csrc/forest_plan.hpp replayed on the CPU (tests/c/forest_store_plan_test.cpp), and the host counterpart
vkmr_host_cpu_forest_proofs against a hashlib restatement (tests/forest_proof_cases.py), the oracle's roots and what the
reference's own CPU path returned."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import forest_cases as fc
import forest_proof_cases as fp
from abi_support import Refusals, assert_bound, assert_exported, isa_record

ENTRY_POINTS = ("vkmr_hip_forest_tree_bytes", "vkmr_hip_reduce_forest_tree_async", "vkmr_hip_forest_proofs_async",
                "vkmr_hip_verify_forest_proofs_async")


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    return fp.build_store_plan_exe(tmp_path_factory.mktemp("forest_store_plan"))


def test_header_declares_and_library_exports_the_stored_forest_entry_points(native):
    from vk_merkle_roots_amd import _abi
    assert_exported(native.HIP_LIB, ENTRY_POINTS)
    for name, nparams in zip(ENTRY_POINTS, [3, 10, 13, 12]):
        assert_bound(name, nparams=nparams)
    assert_exported(native.HOST_LIB, ["vkmr_host_cpu_forest_proofs"])
    assert "vkmr_host_cpu_forest_proofs" in _abi.HOST_SIGNATURES


def test_bad_arguments_are_refused_before_any_hip_call(native):
    from vk_merkle_roots_amd import _abi
    lib = _abi.lib()
    d = C.c_void_p(0x1000)                 # never dereferenced: every call below returns before launching anything
    # build: digests, total, offsets, ntrees, max_count, forest, roots, status
    build = Refusals(lib.vkmr_hip_reduce_forest_tree_async, "vkmr_hip_reduce_forest_tree_async", good=[d, 100, d, 4, 50, d, d, d])
    build.null(0, 2, 5, 6, 7)              # each pointer NULL with ntrees > 0
    # max_count == 0; forest not 16-byte aligned; more leaves than the plan's shifts allow
    build.changed({4: 0}, {5: C.c_void_p(0x1008)}, {1: (1 << 58) + 1})
    build.ok((None, 0, None, 0, 0, None, None, None), (None, 100, None, 0, 7, None, None, None))      # ntrees == 0: nothing to do
    # the roots-only call still names itself in its refusals
    Refusals(lib.vkmr_hip_reduce_forest_async, "vkmr_hip_reduce_forest_async", good=[d, 100, d, 4, 50, d, d, d]).changed({4: 0})

    # gather: digests, forest, total, offsets, ntrees, max_count, trees, indices, k, siblings, heights
    gather = Refusals(lib.vkmr_hip_forest_proofs_async, "vkmr_hip_forest_proofs_async", good=[d, d, 100, d, 4, 50, d, d, 8, d, d])
    gather.null(0, 1, 3, 6, 7, 9, 10)
    gather.changed({5: 0}, {2: (1 << 58) + 1})             # max_count == 0; too many leaves
    # (k * H cells past the launch limit cannot be reached: k < 2^32 and H <= 58 stay below 2^31 workgroups of 256 lanes)
    gather.ok((None, None, 100, None, 4, 50, None, None, 0, None, None))       # k == 0

    # verify: leaves, trees, indices, siblings, heights, k, stride, roots, ntrees, ok
    verify = Refusals(lib.vkmr_hip_verify_forest_proofs_async, "vkmr_hip_verify_forest_proofs_async", good=[d, d, d, d, d, 8, 12, d, 4, d])
    verify.null(0, 1, 2, 3, 4, 7, 9)
    verify.changed({6: 0}, {6: 64}, {6: 100})              # the stride
    verify.ok((None, None, None, None, None, 0, 12, None, 4, None))            # k == 0


def test_forest_tree_bytes_is_its_closed_form(native):
    import vk_merkle_roots_amd as vk
    f = vk.lib().vkmr_hip_forest_tree_bytes
    totals = [0, 1, 2, 3, 4, 5, 127, 128, 129, 1000, (1 << 20) - 1, 1 << 20, (1 << 26) + 3, 1 << 33]
    trees = [1, 2, 3, 64, 1000, 32768, (1 << 32) - 1]
    bounds = [1, 2, 3, 4, 5, 2047, 2048, 2049, 1 << 26, 2**63, 2**64 - 1]
    for total in totals:
        for n in trees:
            assert f(total, n, 0) == 0
            for m in bounds:
                H = max(1, int(min(m, total) - 1).bit_length()) if min(m, total) > 1 else 1
                assert f(total, n, m) == 32 * sum((total >> l) + n for l in range(1, H + 1)), (total, n, m)
                assert f(total, n, m) == 32 * fp.stored_cells(total, n, m)
        for m in bounds:
            assert f(total, 0, m) == 0
    # one level: the roots-only scratch's first buffer; 2^26 leaves in 2^15 trees of 2^11: eleven levels
    assert f(100, 7, 2) == 32 * (50 + 7)
    assert f(1 << 26, 1 << 15, 1 << 11) == 32 * (((1 << 26) - (1 << 15)) + 11 * (1 << 15))


def test_stored_positions_stay_inside_their_level_and_below_the_size_the_abi_reports(native, plan_exe, tmp_path):
    import vk_merkle_roots_amd as vk
    f = vk.lib().vkmr_hip_forest_tree_bytes
    forests = []
    for counts in fc.CASES.values():
        total, largest = sum(counts), max(1, max(counts))
        for first, slack, max_count in ((0, 0, 0), (0, 0, 1 << fc.ceil_log2(largest)), (0, 0, max(total, 1)), (0, 0, 2**63), (37, 11, 0),
                                        (1, 0, largest + 1), (4095, 4097, 2**64 - 1)):
            forests.append((first, slack, max_count, counts))
    got = fp.store_plan_replay(plan_exe, tmp_path, forests)
    for (first, slack, max_count, counts), (levels, summed, high) in zip(forests, got):
        total = first + sum(counts) + slack
        m = max_count or max(1, max(counts))
        assert levels == fp.stride_of(total, m)
        assert high <= summed
        assert f(total, len(counts), m) == 32 * summed      # the sum the C test made on its own
        assert summed == fp.stored_cells(total, len(counts), m)


def test_stored_positions_of_a_thousand_random_forests(plan_exe):
    r = subprocess.run([plan_exe, "--random", "1000"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0 and b"ok: 1000 random forests" in r.stdout, r.stdout.decode()[-2000:]


@pytest.mark.parametrize("name", sorted(fc.CASES))
def test_host_cpu_forest_proofs_equal_the_restatement_and_fold_to_the_oracle_roots(native, oracle, name):
    counts = fc.CASES[name]
    leaves = fc.random_leaves(sum(counts), seed=len(name) * 7919 + sum(counts))
    off = fc.offsets_of(counts)
    trees, indices = fp.all_queries(counts)
    stride = fp.stride_of(sum(counts), max(1, max(counts)))
    if name == "one_big_among_small":
        big = counts.index(100003)
        mine = indices[trees == big]
        assert mine.min() == 0 and mine.max() == 100002
    rc, sib, heights = fp.host_cpu_proofs(leaves, off, trees, indices, stride)
    if trees.shape[0] == 0:                # all_empty: no leaf to ask for
        assert rc == 0
        return
    assert rc == 0
    want_sib, want_heights, _ = fp.gather(leaves, off, trees, indices, stride)
    assert (heights == want_heights).all()
    assert (sib == want_sib).all(), np.nonzero((sib != want_sib).any(axis=(1, 2)))[0][:10]
    want_roots = fc.oracle_roots(oracle, leaves, counts)
    for q in range(trees.shape[0]):
        t, i = int(trees[q]), int(indices[q])
        assert heights[q] == fp.tree_height(counts[t])
        assert (fp.host_fold(leaves[int(off[t]) + i], i, sib[q], heights[q]) == want_roots[t]).all(), (t, i)
        assert not sib[q, int(heights[q]):].any()


def test_ten_reference_trees_as_one_forest_every_proof_folds_to_the_recorded_root(native, oracle, ref_checks):
    leaves, counts = fc.ref_check_forest(oracle)
    assert counts == [1, 2, 3, 5, 8, 13, 64, 77, 256, 301]
    off = fc.offsets_of(counts)
    trees, indices = fp.all_queries(counts)
    stride = fp.stride_of(sum(counts), max(counts))
    rc, sib, heights = fp.host_cpu_proofs(leaves, off, trees, indices, stride)
    assert rc == 0
    want = [t["root"] for t in ref_checks["trees"]]
    for q in range(trees.shape[0]):
        t, i = int(trees[q]), int(indices[q])
        assert oracle.hex(fp.host_fold(leaves[int(off[t]) + i], i, sib[q], heights[q])) == want[t], (t, i)


def test_invalid_queries_empty_trees_and_a_short_stride(native):
    counts = [4, 0, 0, 7, 0, 1, 130]
    leaves = fc.random_leaves(sum(counts), seed=17)
    off = fc.offsets_of(counts)
    # named, tree >= ntrees, index == c_t, empty, empty, named, index far above c_t, the last leaf of the tallest, a lone leaf, tree 2^32 - 1
    trees = [0, 7, 0, 1, 4, 3, 3, 6, 5, 2**32 - 1]
    indices = [3, 0, 4, 0, 0, 6, 2**63, 129, 0, 0]
    rc, sib, heights = fp.host_cpu_proofs(leaves, off, trees, indices, 8)
    assert rc == 0
    assert list(heights) == [2, 0, 0, 0, 0, 3, 0, 8, 1, 0]
    want_sib, want_heights, _ = fp.gather(leaves, off, trees, indices, 8)
    assert (sib == want_sib).all() and (heights == want_heights).all()
    for q in (1, 2, 3, 4, 6, 9):
        assert not sib[q].any()
    assert (sib[8, 0] == leaves[int(off[5])]).all()       # the lone leaf is its own sibling
    # a stride below the tallest proof asked for is refused and nothing is written; the same stride serves the shorter proofs
    pattern = np.uint32(0xA5A5A5A5)
    rc, sib, heights = fp.host_cpu_proofs(leaves, off, trees, indices, 7)
    assert rc != 0 and (sib == pattern).all() and (heights == pattern).all()
    rc, sib, heights = fp.host_cpu_proofs(leaves, off, trees[:7], indices[:7], 3)
    assert rc == 0 and list(heights) == [2, 0, 0, 0, 0, 3, 0]
    # decreasing offsets are refused whatever is asked, and nothing is written
    for bad in ([0, 5, 4, 20], [3, 2], [0, 10, 20, 19]):
        rc, sib, heights = fp.host_cpu_proofs(leaves, np.array(bad, dtype=np.uint64), [0], [0], 8)
        assert rc != 0 and (sib == pattern).all() and (heights == pattern).all(), bad
    # a first offset above 0
    shifted = off + np.uint64(3)
    rc, sib, heights = fp.host_cpu_proofs(fc.random_leaves(sum(counts) + 3, seed=18), shifted, [0, 3], [1, 5], 3)
    assert rc == 0 and list(heights) == [2, 3]


def test_the_restatement_accepts_its_own_proofs_and_rejects_a_changed_one():
    """The acceptance rule the GPU verifier is held to, on the CPU alone: so that a wrong restatement cannot hide a wrong kernel."""
    counts = [5, 1, 9]
    leaves = fc.random_leaves(sum(counts), seed=23)
    off = fc.offsets_of(counts)
    trees, indices = fp.all_queries(counts)
    sib, heights, roots = fp.gather(leaves, off, trees, indices, 5)
    roots = np.stack([roots[t] for t in range(3)])
    for q in range(trees.shape[0]):
        leaf = leaves[int(off[trees[q]]) + int(indices[q])]
        assert fp.accepts(leaf, trees[q], indices[q], sib[q], heights[q], 5, roots)
        assert not fp.accepts(leaf ^ np.uint32(1), trees[q], indices[q], sib[q], heights[q], 5, roots)
        assert not fp.accepts(leaf, trees[q], indices[q], sib[q], 0, 5, roots)
        assert not fp.accepts(leaf, trees[q], indices[q], sib[q], 6, 5, roots)
        assert not fp.accepts(leaf, 3, indices[q], sib[q], heights[q], 5, roots)
        assert not fp.accepts(leaf, trees[q], int(indices[q]) | (1 << int(heights[q])), sib[q], heights[q], 5, roots)


def test_python_layer_refuses_bad_counts_before_any_device_call(native):
    import vk_merkle_roots_amd as vk
    assert vk.MerkleForest(None, None, 1 << 26, [1 << 11] * (1 << 15), None, 1 << 11, None, None).levels == 11
    assert vk.MerkleForest(None, None, 100, [40, 60], None, 2**63, None, None).levels == 7
    assert vk.MerkleForest(None, None, 0, [0, 0], None, 1, None, None).levels == 1
    f = vk.MerkleForest(None, None, 9, [4, 0, 5], None, 5, None, None)
    assert f.ntrees == 3 and list(f.counts) == [4, 0, 5]
    batch = vk.pack_lines(b"a\nb\nc\n")
    with pytest.raises(ValueError):
        vk.merkle_forest_packed(None, batch, [1, 1])
    with pytest.raises(ValueError):
        vk.merkle_forest_packed(None, batch, [1, -1, 3])


def test_the_forest_verifier_holds_one_hash_block_and_the_build_lists_it(native):
    from vk_merkle_roots_amd import isa_prio_pass
    assert isa_prio_pass.EXPECTED_HASH_BLOCKS["verify_forest_proofs_kernel"] == 1
    rec = isa_record(native)
    if rec is not None:                    # written by a build that ran the issue pass (tests/test_isa_prio_pass.py covers its absence)
        assert rec["audit"]["block_count_errors"] == [] and rec["audit"]["unclassified"] == []
        mine = {k: v for k, v in rec["audit"]["blocks"].items() if "forest_proofs_kernel" in k}
        assert list(mine.values()) == [1] and "verify_forest_proofs_kernel" in next(iter(mine))      # the gather holds none
