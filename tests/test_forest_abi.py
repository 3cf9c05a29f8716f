"""The forest reduction without a GPU: the C ABI's declaration and argument checks, the layout and scratch budget of
csrc/forest_plan.hpp replayed on the CPU (tests/c/forest_plan_test.cpp), and the host counterpart
vkmr_host_cpu_forest_roots against the oracle and against what the reference's own CPU path returned."""
import ctypes as C

import numpy as np
import pytest

import forest_cases as fc
from abi_support import Refusals, assert_bound, assert_exported


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    return fc.build_plan_exe(tmp_path_factory.mktemp("forest_plan"))


def test_library_exports_the_forest_symbols_and_the_stub_binds_them(native):
    assert_exported(native.HIP_LIB, ("vkmr_hip_forest_scratch_bytes", "vkmr_hip_reduce_forest_async"))
    assert_bound("vkmr_hip_forest_scratch_bytes")
    assert_bound("vkmr_hip_reduce_forest_async", nparams=10)
    assert_exported(native.HOST_LIB, ["vkmr_host_cpu_forest_roots"])


def test_bad_arguments_are_refused_before_any_hip_call(native):
    from vk_merkle_roots_amd import _abi
    lib = _abi.lib()
    d = C.c_void_p(0x1000)                 # never dereferenced: every call below returns before launching anything
    # digests, total, offsets, ntrees, max_count, scratch, roots, status
    reduce = Refusals(lib.vkmr_hip_reduce_forest_async, "vkmr_hip_reduce_forest_async", good=[d, 100, d, 4, 50, d, d, d])
    reduce.null(0, 2, 5, 6, 7)             # each pointer NULL with ntrees > 0
    reduce.changed({4: 0}, {5: C.c_void_p(0x1008)})        # max_count == 0; scratch not 16-byte aligned
    # ntrees == 0 does nothing whatever the rest
    reduce.ok((None, 0, None, 0, 0, None, None, None), (None, 100, None, 0, 7, None, None, None))


def test_scratch_bytes_is_zero_for_no_tree_and_monotone(native):
    import vk_merkle_roots_amd as vk
    f = vk.lib().vkmr_hip_forest_scratch_bytes
    totals = [0, 1, 2, 3, 4, 5, 127, 128, 129, 1000, (1 << 20) - 1, 1 << 20, (1 << 26) + 3, 1 << 33]
    trees = [1, 2, 3, 64, 1000, 32768, (1 << 32) - 1]
    for total in totals:
        assert f(total, 0) == 0
    for i, total in enumerate(totals):
        for j, n in enumerate(trees):
            b = f(total, n)
            assert b % 32 == 0 and b >= 64
            assert b == 32 * ((total >> 1) + (total >> 2) + 2 * n)      # the expression the header states
            if i:
                assert b >= f(totals[i - 1], n)
            if j:
                assert b >= f(total, trees[j - 1])


def test_positions_never_overlap_and_stay_inside_the_budget(native, plan_exe, tmp_path):
    import vk_merkle_roots_amd as vk
    f = vk.lib().vkmr_hip_forest_scratch_bytes
    forests, want_levels = [], []
    for counts in fc.CASES.values():
        total, largest = sum(counts), max(1, max(counts))
        for first, slack, max_count in ((0, 0, 0), (0, 0, 1 << fc.ceil_log2(largest)), (0, 0, max(total, 1)), (0, 0, 2**63), (37, 11, 0)):
            forests.append((first, slack, max_count, counts))
            m = min(max_count or largest, first + total + slack)
            want_levels.append(max(1, fc.ceil_log2(m)))
    got = fc.plan_replay(plan_exe, tmp_path, forests)
    for (first, slack, _, counts), (launches, written, budget), want in zip(forests, got, want_levels):
        assert launches == want
        assert written <= budget
        # the ABI's size function covers what the plan header says the launches write
        assert f(first + sum(counts) + slack, len(counts)) >= 32 * written
        assert f(first + sum(counts) + slack, len(counts)) == 32 * budget


def test_positions_of_a_thousand_random_forests(plan_exe):
    import subprocess
    r = subprocess.run([plan_exe, "--random", "1000"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0 and b"ok: 1000 random forests" in r.stdout, r.stdout.decode()[-2000:]


@pytest.mark.parametrize("name", sorted(fc.CASES))
def test_host_cpu_forest_roots_equal_the_oracle(native, oracle, name):
    counts = fc.CASES[name]
    leaves = fc.random_leaves(sum(counts), seed=len(name) * 7919 + sum(counts))
    rc, roots = fc.host_cpu_roots(leaves, fc.offsets_of(counts))
    assert rc == 0
    want = fc.oracle_roots(oracle, leaves, counts)
    assert (roots == want).all(), np.nonzero((roots != want).any(axis=1))[0][:10]
    for t, c in enumerate(counts):
        if c == 0:
            assert not roots[t].any()


def test_host_cpu_forest_roots_refuse_decreasing_offsets(native):
    leaves = fc.random_leaves(20, seed=3)
    pattern = np.full(8, 0xA5A5A5A5, dtype=np.uint32)
    for off in ([0, 5, 4, 20], [3, 2], [0, 10, 20, 19]):
        rc, roots = fc.host_cpu_roots(leaves, np.array(off, dtype=np.uint64))
        assert rc != 0, off
        assert (roots == pattern).all()
    rc, _ = fc.host_cpu_roots(leaves, np.array([2, 2, 9, 9, 20], dtype=np.uint64))      # a first offset above 0, empty trees
    assert rc == 0


def test_ten_reference_trees_as_one_forest(native, oracle, ref_checks):
    """The ten string lists the reference's own CPU path hashed (tests/golden/ref_checks.json), reduced as ONE forest."""
    leaves, counts = fc.ref_check_forest(oracle)
    assert counts == [1, 2, 3, 5, 8, 13, 64, 77, 256, 301]
    rc, roots = fc.host_cpu_roots(leaves, fc.offsets_of(counts))
    assert rc == 0
    assert [oracle.hex(r) for r in roots] == [t["root"] for t in ref_checks["trees"]]


def test_python_layer_refuses_counts_that_do_not_fit_before_any_device_call(native):
    import vk_merkle_roots_amd as vk
    from vk_merkle_roots_amd.engine import forest_offsets, forest_status_text
    off, n = forest_offsets([3, 0, 5])
    assert n == 3 and off.dtype == np.uint64 and list(off) == [0, 3, 3, 8]
    with pytest.raises(ValueError):
        forest_offsets([1, -2])
    with pytest.raises(ValueError):
        forest_offsets([1.5])
    assert "bit 0" in forest_status_text(1) and "bit 1" in forest_status_text(2) and "bit 0" in forest_status_text(3)
    batch = vk.pack_lines(b"a\nb\nc\n")
    with pytest.raises(ValueError):
        vk.merkle_roots_packed_forest(None, batch, [1, 1])
