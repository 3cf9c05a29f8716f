"""Leaf updates of a stored forest without a GPU: the C ABI's declaration and argument checks, the host-side checks of
MerkleForest.update and update_packed, the ordering rule, and the addressing of csrc/forest_plan.hpp's update step replayed on
the CPU with the run-head rule of forest_update_level_kernel (tests/c/forest_update_plan_test.cpp).  No compute calls here:
every case returns before the library or the Python layer touches HIP."""
import ctypes as C

import numpy as np
import pytest

import forest_cases as fc
import forest_update_cases as fu
from abi_support import Refusals, assert_bound, assert_exported, assert_key_resolves, assert_no_spills, isa_record
from merkle_model import random_counts
from no_device import NoDevice

NAME = "vkmr_hip_forest_update_async"


def test_header_declares_the_update_and_the_stub_binds_every_argument_of_it():
    # dev, stream, digests, forest, total, offsets, ntrees, max_count, trees, indices, leaves, k, roots, status: the prototype the
    # feature was specified with has these fourteen
    assert_bound(NAME, nparams=14, scalars=[C.c_int, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32], restype=C.c_int)


def test_library_exports_the_update(native):
    assert_exported(native.HIP_LIB, [NAME])


def test_bad_arguments_are_refused_before_any_hip_call(native):
    from vk_merkle_roots_amd import _abi
    lib = _abi.lib()
    d = C.c_void_p(0x1000)                 # never dereferenced: every call below returns before launching anything
    # digests, forest, total, offsets, ntrees, max_count, trees, indices, leaves, k, roots, status
    update = Refusals(lib.vkmr_hip_forest_update_async, NAME, good=[d, d, 100, d, 4, 50, d, d, d, 8, d, d])
    update.null(0, 1, 3, 6, 7, 8, 10, 11)  # each pointer NULL with k > 0
    update.changed({4: 0}, {2: 0}, {5: 0}, {2: (1 << 58) + 1})       # ntrees == 0, total == 0, max_count == 0, too many leaves
    # (a grid that is too large cannot be reached: k < 2^32 entries are fewer than 2^31 workgroups of 256 lanes)
    # k == 0 is a no-op whatever the rest
    update.ok((None, None, 100, None, 4, 50, None, None, None, 0, None, None), (None, None, 0, None, 0, 0, None, None, None, 0, None, None),
              (d, d, (1 << 58) + 1, d, 4, 0, d, d, d, 0, d, d))


COUNTS = [4, 0, 0, 7, 0, 0, 0, 1]          # fc.CASES["empty_adjacent"]


def host_forest(counts=COUNTS):
    import vk_merkle_roots_amd as vk
    return vk.MerkleForest(NoDevice(), None, sum(counts), counts, None, max(1, max(counts)), None, None)


@pytest.mark.parametrize("trees,indices", [([8], [0]),                      # a tree equal to ntrees
                                           ([0], [4]), ([3], [7]), ([7], [1]),  # an index equal to counts[t]
                                           ([1], [0]), ([0, 6], [1, 0]),    # an entry into an empty tree
                                           ([-1], [0]), ([0], [-1]), ([3, 0], [2, -3]),
                                           ([2**32], [0]), ([0], [2**63]), ([0], [2**64 + 5]), ([2**70], [0]),
                                           (np.array([9], dtype=np.uint32), np.array([0], dtype=np.uint64)),
                                           (np.array([-2], dtype=np.int32), np.array([0], dtype=np.int64))])
def test_update_refuses_entries_outside_the_forest(native, trees, indices):
    k = len(indices)
    with pytest.raises(IndexError):
        host_forest().update(trees, indices, np.zeros((k, 8), np.uint32))


def test_update_refuses_every_entry_of_a_forest_of_empty_trees(native):
    with pytest.raises(IndexError):
        host_forest([0, 0]).update([0], [0], np.zeros((1, 8), np.uint32))


@pytest.mark.parametrize("k,shape", [(1, (8,)), (2, (1, 8)), (2, (2, 7)), (1, (1, 8, 1)), (0, (1, 8)), (3, (8, 3))])
def test_update_refuses_leaves_that_are_not_k_by_8(native, k, shape):
    with pytest.raises(ValueError):
        host_forest().update([3] * k, list(range(k)), np.zeros(shape, np.uint32))


@pytest.mark.parametrize("trees,indices", [([0, 3], [1]), ([0], [1, 2]), ([], [1]), ([0], [])])
def test_update_refuses_mismatched_lengths(native, trees, indices):
    with pytest.raises(ValueError):
        host_forest().update(trees, indices, np.zeros((len(indices), 8), np.uint32))


@pytest.mark.parametrize("trees,indices", [([0.5], [1]), ([0], [1.5]), (["a"], [0])])
def test_update_refuses_entries_that_are_not_integers(native, trees, indices):
    with pytest.raises(ValueError):
        host_forest().update(trees, indices, np.zeros((1, 8), np.uint32))


def test_update_packed_refuses_before_any_device_call(native):
    import vk_merkle_roots_amd as vk
    batch = vk.pack_lines(b"a\nb\nc\n")
    assert batch.count == 3
    with pytest.raises(ValueError):
        host_forest().update_packed([0, 3], [0, 1], batch)          # three strings for two entries
    with pytest.raises(ValueError):
        host_forest().update_packed([0, 3], [0, 1, 2], batch)       # not one tree per index
    with pytest.raises(IndexError):
        host_forest().update_packed([0, 3, 8], [0, 1, 0], batch)
    with pytest.raises(IndexError):
        host_forest().update_packed([0, 3, 7], [0, 7, 0], batch)
    with pytest.raises(IndexError):
        host_forest().update_packed([0, 1, 7], [0, 0, 0], batch)    # an empty tree
    with pytest.raises(IndexError):
        host_forest().update_packed([0, -3, 7], [0, 0, 0], batch)


def test_last_occurrence_wins_and_order_is_lexicographic(native):
    f = host_forest([10, 0, 5])
    trees, idx, pos = f._update_order([2, 0, 2, 0], [1, 9, 1, 3])
    assert trees.dtype == np.uint32 and idx.dtype == np.uint64
    assert list(zip(trees.tolist(), idx.tolist())) == [(0, 3), (0, 9), (2, 1)]
    assert list(pos) == [3, 1, 2]
    # the index falls while the tree rises: in order as it stands
    trees, idx, pos = f._update_order([0, 2], [3, 0])
    assert list(zip(trees.tolist(), idx.tolist())) == [(0, 3), (2, 0)] and list(pos) == [0, 1]
    trees, idx, pos = f._update_order([], [])
    assert trees.shape == (0,) and idx.shape == (0,) and pos.shape == (0,)


def test_status_text_names_the_bits(native):
    from vk_merkle_roots_amd import engine
    assert engine.forest_update_status_text(0) == "ok"
    assert "bit 0" in engine.forest_update_status_text(1) and "bit 1" not in engine.forest_update_status_text(1)
    assert "bit 0" in engine.forest_update_status_text(3) and "bit 1" in engine.forest_update_status_text(3)
    assert "unknown" in engine.forest_update_status_text(4)


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    return fu.build_update_plan_exe(tmp_path_factory.mktemp("forest_update_plan"))


def check_replay(plan_exe, directory, cases):
    got = fu.plan_replay(plan_exe, directory, cases)
    for (first, slack, max_count, counts, trees, indices), (H, cells, roots, hashes) in zip(cases, got):
        total = first + sum(counts) + slack
        assert H == fu.fp.stride_of(total, max_count or max(1, max(counts)))
        assert (cells, roots, hashes) == fu.rewritten(counts, trees, indices), (first, slack, max_count, counts[:10])


def test_the_update_step_replayed_over_every_case_table(native, plan_exe, tmp_path):
    cases = []
    for name, counts in sorted(fc.CASES.items()):
        rng = np.random.default_rng(len(name))
        largest = max(1, max(counts))
        sets = list(fu.update_sets(counts, rng).values()) if sum(counts) else []
        sets.append(fu.sorted_entries([]))                         # no entry: nothing is written
        for first, slack in ((0, 0), (5, 7)):
            for max_count in (0, 1 << fc.ceil_log2(largest), 2**63):
                for trees, indices in sets:
                    cases.append((first, slack, max_count, counts, trees, indices))
    check_replay(plan_exe, tmp_path, cases)


def test_the_update_step_replayed_over_a_thousand_random_forests(native, plan_exe, tmp_path):
    rng = np.random.default_rng(20260)
    cases = []
    while len(cases) < 1000:
        counts = random_counts(rng, 1 << 13)
        if not counts or max(counts) == 0:
            continue
        full = [t for t, c in enumerate(counts) if c]
        whole = full[int(rng.integers(0, len(full)))]              # every leaf of one tree
        pairs = [(whole, i) for i in range(counts[whole])]
        pairs += [(t, i) for t in full for i in (0, counts[t] - 1)]   # the first and the last leaf of every tree
        more_trees, more_indices = fu.fp.random_queries(rng, counts, int(rng.integers(0, 200)))
        pairs += list(zip(more_trees.tolist(), more_indices.tolist()))
        trees, indices = fu.sorted_entries(pairs)
        first, slack = (int(rng.integers(1, 1000)), int(rng.integers(1, 1000))) if rng.integers(0, 2) else (0, 0)
        max_count = (0, max(counts) + int(rng.integers(0, 5000)), 2**64 - 1)[len(cases) % 3]
        cases.append((first, slack, max_count, counts, trees, indices))
    check_replay(plan_exe, tmp_path, cases)


def test_the_update_level_kernel_holds_one_hash_block_and_the_build_lists_it(native):
    from vk_merkle_roots_amd import isa_prio_pass
    assert isa_prio_pass.EXPECTED_HASH_BLOCKS["forest_update_level_kernel"] == 1
    assert_key_resolves("forest_update_level_kernel")      # the name must not be taken for the single tree's kernel
    rec = isa_record(native)
    if rec is not None:                    # written by a build that ran the issue pass (tests/test_isa_prio_pass.py covers its absence)
        assert rec["audit"]["block_count_errors"] == [] and rec["audit"]["unclassified"] == []
        mine = {k: v for k, v in rec["audit"]["blocks"].items() if "forest_update" in k}
        assert list(mine.values()) == [1] and "forest_update_level_kernel" in next(iter(mine))   # the check and the leaves hold none
    assert_no_spills(native, ["forest_update_level_kernel"], max_vgprs=64, prefix=True)      # 512 registers a lane, 8 wavefronts per SIMD
