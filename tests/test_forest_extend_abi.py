"""The open tree of a stored forest grown or shrunk by leaves, without a GPU: the C ABI's declarations and argument checks
(vkmr_hip_forest_extend_async, vkmr_hip_forest_shrink_async), the host-side checks of MerkleForest.extend, extend_packed and
shrink, and the range rule of csrc/forest_plan.hpp replayed on the CPU with forest_extend_level_kernel's own tests
(tests/c/forest_extend_plan_test.cpp), the lone-node clause pinned by the failure of the rule without it.  No compute calls
here: every case returns before the library or the Python layer touches HIP."""
import ctypes as C

import numpy as np
import pytest

import forest_extend_cases as fe
from abi_support import Refusals, assert_bound, assert_exported, assert_key_resolves, assert_no_spills, isa_record
from merkle_model import random_counts, tree_height
from no_device import NoDevice

EXTEND, SHRINK = "vkmr_hip_forest_extend_async", "vkmr_hip_forest_shrink_async"
LEVEL_KERNEL = "forest_extend_level_kernel"
KERNELS = ("forest_extend_check_kernel", "forest_extend_offsets_kernel", LEVEL_KERNEL, "forest_extend_scan_kernel")


def test_header_declares_both_and_the_stub_binds_every_argument():
    # dev, stream, digests, forest, total, offsets, ntrees, max_count, tree, count, used, leaves, n_leaves, roots, mutated, status:
    # sixteen; the shrink has r for leaves and n_leaves: fifteen
    for name, nparams, scalars in ((EXTEND, 16, [C.c_int, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64]),
                                   (SHRINK, 15, [C.c_int, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64])):
        assert_bound(name, nparams=nparams, scalars=scalars, restype=C.c_int)


def test_library_exports_both(native):
    assert_exported(native.HIP_LIB, [EXTEND, SHRINK])


def test_bad_arguments_are_refused_before_any_hip_call(native):
    from vk_merkle_roots_amd import _abi
    lib = _abi.lib()
    d = C.c_void_p(0x1000)                 # never dereferenced: every call below returns before launching anything
    # digests, forest, total, offsets, ntrees, max_count, tree, count, used, leaves, n_leaves, roots, mutated, status
    extend = Refusals(lib.vkmr_hip_forest_extend_async, EXTEND, good=[d, d, 100, d, 8, 50, 4, 20, 60, d, 30, d, None, d])
    extend.null(0, 1, 3, 9, 11, 13)        # each needed pointer NULL (mutated, 12, is NULL in `good` already)
    # tree >= ntrees (also the last 32-bit number), count + n_leaves > max_count (also past 2^64), used + n_leaves > total (also
    # past 2^64), more leaves in the tree than in use, max_count == 0, total > 2^58
    extend.changed({6: 8}, {6: 9}, {6: 2**32 - 1}, {10: 31}, {7: 21}, {7: 51, 10: 1}, {7: 2**64 - 1, 10: 2}, {10: 41, 5: 100}, {8: 71}, {8: 101, 10: 1},
                   {8: 2**64 - 1, 10: 2}, {7: 20, 8: 19, 10: 1}, {5: 0}, {2: (1 << 58) + 1})
    # n_leaves == 0 is a no-op whatever the rest
    extend.ok((None, None, 100, None, 8, 50, 4, 20, 60, None, 0, None, None, None), (None, None, 0, None, 0, 0, 9, 9, 3, None, 0, None, None, None),
              (d, d, (1 << 58) + 1, d, 4, 0, 9, 0, 0, d, 0, d, d, d))

    # digests, forest, total, offsets, ntrees, max_count, tree, count, used, r, roots, mutated, status
    shrink = Refusals(lib.vkmr_hip_forest_shrink_async, SHRINK, good=[d, d, 100, d, 8, 50, 4, 20, 60, 7, d, None, d])
    shrink.null(0, 1, 3, 10, 12)
    shrink.changed({6: 8}, {6: 2**32 - 1}, {9: 21}, {9: 2**64 - 1}, {7: 0}, {8: 19}, {8: 101}, {5: 0}, {2: (1 << 58) + 1})
    shrink.ok((None, None, 100, None, 8, 50, 4, 20, 60, 0, None, None, None), (d, d, (1 << 58) + 1, d, 0, 0, 9, 0, 0, 0, d, d, d))


def host_forest(counts=(4, 0, 7, 0, 0, 0), total=20, max_count=8, used_trees=3):
    import vk_merkle_roots_amd as vk
    return vk.MerkleForest(NoDevice(), None, total, list(counts), None, max_count, None, None, used_trees=used_trees)


def test_the_handle_names_its_open_tree(native):
    assert host_forest().open_tree == 2
    assert host_forest(counts=(4, 0, 0), used_trees=2).open_tree == 1         # an empty tree in use is the open tree
    assert host_forest(counts=(0, 0, 0), used_trees=0).open_tree is None
    import vk_merkle_roots_amd as vk
    assert vk.MerkleForest(NoDevice(), None, 11, [4, 0, 7], None, 7, None, None).open_tree == 2   # as a build without a reserve makes it


def test_extend_and_shrink_refuse_on_the_host(native):
    import vk_merkle_roots_amd as vk
    status = object()                                                          # no buffer is looked at before the refusal
    two = vk.pack_lines(b"a\nb\n")
    for forest, n in ((host_forest(counts=(0, 0, 0), used_trees=0), 1),        # no tree in use
                      (host_forest(), 2),                                      # 7 + 2 leaves, max_count 8
                      (host_forest(total=12, max_count=100), 2),               # one free cell
                      (host_forest(total=11), 1)):                             # none
        with pytest.raises(ValueError):
            forest.extend(np.zeros((n, 8), np.uint32))
        with pytest.raises(ValueError):
            forest.extend(np.zeros((n, 8), np.uint32), mutated=True)
        with pytest.raises(ValueError):
            forest.extend_async(status, n, status)
        if n == 2:
            with pytest.raises(ValueError):
                forest.extend_packed(two)
    with pytest.raises(ValueError):
        host_forest(counts=(0, 0, 0), used_trees=0).extend_packed(two)
    for forest, r in ((host_forest(counts=(0, 0, 0), used_trees=0), 1), (host_forest(), 8), (host_forest(counts=(4, 0, 0), used_trees=2), 1),
                      (host_forest(), -1)):
        with pytest.raises(ValueError):
            forest.shrink(r)
        with pytest.raises(ValueError):
            forest.shrink_async(r, status)


def test_calls_of_no_leaf_touch_no_device(native):
    import vk_merkle_roots_amd as vk
    f = host_forest()
    assert f.extend(np.zeros((0, 8), np.uint32)) == 7 and f.shrink(0) == 7
    assert f.extend_packed(vk.pack_lines(b"")) == 7
    assert f.counts.tolist() == [4, 0, 7, 0, 0, 0]


def test_the_counters_follow(native):
    f = host_forest()
    f.extended(1)
    assert (f.counts.tolist(), f.used_leaves, f.free_leaves, f.used_trees, f.open_tree) == ([4, 0, 8, 0, 0, 0], 12, 8, 3, 2)
    f.shrunk(8)
    assert (f.counts.tolist(), f.used_leaves, f.free_leaves, f.used_trees, f.open_tree) == ([4, 0, 0, 0, 0, 0], 4, 16, 3, 2)


def test_the_wrappers_on_raw_buffers_are_not_named_async(native):
    import vk_merkle_roots_amd as vk
    assert callable(vk.HipDevice.forest_extend_enqueue) and callable(vk.HipDevice.forest_shrink_enqueue)
    assert not any(n.startswith(("forest_extend", "forest_shrink")) and n.endswith("_async") for n in dir(vk.HipDevice))


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    return fe.build_extend_plan_exe(tmp_path_factory.mktemp("forest_extend_plan"))


def check_replay(plan_exe, directory, cases):
    got = fe.plan_replay(plan_exe, directory, cases)
    for (first, slack, max_count, behind, c, c2, front), (H, cells, roots, lanes) in zip(cases, got):
        total = first + sum(front) + max(c, c2) + slack
        assert H == fe.fu.fp.stride_of(total, max_count or max([1, c, c2] + list(front)))
        ranges = [fe.dirty(c, c2, l) for l in range(1, H + 1)]
        h2 = tree_height(c2) if c2 else 1
        assert roots == 1 and cells == sum(e - f for l, (f, e) in enumerate(ranges, 1) if l != h2), (c, c2)
        # the range restriction: a launch covers the nodes that change and under a wavefront more, never the tree
        assert lanes <= sum((abs(c2 - c) >> l) + 2 + 63 for l in range(1, H + 1)), (c, c2)


def test_every_pair_of_counts_up_to_130_replayed(native, plan_exe, tmp_path):
    cases = []
    for c in range(131):
        for c2 in range(131):
            if c2 == c:
                continue
            for first, front in ((0, []), (5, []), (0, [0, 0, 0]), (0, [1, 1, 3])):   # o in {0, 5} at t in {0, 3}
                for behind in (0, 2):
                    cases.append((first, (c + c2) % 4, (0, 2**63)[(c + c2) % 2], behind, c, c2, front))
    check_replay(plan_exe, tmp_path, cases)


def test_a_thousand_random_forests_replayed(native, plan_exe, tmp_path):
    rng = np.random.default_rng(20262)
    cases = []
    while len(cases) < 1000:
        front = random_counts(rng, 1 << 13)
        c, c2 = (int(x) for x in rng.integers(0, (5000, 300, 20)[len(cases) % 3], size=2))
        if c == c2:
            continue
        first, slack = (int(rng.integers(1, 1000)), int(rng.integers(1, 1000))) if rng.integers(0, 2) else (0, 0)
        max_count = (0, max([c, c2] + front) + int(rng.integers(0, 5000)), 2**64 - 1)[len(cases) % 3]
        cases.append((first, slack, max_count, int(rng.integers(0, 4)), c, c2, front))
    check_replay(plan_exe, tmp_path, cases)


@pytest.mark.parametrize("c,c2,why", [(2, 3, "a read of a cell that nobody has stored"),     # node 0 of level 1 was the root: never stored
                                      (3, 2, "a root is not the fresh build's"),             # node 0 of level 1 is clean: never carried to the root
                                      (4, 5, "a read of a cell that nobody has stored"), (8, 4, "a root is not the fresh build's")])
def test_the_rule_without_the_lone_node_clause_fails_the_replay(native, plan_exe, tmp_path, c, c2, why):
    case = [(5, 3, 0, 2, c, c2, fe.FRONT)]
    rc, text = fe.run_replay(plan_exe, tmp_path, case, plain=True)
    assert rc != 0 and "FAIL: " + why in text, text
    fe.plan_replay(plan_exe, tmp_path, case)                     # and the rule of forest_plan.hpp passes the same case


def test_the_plain_rule_is_the_rule_wherever_no_level_has_a_lone_node(native, plan_exe, tmp_path):
    cases = [(5, 3, 0, 2, c, c2, fe.FRONT) for c, c2 in ((5, 7), (7, 5), (63, 130), (130, 63), (127, 129), (129, 127), (1025, 1030))]
    rc, text = fe.run_replay(plan_exe, tmp_path, cases, plain=True)
    assert rc == 0 and f"ok: {len(cases)} forests" in text, text[-2000:]


def test_the_kernel_keys_resolve_to_themselves_and_the_build_lists_them(native):
    from vk_merkle_roots_amd import isa_prio_pass
    keys = isa_prio_pass.EXPECTED_HASH_BLOCKS
    assert keys[LEVEL_KERNEL] == 1
    assert_key_resolves(LEVEL_KERNEL)
    for name in KERNELS:                   # existing tests pick their kernels out of the build's record by these substrings
        assert not any(s in name for s in ("forest_append", "forest_truncate", "mutated"))
        assert name == LEVEL_KERNEL or not any(k in name for k in keys), name      # no hash expected in the others
    rec = isa_record(native)
    if rec is not None:                    # written by a build that ran the issue pass (tests/test_isa_prio_pass.py covers its absence)
        assert rec["audit"]["block_count_errors"] == [] and rec["audit"]["unclassified"] == []
        mine = {k: v for k, v in rec["audit"]["blocks"].items() if "forest_extend" in k}
        assert list(mine.values()) == [1] and LEVEL_KERNEL in next(iter(mine))     # the check, the offsets, the scan: none
    assert_no_spills(native, KERNELS, max_vgprs=64)        # 512 registers a lane, 8 wavefronts per SIMD
