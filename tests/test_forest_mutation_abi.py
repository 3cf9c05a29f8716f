"""The mutation flag of a forest without a GPU: the C ABI's declarations and argument checks, the host counterpart
vkmr_host_cpu_forest_mutated against the rule restated in tests/forest_mutation_cases.py, and the build's record of the new
kernels."""
import ctypes as C

import numpy as np
import pytest

import forest_cases as fc
import forest_mutation_cases as fm
from abi_support import Refusals, assert_bound, assert_exported, assert_key_resolves, isa_record

NEW = {"vkmr_hip_reduce_forest_mutated_async": 11, "vkmr_hip_reduce_forest_tree_mutated_async": 11, "vkmr_hip_forest_tree_mutated_async": 9}


def test_library_exports_the_symbols_and_the_stub_binds_them(native):
    from vk_merkle_roots_amd import _abi
    assert_exported(native.HIP_LIB, NEW)
    for name, nargs in NEW.items():
        assert_bound(name, nparams=nargs)
    # the calls beside them keep their arguments
    assert_bound("vkmr_hip_reduce_forest_async", nparams=10)
    assert_bound("vkmr_hip_reduce_forest_tree_async", nparams=10)
    assert_exported(native.HOST_LIB, ["vkmr_host_cpu_forest_mutated"])
    assert_bound("vkmr_host_cpu_forest_mutated", nparams=5, table=_abi.HOST_SIGNATURES, header="vkmr_host.h")


@pytest.mark.parametrize("name", ["vkmr_hip_reduce_forest_mutated_async", "vkmr_hip_reduce_forest_tree_mutated_async"])
def test_the_builds_refuse_bad_arguments_before_any_hip_call(native, name):
    from vk_merkle_roots_amd import _abi
    d = C.c_void_p(0x1000)                    # never dereferenced: every call below returns before launching anything
    # digests, total, offsets, ntrees, max_count, scratch / forest, roots, mutated, status
    build = Refusals(getattr(_abi.lib(), name), name, good=[d, 100, d, 4, 50, d, d, d, d])
    build.null(0, 2, 5, 6, 7, 8)              # each pointer NULL with ntrees > 0; 7 is the new one
    build.changed({4: 0}, {5: C.c_void_p(0x1008)})         # max_count == 0; the level buffer not 16-byte aligned
    # ntrees == 0 does nothing whatever the rest
    build.ok((None, 0, None, 0, 0, None, None, None, None), (None, 100, None, 0, 7, None, None, None, None))


def test_the_scan_refuses_bad_arguments_before_any_hip_call(native):
    from vk_merkle_roots_amd import _abi
    d = C.c_void_p(0x1000)
    # digests, forest, total, offsets, ntrees, max_count, mutated
    scan = Refusals(_abi.lib().vkmr_hip_forest_tree_mutated_async, "vkmr_hip_forest_tree_mutated_async", good=[d, d, 100, d, 4, 50, d])
    scan.null(0, 1, 3, 6)
    scan.changed({5: 0}, {2: (1 << 58) + 1})  # max_count == 0; more leaves than a forest takes
    scan.ok((None, None, 0, None, 0, 0, None), (None, None, 100, None, 0, 7, None))


@pytest.mark.parametrize("name", sorted(fm.CASES))
def test_host_cpu_forest_mutated_equals_the_model(native, name):
    counts = fm.CASES[name]
    off = fm.offsets_of(counts)
    for run in fm.RUNS:
        leaves = fm.leaves_of(name, run)
        want_roots, want = fm.expected(name, run)
        rc, roots, masks = fm.host_cpu_mutated(leaves, off)
        assert rc == 0
        assert (masks == want).all(), (run, np.nonzero(masks != want)[0][:10])
        assert (roots == want_roots).all(), run
        rc2, plain = fc.host_cpu_roots(leaves, off)
        assert rc2 == 0 and (roots == plain).all(), run
        rc3, none, masks3 = fm.host_cpu_mutated(leaves, off, want_roots=False)       # the roots are optional
        assert rc3 == 0 and none is None and (masks3 == want).all(), run
        if run == "random":
            assert not want.any()             # every ragged edge of the table: the duplicate is no pair
        elif run == "equal":
            for t, c in enumerate(counts):    # every level with a genuine pair: all but those with a single node
                assert int(want[t]) == (0 if c < 2 else (1 << fc.ceil_log2(c)) - 1), (t, c)
        else:
            for t, l, _ in fm.planted(counts, fm.seed_of(name), int(run[5:]))[1]:
                assert int(want[t]) == 1 << l, (run, t, l)      # the plant's level and no other


def test_the_nine_plants_of_a_tree_fit_and_cover_its_levels_and_pairs():
    """A self-check of the fixtures (no product code): what plant_choice returns lies inside the tree, the nine combinations
    reach the lowest, the middle and the highest level, and they differ wherever a level has three pairs to choose from (the
    highest level has one pair that fits: its three combinations are one plant, so a tall tree sees seven plants)."""
    for c in (2, 3, 5, 77, 4096, 5000, 100003):
        plants = [fm.plant_choice(c, combo // 3, combo % 3) for combo in range(9)]
        for l, j in plants:
            assert 0 <= j and (2 * j + 2) << l <= c, (c, l, j)
        top = c.bit_length() - 2
        assert {l for l, _ in plants} == {0, top // 2, top}
        if c >= 77:                           # the top level of such a tree holds one pair that fits, every lower one here three or more
            assert len(set(plants)) == 7 and len({p for p in plants if p[0] != top}) == 6, (c, plants)
    assert fm.plant_choice(100003, 1, 1) == (15, 0)       # the highest level at which a whole second block fits
    assert fm.plant_choice(5000, 0, 1) == (0, 2499)       # the last pair of an even level
    assert fm.plant_choice(77, 0, 1) == (0, 37)           # the last genuine pair in front of the ragged edge (leaf 76 has no sibling)
    assert fm.plant_choice(77, 0, 2) == (0, 19) and fm.plant_choice(77, 2, 2) == (2, 4)


def test_the_two_pairs_of_cve_2012_2459(native):
    a, b, c, d, e, f = fc.random_leaves(6, seed=2459)
    for honest, padded, bit in (([a, b, c], [a, b, c, c], 0), ([a, b, c, d, e, f], [a, b, c, d, e, f, e, f], 1)):
        rc, r1, m1 = fm.host_cpu_mutated(np.array(honest), np.array([0, len(honest)], dtype=np.uint64))
        rc2, r2, m2 = fm.host_cpu_mutated(np.array(padded), np.array([0, len(padded)], dtype=np.uint64))
        assert rc == 0 and rc2 == 0
        assert (r1 == r2).all()               # the defect: two leaf lists, one root
        assert int(m1[0]) == 0 and int(m2[0]) == 1 << bit
        assert fm.model(np.array(honest), [len(honest)])[1][0] == 0
        assert fm.model(np.array(padded), [len(padded)])[1][0] == 1 << bit


def test_equal_leaves_in_different_trees_are_no_pair(native):
    counts = [4, 3, 5, 1, 2]
    off = fm.offsets_of(counts)
    leaves = fc.random_leaves(sum(counts), seed=77)
    for t in range(len(counts) - 1):          # the last leaf of tree t equal to the first leaf of tree t + 1
        leaves[int(off[t + 1])] = leaves[int(off[t + 1]) - 1]
    leaves[int(off[2]) + 3] = leaves[int(off[2]) - 1]       # an odd tree's last leaf (tree 1: no sibling) again inside tree 2, an odd cell
    leaves[int(off[4]) + 1] = leaves[int(off[2]) - 1]       # and as tree 4's right leaf (its left one is tree 2's last leaf)
    rc, _, masks = fm.host_cpu_mutated(leaves, off)
    assert rc == 0 and not masks.any(), masks
    assert not fm.model(leaves, counts)[1].any()


def test_host_cpu_forest_mutated_refuses_decreasing_offsets_and_missing_pointers(native):
    leaves = fc.random_leaves(20, seed=3)
    for off in ([0, 5, 4, 20], [3, 2], [0, 10, 20, 19]):
        rc, roots, masks = fm.host_cpu_mutated(leaves, np.array(off, dtype=np.uint64))
        assert rc != 0, off
        assert (roots == 0xA5A5A5A5).all() and (masks == 0xA5A5A5A5A5A5A5A5).all()      # nothing written
    rc, roots, masks = fm.host_cpu_mutated(leaves, np.array([2, 2, 9, 9, 20], dtype=np.uint64))      # a first offset above 0, empty trees
    assert rc == 0 and list(masks) == [0, 0, 0, 0] and not roots[0].any() and not roots[2].any()
    import vk_merkle_roots_amd as vk
    f = vk.host_lib().vkmr_host_cpu_forest_mutated
    off = np.array([0, 20], dtype=np.uint64)
    assert f(leaves.ctypes.data, off.ctypes.data, 1, None, None) != 0                     # no masks
    assert f(None, off.ctypes.data, 1, None, np.zeros(1, dtype=np.uint64).ctypes.data) != 0      # leaves missing
    assert f(None, None, 0, None, None) == 0                                              # no tree: nothing to do


def test_the_new_kernel_holds_one_hash_block_and_shadows_no_key(native):
    from vk_merkle_roots_amd import isa_prio_pass
    keys = isa_prio_pass.EXPECTED_HASH_BLOCKS
    mine = "forest_level_mutated_kernel"
    assert keys[mine] == 1
    assert_key_resolves(mine)
    # the pass matches by substring, first match wins: every other kernel resolves to the key it resolved to without the new one
    before = [k for k in keys if k != mine]
    for k in before:
        for name in (f"_Z{len(k)}{k}PK4Node", f"_Z10{k}ILi64ELi5ELb1EEvPK"):
            assert next(x for x in keys if x in name) == next(x for x in before if x in name), name
    rec = isa_record(native)
    if rec is None:                        # a build without the llvm tools ran no issue pass and wrote no counts: the nm check stands alone
        import subprocess
        syms = subprocess.run(["nm", "-C", native.HIP_LIB], stdout=subprocess.PIPE).stdout.decode()
        assert "forest_level_mutated_kernel" in syms and "forest_scan_mutated_kernel" in syms
        return
    assert rec["audit"]["block_count_errors"] == [] and rec["audit"]["unclassified"] == []
    blocks = {k: v for k, v in rec["audit"]["blocks"].items() if "mutated" in k}
    assert list(blocks.values()) == [1] and mine in next(iter(blocks))      # the scan holds none
    plain = [v for k, v in rec["hash_blocks"].items() if "forest_level_kernel" in k]
    flagged = [v for k, v in rec["hash_blocks"].items() if mine in k]
    assert len(plain) == 1 and len(plain[0]) == 1 and len(flagged) == 1 and len(flagged[0]) == 1
    p, f = plain[0][0], flagged[0][0]
    # the same three compressions: the rotates are the round function's alone and must agree.  The compare is outside the block,
    # but the compiler cuts the block's edges differently (address arithmetic and the store's select move across them), so the
    # VALU and complex counts need not be equal: they stay within 64 of forest_level_kernel's, far from a second compression
    assert f["rotates"] == p["rotates"]
    assert abs(f["valu"] - p["valu"]) <= 64 and abs(f["complex"] - p["complex"]) <= 64, (p, f)


def test_python_layer_refuses_counts_that_do_not_fit_before_any_device_call(native):
    import vk_merkle_roots_amd as vk
    batch = vk.pack_lines(b"a\nb\nc\n")
    with pytest.raises(ValueError):
        vk.merkle_roots_packed_forest_mutated(None, batch, [1, 1])
