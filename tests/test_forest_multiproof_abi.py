"""Multiproofs inside a stored forest without a GPU: the C ABI's declarations and argument checks, the node bound's closed form,
the host counterparts vkmr_host_cpu_forest_multiproof and vkmr_host_cpu_verify_forest_multiproof against a hashlib restatement
(tests/forest_multiproof_cases.py), the oracle's roots and what the reference's own CPU path returned, the per-tree split
against the single tree's multiproof, and one run of both host functions under AddressSanitizer and UBSan in a stand-alone
program (tests/c/forest_multiproof_host_test.cpp).  No compute calls on a device here."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import forest_cases as fc
import forest_multiproof_cases as fm
import multiproof_cases as mc
from abi_support import Refusals, assert_bound, assert_exported, assert_key_resolves, assert_no_spills, isa_record
from conftest import ROOT
from merkle_model import random_counts
from no_device import NoDevice

ENTRY_POINTS = ("vkmr_hip_forest_multiproof_max_nodes", "vkmr_hip_forest_multiproof_scratch_bytes", "vkmr_hip_forest_multiproof_async",
                "vkmr_hip_verify_forest_multiproof_async")
HOST_ENTRY_POINTS = ("vkmr_host_cpu_forest_multiproof", "vkmr_host_cpu_verify_forest_multiproof")
NON_EMPTY = sorted(name for name, counts in fc.CASES.items() if sum(counts))


def case_leaves(name):
    counts = fc.CASES[name]
    return fc.random_leaves(sum(counts), seed=len(name) * 104729 + sum(counts))


def test_header_library_and_stub_agree_on_the_new_symbols(native):
    from vk_merkle_roots_amd import _abi
    assert_exported(native.HIP_LIB, ENTRY_POINTS)
    # max_nodes(total, ntrees, max_count, k); scratch_bytes(k, stride); the gather: dev, s, digests, forest, total, offsets, ntrees,
    # max_count, trees, indices, k, scratch, nodes, nodes_capacity, heights, info; the verifier: dev, s, leaves, trees, indices,
    # heights, k, stride, nodes, m, roots, ntrees, scratch, ok
    assert_bound(ENTRY_POINTS[0], nparams=4, restype=C.c_size_t)
    assert_bound(ENTRY_POINTS[1], nparams=2, restype=C.c_size_t)
    assert_bound(ENTRY_POINTS[2], nparams=16, scalars=[C.c_int, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint64])
    assert_bound(ENTRY_POINTS[3], nparams=14, scalars=[C.c_int, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32])
    assert_exported(native.HOST_LIB, HOST_ENTRY_POINTS)
    assert all(name in _abi.HOST_SIGNATURES for name in HOST_ENTRY_POINTS)


def test_bad_arguments_are_refused_before_any_hip_call(native):
    from vk_merkle_roots_amd import _abi
    lib = _abi.lib()
    d = C.c_void_p(0x1000)                 # never dereferenced: every call below returns before launching anything
    # digests, forest, total, offsets, ntrees, max_count, trees, indices, k, scratch, nodes, nodes_capacity, heights, info
    gather = Refusals(lib.vkmr_hip_forest_multiproof_async, "vkmr_hip_forest_multiproof_async", good=[d, d, 100, d, 4, 50, d, d, 8, d, d, 64, d, d])
    gather.null(0, 1, 3, 6, 7, 9, 10, 12, 13)  # each pointer NULL with k > 0 (the nodes with a capacity above 0)
    gather.changed({4: 0}, {2: 0}, {5: 0}, {2: (1 << 58) + 1}, {9: C.c_void_p(0x1008)})      # ntrees, total, max_count == 0; too many leaves; alignment
    # k == 0 is a no-op whatever the rest
    gather.ok((None, None, 100, None, 4, 50, None, None, 0, None, None, 0, None, None), (None, None, 0, None, 0, 0, None, None, 0, None, None, 7, None, None))

    # leaves, trees, indices, heights, k, stride, nodes, m, roots, ntrees, scratch, ok
    verify = Refusals(lib.vkmr_hip_verify_forest_multiproof_async, "vkmr_hip_verify_forest_multiproof_async", good=[d, d, d, d, 8, 12, d, 30, d, 4, d, d])
    verify.null(0, 1, 2, 3, 6, 8, 10, 11)  # each pointer NULL with k > 0 (the nodes with m > 0)
    verify.changed({5: 0}, {5: 64}, {5: 100}, {10: C.c_void_p(0x1004)})                      # the stride; the scratch's alignment
    verify.ok((None, None, None, None, 0, 12, None, 0, None, 4, None, None), (None, None, None, None, 0, 0, None, 9, None, 0, None, None))   # k == 0


def test_scratch_bytes_is_one_aligned_size_for_gather_and_verifier(native):
    import vk_merkle_roots_amd as vk
    f = vk.lib().vkmr_hip_forest_multiproof_scratch_bytes
    for stride in (1, 2, 11, 26, 63):
        assert f(0, stride) == 0
        for k in (1, 63, 64, 65, 16384, 16385, 1 << 20, (1 << 32) - 1):
            words = (k + 63) // 64
            blocks = (words + 255) // 256
            # k cells, two arrays of stride x words, stride x blocks block starts, the header, k end words
            assert f(k, stride) >= 32 * k + 16 * words * stride + 8 * blocks * stride + 8 * (2 + stride) + 4 * k
            single = vk.lib().vkmr_hip_multiproof_scratch_bytes(k, stride)                    # the single tree's layout, height := stride,
            assert f(k, stride) % 16 == 0 and single <= f(k, stride) < single + 16            # in whole 16-byte units
    for k in (1, 1000):
        assert f(k, 64) == 0 and f(k, 1000) == 0


def test_max_nodes_is_its_closed_form_and_bounds_the_restatement(native):
    import vk_merkle_roots_amd as vk
    f = vk.lib().vkmr_hip_forest_multiproof_max_nodes
    for total in (0, 1, 2, 3, 5, 127, 128, 129, 1000, 1 << 20, (1 << 26) + 3, 1 << 33):
        for ntrees in (0, 1, 2, 64, 32768, (1 << 32) - 1):
            for max_count in (0, 1, 2, 3, 2047, 2048, 2049, 2**63, 2**64 - 1):
                for k in (0, 1, 2, 1000, (1 << 32) - 1):
                    assert f(total, ntrees, max_count, k) == fm.max_nodes(total, ntrees, max_count, k), (total, ntrees, max_count, k)
    assert f(1 << 26, 1 << 15, 1 << 11, 1 << 20) == sum(min(1 << 20, ((1 << 26) >> (l + 1)) + (1 << 15)) for l in range(11))
    attained = []
    for name in NON_EMPTY:
        counts = fc.CASES[name]
        total, largest = sum(counts), max(counts)
        for trees, indices in fm.entry_sets(counts, np.random.default_rng(len(name))).values():
            for max_count in (largest, total, 2**63):
                stride = fm.stride_of(total, max_count)
                m = len(fm.emitted_positions(counts, trees, indices, stride)[0])
                bound = f(total, len(counts), max_count, len(trees))
                assert m <= bound, (name, max_count)
                attained.append(m == bound)
    assert any(attained)                   # all_ones, every leaf: one node per entry at the only level


def test_max_nodes_bounds_a_thousand_random_forests(native):
    import vk_merkle_roots_amd as vk
    f = vk.lib().vkmr_hip_forest_multiproof_max_nodes
    rng = np.random.default_rng(31415)
    done = 0
    while done < 1000:
        counts = random_counts(rng, 1 << 13)
        if not counts or max(counts) == 0:
            continue
        full = [t for t, c in enumerate(counts) if c]
        pairs = [(t, i) for t in full for i in (0, counts[t] - 1)] if done % 2 else []
        more_trees, more_indices = fm.fp.random_queries(rng, counts, int(rng.integers(1, 300)))
        trees, indices = fm.sorted_entries(pairs + list(zip(more_trees.tolist(), more_indices.tolist())))
        total = sum(counts)
        max_count = (max(counts), max(counts) + int(rng.integers(0, 5000)), 2**64 - 1)[done % 3]
        stride = fm.stride_of(total, max_count)
        pos, level_counts = fm.emitted_positions(counts, trees, indices, stride)
        assert sum(level_counts) == len(pos) <= f(total, len(counts), max_count, len(trees)), counts[:10]
        for l, m in enumerate(level_counts):
            assert m <= min(len(trees), (total >> (l + 1)) + len(counts))
        done += 1


def check_host_against_the_model(leaves, counts, trees, indices, stride, want_roots=None):
    """Both host functions on one entry set; (nodes, heights, roots [ntrees, 8])."""
    off = fc.offsets_of(counts)
    want_nodes, want_heights, want_counts, roots = fm.make(leaves, off, trees, indices, stride)
    rc, nodes, heights, info = fm.host_make(leaves, off, trees, indices, stride)
    assert rc == 0 and int(info[0]) == 0
    assert int(info[1]) == want_nodes.shape[0] and [int(x) for x in info[2:]] == want_counts
    assert (heights == want_heights).all()
    assert nodes.shape == want_nodes.shape and (nodes == want_nodes).all(), np.nonzero((nodes != want_nodes).any(axis=1))[0][:10]
    roots = fm.roots_array(roots, len(counts))
    if want_roots is not None:
        for t in set(int(t) for t in trees):
            assert (roots[t] == want_roots[t]).all(), t
    proved = fm.leaves_at(leaves, off, trees, indices)
    assert fm.host_verify(proved, trees, indices, heights, stride, nodes, roots)
    return proved, nodes, heights, roots


@pytest.mark.parametrize("name", NON_EMPTY)
def test_host_cpu_functions_equal_the_restatement_on_every_case_table(native, oracle, name):
    counts = fc.CASES[name]
    leaves = case_leaves(name)
    want_roots = fc.oracle_roots(oracle, leaves, counts)
    rng = np.random.default_rng(len(name) * 31 + 5)
    ran = set()
    for set_name, (trees, indices) in fm.entry_sets(counts, rng).items():
        for stride in sorted({fm.stride_of(sum(counts), max(counts)), fm.stride_of(sum(counts), sum(counts))}):
            proved, nodes, heights, roots = check_host_against_the_model(leaves, counts, trees, indices, stride, want_roots)
        if trees.shape[0] > 3000:          # the restatement's verifier hashes in Python: the large sets are checked above, by the C verifier
            continue
        assert fm.verify(proved, trees, indices, heights, stride, nodes, roots), set_name
        for mutation in fm.mutations(proved, trees, indices, heights, stride, nodes, roots, rng):
            mname, args = mutation[0], mutation[1:]
            want = mname == fm.STILL_ACCEPTED
            lv, tr, ix, hs, nd, rt = args
            assert fm.verify(lv, tr, ix, hs, stride, nd, rt) == want, (set_name, mname)
            assert fm.host_verify(lv, tr, ix, hs, stride, nd, rt) == want, (set_name, mname)
            ran.add(mname)
    assert "node appended" in ran and "leaf changed" in ran and "touched root changed" in ran


def test_every_mutation_runs_somewhere_over_the_tables_and_the_host_verifier_refuses_the_cheap_ones(native):
    """The rejects above skip what a case lacks; nothing may be skipped everywhere.  The leaves and nodes here are dummies, so
    only the mutations that are refused before any hash (order, ranges, heights, node count) go through the host verifier."""
    before_any_hash = {"last node dropped", "node appended", "entries swapped", "entry repeated", "index >= 2^h", "tree >= ntrees", "height 0",
                       "height above stride", "one entry of a tree with another height", "a tree's height + 1", "a tree's height - 1"}
    ran = set()
    for name in NON_EMPTY:
        counts = fc.CASES[name]
        rng = np.random.default_rng(3)
        off = fc.offsets_of(counts)
        stride = fm.stride_of(sum(counts), max(counts))
        for trees, indices in fm.entry_sets(counts, rng).values():
            heights = [fm.tree_height(counts[int(t)]) for t in trees]
            m = len(fm.emitted_positions(counts, trees, indices, stride)[0])
            proved = fm.leaves_at(np.zeros((sum(counts), 8), np.uint32), off, trees, indices)
            for mname, lv, tr, ix, hs, nd, rt in fm.mutations(proved, trees, indices, heights, stride, np.ones((m, 8), np.uint32),
                                                              np.zeros((len(counts), 8), np.uint32), rng):
                ran.add(mname)
                if mname in before_any_hash:
                    assert not fm.host_verify(lv, tr, ix, hs, stride, nd, rt), (name, mname)
    assert ran == set(fm.MUTATIONS) | {fm.STILL_ACCEPTED}


def test_ten_reference_trees_as_one_forest_fold_to_the_recorded_roots(native, oracle, ref_checks):
    leaves, counts = fc.ref_check_forest(oracle)
    assert counts == [1, 2, 3, 5, 8, 13, 64, 77, 256, 301]
    recorded = [t["root"] for t in ref_checks["trees"]]
    rng = np.random.default_rng(77)
    stride = fm.stride_of(sum(counts), max(counts))
    for set_name, (trees, indices) in fm.entry_sets(counts, rng).items():
        proved, nodes, heights, roots = check_host_against_the_model(leaves, counts, trees, indices, stride)
        assert [oracle.hex(roots[t]) for t in range(len(counts))] == recorded, set_name     # every set names every tree
        assert fm.verify(proved, trees, indices, heights, stride, nodes, roots), set_name


def test_host_gather_statuses_capacity_and_refusals(native):
    counts = [4, 0, 0, 7, 0, 1, 130]
    leaves = fc.random_leaves(sum(counts), seed=19)
    off = fc.offsets_of(counts)
    pattern32, pattern64 = np.uint32(0xA5A5A5A5), np.uint64(0xA5A5A5A5A5A5A5A5)
    good = fm.sorted_entries([(0, 1), (0, 3), (3, 0), (3, 6), (5, 0), (6, 128), (6, 129)])
    rc, nodes, heights, info = fm.host_make(leaves, off, *good, 8)
    assert rc == 0 and list(heights) == [2, 2, 3, 3, 1, 8, 8]
    m = int(info[1])
    # bit 0: a tree equal to ntrees, an index equal to its tree's count, an entry into an empty tree; bit 1: out of order, repeated
    for trees, indices, want in (([0, 7], [1, 0], 1), ([0, 3], [4, 0], 1), ([0, 1], [0, 0], 1), ([3, 0], [0, 1], 2), ([0, 0], [2, 1], 2),
                                 ([0, 0], [1, 1], 2), ([3, 0], [7, 0], 3)):
        rc, nodes, heights, info = fm.host_make(leaves, off, trees, indices, 8)
        assert rc == want and int(info[0]) == want, (trees, indices)
        assert (nodes == pattern32).all() and (heights == pattern32).all() and (info[1:] == pattern64).all()
    # bit 2: one cell too few -- M and the counts valid, the heights written, no node; exactly M cells succeed
    rc, nodes, heights, info = fm.host_make(leaves, off, *good, 8, capacity=m - 1)
    assert rc == 4 and int(info[0]) == 4 and int(info[1]) == m and int(info[2:].sum()) == m
    assert (nodes == pattern32).all() and list(heights) == [2, 2, 3, 3, 1, 8, 8]
    rc, nodes, heights, info = fm.host_make(leaves, off, *good, 8, capacity=m)
    assert rc == 0 and nodes.shape[0] == m
    # a stride below the tallest named tree, a stride above 63 and decreasing offsets are refused and nothing is written
    for stride, offsets in ((7, off), (64, off), (8, np.array([0, 5, 4, 20, 20, 20, 20, 150], dtype=np.uint64))):
        rc, nodes, heights, info = fm.host_make(leaves, offsets, *good, stride, capacity=64)
        assert rc < 0 and (nodes == pattern32).all() and (heights == pattern32).all() and (info == pattern64).all(), stride
    # the same stride serves entries that name only the shorter trees
    rc, nodes, heights, info = fm.host_make(leaves, off, [0, 3], [0, 0], 3)
    assert rc == 0 and list(heights) == [2, 3]
    # a lone leaf proves itself with itself
    rc, nodes, heights, info = fm.host_make(leaves, off, [5], [0], 8)
    assert rc == 0 and nodes.shape[0] == 1 and (nodes[0] == leaves[int(off[5])]).all() and [int(x) for x in info[2:]] == [1] + [0] * 7


def test_neighbours_in_another_tree_are_no_siblings(native):
    """Leaf 1 of tree 0 and leaf 0 of tree 1 are adjacent entries whose indices differ by one: each still needs its own sibling."""
    counts = [2, 2]
    leaves = fc.random_leaves(4, seed=29)
    off = fc.offsets_of(counts)
    pos, level_counts = fm.emitted_positions(counts, [0, 1], [1, 0], 1)
    assert pos == [(0, 0, 0), (0, 1, 1)] and level_counts == [2]
    rc, nodes, heights, info = fm.host_make(leaves, off, [0, 1], [1, 0], 1)
    assert rc == 0 and [int(x) for x in info] == [0, 2, 2] and (nodes == leaves[[0, 3]]).all() and list(heights) == [1, 1]
    pos, _ = fm.emitted_positions(counts, [0, 0], [0, 1], 1)
    assert pos == []
    rc, nodes, heights, info = fm.host_make(leaves, off, [0, 0], [0, 1], 1)
    assert rc == 0 and [int(x) for x in info] == [0, 0, 0] and nodes.shape[0] == 0


def test_the_split_of_the_restatement_is_each_tree_s_own_multiproof(native):
    """Guards the restatement's split (the yardstick of ForestMultiproof.split below and on the GPU) against the single tree's
    restatement; of the product it calls the single tree's host verifier and, on each forest proof, the forest's host gather."""
    for name in NON_EMPTY:
        counts = fc.CASES[name]
        if sum(counts) > 20000:
            continue                       # the same rule at every size: the small tables suffice for a per-tree restatement in Python
        leaves = case_leaves(name)
        off = fc.offsets_of(counts)
        stride = fm.stride_of(sum(counts), max(counts))
        rng = np.random.default_rng(len(name))
        for trees, indices in fm.entry_sets(counts, rng).values():
            nodes, heights, _, roots = fm.make(leaves, off, trees, indices, stride)
            rc, host_nodes, host_heights, _ = fm.host_make(leaves, off, trees, indices, stride)
            assert rc == 0 and (host_nodes == nodes).all() and (host_heights == heights).all()
            parts = fm.split(trees, indices, host_heights, host_nodes, stride)
            assert sorted(parts) == sorted(set(int(t) for t in trees))
            assert sum(p[2].shape[0] for p in parts.values()) == nodes.shape[0]
            for t, (idx, h, mine, level_counts) in list(parts.items())[:40]:
                mine_leaves = leaves[int(off[t]): int(off[t + 1])]
                levels = mc.cpu_levels(mine_leaves)
                want, want_counts = mc.make_multiproof(lambda l: levels[l], counts[t], h, idx)
                assert h == len(levels) - 1 and want_counts == level_counts
                assert (mine == want).all(), (name, t)
                assert mc.host_verify(mine_leaves[idx.astype(np.int64)], idx, h, mine, roots[t])


def test_the_two_host_verifiers_agree_on_a_forest_of_one_tree(native):
    """vkmr_host_cpu_verify_multiproof and vkmr_host_cpu_verify_forest_multiproof walk a level with the same helper: on a forest
    of one tree they give the same answer, for the single tree's case tables and for every corruption of a proof in them (an
    index, a node, m, a leaf)."""
    for count in mc.COUNTS:
        rng = np.random.default_rng(4200 + count)
        leaves = mc.random_leaves(rng, count)
        levels = mc.cpu_levels(leaves)
        height, root = len(levels) - 1, levels[-1][0]
        for idx in mc.small_index_sets(count, rng):
            nodes, _ = mc.make_multiproof(lambda l: levels[l], count, height, idx)
            cases = [("as made", leaves[idx], np.array(idx, dtype=np.uint64), nodes)] + mc.mutations(leaves[idx], idx, nodes, height, rng)
            for what, lv, ix, nd in cases:
                one = mc.host_verify(lv, ix, height, nd, root)
                many = fm.host_verify(lv, np.zeros(len(ix), dtype=np.uint32), ix, np.full(len(ix), height, dtype=np.uint32), height, nd, root)
                assert one == many == (what == "as made"), (count, idx, what)


def test_the_product_s_split_equals_the_restatement_s(native):
    import vk_merkle_roots_amd as vk
    counts = fc.CASES["sizes_1_to_130"]
    leaves = case_leaves("sizes_1_to_130")
    off = fc.offsets_of(counts)
    stride = fm.stride_of(sum(counts), max(counts))
    for trees, indices in fm.entry_sets(counts, np.random.default_rng(8)).values():
        nodes, heights, level_counts, _ = fm.make(leaves, off, trees, indices, stride)
        proof = vk.ForestMultiproof(trees, indices, heights, nodes, np.array(level_counts, dtype=np.uint64), stride)
        got, want = proof.split(), fm.split(trees, indices, heights, nodes, stride)
        assert sorted(got) == sorted(want)
        for t, (idx, h, mine, per_level) in want.items():
            assert isinstance(got[t], vk.Multiproof) and got[t].height == h
            assert (got[t].indices == idx).all() and (got[t].nodes == mine).all() and [int(x) for x in got[t].level_counts] == per_level
    with pytest.raises(ValueError):        # a proof that lost a node cannot be regrouped
        vk.ForestMultiproof(trees, indices, heights, nodes[:-1], None, stride).split()


def test_multiproof_refuses_bad_entries_before_any_device_call(native):
    import vk_merkle_roots_amd as vk
    counts = [4, 0, 0, 7, 0, 0, 0, 1]
    forest = vk.MerkleForest(NoDevice(), None, sum(counts), counts, None, 7, None, None)
    for trees, indices in (([8], [0]), ([0], [4]), ([1], [0]), ([-1], [0]), ([0], [-1]), ([2**32], [0])):
        with pytest.raises(IndexError):
            forest.multiproof(trees, indices)
    for trees, indices in (([0, 3], [1]), ([0.5], [1]), ([], [])):
        with pytest.raises(ValueError):
            forest.multiproof(trees, indices)
    from vk_merkle_roots_amd import engine
    assert engine.forest_multiproof_status_text(0) == "ok"
    assert "bit 0" in engine.forest_multiproof_status_text(1) and "bit 1" in engine.forest_multiproof_status_text(2)
    assert "bit 2" in engine.forest_multiproof_status_text(4) and "unknown" in engine.forest_multiproof_status_text(8)


def test_the_level_kernel_holds_one_hash_block_and_the_build_lists_it(native):
    from vk_merkle_roots_amd import isa_prio_pass
    mine = "verify_forest_multiproof_level_kernel"
    assert isa_prio_pass.EXPECTED_HASH_BLOCKS[mine] == 1
    assert_key_resolves(mine)
    rec = isa_record(native)
    if rec is not None:                    # written by a build that ran the issue pass (tests/test_isa_prio_pass.py covers its absence)
        assert rec["audit"]["block_count_errors"] == [] and rec["audit"]["unclassified"] == []
        blocks = {k: v for k, v in rec["audit"]["blocks"].items() if "forest_multiproof" in k}
        assert list(blocks.values()) == [1] and mine in next(iter(blocks))      # the check, the heights, the masks, the gather and the finish hold none
    assert_no_spills(native, [mine], max_vgprs=64, prefix=True)        # 512 registers a lane, 8 wavefronts per SIMD


def test_both_host_functions_under_address_and_undefined_behaviour_sanitizers(native, tmp_path):
    """A stand-alone program (its own main, no Python in the process) over every case table and entry set, once.  The
    sanitizer runtimes are linked statically, so the program needs nothing of the environment it is started in."""
    host = os.path.join(ROOT, "vk_merkle_roots_amd", "csrc", "host")
    exe = str(tmp_path / "forest_multiproof_host_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "include"), "-I", host,
                           os.path.join(ROOT, "tests", "c", "forest_multiproof_host_test.cpp"), os.path.join(host, "host_api.cpp"),
                           os.path.join(host, "cpu_sha256d.cpp"), "-o", exe])
    lines, want = [], []
    for name in NON_EMPTY:
        counts = fc.CASES[name]
        rng = np.random.default_rng(len(name) + 11)
        stride = fm.stride_of(sum(counts), max(counts))
        for trees, indices in fm.entry_sets(counts, rng).values():
            entries = [str(int(x)) for pair in zip(trees, indices) for x in pair]
            lines.append(" ".join([str(stride), str(len(counts))] + [str(c) for c in counts] + [str(len(trees))] + entries))
            level_counts = fm.emitted_positions(counts, trees, indices, stride)[1]
            want.append([sum(level_counts)] + level_counts)
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)    # the environment as it is
    text = r.stdout.decode()
    assert r.returncode == 0 and "FAIL" not in text and "ERROR" not in text and "runtime error" not in text, text[-3000:]
    assert f"ok: {len(lines)} cases" in text
    got = [[int(x) for x in line.split()] for line in text.splitlines()[: len(lines)]]
    assert got == want
