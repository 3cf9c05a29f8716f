"""Applying a multiproof without a GPU: the C ABI's declarations and argument checks, the scratch size's closed form and its
layout replayed from csrc/tree_plan.hpp (tests/c/apply_plan_test.cpp), the host counterparts vkmr_host_cpu_apply_multiproof and
vkmr_host_cpu_apply_forest_multiproof against a hashlib restatement (tests/apply_cases.py) AND against a rebuild of the updated
leaves, every refusal with the new-root buffer untouched, one run of both host functions under AddressSanitizer and UBSan in a
stand-alone program (tests/c/apply_host_test.cpp), and the build records of the two level kernels.  No compute calls on a
device here."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import apply_cases as ac
import forest_cases as fc
import forest_multiproof_cases as fm
from abi_support import Refusals, assert_bound, assert_exported, assert_key_resolves, assert_no_spills, isa_record
from conftest import ROOT
from merkle_model import build_plan_exe, cpu_levels, random_leaves, tree_height

ENTRY_POINTS = ("vkmr_hip_apply_multiproof_scratch_bytes", "vkmr_hip_apply_multiproof_async", "vkmr_hip_apply_forest_multiproof_async")
HOST_ENTRY_POINTS = ("vkmr_host_cpu_apply_multiproof", "vkmr_host_cpu_apply_forest_multiproof")
LEVEL_KERNELS = ("tree_apply_level_kernel", "forest_apply_level_kernel")
# the hash block of the two verifier level kernels as the commit before this one built it: the policy parameter of
# multiproof_verify_level must not change their code
VERIFIER_HASH_BLOCK = {"valu": 3746, "complex": 1959, "simple": 1787, "rotates": 1504}


def test_header_library_and_stub_agree_on_the_new_symbols(native):
    from vk_merkle_roots_amd import _abi
    assert_exported(native.HIP_LIB, ENTRY_POINTS)
    # scratch_bytes(k, levels); the tree: dev, s, old, new, indices, k, count, height, nodes, m, root, scratch, ok, new_root; the
    # forest: dev, s, old, new, trees, indices, counts, k, stride, nodes, m, roots, ntrees, scratch, ok, new_roots
    assert_bound(ENTRY_POINTS[0], nparams=2, restype=C.c_size_t)
    assert_bound(ENTRY_POINTS[1], nparams=14, scalars=[C.c_int, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint64])
    assert_bound(ENTRY_POINTS[2], nparams=16, scalars=[C.c_int, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32])
    assert_exported(native.HOST_LIB, HOST_ENTRY_POINTS)
    for name, nparams in zip(HOST_ENTRY_POINTS, [10, 12]):
        assert_bound(name, nparams=nparams, table=_abi.HOST_SIGNATURES, header="vkmr_host.h")


def test_the_python_wrappers_are_there_and_none_is_named_async(native):
    import vk_merkle_roots_amd as vk
    for name in ("apply_multiproof_scratch_bytes", "apply_multiproof_enqueue", "apply_forest_multiproof_enqueue", "apply_multiproof",
                 "apply_forest_multiproof"):
        assert callable(getattr(vk.HipDevice, name)), name
    assert not [n for n in dir(vk.HipDevice) if "apply" in n and n.endswith("_async")]
    assert callable(vk.MerkleForest.update_with_witness) and callable(vk.MerkleTree.update_with_witness) and callable(vk.UpdateWitness.apply)


def test_bad_arguments_are_refused_before_any_hip_call(native):
    from vk_merkle_roots_amd import _abi
    lib = _abi.lib()
    d = C.c_void_p(0x1000)                 # never dereferenced: every call below returns before launching anything
    # old, new, trees, indices, counts, k, stride, nodes, m, roots, ntrees, scratch, ok, new_roots
    forest = Refusals(lib.vkmr_hip_apply_forest_multiproof_async, "vkmr_hip_apply_forest_multiproof_async", good=[d, d, d, d, d, 8, 12, d, 30, d, 4, d, d, d])
    forest.null(0, 1, 2, 3, 4, 7, 9, 11, 12, 13)   # each pointer NULL with k > 0 (the nodes with m > 0)
    forest.changed({6: 0}, {6: 64}, {6: 100}, {11: C.c_void_p(0x1004)})        # the stride; the scratch's alignment
    forest.ok((None, None, None, None, None, 0, 12, None, 0, None, 4, None, None, None),      # k == 0
              (None, None, None, None, None, 0, 0, None, 9, None, 0, None, None, None))

    # old, new, indices, k, count, height, nodes, m, root, scratch, ok, new_root
    tree = Refusals(lib.vkmr_hip_apply_multiproof_async, "vkmr_hip_apply_multiproof_async", good=[d, d, d, 8, 1000, 10, d, 30, d, d, d, d])
    tree.null(0, 1, 2, 6, 8, 9, 10, 11)
    tree.changed({5: 0}, {5: 64}, {5: 100}, {9: C.c_void_p(0x1008)})           # the height; the scratch's alignment
    tree.ok((None, None, None, 0, 1000, 10, None, 0, None, None, None, None), (None, None, None, 0, 0, 0, None, 5, None, None, None, None))   # k == 0


def test_scratch_bytes_is_its_closed_form_and_the_pinned_sizes_did_not_move(native):
    import vk_merkle_roots_amd as vk
    f = vk.lib().vkmr_hip_apply_multiproof_scratch_bytes
    for levels in (1, 2, 11, 26, 58, 63):
        assert f(0, levels) == 0
        for k in ac.EDGE_KS + (1 << 20, (1 << 32) - 1):
            assert f(k, levels) == ac.scratch_bytes(k, levels), (k, levels)
            assert f(k, levels) % 16 == 0
            verifier = vk.lib().vkmr_hip_forest_multiproof_scratch_bytes(k, levels)
            assert f(k, levels) == verifier + 32 * k + 2 * ((4 * k + 15) // 16 * 16)        # the verifier's scratch, untouched, in front
    for k in (1, 1000):
        assert f(k, 64) == 0 and f(k, 1000) == 0
    pinned = json.load(open(os.path.join(ROOT, "tests", "golden", "abi_sizes.json")))
    assert not any("apply" in key for key in pinned)           # a fixture of the sizes that existed: this call is not in it


def test_the_scratch_layout_replayed_from_the_plan_header(native, tmp_path):
    import vk_merkle_roots_amd as vk
    exe = build_plan_exe(tmp_path, "apply_plan_test")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    text = r.stdout.decode()
    assert r.returncode == 0 and "FAIL" not in text and "ok: 36 layouts" in text, text[-2000:]
    rows = [tuple(int(x) for x in line.split()) for line in text.splitlines()[:36]]
    assert sorted(set(k for k, _, _ in rows)) == sorted(ac.EDGE_KS)
    for k, levels, nbytes in rows:
        assert vk.lib().vkmr_hip_apply_multiproof_scratch_bytes(k, levels) == nbytes == ac.scratch_bytes(k, levels), (k, levels)


def witness_of(leaves, counts, trees, indices, stride, rng, cache):
    """(old leaves at the entries, random new leaves, per-entry counts, nodes, heights, roots [ntrees, 8])."""
    off = fc.offsets_of(counts)
    nodes, heights, _, roots = fm.make(leaves, off, trees, indices, stride, cache)
    return fm.leaves_at(leaves, off, trees, indices), random_leaves(rng, len(trees)), ac.counts_of(counts, trees), nodes, heights, \
        fm.roots_array(roots, len(counts))


@pytest.mark.parametrize("pattern", ac.LEAF_PATTERNS)
@pytest.mark.parametrize("name", ac.NON_EMPTY)
def test_host_functions_equal_the_restatement_and_a_rebuild_on_every_case_table(native, name, pattern):
    counts = fc.CASES[name]
    leaves = ac.case_leaves(name, pattern)
    off = fc.offsets_of(counts)
    rng = np.random.default_rng(len(name) * 131 + len(pattern))
    stride = fm.stride_of(sum(counts), max(counts))
    cache, ran, trees_tried = {}, set(), 0
    for set_name, (trees, indices) in ac.entry_sets(counts, rng).items():
        old, new, cs, nodes, heights, roots = witness_of(leaves, counts, trees, indices, stride, rng, cache)
        r, got = ac.host_apply_forest(old, new, trees, indices, cs, stride, nodes, roots)
        assert r == 1, set_name
        want = ac.rebuilt_roots(ac.updated(leaves, counts, trees, indices, new), counts, trees)
        named = sorted(want)
        assert all((got[t] == want[t]).all() for t in named), (set_name, [t for t in named if (got[t] != want[t]).any()][:10])
        others = np.ones(len(counts), dtype=bool)
        others[named] = False
        assert (got[others] == ac.CANARY).all(), set_name                   # cells of unnamed trees are never written
        r, in_place = ac.host_apply_forest(old, new, trees, indices, cs, stride, nodes, roots, in_place=True)
        assert r == 1 and (in_place[named] == got[named]).all() and (in_place[others] == roots[others]).all(), set_name
        # the single tree's call on up to 20 trees spread over the forest, the proof split per tree
        parts = fm.split(trees, indices, heights, nodes, stride)
        for t in named[:: max(1, len(named) // 20)][:20]:
            idx, h, mine, _ = parts[t]
            rows = np.flatnonzero(np.asarray(trees) == t)
            r, root = ac.host_apply_tree(old[rows], new[rows], idx, counts[t], h, mine, roots[t])
            assert r == 1 and (root == want[t]).all(), (set_name, t)
            if idx.shape[0] <= 300:
                assert (ac.apply_tree(old[rows], new[rows], idx, counts[t], h, mine, roots[t]) == want[t]).all(), (set_name, t)
            trees_tried += 1
        if trees.shape[0] > 3000:          # the restatement hashes in Python: the large sets are checked above, against the rebuild
            continue
        model = ac.apply_forest(old, new, trees, indices, cs, stride, nodes, roots)
        assert model is not None and (model[named] == got[named]).all(), set_name
        for mname, lv, tr, ix, hs, nd, rt in fm.mutations(old, trees, indices, heights, stride, nodes, roots, rng):
            accepted = mname == fm.STILL_ACCEPTED
            mcs = ac.counts_for_heights(hs, tr, counts)
            r, out = ac.host_apply_forest(lv, new, tr, ix, mcs, stride, nd, rt)
            assert (r == 1) == accepted, (set_name, mname)
            assert (ac.apply_forest(lv, new, tr, ix, mcs, stride, nd, rt) is not None) == accepted, (set_name, mname)
            if accepted:
                assert (out[named] == got[named]).all(), (set_name, mname)
            else:
                assert (out == ac.CANARY).all(), (set_name, mname)          # a refusal writes nothing
            ran.add(mname)
    assert trees_tried and "node appended" in ran and "leaf changed" in ran and "touched root changed" in ran


def test_every_mutation_runs_somewhere_over_the_tables():
    ran = set()
    for name in ac.NON_EMPTY:
        counts = fc.CASES[name]
        rng = np.random.default_rng(3)
        off = fc.offsets_of(counts)
        stride = fm.stride_of(sum(counts), max(counts))
        for trees, indices in ac.entry_sets(counts, rng).values():
            heights = [tree_height(counts[int(t)]) for t in trees]
            m = len(fm.emitted_positions(counts, trees, indices, stride)[0])
            proved = fm.leaves_at(np.zeros((sum(counts), 8), np.uint32), off, trees, indices)
            ran |= {mut[0] for mut in fm.mutations(proved, trees, indices, heights, stride, np.ones((m, 8), np.uint32),
                                                   np.zeros((len(counts), 8), np.uint32), rng)}
    assert ran == set(fm.MUTATIONS) | {fm.STILL_ACCEPTED}


def small_forest():
    counts = [4, 0, 6, 7, 0, 1, 130, 10]
    leaves = fc.random_leaves(sum(counts), seed=23)
    trees, indices = fm.sorted_entries([(0, 1), (0, 3), (2, 4), (3, 0), (3, 6), (5, 0), (6, 128), (6, 129), (7, 8)])
    stride = 8
    rng = np.random.default_rng(5)
    return (counts, leaves, trees, indices, stride) + witness_of(leaves, counts, trees, indices, stride, rng, {})


def test_the_new_refusals_count_0_index_outside_the_count_and_two_counts_in_one_tree(native):
    counts, leaves, trees, indices, stride, old, new, cs, nodes, heights, roots = small_forest()
    assert ac.host_apply_forest(old, new, trees, indices, cs, stride, nodes, roots)[0] == 1
    refused = {}
    c = cs.copy()
    c[trees == 3] = 0
    refused["count 0"] = c
    c = cs.copy()
    c[trees == 6] = 129                   # index 129 >= 129, < 2^8, and height(129) == height(130)
    assert tree_height(129) == tree_height(130)
    refused["index >= count but < 2^h"] = c
    c = cs.copy()
    c[int(np.flatnonzero(trees == 0)[0])] = 3          # index 1 < 3 and height(3) == height(4): only the count differs inside the tree's run
    assert tree_height(3) == tree_height(4)
    refused["one entry of a tree with another count"] = c
    for what, bad in refused.items():
        r, out = ac.host_apply_forest(old, new, trees, indices, bad, stride, nodes, roots)
        assert r == 0 and (out == ac.CANARY).all(), what
        assert ac.apply_forest(old, new, trees, indices, bad, stride, nodes, roots) is None, what
    # the single tree's call: a count of 0, an index at the count, a count above 2^height
    rows = np.flatnonzero(trees == 6)
    idx, h, mine, _ = fm.split(trees, indices, heights, nodes, stride)[6]
    assert ac.host_apply_tree(old[rows], new[rows], idx, 130, h, mine, roots[6])[0] == 1
    for count, height in ((0, h), (129, h), (130, h - 1), (2**h + 1, h)):
        r, out = ac.host_apply_tree(old[rows], new[rows], idx, count, height, mine, roots[6])
        assert r == 0 and (out == ac.CANARY).all(), (count, height)
        assert ac.apply_tree(old[rows], new[rows], idx, count, height, mine, roots[6]) is None, (count, height)


def test_a_count_of_the_right_height_and_the_wrong_parity_gives_another_root(native):
    """The counts matter: c + 1 or c - 1 with the same height and the index still inside passes every check -- the old fold
    never sees a count -- and the new root is not the rebuilt forest's.  What the header says of unauthenticated counts."""
    counts, leaves, trees, indices, stride, old, new, cs, nodes, heights, roots = small_forest()
    want = ac.rebuilt_roots(ac.updated(leaves, counts, trees, indices, new), counts, trees)
    # tree 2 (6 leaves, entry 4 = the left of the last pair) and tree 7 (10 leaves, entry 8): above level 0 their path is the
    # last node of an odd level; told 5 or 7 (9 or 11) leaves the fold duplicates at other levels
    for t, lies in ((2, (5, 7)), (7, (9, 11))):
        for lie in lies:
            assert tree_height(lie) == tree_height(counts[t]) and int(indices[trees == t].max()) < lie
            c = cs.copy()
            c[trees == t] = lie
            r, got = ac.host_apply_forest(old, new, trees, indices, c, stride, nodes, roots)
            assert r == 1, (t, lie)
            assert (got[t] != want[t]).any(), (t, lie)
            others = [u for u in want if u != t]
            assert all((got[u] == want[u]).all() for u in others)
            assert (ac.apply_forest(old, new, trees, indices, c, stride, nodes, roots)[t] == got[t]).all()


def test_a_tree_taller_than_its_count_needs(native):
    """vkmr_hip_reduce_tree_async allows a height above the minimal one: the levels above hold one node, hashed with itself."""
    rng = np.random.default_rng(77)
    for count, height in ((1, 1), (1, 3), (5, 3), (5, 5), (8, 4), (77, 9)):
        leaves = random_leaves(rng, count)
        levels = cpu_levels(leaves, height)
        for idx in ([0], [count - 1], sorted(set([0, count // 2, (count - 1) & ~1, count - 1]))):
            nodes, _ = fm.mc.make_multiproof(lambda l: levels[l], count, height, idx)
            new = random_leaves(rng, len(idx))
            after = leaves.copy()
            after[idx] = new
            want = cpu_levels(after, height)[-1][0]
            r, got = ac.host_apply_tree(leaves[idx], new, idx, count, height, nodes, levels[-1][0])
            assert r == 1 and (got == want).all(), (count, height, idx)
            assert (ac.apply_tree(leaves[idx], new, idx, count, height, nodes, levels[-1][0]) == want).all()


def test_both_level_kernels_hold_one_hash_block_and_the_verifiers_kept_theirs(native):
    from vk_merkle_roots_amd import isa_prio_pass
    expected = isa_prio_pass.EXPECTED_HASH_BLOCKS
    for mine in LEVEL_KERNELS:
        assert expected[mine] == 1
        assert_key_resolves(mine)
    rec = isa_record(native)
    if rec is not None:                    # written by a build that ran the issue pass (tests/test_isa_prio_pass.py covers its absence)
        assert rec["audit"]["block_count_errors"] == [] and rec["audit"]["unclassified"] == []
        blocks = {k: v for k, v in rec["audit"]["blocks"].items() if "apply_" in k}
        assert sorted(blocks.values()) == [1, 1] and all(any(m in k for k in blocks) for m in LEVEL_KERNELS)   # the heights and the commits hold none
        for kernel in ("verify_multiproof_level_kernel", "verify_forest_multiproof_level_kernel") + LEVEL_KERNELS:
            mine = [v for k, v in rec["hash_blocks"].items() if re.match(r"_Z\d+" + kernel + "PK", k)]
            assert mine == [[VERIFIER_HASH_BLOCK]], (kernel, mine)
    assert_no_spills(native, LEVEL_KERNELS, max_vgprs=64, prefix=True)         # 512 registers a lane, 8 wavefronts per SIMD


def test_both_host_functions_under_address_and_undefined_behaviour_sanitizers(native, tmp_path):
    """A stand-alone program (its own main, no Python in the process) over every case table and entry set, once.  The
    sanitizer runtimes are linked statically, so the program needs nothing of the environment it is started in."""
    host = os.path.join(ROOT, "vk_merkle_roots_amd", "csrc", "host")
    exe = str(tmp_path / "apply_host_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "include"), "-I", host,
                           os.path.join(ROOT, "tests", "c", "apply_host_test.cpp"), os.path.join(host, "host_api.cpp"),
                           os.path.join(host, "cpu_sha256d.cpp"), "-o", exe])
    lines, want = [], []
    for name in ac.NON_EMPTY:
        counts = fc.CASES[name]
        rng = np.random.default_rng(len(name) + 17)
        stride = fm.stride_of(sum(counts), max(counts))
        for trees, indices in ac.entry_sets(counts, rng).values():
            entries = [str(int(x)) for pair in zip(trees, indices) for x in pair]
            lines.append(" ".join([str(stride), str(len(counts))] + [str(c) for c in counts] + [str(len(trees))] + entries))
            want.append([len(fm.emitted_positions(counts, trees, indices, stride)[0]), len(set(int(t) for t in trees))])
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)    # the environment as it is
    text = r.stdout.decode()
    assert r.returncode == 0 and "FAIL" not in text and "ERROR" not in text and "runtime error" not in text, text[-3000:]
    assert f"ok: {len(lines)} cases" in text
    got = [[int(x) for x in line.split()] for line in text.splitlines()[: len(lines)]]
    assert got == want
