"""Inclusion proofs as of an earlier count without a GPU: the C ABI's declaration and argument checks
(vkmr_hip_forest_proofs_at_async), the rules of csrc/proofs_at_plan.hpp replayed with values (tests/c/proofs_at_plan_test.cpp, its
own program under AddressSanitizer and UBSan), the CPU twin (vkmr_host_cpu_forest_proofs_at) against the hashlib model of
tests/proofs_at_cases.py byte for byte, against vkmr_host_cpu_fold_proof and against the consistency twin's peaks, and the host
side of MerkleForest.proofs_at / roots_at.  No compute call on a device here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import consistency_cases as cc
import frontier_cases as fr
import proofs_at_cases as pc
from abi_support import Refusals, assert_bound, assert_exported, assert_key_resolves, assert_no_spills, isa_record
from conftest import ROOT
from merkle_model import host_fold, random_counts
from no_device import NoDevice

ENTRY_POINT, NPARAMS = "vkmr_hip_forest_proofs_at_async", 21
HOST_ENTRY_POINT, HOST_NPARAMS = "vkmr_host_cpu_forest_proofs_at", 14
EDGE = "proofs_at_edge_kernel"
KERNELS = ("proofs_at_check_kernel", EDGE, "proofs_at_gather_kernel")
NAMES_OTHER_TESTS_COUNT = ("frontier", "consistency", "mutated", "apply_", "_audit_", "forest_multiproof", "forest_update", "forest_extend", "forest_append",
                           "forest_truncate", "forest_proofs_kernel", "forest_copy", "forest_drop_front")


def test_header_declares_it_and_the_stub_binds_every_argument():
    text = open(os.path.join(ROOT, "include", "vkmr_hip.h")).read()
    from vk_merkle_roots_amd import _abi
    assert_bound(ENTRY_POINT, nparams=NPARAMS, restype=C.c_int)
    assert_bound(HOST_ENTRY_POINT, nparams=HOST_NPARAMS, restype=C.c_int, table=_abi.HOST_SIGNATURES, header="vkmr_host.h")
    # the header says how the proofs are verified, and no longer says that they are not offered
    assert "Not offered: inclusion proofs as of an earlier count" not in text
    block = text[text.index("INCLUSION PROOFS AS OF AN EARLIER COUNT"): text.index(ENTRY_POINT + "(")]
    assert "no new verifier" in block and "vkmr_hip_verify_forest_proofs_async" in block and "trees_dev := epochs_dev" in block
    assert not re.search(r"VKMR_API[^;]*verify\w*proofs_at", text)


def test_libraries_export_them(native):
    assert_exported(native.HIP_LIB, [ENTRY_POINT])
    assert_exported(native.HOST_LIB, [HOST_ENTRY_POINT])


def test_bad_arguments_are_refused_before_any_hip_call(native):
    from vk_merkle_roots_amd import _abi
    lib = _abi.lib()
    d = C.c_void_p(0x1000)                 # never dereferenced: every call below returns before launching anything
    # 0 digests, 1 forest, 2 total, 3 offsets, 4 ntrees, 5 max_count, 6 roots, 7 epoch trees, 8 epoch counts, 9 E, 10 epochs, 11 indices, 12 k, 13 stride,
    # 14 edges, 15 old roots, 16 siblings, 17 heights, 18 status
    proofs = Refusals(lib.vkmr_hip_forest_proofs_at_async, ENTRY_POINT, good=[d, d, 100, d, 8, 50, d, d, d, 5, d, d, 9, 6, d, d, d, d, d])
    proofs.null(0, 1, 3, 6, 7, 8, 10, 11, 14, 15, 16, 17, 18)
    # stride outside 1..63 (the verifier's range), and what vkmr_hip_forest_consistency_async refuses of the forest: stride 5 -- a
    # tree of 50 leaves has six bits --, no max_count, too many leaves
    proofs.changed({13: 0}, {13: 64}, {13: 65}, {13: 5}, {5: 0}, {2: (1 << 58) + 1})
    # k == 0 is a call like any other: the epochs' buffers are still needed
    proofs.changed(*({10: None, 11: None, 12: 0, 16: None, 17: None, i: None} for i in (7, 8, 14, 15, 18)))
    proofs.ok((None, None, 0, None, 0, 0, None, None, None, 0, None, None, 0, 0, None, None, None, None, None),        # no epoch: nothing to do
              (None, None, 0, None, 0, 0, None, None, None, 0, None, None, 7, 0, None, None, None, None, None))
    # and the twin
    import vk_merkle_roots_amd as vk
    host = vk.host_lib()
    z = np.zeros(64, np.uint64)
    p = z.ctypes.data
    twin = host.vkmr_host_cpu_forest_proofs_at
    assert twin(p, p, 1, p, p, 1, p, p, 1, 0, p, p, p, p) == -1 and twin(p, p, 1, p, p, 1, p, p, 1, 64, p, p, p, p) == -1
    assert twin(p, p, 1, None, p, 1, p, p, 1, 8, p, p, p, p) == -1 and twin(p, p, 1, p, p, 1, p, p, 1, 8, p, None, p, p) == -1
    assert twin(p, p, 1, p, p, 1, p, p, 1, 8, p, p, None, p) == -1 and twin(p, None, 1, p, p, 0, p, p, 3, 8, p, p, p, p) == 0


# ---- the replay of the plan ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    return pc.build_proofs_at_plan_exe(tmp_path_factory.mktemp("proofs_at_plan"))


def expect(counts, epochs):
    """(edge cells, node hashes, proofs) of a case, from the rule alone."""
    return (sum(len(pc.edge_levels(c)) for _, c in epochs), sum(pc.hashes(c) for _, c in epochs), sum(c for _, c in epochs))


def test_every_pair_up_to_130_replayed(plan_exe, tmp_path):
    pairs = [(c, c2) for c2 in range(1, 131) for c in range(c2 + 1)]
    cases = [(c2 % 5, max(1, c2.bit_length()) + c % 3, [c2], [(0, c)]) for c, c2 in pairs]         # each alone: the tightest stride, and up to two cells more
    counts = cc.square_counts(130)                                                                 # an empty tree in front of every seventh
    trees, old = cc.every_pair(counts)
    cases.append((7, 8, counts, list(zip(trees.tolist(), old.tolist()))))                          # and side by side in one forest at an odd offset
    cases.append((1, 63, counts, list(zip(trees.tolist()[::-1], old.tolist()[::-1]))))             # the widest row, the epochs backwards
    got = pc.plan_replay(plan_exe, tmp_path, cases)
    for (c, c2), (cells, hashes, proofs, status) in zip(pairs, got):
        assert status == 0 and (cells, hashes, proofs) == expect([c2], [(0, c)]) and hashes <= pc.tree_height(max(c, 1)), (c, c2)
    assert sum(g[2] for g in got[: len(pairs)]) == 374660                                          # every leaf of every pair 1 <= c <= c2
    for g in got[-2:]:
        assert g == tuple(sum(x[i] for x in got[: len(pairs)]) for i in range(3)) + (0,)


def test_a_thousand_random_forests_replayed(plan_exe, tmp_path):
    rng = np.random.default_rng(20265)
    cases = []
    while len(cases) < 1000:
        counts = random_counts(rng, 9000)
        if not counts:
            continue
        stride = int(rng.integers(max(max(counts).bit_length(), 1), 64))
        epochs = []
        for _ in range(int(rng.integers(1, 12))):
            t = int(rng.integers(0, len(counts)))
            n = counts[t]
            kind = int(rng.integers(0, 4))
            c = n if kind == 0 else int(rng.integers(0, n + 1)) if kind == 1 else min(n, 1 << int(rng.integers(0, 14))) if kind == 2 else max(0, n - int(rng.integers(0, 3)))
            epochs.append((t, c))
        cases.append((int(rng.integers(0, 70)) * int(rng.integers(0, 2)), stride, counts, epochs))
    got = pc.plan_replay(plan_exe, tmp_path, cases)
    for (_, _, counts, epochs), g in zip(cases, got):
        assert g == expect(counts, epochs) + (0,)


def test_the_replay_reports_the_refusals(plan_exe, tmp_path):
    cases = [(3, stride, pc.REFUSAL_COUNTS, list(zip(trees, old))) for _, _, trees, old, stride, _ in pc.REFUSALS]
    got = pc.plan_replay(plan_exe, tmp_path, cases)
    assert [g[3] for g in got] == [r[1] for r in pc.REFUSALS] and all(g[:3] == (0, 0, 0) for g in got)


# ---- the CPU twin against the model ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def whole_square(native):
    """Every epoch 1 <= c <= count of every tree of square(130), a few of c == 0, every leaf of every epoch, shuffled, some bad
    queries among them: the twin's answer between canaries, and the model's."""
    forest = pc.square()
    assert int(forest.offsets[0]) > 0 and forest.counts.count(0) == 18
    epoch_trees, epoch_counts = pc.every_epoch(forest.counts)
    empty = [t for t, n in enumerate(forest.counts) if n == 0][:3]
    epoch_trees = np.concatenate([epoch_trees, np.array(empty + [5, 130], np.uint32)])
    epoch_counts = np.concatenate([epoch_counts, np.zeros(len(empty) + 2, np.uint64)])               # c == 0 of empty trees and of trees with leaves
    rng = np.random.default_rng(510)
    order = rng.permutation(epoch_trees.shape[0])                                                  # out of order
    epoch_trees, epoch_counts = epoch_trees[order], epoch_counts[order]
    E = int(epoch_trees.shape[0])
    epochs, indices = pc.every_leaf(epoch_counts)
    assert epochs.shape[0] == 374660
    bad = 200
    epochs = np.concatenate([epochs, rng.integers(E, 1 << 32, size=bad, dtype=np.uint64).astype(np.uint32), rng.integers(0, E, size=2 * bad).astype(np.uint32)])
    indices = np.concatenate([indices, rng.integers(0, 4, size=bad).astype(np.uint64),
                              epoch_counts[epochs[-2 * bad:].astype(np.int64)] + rng.integers(0, 2, size=2 * bad).astype(np.uint64) * np.uint64(1 << 45)])
    order = rng.permutation(epochs.shape[0])
    epochs, indices = epochs[order], indices[order]
    got = pc.host_proofs_at(forest.leaves, forest.offsets, epoch_trees, epoch_counts, epochs, indices, stride=8)
    want = pc.forest_model(forest, epoch_trees, epoch_counts, epochs, indices, stride=8)
    return forest, epoch_trees, epoch_counts, epochs, indices, got, want


def test_every_leaf_of_every_pair_up_to_130_in_one_batched_call(whole_square):
    forest, epoch_trees, epoch_counts, epochs, indices, got, want = whole_square
    assert got[0] == 0
    for what, a, b in zip(("edges", "old roots", "siblings", "heights"), got[1:], want):          # byte for byte: no canary is left, every cell is the model's
        assert a.shape == b.shape and (a == b).all(), (what, np.nonzero((a != b).reshape(a.shape[0], -1).any(axis=1))[0][:8])
    _, edges, old_roots, siblings, heights = got
    for e in range(0, epoch_trees.shape[0], 7):                                                    # the old roots: the trees built from the first c leaves
        assert (old_roots[e] == forest.old_root(int(epoch_trees[e]), int(epoch_counts[e]))).all(), e
    for e, c in enumerate(epoch_counts.tolist()):                                                  # the written set of the edge row
        assert [l for l in range(8) if edges[e, l].any()] == pc.edge_levels(c), (e, c)


def test_zeros_above_the_height_and_bad_queries_get_height_0(whole_square):
    _, epoch_trees, epoch_counts, epochs, indices, got, _ = whole_square
    _, _, _, siblings, heights = got
    E = epoch_trees.shape[0]
    inside = epochs < E
    c = np.zeros(epochs.shape[0], np.uint64)
    c[inside] = epoch_counts[epochs[inside].astype(np.int64)]
    good = inside & (indices < c)
    assert int((~good).sum()) == 600 and int((~inside).sum()) == 200
    assert (heights[~good] == 0).all() and not siblings[~good].any()
    assert (heights[good] == [pc.tree_height(int(x)) for x in c[good]]).all()
    above = np.arange(8)[None, :] >= heights[:, None]
    assert not siblings[above].any() and siblings[~above].reshape(-1, 8).any(axis=1).all()          # zero above the height, a digest below it


def test_the_twins_proofs_fold_to_the_old_roots(whole_square):
    forest, epoch_trees, epoch_counts, epochs, indices, got, _ = whole_square
    _, _, old_roots, siblings, heights = got
    good = np.nonzero(heights)[0]
    for q in good[:: max(1, good.shape[0] // 1500)]:                                               # vkmr_host_cpu_fold_proof: a sample of every kind of epoch
        e = int(epochs[q])
        leaf = forest.tree(int(epoch_trees[e]))[int(indices[q])]
        assert (host_fold(leaf, int(indices[q]), siblings[q], int(heights[q])) == old_roots[e]).all(), (q, e)


def test_the_old_roots_are_the_consistency_peaks_walked_to_their_root(whole_square):
    forest, epoch_trees, epoch_counts, _, _, got, _ = whole_square
    status, new_counts, peaks, _ = cc.host_gather(forest.leaves, forest.offsets, epoch_trees, epoch_counts, stride=8)
    assert status == 0
    rc, walked = fr.host_roots(epoch_counts, peaks)                                                # vkmr_host_cpu_frontier_roots
    assert rc == 0 and (walked == got[2]).all()


def test_no_query(native):
    forest = pc.Forest([9, 0, 130, 64], seed=511, first=1)
    epoch_trees, epoch_counts = [2, 0, 2, 3, 1, 3, 2], [130, 9, 64, 64, 0, 1, 77]
    status, edges, old_roots, siblings, heights = pc.host_proofs_at(forest.leaves, forest.offsets, epoch_trees, epoch_counts, [], [], stride=8)
    want = pc.forest_model(forest, epoch_trees, epoch_counts, [], [], stride=8)
    assert status == 0 and (edges == want[0]).all() and (old_roots == want[1]).all() and siblings.shape == (0, 8, 8) and heights.shape == (0,)
    assert all((old_roots[e] == forest.old_root(t, c)).all() for e, (t, c) in enumerate(zip(epoch_trees, epoch_counts)))
    assert (old_roots[0] == forest.roots()[2]).all() and not old_roots[4].any()                   # c == c2: the root now; c == 0: zero
    assert not edges[[2, 3, 4]].any()                                                              # 64 is a power of two, 0 is not begun: no edge
    assert [[l for l in range(8) if edges[e, l].any()] for e in (0, 1, 5, 6)] == [[2, 3, 4, 5, 6, 7], [1, 2, 3], [], [1, 2, 3, 4, 5, 6]]
    assert [pc.edge_levels(c) for c in (130, 9, 1, 77)] == [[2, 3, 4, 5, 6, 7], [1, 2, 3], [], [1, 2, 3, 4, 5, 6]]


@pytest.mark.parametrize("what,status,trees,old,stride,max_count", pc.REFUSALS, ids=[r[0] for r in pc.REFUSALS])   # each alone, and all three
def test_every_status_bit_is_reported_and_nothing_written(native, what, status, trees, old, stride, max_count):
    import vk_merkle_roots_amd as vk
    forest = pc.Forest(pc.REFUSAL_COUNTS, seed=414)
    got = pc.host_proofs_at(forest.leaves, forest.offsets, trees, old, [0, 0, len(trees)], [0, 1, 0], stride=stride)
    assert got[0] == status, what
    assert all((a == pc.CANARY).all() for a in got[1:4]) and (got[4] == pc.HEIGHT_FILL).all()      # the canaries untouched
    for bit in range(3):
        assert (f"bit {bit}:" in vk.consistency_status_text(status)) == bool(status >> bit & 1)
    # and the same call with the fault taken out goes through
    fine = pc.host_proofs_at(forest.leaves, forest.offsets, [0, 3, 2], [5, 100, 9], [0, 1, 3], [4, 99, 0], stride=8)
    assert fine[0] == 0 and fine[4].tolist() == [3, 7, 0] and not (fine[1] == pc.CANARY).all(axis=2).any()


# ---- the Python layer ------------------------------------------------------------------------------------------------------------------
def test_the_handle_refuses_on_the_host_and_answers_no_epoch_without_a_device(native):
    import vk_merkle_roots_amd as vk
    forest = vk.MerkleForest(NoDevice(), None, 16, [4, 5, 7], None, 7, None, None)
    with pytest.raises(ValueError):
        forest.proofs_at([4, 5], [0], [0])                   # one old count per tree
    with pytest.raises(ValueError):
        forest.proofs_at([4, 5, 7], [0, 1], [0])             # one epoch per index
    with pytest.raises(ValueError):
        forest.proofs_at([4, 5, 7], [0], [0], trees=[0, 1])
    siblings, heights, old_roots = forest.proofs_at([], [0, 0], [1, 2], trees=[])
    assert siblings.shape == (2, 3, 8) and not siblings.any() and heights.tolist() == [0, 0] and old_roots.shape == (0, 8)
    assert forest.roots_at([], trees=[]).shape == (0, 8)


def test_the_wrapper_on_raw_buffers_is_not_named_async(native):
    import vk_merkle_roots_amd as vk
    assert callable(vk.HipDevice.forest_proofs_at_enqueue) and callable(vk.MerkleForest.proofs_at) and callable(vk.MerkleForest.roots_at)
    assert not any("proofs_at" in n and n.endswith("_async") for n in dir(vk.HipDevice))


def test_the_kernel_key_resolves_to_itself_and_the_build_lists_it(native):
    from vk_merkle_roots_amd import isa_prio_pass
    keys = isa_prio_pass.EXPECTED_HASH_BLOCKS
    assert keys[EDGE] == 1
    assert_key_resolves(EDGE)
    for name in KERNELS:
        assert name == EDGE or not any(k in name for k in keys), name                              # no hash expected in the others
        assert not any(s in name for s in NAMES_OTHER_TESTS_COUNT), name
    text = open(os.path.join(ROOT, "vk_merkle_roots_amd", "csrc", "proofs_at_kernels.hpp")).read()
    assert len(re.findall(r"\bhash_pair\(", text)) == 1 and sorted(re.findall(r"void (\w+_kernel)\(", text)) == sorted(KERNELS)
    from vk_merkle_roots_amd import build
    assert os.path.join(build.CSRC, "proofs_at_plan.hpp") in build.host_headers()
    rec = isa_record(native)
    if rec is not None:                    # written by a build that ran the issue pass (tests/test_isa_prio_pass.py covers its absence)
        assert rec["audit"]["block_count_errors"] == [] and rec["audit"]["unclassified"] == []
        mine = {k: v for k, v in rec["audit"]["blocks"].items() if "proofs_at" in k}
        assert list(mine.values()) == [1] and EDGE in next(iter(mine))
    assert_no_spills(native, KERNELS)
