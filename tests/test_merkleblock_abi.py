"""Partial Merkle trees in BIP37 order without a GPU: the C ABI's declarations and argument checks
(vkmr_hip_forest_merkleblocks_async, vkmr_hip_tree_merkleblock_async), the closed form of csrc/merkleblock_plan.hpp replayed with
values against a recursive walk (tests/c/merkleblock_plan_test.cpp, its own program under AddressSanitizer and UBSan), the CPU
twin (vkmr_host_cpu_forest_merkleblocks) against the hashlib model of tests/merkleblock_cases.py byte for byte, the receiver's
side (vkmr_host_cpu_merkleblock_extract) and its refusals, the wire form, and the host side of the Python handles.  No compute
call on a device here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import forest_multiproof_cases as fm
import merkleblock_cases as mb
from abi_support import Refusals, assert_bound, assert_exported, assert_no_spills, isa_record
from conftest import ROOT
from merkle_model import cpu_levels, node, random_counts, random_leaves
from no_device import NoDevice

FOREST, TREE = "vkmr_hip_forest_merkleblocks_async", "vkmr_hip_tree_merkleblock_async"
SIZES = ("vkmr_hip_forest_merkleblocks_max_hashes", "vkmr_hip_forest_merkleblocks_max_flag_bytes", "vkmr_hip_forest_merkleblocks_scratch_bytes")
HOST = {"vkmr_host_cpu_forest_merkleblocks": 16, "vkmr_host_cpu_merkleblock_extract": 9}
KERNELS = ("merkleblock_tree_sums_kernel", "merkleblock_forest_sums_kernel", "merkleblock_starts_kernel", "merkleblock_tree_places_kernel",
           "merkleblock_forest_places_kernel", "merkleblock_byte_sums_kernel", "merkleblock_byte_starts_kernel", "merkleblock_byte_places_kernel",
           "merkleblock_zero_kernel", "merkleblock_tree_emit_kernel", "merkleblock_forest_emit_kernel", "merkleblock_flags_kernel")
NAMES_OTHER_TESTS_COUNT = ("frontier", "consistency", "mutated", "apply_", "_audit_", "forest_multiproof", "forest_update", "forest_extend", "forest_append",
                           "forest_truncate", "forest_proofs_kernel", "forest_copy", "forest_drop_front", "verify_", "proofs_at", "multiproof_", "_diff_",
                           "find_", "sort_")


# ---- declaration and binding -------------------------------------------------------------------------------------------------------
def test_header_declares_them_and_the_stub_binds_every_argument():
    from vk_merkle_roots_amd import _abi
    assert_bound(FOREST, nparams=22, restype=C.c_int)
    assert_bound(TREE, nparams=19, restype=C.c_int)
    assert_bound(SIZES[0], nparams=4, scalars=[C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32], restype=C.c_size_t)
    assert_bound(SIZES[1], nparams=4, scalars=[C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32], restype=C.c_size_t)
    assert_bound(SIZES[2], nparams=2, scalars=[C.c_uint32, C.c_uint32], restype=C.c_size_t)
    for name, n in HOST.items():
        assert_bound(name, nparams=n, restype=C.c_int, table=_abi.HOST_SIGNATURES, header="vkmr_host.h")
    text = open(os.path.join(ROOT, "include", "vkmr_hip.h")).read()
    block = text[text.index("PARTIAL MERKLE TREES IN BIP37 ORDER"): text.index(SIZES[0] + "(")]
    for said in ("THE LONE LEAF", "TraverseAndBuild", "bit i & 7 of byte i >> 3", "bit 2", "atomicOr", "never a launch per tree", "Not offered: a batched"):
        assert said in block, said


def test_libraries_export_them(native):
    assert_exported(native.HIP_LIB, [FOREST, TREE, *SIZES])
    assert_exported(native.HOST_LIB, list(HOST))


def test_bad_arguments_are_refused_before_any_hip_call(native):
    from vk_merkle_roots_amd import _abi
    lib = _abi.lib()
    d = C.c_void_p(0x1000)                 # never dereferenced: every call below returns before launching anything
    # 0 digests, 1 forest, 2 total, 3 offsets, 4 ntrees, 5 max_count, 6 trees, 7 indices, 8 k, 9 scratch, 10 block trees, 11 block counts,
    # 12 bit counts, 13 hash starts, 14 byte starts, 15 hashes, 16 hash capacity, 17 flags, 18 flag capacity, 19 info
    forest = Refusals(lib.vkmr_hip_forest_merkleblocks_async, FOREST, good=[d, d, 100, d, 8, 50, d, d, 9, d, d, d, d, d, d, d, 70, d, 40, d])
    forest.null(0, 1, 3, 6, 7, 9, 10, 11, 12, 13, 14, 15, 17, 19)
    # what the multiproof gather refuses: no tree, no leaf, no max_count, too many leaves, scratch off the 16-byte grid; and flags off the 4-byte grid
    forest.changed({4: 0}, {2: 0}, {5: 0}, {2: (1 << 58) + 1}, {9: C.c_void_p(0x1008)}, {17: C.c_void_p(0x1002)})
    forest.ok([None] * 2 + [0, None, 0, 0, None, None, 0] + [None] * 7 + [0, None, 0, None],      # k == 0: nothing to do, whatever else
              [d, d, 100, d, 8, 50, d, d, 9, d, d, d, d, d, d, None, 0, None, 0, d][:8] + [0] + [None] * 7 + [0, None, 0, None])
    # 0 digests, 1 tree, 2 count, 3 height, 4 indices, 5 k, 6 scratch, 7..11 the per-block arrays, 12 hashes, 13 capacity, 14 flags, 15 capacity, 16 info
    tree = Refusals(lib.vkmr_hip_tree_merkleblock_async, TREE, good=[d, d, 100, 7, d, 9, d, d, d, d, d, d, d, 70, d, 40, d])
    tree.null(0, 1, 4, 6, 7, 8, 9, 10, 11, 12, 14, 16)
    tree.changed({2: 0}, {3: 0}, {3: 6}, {3: 8}, {3: 64}, {2: 1, 3: 0}, {6: C.c_void_p(0x1008)}, {14: C.c_void_p(0x1001)})
    tree.ok([None, None, 0, 0, None, 0, None] + [None] * 6 + [0, None, 0, None])
    assert lib.vkmr_hip_forest_merkleblocks_scratch_bytes(0, 8) == 0 and lib.vkmr_hip_forest_merkleblocks_scratch_bytes(5, 64) == 0
    assert lib.vkmr_hip_forest_merkleblocks_scratch_bytes(5, 8) % 16 == 0 and lib.vkmr_hip_forest_merkleblocks_scratch_bytes(5, 8) > 0
    assert lib.vkmr_hip_forest_merkleblocks_max_hashes(0, 3, 9, 4) == 0 and lib.vkmr_hip_forest_merkleblocks_max_flag_bytes(9, 0, 9, 4) == 0
    # and the twins
    import vk_merkle_roots_amd as vk
    host = vk.host_lib()
    z = np.zeros(64, np.uint64)
    p = z.ctypes.data
    twin = host.vkmr_host_cpu_forest_merkleblocks
    good = [p, p, 1, p, p, 1, p, p, p, p, p, p, 4, p, 4, p]
    for i in (0, 1, 3, 4, 6, 7, 8, 9, 10, 11, 13, 15):
        assert twin(*[None if j == i else a for j, a in enumerate(good)]) == -1, i
    assert twin(*[0 if j == 5 else a for j, a in enumerate(good)]) == -1                       # k == 0
    down = np.array([5, 3], np.uint64)
    assert twin(*[down.ctypes.data if j == 1 else a for j, a in enumerate(good)]) == -2        # the offsets decrease


# ---- the replay of the plan --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    return mb.build_merkleblock_plan_exe(tmp_path_factory.mktemp("merkleblock_plan"))


def check_replay(plan_exe, tmp_path, cases):
    got = mb.plan_replay(plan_exe, tmp_path, cases)
    for (_, counts, entries), g in zip(cases, got):
        assert g == mb.expect(counts, entries), (counts, entries[:8], g)
    return got


def test_every_subset_of_every_count_up_to_11_replayed(plan_exe, tmp_path):
    cases = [(c, [c], [(0, i) for i in range(c) if m >> i & 1]) for c in range(1, 12) for m in range(1, 1 << c)]
    assert len(cases) == 4083
    check_replay(plan_exe, tmp_path, cases)


def test_every_single_leaf_and_adjacent_pair_up_to_130_replayed(plan_exe, tmp_path):
    cases = [(c, [c], [(0, i)]) for c in range(1, 131) for i in range(c)]
    cases += [(c, [c], [(0, i), (0, i + 1)]) for c in range(2, 131) for i in range(c - 1)]
    # and side by side in one forest, empty trees in between: every leaf's own tree would be a forest too large, so leaf j of every tree
    counts = mb.square_counts(130)
    for j in (0, 1, 2, 63, 64, 65, 128, 129):
        cases.append((130, counts, [(t, j) for t, c in enumerate(counts) if j < c]))
    cases.append((1 << 40, counts, [(t, i) for t, c in enumerate(counts) for i in range(c)]))   # every leaf: no hash but the leaves
    got = check_replay(plan_exe, tmp_path, cases)
    assert got[-1][2] == sum(counts)


def test_a_thousand_random_forests_replayed(plan_exe, tmp_path):
    rng = np.random.default_rng(20271)
    cases = []
    while len(cases) < 1000:
        counts = random_counts(rng, 9000)
        if not counts or not any(counts):
            continue
        share = float(rng.choice([0.002, 0.02, 0.3, 0.9]))
        t, i = mb.random_entries(counts, rng, share)
        max_count = max(counts) if rng.integers(0, 2) else sum(counts) + int(rng.integers(0, 1000))
        cases.append((max_count, counts, list(zip(t.tolist(), i.tolist()))))
    check_replay(plan_exe, tmp_path, cases)


# ---- the CPU twin against the model ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def square_sets(native):
    """The 0..130 forest (empty trees in between, a nonzero first offset) and its entry sets, each with the twin's answer and the
    model's."""
    forest = mb.square()
    assert int(forest.offsets[0]) > 0 and forest.counts.count(0) == 18
    rng = np.random.default_rng(711)
    sets = {"every leaf": mb.every_leaf(forest.counts), "one in ten": mb.random_entries(forest.counts, rng, 0.1),
            "half": mb.random_entries(forest.counts, rng, 0.5)}
    for j, e in enumerate(mb.single_leaf_batches(forest.counts)):
        sets[f"leaf {j} of every tree"] = e
    out = {}
    for name, (trees, idx) in sets.items():
        rc, got = mb.host_merkleblocks(forest.leaves, forest.offsets, trees, idx)
        out[name] = (trees, idx, rc, got, mb.model(forest, trees, idx))
    return forest, out


def test_the_twin_is_the_model_byte_for_byte(square_sets):
    _, sets = square_sets
    assert len(sets) == 133
    for name, (_, _, rc, got, want) in sets.items():
        assert rc == 0, name
        mb.assert_outputs(got, want, name)


def test_the_two_worked_cases(native):
    leaves = random_leaves(np.random.default_rng(7), 7)
    lv = cpu_levels(leaves)
    for matched, byte, cells in (([5], 0x2D, [(2, 0), (0, 4), (0, 5), (1, 3)]), ([6], 0x35, [(2, 0), (1, 2), (0, 6)])):
        rc, out = mb.host_merkleblocks(leaves, [0, 7], [0], matched)
        n = len(cells)
        assert rc == 0 and out[7][:4].tolist() == [0, 1, n, 1] and out[6][0] == byte and out[2][0] == (7 if matched == [5] else 6)
        assert (out[5][:n] == np.stack([lv[l][p] for l, p in cells])).all()
        assert mb.walk(7, matched) == ([int(x) for x in f"{byte:08b}"[::-1][: out[2][0]]], cells)


def test_the_lone_leaf_has_two_flags_and_one_hash(native):
    leaf = random_leaves(np.random.default_rng(8), 1)
    rc, out = mb.host_merkleblocks(leaf, [0, 1], [0], [0])
    assert rc == 0 and out[2][0] == 2 and out[6][0] == 0x03 and out[7][:4].tolist() == [0, 1, 1, 1] and (out[5][0] == leaf[0]).all()
    code, root, idx, leaves = mb.host_extract(1, leaf, bytes([0x03]))
    assert code == 0 and (root == node(leaf[0], leaf[0])).all() and idx.tolist() == [0]
    code, root, idx, _ = mb.host_extract(1, leaf, bytes([0x01]))                                 # Bitcoin's one flag reads here as "no match below the root"
    assert code == 0 and (root == node(leaf[0], leaf[0])).all() and idx.tolist() == []


def test_hashes_are_the_leaves_and_the_multiproof_nodes_minus_the_edge_nodes(square_sets):
    forest, sets = square_sets
    for name in ("one in ten", "half", "every leaf", "leaf 0 of every tree", "leaf 64 of every tree"):
        trees, idx, _, got, _ = sets[name]
        rc, nodes, heights, info = fm.host_make(forest.leaves, forest.offsets, trees, idx, 8)     # vkmr_host_cpu_forest_multiproof
        assert rc == 0
        pos, _ = fm.emitted_positions(forest.counts, trees, idx, 8)
        groups = mb.by_tree(trees, idx)
        A = {(t, l): set(i >> l for i in ix) for t, ix in groups.items() for l in range(8)}
        at_edge = [(l, t, c) for l, t, c in pos if c in A[t, l]]                                  # the node put in as its own sibling
        assert int(got[7][2]) == len(idx) + len(pos) - len(at_edge), name
        for b, t in enumerate(got[0][: int(got[7][1])].tolist()):
            mine = {(l, c) for l, tt, c in pos if tt == t and c not in A[t, l]} | {(0, i) for i in groups[t]}
            assert mine == set(mb.walk(forest.counts[t], groups[t])[1]), (name, t)
        carried = {nodes[j].tobytes() for j, (l, t, c) in enumerate(pos) if c not in A[t, l]}        # and the cells themselves
        assert carried <= {h.tobytes() for h in got[5][: int(got[7][2])]}, name


@pytest.mark.parametrize("what", ["tree outside", "index outside", "empty tree", "out of order", "repeated", "both"])
def test_status_bits_0_and_1_with_nothing_written(native, what):
    forest = mb.Forest([5, 0, 9, 129], seed=414)
    trees, idx, status = {"tree outside": ([0, 4], [1, 0], 1), "index outside": ([0, 2], [1, 9], 1), "empty tree": ([0, 1], [1, 0], 1),
                          "out of order": ([2, 0], [1, 1], 2), "repeated": ([2, 2, 3], [4, 4, 0], 2), "both": ([3, 3], [500, 2], 3)}[what]
    rc, out = mb.host_merkleblocks(forest.leaves, forest.offsets, trees, idx)
    assert rc == status and int(out[7][0]) == status
    out[7][0] = mb.CANARY64
    mb.assert_untouched(out)
    import vk_merkle_roots_amd as vk
    for bit in range(3):
        assert (f"bit {bit}:" in vk.merkleblocks_status_text(status)) == bool(status >> bit & 1)


def test_bit_2_writes_the_rows_and_the_totals_and_no_hash_or_flag(native):
    forest = mb.Forest([5, 0, 9, 129], seed=415)
    trees, idx = mb.sorted_entries([(0, 1), (2, 3), (2, 8), (3, 77), (3, 128)])
    want = mb.model(forest, trees, idx)
    n, m = int(want[7][2]), int(want[7][3])
    for hc, fc in ((n - 1, m), (n, m - 1), (0, 0)):
        rc, out = mb.host_merkleblocks(forest.leaves, forest.offsets, trees, idx, hash_capacity=hc, flag_capacity=fc)
        assert rc == 4 and out[7][:4].tolist() == [4, 3, n, m]
        mb.assert_untouched(out, upto=(5, 6))
        for i in range(5):
            assert (out[i][: want[i].shape[0]] == want[i]).all()
        rc, out = mb.host_merkleblocks(forest.leaves, forest.offsets, trees, idx, hash_capacity=int(out[7][2]), flag_capacity=int(out[7][3]))
        assert rc == 0
        mb.assert_outputs(out, want)


# ---- extract -----------------------------------------------------------------------------------------------------------------------
def blocks_of(out):
    B = int(out[7][1])
    for b in range(B):
        yield (int(out[0][b]), int(out[1][b]), out[5][int(out[3][b]): int(out[3][b + 1])], out[6][int(out[4][b]): int(out[4][b + 1])].tobytes())


def test_extract_gives_the_forests_roots_and_the_entries(square_sets):
    forest, sets = square_sets
    roots = forest.roots()
    checked = 0
    for name, (trees, idx, _, got, _) in sets.items():
        groups = mb.by_tree(trees, idx)
        for t, c, hashes, flags in blocks_of(got):
            code, root, found, leaves = mb.host_extract(c, hashes, flags)
            assert code == 0 and (root == roots[t]).all() and found.tolist() == groups[t], (name, t)
            assert (leaves == forest.tree(t)[groups[t]]).all()
            if checked % 40 == 0:                                       # the restated receiver agrees
                mcode, mroot, midx, _ = mb.extract(c, hashes, flags)
                assert mcode == 0 and (mroot == root).all() and midx == groups[t]
            checked += 1
    assert checked == sum(len(mb.by_tree(t, i)) for t, i, _, _, _ in sets.values()) > 8000     # every block of every set the twin test runs


def test_every_refusal_of_the_extract_by_one_corrupted_field(native):
    R = mb.EXTRACT_REFUSALS
    leaves = random_leaves(np.random.default_rng(9), 7)
    rc, out = mb.host_merkleblocks(leaves, [0, 7], [0, 0], [2, 5])
    assert rc == 0
    (_, c, hashes, flags), = blocks_of(out)
    bits = int(out[2][0])
    assert mb.host_extract(c, hashes, flags)[0] == 0 and len(flags) == 2 and bits > 8
    assert mb.host_extract(0, hashes, flags)[0] == R["count == 0"]
    assert mb.host_extract(len(hashes) - 1, hashes, flags)[0] == R["more hashes than leaves"]
    many = random_leaves(np.random.default_rng(10), 17)
    assert mb.host_extract(40, many, flags)[0] == R["fewer flag bits than hashes"]
    assert mb.host_extract(c, hashes, flags[:1])[0] == R["read past the end"]                  # a flag past the end
    assert mb.host_extract(c, hashes[:-1], flags)[0] == R["read past the end"]                 # a hash past the end
    assert mb.host_extract(c, np.concatenate([hashes, many[:1]]), flags)[0] == R["hashes left over"]
    assert mb.host_extract(c, hashes, flags + b"\0")[0] == R["flag bytes left over"]
    for code, (got, want) in {"model": (mb.extract(c, hashes, flags + b"\0")[0], R["flag bytes left over"]),
                              "model 2": (mb.extract(c, hashes[:-1], flags)[0], R["read past the end"])}.items():
        assert got == want, code
    import vk_merkle_roots_amd as vk
    host = vk.host_lib()
    z = np.zeros(64, np.uint64)
    p = z.ctypes.data
    for i in (1, 3, 5, 6, 7, 8):
        args = [7, p, 2, p, 1, p, p, p, p]
        args[i] = None
        assert host.vkmr_host_cpu_merkleblock_extract(*args) == R["null pointer"], i
    # padding bits are not inspected, as in Core
    padded = bytearray(flags)
    padded[-1] |= 0x80
    assert bits % 8 and mb.host_extract(c, hashes, bytes(padded))[0] == 0


def test_a_flipped_hash_gives_another_root(native):
    forest = mb.Forest([37], seed=11, first=0)
    rc, out = mb.host_merkleblocks(forest.leaves, forest.offsets, [0, 0, 0], [3, 20, 36])
    (_, c, hashes, flags), = blocks_of(out)
    _, root, _, _ = mb.host_extract(c, hashes, flags)
    assert (root == forest.roots()[0]).all()
    for j in range(hashes.shape[0]):
        bad = hashes.copy()
        bad[j, j % 8] ^= np.uint32(1 << (j % 32))
        code, other, _, _ = mb.host_extract(c, bad, flags)
        assert code == 0 and (other != root).any(), j


def test_of_two_trees_with_one_root_only_the_mutated_one_is_refused(native):
    a, b, c = random_leaves(np.random.default_rng(12), 3)
    three, four = np.stack([a, b, c]), np.stack([a, b, c, c])
    assert (cpu_levels(three)[-1][0] == cpu_levels(four)[-1][0]).all()                            # CVE-2012-2459
    rc, out = mb.host_merkleblocks(three, [0, 3], [0], [2])
    (_, n, hashes, flags), = blocks_of(out)
    code, root, idx, _ = mb.host_extract(n, hashes, flags)
    assert code == 0 and idx.tolist() == [2] and (root == cpu_levels(three)[-1][0]).all()
    rc, out = mb.host_merkleblocks(four, [0, 4], [0], [3])
    (_, n, hashes, flags), = blocks_of(out)
    assert n == 4 and mb.walk(4, [3])[1][-1] == (0, 3)
    assert mb.host_extract(n, hashes, flags)[0] == mb.EXTRACT_REFUSALS["equal children"] == mb.extract(n, hashes, flags)[0]


# ---- the wire form and the Python layer --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nhashes", [0, 1, 252, 253, 254, 70000])
def test_serialize_then_parse_round_trips(native, nhashes):
    import vk_merkle_roots_amd as vk
    rng = np.random.default_rng(nhashes)
    hashes, flags = random_leaves(rng, nhashes), rng.integers(0, 256, size=(nhashes * 2 + 7) // 8 + (nhashes == 252), dtype=np.uint8)
    tree = vk.PartialMerkleTree(max(nhashes, 1) * 3, hashes, flags)
    wire = tree.serialize()
    prefix = 1 if nhashes < 253 else 3 if nhashes < 65536 else 5
    assert wire[:4] == (max(nhashes, 1) * 3).to_bytes(4, "little") and len(wire) == 4 + prefix + 32 * nhashes + (1 if flags.size < 253 else 3) + flags.size
    if nhashes == 253:
        assert wire[4:7] == bytes([253, 253, 0])
    if nhashes:
        assert wire[4 + prefix: 8 + prefix] == int(hashes[0, 0]).to_bytes(4, "big")              # digest_hex's byte order
    back = vk.PartialMerkleTree.parse(wire)
    assert back.count == tree.count and (back.hashes == hashes).all() and (back.flags == flags).all() and back.serialize() == wire
    with pytest.raises(ValueError):
        vk.PartialMerkleTree.parse(wire + b"\0")
    for cut in (1, 2, 3, 5, len(wire) - 1):
        if cut < len(wire):
            with pytest.raises(ValueError):
                vk.PartialMerkleTree.parse(wire[:cut])


def test_the_wire_form_refuses_a_count_of_2_to_the_32(native):
    import vk_merkle_roots_amd as vk
    leaf = random_leaves(np.random.default_rng(1), 1)
    assert len(vk.PartialMerkleTree((1 << 32) - 1, leaf, b"\x03").serialize()) == 4 + 1 + 32 + 1 + 1
    with pytest.raises(ValueError):
        vk.PartialMerkleTree(1 << 32, leaf, b"\x03").serialize()


def test_a_serialized_block_extracts_after_parsing(native):
    import vk_merkle_roots_amd as vk
    forest = mb.Forest([600], seed=13, first=0)
    idx = sorted(set(np.random.default_rng(14).integers(0, 600, size=400).tolist()))
    rc, out = mb.host_merkleblocks(forest.leaves, forest.offsets, [0] * len(idx), idx)
    B = int(out[7][1])
    blocks = vk.PartialMerkleTrees(out[0][:B], out[1][:B], out[2][:B], out[3][: B + 1], out[4][: B + 1], out[5][: int(out[7][2])], out[6][: int(out[7][3])])
    assert len(blocks) == 1 and blocks[0].hashes.shape[0] >= 253                                  # the three-byte CompactSize on a real block
    with pytest.raises(IndexError):
        blocks[1]
    root, found, leaves = vk.PartialMerkleTree.parse(blocks[-1].serialize()).extract()
    assert (root == forest.roots()[0]).all() and found.tolist() == idx and (leaves == forest.leaves[idx]).all()
    broken = vk.PartialMerkleTree(600, blocks[0].hashes[:-1], blocks[0].flags)
    with pytest.raises(ValueError, match="past the end"):
        broken.extract()


def test_the_handles_refuse_on_the_host_without_a_device(native):
    import vk_merkle_roots_amd as vk
    forest = vk.MerkleForest(NoDevice(), None, 16, [4, 5, 7], None, 7, None, None)
    with pytest.raises(ValueError):
        forest.merkleblocks([0, 1], [0])                     # one tree per index
    with pytest.raises(ValueError):
        forest.merkleblocks([], [])                          # no entry
    with pytest.raises(IndexError):
        forest.merkleblocks([3], [0])
    with pytest.raises(IndexError):
        forest.merkleblocks([1], [5])
    with pytest.raises(ValueError):
        forest.merkleblocks_of(np.zeros((0, 8), np.uint32))
    tree = vk.MerkleTree(NoDevice(), None, 5, 3, None)
    with pytest.raises(IndexError):
        tree.merkleblock([5])
    with pytest.raises(ValueError):
        tree.merkleblock([])
    with pytest.raises(ValueError):
        vk.MerkleTree(NoDevice(), None, 5, 4, None).merkleblock([0])      # stored with another height than the walk needs
    with pytest.raises(ValueError):
        vk.MerkleTree(NoDevice(), None, 1, 0, None).merkleblock_of(np.zeros((1, 8), np.uint32))


def test_the_wrappers_on_raw_buffers_are_not_named_async(native):
    import vk_merkle_roots_amd as vk
    assert callable(vk.HipDevice.forest_merkleblocks_enqueue) and callable(vk.HipDevice.tree_merkleblock_enqueue)
    assert not any("merkleblock" in n and n.endswith("_async") for n in dir(vk.HipDevice))
    for name in ("merkleblocks", "merkleblocks_of", "merkleblocks_async"):
        assert callable(getattr(vk.MerkleForest, name))
    for name in ("merkleblock", "merkleblock_of", "merkleblocks_async"):
        assert callable(getattr(vk.MerkleTree, name))
    assert vk.PartialMerkleTree and vk.PartialMerkleTrees and vk.merkleblocks_status_text(4).startswith("bit 2")


# ---- the build ---------------------------------------------------------------------------------------------------------------------
def test_the_kernels_hash_nothing_shadow_no_key_and_spill_nothing(native):
    from vk_merkle_roots_amd import build, isa_prio_pass
    keys = isa_prio_pass.EXPECTED_HASH_BLOCKS
    for name in KERNELS:
        assert name.startswith("merkleblock_") and name.endswith("_kernel")
        assert not any(k in name for k in keys), name                                             # no hash expected in any of them
        assert not any(s in name for s in NAMES_OTHER_TESTS_COUNT), name
    text = open(os.path.join(ROOT, "vk_merkle_roots_amd", "csrc", "merkleblock_kernels.hpp")).read()
    assert not re.search(r"\bhash_(pair|parent)\(", text) and sorted(re.findall(r"void (\w+_kernel)\(", text)) == sorted(KERNELS)
    assert os.path.join(build.CSRC, "merkleblock_plan.hpp") in build.host_headers()
    rec = isa_record(native)
    if rec is not None:
        assert rec["audit"]["block_count_errors"] == [] and rec["audit"]["unclassified"] == []
        assert not any("merkleblock" in k for k in rec["audit"]["blocks"])
    assert_no_spills(native, KERNELS)
