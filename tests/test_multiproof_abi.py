"""Multiproofs: the C ABI's declarations, the closed-form buffer bound, the argument checks, the host verifier
(vkmr_host_cpu_verify_multiproof) against the hashlib restatement in tests/multiproof_cases.py, and the host-side checks of
MerkleTree.multiproof.  No compute calls: every case returns before the library touches HIP, so this runs without a GPU."""
import ctypes as C

import numpy as np
import pytest

import multiproof_cases as mc
from abi_support import Refusals, assert_bound, assert_exported
from no_device import NoDevice

ENTRY_POINTS = ("vkmr_hip_multiproof_max_nodes", "vkmr_hip_multiproof_scratch_bytes", "vkmr_hip_tree_multiproof_async",
                "vkmr_hip_verify_multiproof_async")


def test_header_declares_library_exports_and_stub_binds(native):
    from vk_merkle_roots_amd import _abi
    assert_exported(native.HIP_LIB, ENTRY_POINTS)
    lib = _abi.lib()
    for name in ENTRY_POINTS:
        assert_bound(name, nparams={"vkmr_hip_tree_multiproof_async": 12, "vkmr_hip_verify_multiproof_async": 11}.get(name))
        assert list(getattr(lib, name).argtypes) == _abi.SIGNATURES[name][1], name
    assert_exported(native.HOST_LIB, ["vkmr_host_cpu_verify_multiproof"])
    assert _abi.host_lib().vkmr_host_cpu_verify_multiproof.restype is C.c_int


def test_max_nodes_is_the_closed_form(native):
    from vk_merkle_roots_amd import _abi
    lib = _abi.lib()
    top = 2**32 - 1
    for count in list(range(1, 301)) + [1 << 26, (1 << 32) + 1]:
        h0 = int(count - 1).bit_length()                  # the smallest height that reduces count to one node
        for height in range(h0, 64):
            for k in (0, 1, 2, 7, min(count, top), top):
                assert lib.vkmr_hip_multiproof_max_nodes(count, height, k) == mc.max_nodes(count, height, k), (count, height, k)
    assert lib.vkmr_hip_multiproof_max_nodes(0, 3, 5) == 0
    assert lib.vkmr_hip_multiproof_max_nodes(5, 64, 5) == 0
    assert lib.vkmr_hip_multiproof_max_nodes(1 << 26, 26, 1 << 20) == 7340031


def test_scratch_bytes(native):
    from vk_merkle_roots_amd import _abi
    lib = _abi.lib()
    assert lib.vkmr_hip_multiproof_scratch_bytes(0, 5) == 0
    assert lib.vkmr_hip_multiproof_scratch_bytes(5, 64) == 0
    last = 0
    for k in (1, 64, 65, 1000, 1 << 20):
        b = lib.vkmr_hip_multiproof_scratch_bytes(k, 26)
        assert b >= 36 * k and b % 4 == 0 and b > last     # a cell and a run end per entry, and the ranking words
        last = b


def test_bad_arguments_are_refused_before_any_hip_call(native):
    from vk_merkle_roots_amd import _abi
    lib = _abi.lib()
    d = C.c_void_p(0x1000)           # never dereferenced: every call below returns before launching anything
    # digests, tree, count, height, indices, k, scratch, nodes, capacity, info
    gather = Refusals(lib.vkmr_hip_tree_multiproof_async, "vkmr_hip_tree_multiproof_async", good=[d, d, 8, 3, d, 4, d, d, 7, d])
    gather.null(0, 1, 4, 6, 7, 9)    # each pointer NULL with k > 0
    gather.changed(*({2: count, 3: height} for count, height in ((8, 2), (9, 3), (8, 64), (0, 3), (0, 0), (2, 0))))
    gather.ok((None, None, 8, 3, None, 0, None, None, 0, None), (None, None, 0, 64, None, 0, None, None, 0, None))
    # leaves, indices, k, height, nodes, m, root, scratch, ok
    verify = Refusals(lib.vkmr_hip_verify_multiproof_async, "vkmr_hip_verify_multiproof_async", good=[d, d, 4, 3, d, 5, d, d, d])
    verify.null(0, 1, 4, 6, 7, 8)
    verify.changed({3: 0}, {3: 64}, {3: 100})              # the height
    verify.ok((None, None, 0, 3, None, 0, None, None, None))


def test_known_sizes_of_the_restatement():
    """The contract's worked examples: all leaves proved leaves only the self-sibling cells; k = 1 is the single proof."""
    for count, height, m in ((128, 7, 0), (129, 8, 7), (1000, 10, 2)):
        assert len(mc.emitted_positions(count, height, range(count))[0]) == m
    pos, counts = mc.emitted_positions(1000, 12, [999])
    assert len(pos) == 12 and counts == [1] * 12
    assert [c for _, c in pos] == [(999 >> l) ^ 1 if (999 >> l) ^ 1 < -(-1000 >> l) else 999 >> l for l in range(12)]


@pytest.mark.parametrize("count", mc.COUNTS)
def test_host_verifier_against_the_restatement(native, count):
    rng = np.random.default_rng(500 + count)
    h0 = mc.tree_height(count)
    leaves = mc.random_leaves(rng, count)
    levels = mc.cpu_levels(leaves, h0 + 2)
    for height in (h0, h0 + 2):
        root = levels[height][0]
        for idx in mc.small_index_sets(count, rng):
            nodes, counts = mc.make_multiproof(lambda l: levels[l], count, height, idx)
            assert sum(counts) == nodes.shape[0] <= mc.max_nodes(count, height, len(idx))
            proved = leaves[idx]
            assert mc.verify_multiproof(proved, idx, height, nodes, root), (count, height, idx)
            assert mc.host_verify(proved, idx, height, nodes, root), (count, height, idx)
            if len(idx) == 1:                 # the single proof, sibling by sibling
                i = idx[0]
                for l in range(height):
                    p = i >> l
                    assert (nodes[l] == levels[l][p ^ 1 if p ^ 1 < levels[l].shape[0] else p]).all()
            for name, lv, ix, nd in mc.mutations(proved, idx, nodes, height, rng):
                assert not mc.verify_multiproof(lv, ix, height, nd, root), (count, height, idx, name)
                assert not mc.host_verify(lv, ix, height, nd, root), (count, height, idx, name)
            wrong = root.copy()
            wrong[7] ^= np.uint32(1 << 31)
            assert not mc.host_verify(proved, idx, height, nodes, wrong)


def test_host_verifier_refuses_bad_arguments(native):
    z = np.zeros((1, 8), np.uint32)
    assert not mc.host_verify(z[:0], [], 3, z[:0], z[0])          # no leaf proves nothing
    assert not mc.host_verify(z, [0], 64, z[:0], z[0])


def host_tree(count=10, height=4):
    import vk_merkle_roots_amd as vk
    return vk.MerkleTree(NoDevice(), None, count, height, None)


@pytest.mark.parametrize("indices", [[10], [0, 10], [-1], [3, -2], [2**40], np.array([11], dtype=np.uint64), np.array([-5], dtype=np.int32)])
def test_multiproof_refuses_indices_outside_the_tree(native, indices):
    with pytest.raises(IndexError):
        host_tree().multiproof(indices)


def test_multiproof_refuses_indices_that_are_not_integers_and_none_at_all(native):
    with pytest.raises(ValueError):
        host_tree().multiproof([1.5])
    with pytest.raises(ValueError):
        host_tree().multiproof([])


def test_the_python_layer_exports_the_type(native):
    import vk_merkle_roots_amd as vk
    p = vk.Multiproof(np.array([1], np.uint64), np.zeros((3, 8), np.uint32), np.array([1, 1, 1], np.uint64), 3)
    assert p.height == 3 and p.nodes.shape == (3, 8)
