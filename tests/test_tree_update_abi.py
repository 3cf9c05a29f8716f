"""Leaf updates of a stored tree: the C ABI's declaration, the argument checks and the host-side checks of MerkleTree.update.
No compute calls here: every case returns before the library or the Python layer touches HIP, so this runs without a GPU."""
import ctypes as C

import numpy as np
import pytest

from abi_support import Refusals, assert_bound
from no_device import NoDevice


def test_header_declares_the_update_and_the_stub_binds_it():
    assert_bound("vkmr_hip_tree_update_async", nparams=10, restype=C.c_int)


def test_bad_arguments_are_refused_before_any_hip_call(native):
    from vk_merkle_roots_amd import _abi
    lib = _abi.lib()
    d = C.c_void_p(0x1000)           # never dereferenced: every call below returns before launching anything
    update = Refusals(lib.vkmr_hip_tree_update_async, "vkmr_hip_tree_update_async", good=[d, d, 8, 3, d, d, 4, d])  # digests, tree, count, height, indices, leaves, k, status
    update.null(0, 1, 4, 5, 7)       # each pointer NULL with k > 0
    update.changed(*({2: count, 3: height} for count, height in ((8, 2), (9, 3), (8, 64), (0, 3), (0, 0), (2, 0))))
    # k == 0 is a no-op whatever the rest
    update.ok((None, None, 8, 3, None, None, 0, None), (None, None, 0, 64, None, None, 0, None))


def host_tree(count=10, height=4):
    import vk_merkle_roots_amd as vk
    return vk.MerkleTree(NoDevice(), None, count, height, None)


@pytest.mark.parametrize("indices", [[10], [0, 10], [-1], [3, -2], [2**40], np.array([11], dtype=np.uint64),
                                     np.array([-5], dtype=np.int32)])
def test_update_refuses_indices_outside_the_tree(native, indices):
    k = len(indices)
    with pytest.raises(IndexError):
        host_tree().update(indices, np.zeros((k, 8), np.uint32))


@pytest.mark.parametrize("k,shape", [(1, (8,)), (2, (1, 8)), (2, (2, 7)), (1, (1, 8, 1)), (0, (1, 8)), (3, (8, 3))])
def test_update_refuses_leaves_that_are_not_k_by_8(native, k, shape):
    with pytest.raises(ValueError):
        host_tree().update(list(range(k)), np.zeros(shape, np.uint32))


def test_update_refuses_indices_that_are_not_integers(native):
    with pytest.raises(ValueError):
        host_tree().update([1.5], np.zeros((1, 8), np.uint32))


def test_update_packed_refuses_before_any_device_call(native):
    import vk_merkle_roots_amd as vk
    batch = vk.pack_lines(b"a\nb\nc\n")
    assert batch.count == 3
    with pytest.raises(ValueError):
        host_tree().update_packed([0, 1], batch)
    with pytest.raises(IndexError):
        host_tree().update_packed([0, 1, 10], batch)
    with pytest.raises(IndexError):
        host_tree().update_packed([0, -1, 2], batch)


def test_last_occurrence_wins_and_order_is_sorted(native):
    t = host_tree(count=100, height=7)
    idx, pos = t._update_order([7, 3, 7, 99, 3, 0])
    assert idx.dtype == np.uint64 and list(idx) == [0, 3, 7, 99]
    assert list(pos) == [5, 4, 2, 3]
