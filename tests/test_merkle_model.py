"""tests/merkle_model.py, the one hashlib restatement of the tree that the tree, multiproof and forest tests compare with,
anchored to the host library's CPU backend (vkmr_host_cpu_reduce, vkmr_host_cpu_fold_proof).  No GPU."""
import numpy as np
import pytest

import merkle_model as mm


def host_reduce(leaves, height):
    import vk_merkle_roots_amd as vk
    leaves = np.ascontiguousarray(leaves, dtype=np.uint32)
    root = np.zeros(8, dtype=np.uint32)
    assert vk.host_lib().vkmr_host_cpu_reduce(leaves.ctypes.data, leaves.shape[0], height, root.ctypes.data) == 0
    return root


@pytest.mark.parametrize("count", [1, 2, 3, 5, 8, 9])
def test_the_model_equals_the_host_cpu_backend(native, count):
    leaves = mm.random_leaves(np.random.default_rng(count), count)
    height = mm.tree_height(count)
    levels = mm.cpu_levels(leaves)
    assert len(levels) == height + 1 and [lv.shape[0] for lv in levels] == [-(-count >> l) for l in range(height + 1)]
    root = levels[-1][0]
    assert (root == host_reduce(leaves, height)).all()
    assert all((a == b).all() for a, b in zip(levels, mm.cpu_levels(leaves, height)))
    for index in range(count):      # the gathered path of every leaf folds to that root, by the model and by the host library
        path = mm.proof_path(levels, index, height)
        assert (mm.fold(leaves[index], index, path, height) == root).all(), index
        assert (mm.host_fold(leaves[index], index, path, height) == root).all(), index
