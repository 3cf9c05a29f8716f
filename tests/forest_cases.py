"""Case tables for the forest reduction (vkmr_hip_reduce_forest_async), shared by the CPU tests (tests/test_forest_abi.py) and
the GPU tests (tests/test_gpu_forest.py), and the helpers both use.  A plain module: no fixtures, no GPU.

A case is a list of tree sizes; the leaves of all trees lie back to back from cell 0."""
import ctypes as C
import os

import numpy as np

import merkle_model
from merkle_model import ROOT  # noqa: F401


def _edges():
    sizes = []
    for k in range(14):                       # [1, 2^k, 2^k - 1, 2^k + 1] for k <= 13 (2^0 - 1 is an empty tree)
        sizes += [1, 1 << k, (1 << k) - 1, (1 << k) + 1]
    return sizes


CASES = {
    "sizes_1_to_130": list(range(1, 131)),
    "all_ones": [1] * 1000,
    "all_twos": [2] * 1000,
    "power_of_two_edges": _edges(),
    "one_big_among_small": [3] * 500 + [100003] + [3] * 500,
    "empty_first": [0, 5, 3, 9],
    "empty_last": [5, 3, 9, 0],
    "empty_adjacent": [4, 0, 0, 7, 0, 0, 0, 1],
    "all_empty": [0, 0, 0, 0, 0],
    "one_tree_of_1": [1],
    "one_tree_of_77": [77],
    "one_tree_of_4096": [4096],
    "one_tree_of_5000": [5000],
}


def offsets_of(counts):
    off = np.zeros(len(counts) + 1, dtype=np.uint64)
    np.cumsum(np.asarray(counts, dtype=np.uint64), out=off[1:])
    return off


def random_leaves(total, seed):
    """[total, 8] uint32 digests: any bits are a valid digest."""
    return np.random.default_rng(seed).integers(0, 2**32, size=(total, 8), dtype=np.uint32)


def oracle_roots(oracle, leaves, counts):
    """[ntrees, 8]: oracle.root of every tree (all-zero for an empty one)."""
    off = offsets_of(counts)
    out = np.zeros((len(counts), 8), dtype=np.uint32)
    for t, c in enumerate(counts):
        if c:
            out[t] = oracle.root(leaves[int(off[t]): int(off[t + 1])])
    return out


def host_cpu_roots(leaves, offsets):
    """(return code, [ntrees, 8]) of vkmr_host_cpu_forest_roots; the roots start as a 0xA5 pattern."""
    import vk_merkle_roots_amd as vk
    leaves = np.ascontiguousarray(leaves, dtype=np.uint32).reshape(-1, 8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    ntrees = offsets.shape[0] - 1
    roots = np.full((ntrees, 8), 0xA5A5A5A5, dtype=np.uint32)
    rc = vk.host_lib().vkmr_host_cpu_forest_roots(leaves.ctypes.data if leaves.size else None, offsets.ctypes.data, ntrees, roots.ctypes.data)
    return rc, roots


def build_plan_exe(directory):
    """tests/c/forest_plan_test.cpp compiled into `directory`; its path."""
    return merkle_model.build_plan_exe(directory, "forest_plan_test")


def plan_replay(exe, directory, forests):
    """For each (first_offset, slack, max_count, counts): (launches, scratch cells written, scratch cells budgeted) as the plan
    header gives them; the C test has checked overlap, bounds and the last level on the way."""
    return merkle_model.forests_replay(exe, directory, forests, "forests.txt")


def ceil_log2(n):
    return int(n - 1).bit_length() if n > 1 else 0


def ref_check_forest(oracle):
    """(leaves, counts) of the ten string lists of conftest.ref_check_inputs() as ONE forest of ten trees."""
    from conftest import ref_check_inputs
    _, trees = ref_check_inputs()
    leaves = np.array([oracle.leaf(s) for strs in trees for s in strs], dtype=np.uint32)
    return leaves, [len(strs) for strs in trees]
