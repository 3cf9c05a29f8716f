"""The mutation flag of a forest (vkmr_hip_reduce_forest_mutated_async, vkmr_host_cpu_forest_mutated) restated with hashlib and
numpy, and the inputs the CPU tests (tests/test_forest_mutation_abi.py) and the GPU tests (tests/test_gpu_forest_mutation.py)
share.  A plain module: no fixtures, no GPU.

The rule.  Level l of a tree over c leaves has n_l = ceil(c / 2^l) nodes, for 0 <= l < h = max(1, ceil(log2 c)).  Bit l of the
tree's mask is set iff node 2j equals node 2j + 1 for some j with 2j + 1 < n_l: a pair in which both nodes exist.  The last
node of an odd level, which is hashed with itself, is no such pair.  (Bitcoin Core's ComputeMerkleRoot(hashes, &mutated),
with the level kept.)

Planting.  Copying the leaves [2j * 2^l, (2j + 1) * 2^l) of a tree onto [(2j + 1) * 2^l, (2j + 2) * 2^l) makes nodes 2j and
2j + 1 of its level l equal; the second block must lie wholly inside the tree."""
import functools
import hashlib

import numpy as np

import forest_cases as fc
from forest_cases import CASES, offsets_of  # noqa: F401

RUNS = ("random", "equal") + tuple(f"plant{v}" for v in range(9))


def _sha256d(b):
    return hashlib.sha256(hashlib.sha256(b).digest()).digest()


def tree_root_and_mask(leaves):
    """(root [8] uint32, mask) of one tree over `leaves` ([c, 8] uint32, c >= 1), by the rule above."""
    raw = np.ascontiguousarray(leaves, dtype=np.uint32).astype(">u4").tobytes()
    cur = [raw[i: i + 32] for i in range(0, len(raw), 32)]
    mask, l = 0, 0
    while True:
        n = len(cur)
        if any(cur[2 * j] == cur[2 * j + 1] for j in range(n // 2)):      # 2j + 1 < n: both nodes exist
            mask |= 1 << l
        cur = [_sha256d(cur[2 * j] + cur[min(2 * j + 1, n - 1)]) for j in range((n + 1) // 2)]
        l += 1
        if len(cur) == 1:
            return np.frombuffer(cur[0], dtype=">u4").astype(np.uint32), mask


def model(leaves, counts):
    """(roots [ntrees, 8] uint32, masks [ntrees] uint64); an empty tree gets an all-zero root and mask 0."""
    off = offsets_of(counts)
    roots = np.zeros((len(counts), 8), dtype=np.uint32)
    masks = np.zeros(len(counts), dtype=np.uint64)
    for t, c in enumerate(counts):
        if c:
            roots[t], m = tree_root_and_mask(leaves[int(off[t]): int(off[t + 1])])
            masks[t] = m
    return roots, masks


def plant(leaves, first, c, l, j):
    """The hit (level l, pair j) planted into the tree of c leaves at cell `first` of `leaves`, in place."""
    b = 1 << l
    assert (2 * j + 2) * b <= c, (c, l, j)
    leaves[first + (2 * j + 1) * b: first + (2 * j + 2) * b] = leaves[first + 2 * j * b: first + (2 * j + 1) * b]


def plant_choice(c, which_level, which_pair):
    """(l, j) of the plant a tree of c >= 2 leaves takes: the level is the lowest (0), the highest at which a whole second block
    fits (floor(log2 c) - 1) or the one halfway (which_level 0, 1, 2); the pair is the first, the last that fits -- the last
    genuine pair in front of a ragged edge -- or the middle one (which_pair 0, 1, 2)."""
    top = int(c).bit_length() - 2
    l = (0, top, top // 2)[which_level]
    fits = c >> (l + 1)
    return l, (0, fits - 1, fits // 2)[which_pair]


def planted(counts, seed, v):
    """(leaves, plants): random leaves with one plant per tree of at least two leaves; tree t takes combination (v + t) % 9 of
    the three levels and three pairs, so the nine variants give every tree every combination.  plants = [(t, l, j)]."""
    leaves = fc.random_leaves(sum(counts), seed)
    off = offsets_of(counts)
    plants = []
    for t, c in enumerate(counts):
        if c >= 2:
            combo = (v + t) % 9
            l, j = plant_choice(c, combo // 3, combo % 3)
            plant(leaves, int(off[t]), c, l, j)
            plants.append((t, l, j))
    return leaves, plants


def seed_of(name):
    return len(name) * 7919 + sum(CASES[name])


def leaves_of(name, run):
    """The leaves of case `name` in one of RUNS: random, every leaf equal, or planted variant v."""
    counts = CASES[name]
    if run == "random":
        return fc.random_leaves(sum(counts), seed_of(name))
    if run == "equal":
        return np.tile(fc.random_leaves(1, seed_of(name)), (sum(counts), 1))
    return planted(counts, seed_of(name), int(run[5:]))[0]


@functools.lru_cache(maxsize=None)
def expected(name, run):
    """model() of leaves_of(name, run), computed once per process and shared (read-only) by the tests."""
    roots, masks = model(leaves_of(name, run), CASES[name])
    roots.setflags(write=False)
    masks.setflags(write=False)
    return roots, masks


def host_cpu_mutated(leaves, offsets, want_roots=True):
    """(return code, roots [ntrees, 8] or None, masks [ntrees]) of vkmr_host_cpu_forest_mutated; both start as a 0xA5 pattern."""
    import vk_merkle_roots_amd as vk
    leaves = np.ascontiguousarray(leaves, dtype=np.uint32).reshape(-1, 8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    ntrees = offsets.shape[0] - 1
    roots = np.full((ntrees, 8), 0xA5A5A5A5, dtype=np.uint32) if want_roots else None
    masks = np.full(ntrees, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    rc = vk.host_lib().vkmr_host_cpu_forest_mutated(leaves.ctypes.data if leaves.size else None, offsets.ctypes.data, ntrees,
                                                   roots.ctypes.data if want_roots else None, masks.ctypes.data)
    return rc, roots, masks
