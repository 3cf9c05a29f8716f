"""The sort and dedup of leaf entries (vkmr_hip_forest_sort_entries_async, vkmr_hip_tree_sort_entries_async and their CPU
twins) restated with numpy -- lexsort, last occurrence wins, the four counters: MerkleForest._update_order's rule with the
drop rule in front -- and the case tables tests/test_sort_entries_abi.py and tests/test_gpu_sort_entries.py share.  A plain
module: no fixtures, no GPU."""
import functools
import os
import re
import zlib

import numpy as np

import merkle_model

NO_TREE = 0xFFFFFFFF
NOT_FOUND = 0xFFFFFFFFFFFFFFFF


# ---- the sizes of csrc/sort_plan.hpp, read / restated -----------------------------------------------------------------------

def plan_constants():
    """{name: value} of the VKMR_SORT_* constants, read from the header's text."""
    text = open(os.path.join(merkle_model.ROOT, "vk_merkle_roots_amd", "csrc", "sort_plan.hpp")).read()
    return {name: int(value) for name, value in re.findall(r"#define\s+(VKMR_SORT_\w+)\s+(\d+)u?\b", text)}


def tile_keys():
    c = plan_constants()
    return c["VKMR_SORT_THREADS"] * c["VKMR_SORT_KEYS_PER_LANE"]


def passes(total):
    return (int(total).bit_length() + 7) // 8


def groups(k):
    return -(-k // tile_keys())


def second_trip_k():
    """The smallest k at which a scan workgroup takes a second trip over its bin's words: one tile more than a span of them."""
    return plan_constants()["VKMR_SORT_SCAN_SPAN"] * tile_keys() + 1


def scratch_bytes(k):
    """The layout of sort_plan.hpp written out: every part in whole 16-byte units."""
    if k == 0:
        return 0
    c = plan_constants()
    up = lambda n: (n + 15) // 16 * 16                                  # noqa: E731
    words = -(-k // 64)
    blocks = -(-words // c["VKMR_SORT_RANK_BLOCK_WORDS"])
    return (2 * up(8 * k) + 2 * up(4 * k) + up(4 * c["VKMR_SORT_BINS"] * groups(k)) + up(4 * c["VKMR_SORT_BINS"]) + 2 * up(8 * words) +
            up(8 * blocks) + 32)


# ---- the model --------------------------------------------------------------------------------------------------------------

def model(offsets, trees, indices):
    """(trees_out uint32 [n], indices_out uint64 [n], order_out uint32 [n], info [4]) of the k entries (trees[q], indices[q])
    in a forest of `offsets` (ntrees + 1 of them, or none): the valid entries (tree < ntrees, index < its count) sorted by
    (tree, index) with a stable sort, the last of every run of equal pairs kept, with the q it came from; info = survivors,
    markers (tree == NO_TREE), other entries that are not valid, valid entries dropped as earlier repeats."""
    off = np.asarray(offsets, dtype=np.uint64).reshape(-1)
    ntrees = max(0, off.shape[0] - 1)
    trees, indices = np.asarray(trees, dtype=np.uint32).reshape(-1), np.asarray(indices, dtype=np.uint64).reshape(-1)
    marker = trees == NO_TREE
    valid = ~marker & (trees < ntrees)
    if ntrees:
        counts = off[1:] - off[:-1]
        valid[valid] = indices[valid] < counts[trees[valid].astype(np.int64)]
    q = np.flatnonzero(valid)
    order = np.lexsort((indices[q], trees[q]))                          # stable: repeats stay in call order
    st, si, sq = trees[q][order], indices[q][order], q[order]
    last = np.ones(st.shape[0], dtype=bool)
    last[:-1] = (st[1:] != st[:-1]) | (si[1:] != si[:-1])
    n = int(last.sum())
    info = [n, int(marker.sum()), int((~marker & ~valid).sum()), int(q.shape[0]) - n]
    return st[last], si[last], sq[last].astype(np.uint32), info


def tree_model(count, indices):
    """The same for one tree of `count` leaves: (indices_out, order_out, info); the marker is NOT_FOUND."""
    indices = np.asarray(indices, dtype=np.uint64).reshape(-1)
    trees = np.where(indices == np.uint64(NOT_FOUND), NO_TREE, 0).astype(np.uint32)
    _, si, sq, info = model([0, count], trees, indices)
    return si, sq, info


def flat_keys(total, offsets, trees, indices):
    """uint64 [k]: the key the sort gives every entry -- offsets[t] + index, or the sentinel `total`."""
    off = np.asarray(offsets, dtype=np.uint64).reshape(-1)
    trees, indices = np.asarray(trees, dtype=np.uint32).reshape(-1), np.asarray(indices, dtype=np.uint64).reshape(-1)
    keys = np.full(trees.shape[0], total, dtype=np.uint64)
    ntrees = max(0, off.shape[0] - 1)
    ok = (trees != NO_TREE) & (trees < ntrees)
    if ntrees:
        ok[ok] = indices[ok] < (off[1:] - off[:-1])[trees[ok].astype(np.int64)]
        keys[ok] = off[trees[ok].astype(np.int64)] + indices[ok]
    return keys


# ---- the case tables --------------------------------------------------------------------------------------------------------

# name -> (total, offsets): one pass; 9 bits (a ragged last digit), a first offset above 0 and cells behind the last tree;
# three passes; the upper key word, six passes, an empty tree
FORESTS = {
    "total_200": (200, [0, 60, 60, 200]),
    "total_300": (300, [3, 100, 100, 290]),
    "total_65537": ((1 << 16) + 1, [0, 1, 30000, 30000, (1 << 16) + 1]),
    "total_2p40": (1 << 40, [0, (1 << 33) + 5, (1 << 33) + 5, 1 << 40]),
}
SHAPES = ("random", "sorted", "reversed", "one_pair", "one_bin", "all_invalid", "mixed")


def k_values():
    t = tile_keys()
    return (1, 63, 64, 65, t - 1, t, t + 1, 2 * t + 3, second_trip_k())


def seed_of(*parts):
    return zlib.crc32(repr(parts).encode())


def entries_at(offsets, flat):
    """(trees uint32, indices uint64) of flat positions inside [offsets[0], offsets[-1]): never an empty tree."""
    off = np.asarray(offsets, dtype=np.uint64)
    flat = np.asarray(flat, dtype=np.uint64)
    t = np.searchsorted(off, flat, side="right") - 1
    return t.astype(np.uint32), flat - off[t]


def invalid_entries(rng, offsets, k, markers=True):
    """k entries none of which is valid: markers, trees past the forest, indices at and past their tree's count (an empty
    tree's index 0 among them)."""
    off = np.asarray(offsets, dtype=np.uint64)
    ntrees = off.shape[0] - 1
    counts = off[1:] - off[:-1]
    kind = rng.integers(0 if markers else 1, 4, size=k)
    trees = rng.integers(0, ntrees, size=k).astype(np.uint32)
    indices = counts[trees.astype(np.int64)] + rng.integers(0, 3, size=k).astype(np.uint64)      # kind 1: just past the tree
    far = kind == 2
    indices[far] = np.uint64(NOT_FOUND) - rng.integers(0, 2, size=int(far.sum())).astype(np.uint64)   # a valid tree with a marker's index
    past = kind == 3
    trees[past] = (ntrees + rng.integers(0, 3, size=int(past.sum()))).astype(np.uint32)
    indices[past] = rng.integers(0, 5, size=int(past.sum())).astype(np.uint64)
    mark = kind == 0
    trees[mark] = NO_TREE
    indices[mark] = np.where(rng.integers(0, 2, size=int(mark.sum())) == 0, np.uint64(NOT_FOUND), np.uint64(0))
    return trees, indices


class Case:
    def __init__(self, total, offsets, trees, indices):
        self.total, self.offsets = int(total), np.ascontiguousarray(offsets, dtype=np.uint64)
        self.ntrees = max(0, int(self.offsets.shape[0]) - 1)
        self.trees, self.indices = np.ascontiguousarray(trees, dtype=np.uint32), np.ascontiguousarray(indices, dtype=np.uint64)
        self.k = int(self.trees.shape[0])
        self.want = model(self.offsets, self.trees, self.indices)


@functools.lru_cache(maxsize=None)
def forest_case(name, shape, k):
    total, offsets = FORESTS[name]
    rng = np.random.default_rng(seed_of(name, shape, k))
    lo, hi = int(offsets[0]), int(offsets[-1])
    if shape in ("random", "mixed"):
        flat = rng.integers(lo, hi, size=k, dtype=np.uint64)
        if k > 4:
            flat[rng.integers(0, k, size=k // 8 + 1)] = flat[rng.integers(0, k, size=k // 8 + 1)]      # repeats, far apart
    elif shape in ("sorted", "reversed"):
        flat = np.sort(rng.integers(lo, hi, size=k, dtype=np.uint64))
        if shape == "reversed":
            flat = flat[::-1]
    elif shape == "one_pair":
        flat = np.full(k, rng.integers(lo, hi), dtype=np.uint64)
    elif shape == "one_bin":           # one low byte throughout: every key in bin 7 of the first digit (one key where the forest is small)
        flat = np.uint64(lo - lo % 256 + 256 + 7) + np.uint64(256) * rng.integers(0, max(1, (hi - lo) // 256 - 1), size=k, dtype=np.uint64)
        flat = np.minimum(flat, np.uint64(hi - 1)) if hi - lo < 1024 else flat
    if shape == "all_invalid":
        trees, indices = invalid_entries(rng, offsets, k)
    else:
        trees, indices = entries_at(offsets, flat)
    if shape == "mixed" and k > 1:
        bad = rng.random(k) < 0.3
        bt, bi = invalid_entries(rng, offsets, int(bad.sum()))
        trees[bad], indices[bad] = bt, bi
    return Case(total, offsets, trees, indices)


TREE_COUNTS = (200, 300, (1 << 16) + 1, 1 << 40)


@functools.lru_cache(maxsize=None)
def tree_case(count, k):
    """(indices, model's answer): random indices of one tree with repeats, NOT_FOUND markers and indices at and past `count`."""
    rng = np.random.default_rng(seed_of("tree", count, k))
    idx = rng.integers(0, count, size=k, dtype=np.uint64)
    if k > 4:
        idx[rng.integers(0, k, size=k // 8 + 1)] = idx[rng.integers(0, k, size=k // 8 + 1)]
    r = rng.random(k)
    idx[r < 0.15] = np.uint64(NOT_FOUND)
    idx[(r >= 0.15) & (r < 0.25)] = np.uint64(count) + rng.integers(0, 3, size=int(((r >= 0.15) & (r < 0.25)).sum())).astype(np.uint64)
    return idx, tree_model(count, idx)


def random_forest_case(rng):
    """A small random forest -- no tree, empty trees, a first offset above 0, cells behind the last tree -- and a random batch."""
    ntrees = int(rng.integers(0, 9))
    counts = rng.integers(0, 40, size=ntrees) * (rng.random(ntrees) < 0.7)
    first = int(rng.integers(0, 6)) if ntrees else 0
    offsets = (np.concatenate([[0], np.cumsum(counts)]) + first).astype(np.uint64) if ntrees else np.zeros(int(rng.integers(0, 2)), dtype=np.uint64)
    total = (int(offsets[-1]) if ntrees else 0) + int(rng.integers(0, 6))
    k = int(rng.integers(0, 200))
    if ntrees and int(offsets[-1]) > first and k:
        trees, indices = entries_at(offsets, rng.integers(first, int(offsets[-1]), size=k, dtype=np.uint64))
        bad = rng.random(k) < 0.3
        bt, bi = invalid_entries(rng, offsets, int(bad.sum()))
        trees[bad], indices[bad] = bt, bi
    else:
        trees = np.where(rng.random(k) < 0.5, NO_TREE, rng.integers(0, 5, size=k)).astype(np.uint32)
        indices = rng.integers(0, 5, size=k).astype(np.uint64)
    return Case(total, offsets, trees, indices)


# ---- the CPU twins ----------------------------------------------------------------------------------------------------------

PATTERN32, PATTERN64 = 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5


def host_cpu_forest_sort(case):
    """(return code, trees_out, indices_out, order_out, info) of vkmr_host_cpu_forest_sort_entries; the outputs start as a 0xA5 pattern."""
    import vk_merkle_roots_amd as vk
    k = case.k
    to, io, oo = np.full(k, PATTERN32, dtype=np.uint32), np.full(k, PATTERN64, dtype=np.uint64), np.full(k, PATTERN32, dtype=np.uint32)
    info = np.full(4, PATTERN64, dtype=np.uint64)
    rc = vk.host_lib().vkmr_host_cpu_forest_sort_entries(case.total, case.offsets.ctypes.data if case.offsets.size else None, case.ntrees,
                                                         case.trees.ctypes.data, case.indices.ctypes.data, k, to.ctypes.data, io.ctypes.data,
                                                         oo.ctypes.data, info.ctypes.data)
    return rc, to, io, oo, info


def host_cpu_tree_sort(count, indices):
    import vk_merkle_roots_amd as vk
    indices = np.ascontiguousarray(indices, dtype=np.uint64)
    k = int(indices.shape[0])
    io, oo, info = np.full(k, PATTERN64, dtype=np.uint64), np.full(k, PATTERN32, dtype=np.uint32), np.full(4, PATTERN64, dtype=np.uint64)
    rc = vk.host_lib().vkmr_host_cpu_tree_sort_entries(count, indices.ctypes.data, k, io.ctypes.data, oo.ctypes.data, info.ctypes.data)
    return rc, io, oo, info


def assert_equals_the_model(want, got, what):
    """got = (trees_out or None, indices_out, order_out, info) against the model's (trees, indices, order, info): the four
    counters, and cells [0, n) of every output, exactly."""
    wt, wi, wo, winfo = want
    gt, gi, go, ginfo = got
    assert [int(x) for x in ginfo] == winfo, (what, [int(x) for x in ginfo], winfo)
    n = winfo[0]
    assert sum(winfo) == int(np.asarray(go).shape[0]), what
    if gt is not None:
        assert (gt[:n] == wt).all(), (what, "trees", np.flatnonzero(gt[:n] != wt)[:8])
    assert (gi[:n] == wi).all(), (what, "indices", np.flatnonzero(gi[:n] != wi)[:8])
    assert (go[:n] == wo).all(), (what, "order", np.flatnonzero(go[:n] != wo)[:8])
