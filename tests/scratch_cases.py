"""ONE table with a row per entry point of include/vkmr_hip.h that takes a `scratch_dev`, for the scratch contract the header
states ("Scratch buffers"): what the scratch holds on entry does not matter, the call stays inside the bytes its size function
named, and the next call may take the same scratch on the same stream with no wait in between.  A plain module: no fixtures, no
GPU.  tests/test_scratch_cases.py holds the table to the header and to the CPU; tests/test_gpu_scratch.py runs every row from
dirty scratch of exactly its size.

A row names the ABI function, the size function the header names for it and the least alignment the header promises, and gives
per variant ("large", "small") a Case: the arguments of the size function, the arguments of the call by parameter name, and what
every output buffer must hold afterwards, canaries of unwritten cells included -- from the CPU twin in libvkmr_host.so, or from
the case module's model where no twin exists.  The inputs are those of the existing case modules.

`large` is the smallest shape at which every part of the scratch is used by more than one workgroup: k = 2 tile_keys + 3 for the
radix sorts, 16 385 entries (more than 256 ballot words) where the three ranking kernels run, a table above one workgroup's
lanes for find, more than one VKMR_MERGE_SCAN_ROW of slots for merge, a count that goes bulk -> collapse -> tail for the
reductions.  `small` has k or a count of 63 to 65 in a forest of a few hundred leaves, and differs from `large` in every
argument of the size function.  The reductions are the exception: up to 128 digests the header allows a NULL scratch (the tail
kernel never touches it), so their `small` is 193 digests, collapse -> tail."""
import functools
from typing import NamedTuple

import numpy as np

import abi_support
import apply_cases as ac
import audit_cases as au
import diff_cases as dc
import find_cases as fn
import forest_cases as fc
import forest_multiproof_cases as fm
import frontier_cases as fx
import leafsort_cases as lc
import merge_cases as mg
import range_cases as rg
import reduce_cases as rc
import sort_cases as sc
from merkle_model import tree_height

VARIANTS = ("large", "small")
GUARD = 8                                   # guard items on either side of every output
BIG_RUN = np.arange(7, 7 + 16385, dtype=np.uint64)     # test_gpu_tree_forest_twins.py's: one 16384-entry block and 256 ballot words, crossed
BIG = 16400                                 # the tree it lies in


def pattern(dtype):
    """The canary of an output of `dtype`: every byte 0xA5, the pattern of the case modules."""
    return int.from_bytes(b"\xA5" * np.dtype(dtype).itemsize, "little")


def canary(n, dtype, width=1):
    return np.full(int(n) * width, pattern(dtype), dtype=dtype)


# ---- what a Case's arguments are made of ----------------------------------------------------------------------------------------------
class In:
    """An input array, uploaded as it is."""

    def __init__(self, arr, dtype=None):
        self.arr = np.ascontiguousarray(arr, dtype=dtype)


class Host:
    """An argument the call reads on the HOST at call time (vkmr_hip_reduce_proofs_async's indices)."""

    def __init__(self, arr, dtype):
        self.arr = np.ascontiguousarray(arr, dtype=dtype)


class Out:
    """An output of n items of `width` words of `dtype`, allocated pre-filled with the canary between GUARD items of it."""

    def __init__(self, name, n, dtype, width=1):
        self.name, self.n, self.dtype, self.width = name, int(n), np.dtype(dtype), width


class Scratch:
    """Where the scratch pointer goes (plus `offset` bytes: the harness's own pseudo-rows point behind the scratch)."""

    def __init__(self, offset=0):
        self.offset = int(offset)


SCRATCH = Scratch()


class Part:
    def __init__(self, owner, what):
        self.owner, self.what = owner, what


class StoredForest:
    """A stored forest as an input: prepare() builds it on the device with vkmr_hip_reduce_forest_tree_async, which takes no scratch
    (the CPU twins build their own levels from the leaves)."""

    def __init__(self, cells, offsets, max_count):
        self.cells, self.offsets = np.ascontiguousarray(cells, dtype=np.uint32).reshape(-1, 8), np.ascontiguousarray(offsets, dtype=np.uint64)
        self.total, self.ntrees, self.max_count = int(self.cells.shape[0]), int(self.offsets.shape[0]) - 1, int(max_count)
        self.leaves, self.offs, self.levels, self.roots = (Part(self, w) for w in ("leaves", "offsets", "levels", "roots"))

    def build(self, gpu, tmp):
        bufs = {"leaves": tmp.upload(self.cells), "offsets": tmp.upload(self.offsets),
                "levels": tmp.upload(np.full(max(8, gpu.forest_tree_bytes(self.total, self.ntrees, self.max_count) // 4), 0xC3C3C3C3, np.uint32)),
                "roots": tmp.upload(np.full(8 * self.ntrees, 0xC3C3C3C3, np.uint32))}
        status = tmp.upload(np.full(1, 0xDEADBEEF, np.uint32))
        gpu._call("vkmr_hip_reduce_forest_tree_async", bufs["leaves"], self.total, bufs["offsets"], self.ntrees, self.max_count, bufs["levels"],
                  bufs["roots"], status)
        assert int(gpu.download(status, 4)[0]) == 0
        return bufs


class StoredTree:
    """A stored tree as an input, built in prepare() by vkmr_hip_reduce_tree_async."""

    def __init__(self, leaves, height):
        self.cells, self.height = np.ascontiguousarray(leaves, dtype=np.uint32).reshape(-1, 8), int(height)
        self.count = int(self.cells.shape[0])
        self.leaves, self.levels = Part(self, "leaves"), Part(self, "levels")

    def build(self, gpu, tmp):
        nbytes = int(gpu.lib.vkmr_hip_tree_bytes(self.count, self.height))
        bufs = {"leaves": tmp.upload(self.cells), "levels": tmp.upload(np.full(max(8, nbytes // 4), 0xC3C3C3C3, np.uint32))}
        gpu._call("vkmr_hip_reduce_tree_async", bufs["leaves"], self.count, self.height, bufs["levels"])
        gpu.sync()
        return bufs


class Case(NamedTuple):
    size_args: tuple           # what the row's size function takes
    args: dict                 # parameter name (behind dev and the stream) -> In, Host, Out, SCRATCH, a Part, an integer or None
    expected: dict             # output name -> what the whole buffer between its guards must hold
    unspecified: dict = {}     # output name -> the first item the header calls unspecified (rows with Row.allows only)


class Row(NamedTuple):
    name: str                  # the ABI function
    size_fn: str               # the ABI's own size function for its scratch
    align: int                 # the least alignment of scratch_dev the header promises
    case: object               # variant -> Case
    allows: str = ""           # the header's sentence that lets the row leave cells out of the comparison
    fixed: tuple = ()          # the arguments of the size function that the header fixes for this entry point, by position

    def size(self, variant):
        return self.case(variant).size_args

    def expected(self, variant):
        return self.case(variant).expected

    def prepare(self, gpu, tmp, variant):
        """The inputs uploaded and every output allocated between guards, all canary.  (enqueue(scratch_ptr, stream), read()):
        read() gives {name: the whole output buffer} and fails when a guard item was written; it leaves the outputs canary again."""
        case = self.case(variant)
        params = [name for _, name in abi_support.declarations()[self.name].params[2:]]
        assert sorted(params) == sorted(case.args), (self.name, sorted(set(params) ^ set(case.args)))
        built, outs, values, keep = {}, [], [], []
        for p in params:
            v = case.args[p]
            if isinstance(v, In):
                v = tmp.upload(v.arr)
            elif isinstance(v, Host):
                keep.append(v.arr)
                v = v.arr.ctypes.data
            elif isinstance(v, Part):
                if id(v.owner) not in built:
                    built[id(v.owner)] = v.owner.build(gpu, tmp)
                v = built[id(v.owner)][v.what]
            elif isinstance(v, Out):
                host = canary(v.n + 2 * GUARD, v.dtype, v.width)
                buf = tmp.upload(host)
                outs.append((v, buf, host))
                v = buf.at(GUARD * v.width * v.dtype.itemsize)
            values.append(v)

        def enqueue(scratch_ptr, stream):
            gpu._call(self.name, *[scratch_ptr + v.offset if isinstance(v, Scratch) else v for v in values], stream=stream)

        def read():
            got = {}
            for o, buf, host in outs:
                raw = gpu.download(buf, host.nbytes, dtype=o.dtype)
                edge = GUARD * o.width
                assert (raw[:edge] == host[:edge]).all() and (raw[raw.shape[0] - edge:] == host[:edge]).all(), (self.name, o.name, "guard items written")
                got[o.name] = raw[edge: raw.shape[0] - edge]
                gpu._call("vkmr_hip_memcpy_h2d_async", buf, host.ctypes.data, host.nbytes)
            gpu.sync()
            return got

        enqueue.keep = keep
        return enqueue, read


def differences(case, got):
    """The outputs of a run that are not what the case expects, by name with the first items that differ; [] when all are."""
    out = []
    assert sorted(got) == sorted(case.expected), (sorted(got), sorted(case.expected))
    for name, want in case.expected.items():
        a, b = np.asarray(got[name]).reshape(-1), np.asarray(want).reshape(-1)
        assert a.dtype == b.dtype and a.shape == b.shape, (name, a.dtype, b.dtype, a.shape, b.shape)
        if name in case.unspecified:
            width = a.shape[0] // max(1, _items(case, name))
            a, b = a[: case.unspecified[name] * width], b[: case.unspecified[name] * width]
        if a.tobytes() != b.tobytes():
            out.append((name, np.flatnonzero(a != b)[:8].tolist()))
    return out


def _items(case, name):
    return next(v.n for v in case.args.values() if isinstance(v, Out) and v.name == name)


# ---- helpers of the rows ----------------------------------------------------------------------------------------------------------------
def _host(name, *args):
    """A CPU twin of libvkmr_host.so over numpy arrays (an empty one goes as NULL); its return code."""
    import vk_merkle_roots_amd as vk
    return getattr(vk.host_lib(), name)(*[(a.ctypes.data if a.size else None) if isinstance(a, np.ndarray) else a for a in args])


def _cells(a):
    return np.ascontiguousarray(a, dtype=np.uint32).reshape(-1, 8)


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32).reshape(-1)


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64).reshape(-1)


def _digests(name, n):
    return Out(name, n, np.uint32, 8)


def _one(value, dtype):
    return np.array([value], dtype=dtype)


# ---- the reductions -----------------------------------------------------------------------------------------------------------------------
# one slice: bulk takes over at 2048 wavefronts of 128 nodes (csrc/reduce_plan.hpp next_step), a quarter of reduce_cases'
# FIRST_PASS_BASE[1]; 129 is one of its edge_offsets: bulk (one level) -> collapse -> collapse -> tail.  193: collapse -> tail.
REDUCE_COUNT = {"large": rc.FIRST_PASS_BASE[1] // 4 + 129, "small": 193}
assert 129 in rc.edge_offsets(1)


@functools.lru_cache(maxsize=None)
def _reduce_input(variant):
    count = REDUCE_COUNT[variant]
    leaves = fc.random_leaves(count, seed=9100 + count)
    return leaves, count, tree_height(count)


def _cpu_reduce(leaves, height):
    leaves = _cells(leaves)
    if height == 0:
        return leaves[0].copy()
    root = np.zeros(8, np.uint32)
    assert _host("vkmr_host_cpu_reduce", leaves, int(leaves.shape[0]), int(height), root) == 0
    return root


@functools.lru_cache(maxsize=None)
def _reduce_root(variant):
    leaves, count, height = _reduce_input(variant)
    return _cpu_reduce(leaves, height)


def _siblings(leaves, count, height, index):
    """The path of vkmr_hip_proof_async: at level l the root of the neighbouring sub-tree of 2^l leaves, by the CPU's reduce."""
    out = np.zeros((height, 8), np.uint32)
    for l in range(height):
        p, n = int(index) >> l, -(-count >> l)
        s = p ^ 1 if (p ^ 1) < n else p
        out[l] = _cpu_reduce(leaves[s << l: min(count, (s + 1) << l)], l)
    return out


@functools.lru_cache(maxsize=None)
def _reduce(variant):
    leaves, count, height = _reduce_input(variant)
    return Case((count,), {"digests_dev": In(leaves), "count": count, "height": height, "scratch_dev": SCRATCH, "root_dev": _digests("root", 1)},
                {"root": _reduce_root(variant)})


@functools.lru_cache(maxsize=None)
def _proof(variant):
    leaves, count, height = _reduce_input(variant)
    index = count - 1                                              # the odd edge: its own sibling at level 0
    return Case((count,), {"digests_dev": In(leaves), "count": count, "height": height, "index": index, "scratch_dev": SCRATCH,
                           "siblings_dev": _digests("siblings", height), "root_dev": _digests("root", 1)},
                {"siblings": _siblings(leaves, count, height, index), "root": _reduce_root(variant)})


@functools.lru_cache(maxsize=None)
def _reduce_proofs(variant):
    leaves, count, height = _reduce_input(variant)
    indices = [0, count // 2 + 1, count - 1]
    return Case((count,), {"digests_dev": In(leaves), "count": count, "height": height, "scratch_dev": SCRATCH, "root_dev": _digests("root", 1),
                           "indices": Host(indices, np.uint64), "k": len(indices), "siblings_dev": _digests("siblings", len(indices) * height)},
                {"root": _reduce_root(variant), "siblings": np.concatenate([_siblings(leaves, count, height, i) for i in indices])})


@functools.lru_cache(maxsize=None)
def _combine(variant):
    leaves, count, height = _reduce_input(variant)
    root = np.zeros(8, np.uint32)
    assert _host("vkmr_host_cpu_combine", leaves, count, root) == 0
    return Case((count,), {"roots_dev": In(leaves), "n": count, "scratch_dev": SCRATCH, "root_dev": _digests("root", 1)}, {"root": root})


@functools.lru_cache(maxsize=None)
def _reduce_slices(variant):
    # 257 slices of 1024: 8 wavefronts a slice, 2056 in all -> bulk (one level) -> collapse -> tail; 3 slices of 256: collapse -> tail
    capacity, nslices, last = {"large": (1024, 257, 129), "small": (256, 3, 127)}[variant]
    assert last in rc.slice_lasts(capacity, nslices)
    leaves = fc.random_leaves(capacity * nslices, seed=9200 + capacity)
    height = capacity.bit_length() - 1
    roots = np.stack([_cpu_reduce(leaves[q * capacity: q * capacity + (last if q == nslices - 1 else capacity)], height) for q in range(nslices)])
    return Case((capacity, nslices), {"digests_dev": In(leaves), "nslices": nslices, "capacity": capacity, "count_last": last, "height": height,
                                      "scratch_dev": SCRATCH, "roots_dev": _digests("roots", nslices)}, {"roots": roots})


@functools.lru_cache(maxsize=None)
def _sizes(variant):
    # 11 and 3 workgroups of 4096 sizes (csrc/meta_kernels.hpp), a ragged last one: (workgroups + 1) words of scratch, whole 16 bytes
    count = {"large": 10 * 4096 + 65, "small": 2 * 4096 + 65}[variant]
    sizes = np.random.default_rng(9300 + count).integers(0, 1 << 16, size=count).astype(np.uint16)
    first_word = 77 if variant == "large" else 5
    words = (sizes.astype(np.uint64) + 3) // 4
    meta = np.zeros((count, 2), np.uint32)
    meta[:, 0] = (first_word + np.concatenate([[0], np.cumsum(words)[:-1]])).astype(np.uint32)      # the model: no CPU twin exists
    meta[:, 1] = sizes
    return Case((count,), {"sizes_dev": In(sizes), "count": count, "first_word": first_word, "scratch_dev": SCRATCH, "meta_dev": Out("meta", count, np.uint32, 2)},
                {"meta": meta})


# ---- the forest reduction -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _forest_input(variant):
    counts = fc.CASES["power_of_two_edges"] if variant == "large" else [65, 0, 64, 63, 130]
    leaves = fc.random_leaves(sum(counts), seed=9400 + len(counts))
    off = fc.offsets_of(counts)
    for t, c in enumerate(counts):                                 # equal pairs on two levels of every tree of four or more: the masks are not all zero
        if c >= 4:
            leaves[int(off[t]) + 1] = leaves[int(off[t])]
            leaves[int(off[t]) + 2: int(off[t]) + 4] = leaves[int(off[t]): int(off[t]) + 2]
    return leaves, counts, off


@functools.lru_cache(maxsize=None)
def _reduce_forest(variant, mutated=False):
    leaves, counts, off = _forest_input(variant)
    ntrees = len(counts)
    roots, masks = np.zeros((ntrees, 8), np.uint32), np.zeros(ntrees, np.uint64)
    assert _host("vkmr_host_cpu_forest_mutated", leaves, off, ntrees, roots, masks) == 0 and masks.any()
    args = {"digests_dev": In(leaves), "total": int(leaves.shape[0]), "offsets_dev": In(off), "ntrees": ntrees, "max_count": max(counts), "scratch_dev": SCRATCH,
            "roots_dev": _digests("roots", ntrees), "status_dev": Out("status", 1, np.uint32)}
    expected = {"roots": roots, "status": _one(0, np.uint32)}
    if mutated:
        args["mutated_dev"] = Out("mutated", ntrees, np.uint64)
        expected["mutated"] = masks
    return Case((int(leaves.shape[0]), ntrees), args, expected)


# ---- find -------------------------------------------------------------------------------------------------------------------------------------
def _find_case(variant):
    return fn.size_case(5000, 4097) if variant == "large" else fn.size_case(65, 63)      # a table of 8192 slots: 32 workgroups' lanes; of 128


@functools.lru_cache(maxsize=None)
def _forest_find(variant):
    c = _find_case(variant)
    rcode, trees, indices = fn.host_cpu_forest_find(c)
    assert rcode == 0
    return Case((c.k,), {"digests_dev": In(c.cells), "total": c.total, "offsets_dev": In(c.offsets), "ntrees": c.ntrees, "queries_dev": In(c.queries), "k": c.k,
                         "scratch_dev": SCRATCH, "trees_dev": Out("trees", c.k, np.uint32), "indices_dev": Out("indices", c.k, np.uint64)},
                {"trees": trees, "indices": indices})


@functools.lru_cache(maxsize=None)
def _tree_find(variant):
    c = _find_case(variant)
    rcode, indices = fn.host_cpu_tree_find(c.cells, c.queries)
    assert rcode == 0
    return Case((c.k,), {"digests_dev": In(c.cells), "count": c.total, "queries_dev": In(c.queries), "k": c.k, "scratch_dev": SCRATCH,
                         "indices_dev": Out("indices", c.k, np.uint64)}, {"indices": indices})


# ---- the radix sort of entries --------------------------------------------------------------------------------------------------------------
UNSPECIFIED_BEHIND_N = "Cells at and behind n are unspecified."      # include/vkmr_hip.h, SORT AND DEDUP LEAF ENTRIES


@functools.lru_cache(maxsize=None)
def _forest_sort_entries(variant):
    k = 2 * sc.tile_keys() + 3 if variant == "large" else 65
    assert k in sc.k_values()
    c = sc.forest_case("total_65537" if variant == "large" else "total_300", "mixed", k)
    rcode, trees, indices, order, info = sc.host_cpu_forest_sort(c)
    assert rcode == 0
    n = int(info[0])
    return Case((c.total, k), {"total": c.total, "offsets_dev": In(c.offsets), "ntrees": c.ntrees, "trees_dev": In(c.trees), "indices_dev": In(c.indices), "k": k,
                               "scratch_dev": SCRATCH, "trees_out_dev": Out("trees_out", k, np.uint32), "indices_out_dev": Out("indices_out", k, np.uint64),
                               "order_out_dev": Out("order_out", k, np.uint32), "info_dev": Out("info", 4, np.uint64)},
                {"trees_out": trees, "indices_out": indices, "order_out": order, "info": info}, {"trees_out": n, "indices_out": n, "order_out": n})


@functools.lru_cache(maxsize=None)
def _tree_sort_entries(variant):
    k = 2 * sc.tile_keys() + 3 if variant == "large" else 65
    count = sc.TREE_COUNTS[2] if variant == "large" else sc.TREE_COUNTS[1]
    idx, _ = sc.tree_case(count, k)
    rcode, indices, order, info = sc.host_cpu_tree_sort(count, idx)
    assert rcode == 0
    n = int(info[0])
    return Case((count, k), {"count": count, "indices_dev": In(idx), "k": k, "scratch_dev": SCRATCH, "indices_out_dev": Out("indices_out", k, np.uint64),
                             "order_out_dev": Out("order_out", k, np.uint32), "info_dev": Out("info", 4, np.uint64)},
                {"indices_out": indices, "order_out": order, "info": info}, {"indices_out": n, "order_out": n})


# ---- the radix sort of leaves ---------------------------------------------------------------------------------------------------------------
def _leafsort_trees(variant):
    """The trees of 130, 1 023 (with its run of 40 leaves under one key: the tie run) and 1 024 leaves: 2 177 = 2 tile_keys + 129;
    the trees of 63 and 65."""
    trees = lc.forest_trees()
    assert lc.COUNTS[13:16] == [130, 1023, 1024] and sum(lc.COUNTS[13:16]) > 2 * lc.tile_keys() + 3 and [lc.COUNTS[10], lc.COUNTS[12]] == [63, 65]
    return trees[13:16] if variant == "large" else [trees[10], trees[12]]


@functools.lru_cache(maxsize=None)
def _forest_sort_leaves(variant):
    trees = _leafsort_trees(variant)
    cells, offsets = lc.lay(trees, *lc.PLACEMENTS[1])
    max_count = max(len(t) for t in trees)
    rcode, out, order, info = lc.host_sort(cells, offsets, max_count)
    assert rcode == 0 and int(info[0]) == 0 and (variant == "small" or int(info[2]) >= lc.RUN)
    total = int(cells.shape[0])
    return Case((total,), {"digests_in_dev": In(cells), "total": total, "offsets_dev": In(offsets), "ntrees": len(trees), "max_count": max_count, "scratch_dev": SCRATCH,
                           "digests_out_dev": _digests("digests_out", total), "order_out_dev": Out("order_out", total, np.uint32),
                           "info_dev": Out("info", 4, np.uint64)}, {"digests_out": out, "order_out": order, "info": info})


@functools.lru_cache(maxsize=None)
def _tree_sort_leaves(variant):
    rows = np.concatenate(_leafsort_trees(variant)[:3 if variant == "large" else 1])
    rcode, out, order, info = lc.host_tree_sort(rows)
    assert rcode == 0 and int(info[0]) == 0
    count = int(rows.shape[0])
    return Case((count,), {"digests_in_dev": In(rows), "count": count, "scratch_dev": SCRATCH, "digests_out_dev": _digests("digests_out", count),
                           "order_out_dev": Out("order_out", count, np.uint32), "info_dev": Out("info", 4, np.uint64)},
                {"digests_out": out, "order_out": order, "info": info})


# ---- merge --------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _merge_case(variant, one_tree):
    A, B = mg.forest_sides()
    if one_tree:                      # every leaf of the forest's sides as one tree a side; the trees of 63 leaves
        a, b = (sorted(set(sum(A, []))), sorted(sum(B, []))) if variant == "large" else (A[10], B[10])
        return mg.Case("one tree a side", *mg.lay([a]), *mg.lay([b]))
    if variant == "large":
        return mg.forest_cases()[1]
    return mg.Case("the trees of 63 and 65", *mg.lay([A[10], A[12]], 3, 5), *mg.lay([B[10], B[12]], 2, 1, seed=8))


def _merge(variant, one_tree):
    c = _merge_case(variant, one_tree)
    op = 0                                                          # union: both sides are emitted
    capacity = mg.default_capacity(c, op)
    rcode, out, out_offsets, origin, info = mg.host_merge(c, op, capacity, one_tree=one_tree)
    assert rcode == 0 and int(info[0]) == 0
    a_total, b_total, ntrees = int(c.a_cells.shape[0]), int(c.b_cells.shape[0]), len(c.a_offsets) - 1
    assert variant == "small" or a_total + b_total + 2 > mg.SCAN_ROW
    args = {"a_digests_dev": In(c.a_cells), "b_digests_dev": In(c.b_cells), "op": op, "scratch_dev": SCRATCH, "out_digests_dev": _digests("out_digests", capacity),
            "out_capacity": capacity, "origin_out_dev": Out("origin_out", capacity, np.uint64), "info_dev": Out("info", 4, np.uint64)}
    expected = {"out_digests": out, "origin_out": origin, "info": info}
    if one_tree:
        args.update({"a_count": a_total, "b_count": b_total})
    else:
        args.update({"a_total": a_total, "a_offsets_dev": In(c.a_offsets), "b_total": b_total, "b_offsets_dev": In(c.b_offsets), "ntrees": ntrees,
                     "out_offsets_dev": Out("out_offsets", ntrees + 1, np.uint64)})
        expected["out_offsets"] = out_offsets
    return Case((a_total, b_total, ntrees), args, expected)


_forest_merge = functools.lru_cache(maxsize=None)(lambda variant: _merge(variant, False))
_tree_merge = functools.lru_cache(maxsize=None)(lambda variant: _merge(variant, True))


# ---- multiproofs: gather, verify, apply ---------------------------------------------------------------------------------------------------------
class _Proved(NamedTuple):
    leaves: np.ndarray         # the forest's leaves
    counts: list
    offsets: np.ndarray
    trees: np.ndarray
    indices: np.ndarray
    stride: int
    capacity: int              # cells of the node buffer: M and a few more, which stay canary
    nodes: np.ndarray          # [capacity, 8]
    heights: np.ndarray
    info: np.ndarray           # [2 + stride]
    roots: np.ndarray


@functools.lru_cache(maxsize=None)
def _proved(variant, one_tree):
    """The forest: the 16 385 consecutive leaves of a tree of 16 400 between an empty tree and one of three leaves; every fifth leaf
    of the trees of 65, 64, 63 and 130: 65 entries.  One tree: vkmr_hip_multiproof_scratch_bytes is the bare layout, 36 k bytes and
    8 bytes a block and level, not rounded (its forest twin rounds it up to 16), so whole 16-byte units take k a multiple of 4
    and an even blocks x height: 16 388 consecutive leaves of the tree of 16 400, every fourth leaf of a tree of 64."""
    if variant == "large":
        counts = [BIG] if one_tree else [0, BIG, 3]
        indices = np.arange(7, 7 + 16388, dtype=np.uint64) if one_tree else BIG_RUN
        trees = np.full(indices.shape[0], 0 if one_tree else 1, np.uint32)
    else:
        counts = [64] if one_tree else [65, 0, 64, 63, 130]
        trees, indices = fm.sorted_entries((t, i) for t, c in enumerate(counts) for i in range(0, c, 4 if one_tree else 5))
    leaves, offsets = fc.random_leaves(sum(counts), seed=9500 + len(counts) + sum(counts)), fc.offsets_of(counts)
    k, stride = int(trees.shape[0]), tree_height(max(counts))
    rcode, nodes, heights, info = fm.host_make(leaves, offsets, trees, indices, stride)
    assert rcode == 0 and int(info[0]) == 0
    capacity = int(info[1]) + 3
    rcode, _, heights, info = fm.host_make(leaves, offsets, trees, indices, stride, capacity)
    assert rcode == 0
    padded = canary(capacity, np.uint32, 8).reshape(capacity, 8)
    padded[: nodes.shape[0]] = nodes
    rcode, roots = fc.host_cpu_roots(leaves, offsets)
    assert rcode == 0 and k in ((16385, 65) if not one_tree else (16388, 16))
    return _Proved(leaves, counts, offsets, trees, indices, stride, capacity, padded, heights, info, roots)


@functools.lru_cache(maxsize=None)
def _forest_multiproof(variant):
    p = _proved(variant, False)
    sf = StoredForest(p.leaves, p.offsets, max(p.counts))
    k = int(p.trees.shape[0])
    return Case((k, p.stride), {"digests_dev": sf.leaves, "forest_dev": sf.levels, "total": sf.total, "offsets_dev": sf.offs, "ntrees": sf.ntrees,
                                "max_count": sf.max_count, "trees_dev": In(p.trees), "indices_dev": In(p.indices), "k": k, "scratch_dev": SCRATCH,
                                "nodes_dev": _digests("nodes", p.capacity), "nodes_capacity": p.capacity, "heights_dev": Out("heights", k, np.uint32),
                                "info_dev": Out("info", 2 + p.stride, np.uint64)}, {"nodes": p.nodes, "heights": p.heights, "info": p.info})


@functools.lru_cache(maxsize=None)
def _tree_multiproof(variant):
    p = _proved(variant, True)
    st = StoredTree(p.leaves, p.stride)
    k = int(p.indices.shape[0])
    return Case((k, p.stride), {"digests_dev": st.leaves, "tree_dev": st.levels, "count": st.count, "height": st.height, "indices_dev": In(p.indices), "k": k,
                                "scratch_dev": SCRATCH, "nodes_dev": _digests("nodes", p.capacity), "nodes_capacity": p.capacity,
                                "info_dev": Out("info", 2 + p.stride, np.uint64)}, {"nodes": p.nodes, "info": p.info})


@functools.lru_cache(maxsize=None)
def _verify_forest_multiproof(variant):
    p = _proved(variant, False)
    k, m = int(p.trees.shape[0]), int(p.info[1])
    proved = fm.leaves_at(p.leaves, p.offsets, p.trees, p.indices)
    assert fm.host_verify(proved, p.trees, p.indices, p.heights, p.stride, p.nodes[:m], p.roots)
    return Case((k, p.stride), {"leaves_dev": In(proved), "trees_dev": In(p.trees), "indices_dev": In(p.indices), "heights_dev": In(p.heights), "k": k,
                                "stride": p.stride, "nodes_dev": In(p.nodes[:m]), "m": m, "roots_dev": In(p.roots), "ntrees": len(p.counts), "scratch_dev": SCRATCH,
                                "ok_dev": Out("ok", 1, np.uint32)}, {"ok": _one(1, np.uint32)})


@functools.lru_cache(maxsize=None)
def _verify_multiproof(variant):
    p = _proved(variant, True)
    k, m = int(p.indices.shape[0]), int(p.info[1])
    proved = p.leaves[p.indices.astype(np.int64)]
    assert _host("vkmr_host_cpu_verify_multiproof", _cells(proved), _u64(p.indices), k, p.stride, _cells(p.nodes[:m]), m, _cells(p.roots)) == 1
    return Case((k, p.stride), {"leaves_dev": In(proved), "indices_dev": In(p.indices), "k": k, "height": p.stride, "nodes_dev": In(p.nodes[:m]), "m": m,
                                "root_dev": In(p.roots), "scratch_dev": SCRATCH, "ok_dev": Out("ok", 1, np.uint32)}, {"ok": _one(1, np.uint32)})


def _new_leaves(p):
    return fc.random_leaves(int(p.indices.shape[0]), seed=9600 + int(p.indices.shape[0]))


@functools.lru_cache(maxsize=None)
def _apply_forest_multiproof(variant):
    p = _proved(variant, False)
    k, m, ntrees = int(p.trees.shape[0]), int(p.info[1]), len(p.counts)
    old, new, counts = fm.leaves_at(p.leaves, p.offsets, p.trees, p.indices), _new_leaves(p), ac.counts_of(p.counts, p.trees)
    new_roots = canary(ntrees, np.uint32, 8).reshape(ntrees, 8)          # the cells of trees no entry names are never written
    assert _host("vkmr_host_cpu_apply_forest_multiproof", _cells(old), _cells(new), _u32(p.trees), _u64(p.indices), _u64(counts), k, p.stride,
                 _cells(p.nodes[:m]), m, _cells(p.roots), ntrees, new_roots) == 1
    return Case((k, p.stride), {"old_leaves_dev": In(old), "new_leaves_dev": In(new), "trees_dev": In(p.trees), "indices_dev": In(p.indices),
                                "counts_dev": In(counts), "k": k, "stride": p.stride, "nodes_dev": In(p.nodes[:m]), "m": m, "roots_dev": In(p.roots),
                                "ntrees": ntrees, "scratch_dev": SCRATCH, "ok_dev": Out("ok", 1, np.uint32), "new_roots_dev": _digests("new_roots", ntrees)},
                {"ok": _one(1, np.uint32), "new_roots": new_roots})


@functools.lru_cache(maxsize=None)
def _apply_multiproof(variant):
    p = _proved(variant, True)
    k, m = int(p.indices.shape[0]), int(p.info[1])
    old, new = p.leaves[p.indices.astype(np.int64)], _new_leaves(p)
    ok, new_root = ac.host_apply_tree(old, new, p.indices, p.counts[0], p.stride, p.nodes[:m], p.roots[0])
    assert ok == 1
    return Case((k, p.stride), {"old_leaves_dev": In(old), "new_leaves_dev": In(new), "indices_dev": In(p.indices), "k": k, "count": p.counts[0], "height": p.stride,
                                "nodes_dev": In(p.nodes[:m]), "m": m, "root_dev": In(p.roots), "scratch_dev": SCRATCH, "ok_dev": Out("ok", 1, np.uint32),
                                "new_root_dev": _digests("new_root", 1)}, {"ok": _one(1, np.uint32), "new_root": new_root})


# ---- merkleblocks -----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _merkleblocks(variant, one_tree):
    p = _proved(variant, one_tree)
    k, ntrees = int(p.trees.shape[0]), len(p.counts)

    def twin(hash_capacity, flag_capacity):
        out = [canary(k, np.uint32), canary(k, np.uint64), canary(k, np.uint64), canary(k + 1, np.uint64), canary(k + 1, np.uint64),
               canary(hash_capacity, np.uint32, 8), canary(flag_capacity, np.uint8), canary(4, np.uint64)]
        assert _host("vkmr_host_cpu_forest_merkleblocks", _cells(p.leaves), p.offsets, ntrees, _u32(p.trees), _u64(p.indices), k, *out[:6], hash_capacity,
                     out[6], flag_capacity, out[7]) == 0
        return out
    info = twin(66 * k, 26 * k)[7]
    hash_capacity, flag_capacity = int(info[2]) + 3, int(info[3]) + 5          # a few cells and bytes behind the used ones: they stay canary
    out = twin(hash_capacity, flag_capacity)
    names = ("block_trees", "block_counts", "bit_counts", "hash_starts", "byte_starts", "hashes", "flags", "info")
    args = {"indices_dev": In(p.indices), "k": k, "scratch_dev": SCRATCH, "block_trees_dev": Out("block_trees", k, np.uint32),
            "block_counts_dev": Out("block_counts", k, np.uint64), "bit_counts_dev": Out("bit_counts", k, np.uint64),
            "hash_starts_dev": Out("hash_starts", k + 1, np.uint64), "byte_starts_dev": Out("byte_starts", k + 1, np.uint64),
            "hashes_dev": _digests("hashes", hash_capacity), "hash_capacity": hash_capacity, "flags_dev": Out("flags", flag_capacity, np.uint8),
            "flag_capacity": flag_capacity, "info_dev": Out("info", 4, np.uint64)}
    if one_tree:
        st = StoredTree(p.leaves, p.stride)
        args.update({"digests_dev": st.leaves, "tree_dev": st.levels, "count": st.count, "height": st.height})
    else:
        sf = StoredForest(p.leaves, p.offsets, max(p.counts))
        args.update({"digests_dev": sf.leaves, "forest_dev": sf.levels, "total": sf.total, "offsets_dev": sf.offs, "ntrees": ntrees, "max_count": sf.max_count,
                     "trees_dev": In(p.trees)})
    return Case((k, p.stride), args, dict(zip(names, out)))


_forest_merkleblocks = functools.lru_cache(maxsize=None)(lambda variant: _merkleblocks(variant, False))
_tree_merkleblock = functools.lru_cache(maxsize=None)(lambda variant: _merkleblocks(variant, True))


# ---- diff ---------------------------------------------------------------------------------------------------------------------------------------------
def _diff_case(variant):
    """8 193 leaves side by side in a tree of 20 000: two mask bits an entry, 257 ranking words; 64 side by side in a tree of 150.
    capacity == n: every cell of the outputs is written (cells at and behind n would be unspecified)."""
    return dc.case("twenty_thousand", "run_of_8193") if variant == "large" else dc.case("side_by_side", "run_of_64")


@functools.lru_cache(maxsize=None)
def _forest_diff(variant):
    c = _diff_case(variant)
    a, b = StoredForest(c.a, c.offsets, c.max_count), StoredForest(c.b, c.offsets, c.max_count)
    return Case((c.n,), {"digests_a_dev": a.leaves, "forest_a_dev": a.levels, "roots_a_dev": a.roots, "digests_b_dev": b.leaves, "forest_b_dev": b.levels,
                         "roots_b_dev": b.roots, "total": c.total, "offsets_dev": In(c.offsets), "ntrees": c.ntrees, "max_count": c.max_count, "scratch_dev": SCRATCH,
                         "trees_out_dev": Out("trees_out", c.n, np.uint32), "indices_out_dev": Out("indices_out", c.n, np.uint64),
                         "leaves_b_out_dev": _digests("leaves_b_out", c.n), "capacity": c.n, "info_dev": Out("info", 4, np.uint64)},
                {"trees_out": c.trees, "indices_out": c.indices, "leaves_b_out": c.leaves_b, "info": np.array(c.info, dtype=np.uint64)})     # dc.model: no CPU twin


@functools.lru_cache(maxsize=None)
def _tree_diff(variant):
    c = _diff_case(variant)
    wa, wb = c.window(c.a), c.window(c.b)                          # the same leaves as ONE tree over the forest's cells
    count = int(wa.shape[0])
    height = tree_height(count)
    a, b = StoredTree(wa, height), StoredTree(wb, height)
    flat = np.flatnonzero((wa != wb).any(axis=1)).astype(np.uint64)
    assert (flat == _u64(c.flat)).all() and flat.shape[0] == c.n
    return Case((c.n,), {"digests_a_dev": a.leaves, "tree_a_dev": a.levels, "digests_b_dev": b.leaves, "tree_b_dev": b.levels, "count": count, "height": height,
                         "scratch_dev": SCRATCH, "indices_out_dev": Out("indices_out", c.n, np.uint64), "leaves_b_out_dev": _digests("leaves_b_out", c.n),
                         "capacity": c.n, "info_dev": Out("info", 4, np.uint64)},
                {"indices_out": flat, "leaves_b_out": wb[flat.astype(np.int64)], "info": np.array(dc.tree_counters(count, height, flat), dtype=np.uint64)})


# ---- audit --------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _audit_forest(variant):
    """audit_cases' largest forest twice over (17 758 leaves: 279 ballot words over its levels), the trees of 63, 64 and 65; an inner
    cell of levels 1 and 2 of the tallest tree and a root flipped: bad nodes on three levels."""
    counts = au.FORESTS[8][1] * 2 if variant == "large" else au.FORESTS[1][1]
    f = au.Forest(counts, seed=9700 + len(counts))
    picked = [c for c in au.forest_corruptions(f) if c[0] == "a_root" or c[0].endswith("_l1") and c[0].startswith("inner") or c[0].endswith("_l2") and c[0].startswith("inner")]
    assert len(picked) == 3
    for _, _, write, _ in picked:
        write()
    return f


@functools.lru_cache(maxsize=None)
def _forest_audit(variant):
    f = _audit_forest(variant)
    capacity = 8 if variant == "large" else 6
    rcode, info, masks, trees, levels, nodes = au.host_forest_audit(f, capacity)
    n_bad = int(info[1])
    assert rcode == 0 and int(info[0]) == 0 and 3 <= n_bad < capacity and len(set(levels[:n_bad].tolist())) >= 2      # cells behind n_bad stay canary
    assert variant == "small" or sum(-(-((f.total >> l) + f.ntrees) // 64) for l in range(1, f.levels + 1)) > 256
    return Case((f.total, f.ntrees, capacity), {"digests_dev": In(f.leaves), "forest_dev": In(f.forest), "roots_dev": In(f.roots), "total": f.total,
                                                "offsets_dev": In(f.offsets), "ntrees": f.ntrees, "max_count": f.max_count, "scratch_dev": SCRATCH,
                                                "masks_dev": Out("masks", f.ntrees, np.uint64), "bad_trees_dev": Out("bad_trees", capacity, np.uint32),
                                                "bad_levels_dev": Out("bad_levels", capacity, np.uint32), "bad_nodes_dev": Out("bad_nodes", capacity, np.uint64),
                                                "capacity": capacity, "info_dev": Out("info", 4, np.uint64)},
                {"masks": masks, "bad_trees": trees, "bad_levels": levels, "bad_nodes": nodes, "info": info})


@functools.lru_cache(maxsize=None)
def _tree_audit(variant):
    """A tree of 16 400 leaves (16 414 nodes above them: 257 ballot words and more) and the tree of 65; an inner cell of levels 1 and 2
    and the root flipped."""
    tr = au.Tree(BIG if variant == "large" else 65, seed=9800)
    for name, _, write, _ in au.tree_corruptions(tr):
        if name in ("the_root", "inner_l1", "inner_l2"):
            write()
    capacity = 8 if variant == "large" else 6
    rcode, info, levels, nodes = au.host_tree_audit(tr, capacity)
    n_bad = int(info[1])
    assert rcode == 0 and int(info[0]) == 0 and 3 <= n_bad < capacity and len(set(levels[:n_bad].tolist())) >= 2
    return Case((tr.count, 1, capacity), {"digests_dev": In(tr.leaves), "tree_dev": In(tr.tree), "count": tr.count, "height": tr.height, "scratch_dev": SCRATCH,
                                          "bad_levels_dev": Out("bad_levels", capacity, np.uint32), "bad_nodes_dev": Out("bad_nodes", capacity, np.uint64),
                                          "capacity": capacity, "info_dev": Out("info", 4, np.uint64)}, {"bad_levels": levels, "bad_nodes": nodes, "info": info})


# ---- frontier extend ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _frontier_extend(variant):
    """frontier_cases' EDGES (100 trees, 6 450 new leaves); the nine of them with 63, 64 or 65 leaves taking 63, 64 or 65."""
    b = fx.edges() if variant == "large" else fx.Batch([p for p in fx.EDGES if p[0] in (63, 64, 65) and p[1] in (63, 64, 65)], seed=304)
    status, new_counts, new_peaks, roots = fx.host_extend(b.counts, b.peaks, b.leaves, b.offsets)
    assert status == 0
    total_new, max_new = int(b.offsets[-1]), max(b.new_counts)
    return Case((total_new, b.T), {"counts_dev": In(b.counts), "peaks_dev": In(b.peaks), "stride": b.stride, "T": b.T, "leaves_dev": In(b.leaves),
                                   "total_new": total_new, "offsets_dev": In(b.offsets), "max_new": max_new, "scratch_dev": SCRATCH,
                                   "new_counts_dev": Out("new_counts", b.T, np.uint64), "new_peaks_dev": _digests("new_peaks", b.T * b.stride),
                                   "roots_dev": _digests("roots", b.T), "status_dev": Out("status", 1, np.uint32)},
                {"new_counts": new_counts, "new_peaks": new_peaks, "roots": roots, "status": _one(0, np.uint32)})


# ---- range proofs ---------------------------------------------------------------------------------------------------------------------------------------
class _Ranges(NamedTuple):
    cells: np.ndarray
    offsets: np.ndarray
    counts: list
    roots: np.ndarray
    trees: np.ndarray
    lo: np.ndarray
    hi: np.ndarray
    stride: int
    got: tuple                 # (firsts, leaf_starts, leaves [n, 8], left, right, heights, info) of the CPU twin


@functools.lru_cache(maxsize=None)
def _ranges(variant, one_tree):
    """range_cases' forest and all its queries; its first nine trees (157 leaves, none above 65) and the queries into them.  One
    tree: the tree of 2 500 (of 65) and its queries, over and over until they fill more than one workgroup of 256 (64 queries)."""
    f = rg.forest()
    _, trees, lo, hi = f.queries()
    if one_tree:
        t = 12 if variant == "large" else 8
        mine = np.flatnonzero(trees == t)
        mine = np.resize(mine, 300 if variant == "large" else 64)
        cells, offsets, counts, roots = f.trees[t], fc.offsets_of([f.counts[t]]), [f.counts[t]], f.roots[t: t + 1]
        trees, lo, hi = np.zeros(mine.shape[0], np.uint32), lo[mine], hi[mine]
    elif variant == "large":
        (cells, offsets), counts, roots = f.placed(first=37, slack=100), f.counts, f.roots
    else:
        keep = trees < 9
        cells, offsets, counts, roots = np.concatenate(f.trees[:9]), fc.offsets_of(f.counts[:9]), f.counts[:9], f.roots[:9]
        trees, lo, hi = trees[keep], lo[keep], hi[keep]
    stride = tree_height(max(counts))
    counted = rg.host_range(cells, offsets, trees, lo, hi, stride, capacity=0, guard=0)
    n = int(counted[7][1])
    got = rg.host_range(cells, offsets, trees, lo, hi, stride, capacity=n, guard=0)
    assert got[0] == 0 and int(got[7][0]) == 0 and n > 0
    return _Ranges(cells, offsets, list(counts), roots, trees, lo, hi, stride, got[1:])


def _range(variant, one_tree):
    r = _ranges(variant, one_tree)
    firsts, starts, leaves, left, right, heights, info = r.got
    Q, n = int(r.trees.shape[0]), int(leaves.shape[0])
    args = {"lo_dev": In(r.lo), "hi_dev": In(r.hi), "Q": Q, "scratch_dev": SCRATCH, "firsts_out_dev": Out("firsts", Q, np.uint64),
            "leaf_starts_out_dev": Out("leaf_starts", Q + 1, np.uint64), "leaves_out_dev": _digests("leaves", n), "leaves_capacity": n,
            "left_out_dev": _digests("left", Q * r.stride), "right_out_dev": _digests("right", Q * r.stride), "info_dev": Out("info", 4, np.uint64)}
    expected = {"firsts": firsts, "leaf_starts": starts, "leaves": leaves, "left": left, "right": right, "info": info}
    if one_tree:
        st = StoredTree(r.cells, r.stride)
        args.update({"digests_dev": st.leaves, "tree_dev": st.levels, "count": st.count, "height": st.height})
    else:
        sf = StoredForest(r.cells, r.offsets, max(r.counts))
        args.update({"digests_dev": sf.leaves, "forest_dev": sf.levels, "total": sf.total, "offsets_dev": sf.offs, "ntrees": sf.ntrees, "max_count": sf.max_count,
                     "trees_dev": In(r.trees), "stride": r.stride, "heights_out_dev": Out("heights", Q, np.uint32)})
        expected["heights"] = heights
    return Case((0, Q), args, expected)                              # "scratch_dev: vkmr_hip_range_scratch_bytes(0, Q) bytes"


def _verify_range(variant, one_tree):
    r = _ranges(variant, one_tree)
    firsts, starts, leaves, left, right, heights, info = r.got
    Q, n = int(r.trees.shape[0]), int(leaves.shape[0])
    verdict, in_first, in_count = rg.host_verify(r.trees, r.lo, r.hi, firsts, starts, leaves, left, right, heights, r.roots, r.counts)
    assert (verdict == 1).sum() > Q // 2 and in_count.any()
    args = {"lo_dev": In(r.lo), "hi_dev": In(r.hi), "firsts_dev": In(firsts), "leaf_starts_dev": In(starts), "leaves_dev": In(leaves), "nleaves": n,
            "left_dev": In(left), "right_dev": In(right), "Q": Q, "scratch_dev": SCRATCH, "verdict_dev": Out("verdict", Q, np.uint32),
            "in_first_dev": Out("in_first", Q, np.uint64), "in_count_dev": Out("in_count", Q, np.uint64)}
    if one_tree:
        args.update({"height": r.stride, "root_dev": In(r.roots), "count": r.counts[0]})
    else:
        args.update({"trees_dev": In(r.trees), "heights_dev": In(heights), "stride": r.stride, "roots_dev": In(r.roots), "counts_dev": In(r.counts, np.uint64),
                     "ntrees": len(r.counts)})
    return Case((n, Q), args, {"verdict": verdict, "in_first": in_first, "in_count": in_count})


_forest_range = functools.lru_cache(maxsize=None)(lambda variant: _range(variant, False))
_tree_range = functools.lru_cache(maxsize=None)(lambda variant: _range(variant, True))
_verify_forest_range = functools.lru_cache(maxsize=None)(lambda variant: _verify_range(variant, False))
_verify_tree_range = functools.lru_cache(maxsize=None)(lambda variant: _verify_range(variant, True))


# ---- the table ------------------------------------------------------------------------------------------------------------------------------------------
ROWS = [
    Row("vkmr_hip_reduce_async", "vkmr_hip_reduce_scratch_bytes", 16, _reduce),
    Row("vkmr_hip_metadata_from_sizes_async", "vkmr_hip_sizes_scratch_bytes", 16, _sizes),
    Row("vkmr_hip_reduce_slices_async", "vkmr_hip_reduce_slices_scratch_bytes", 16, _reduce_slices),
    Row("vkmr_hip_proof_async", "vkmr_hip_reduce_scratch_bytes", 16, _proof),
    Row("vkmr_hip_reduce_proofs_async", "vkmr_hip_reduce_scratch_bytes", 16, _reduce_proofs),
    Row("vkmr_hip_reduce_levels_async", "vkmr_hip_reduce_levels_scratch_bytes", 16, _reduce),
    Row("vkmr_hip_tree_multiproof_async", "vkmr_hip_multiproof_scratch_bytes", 16, _tree_multiproof),
    Row("vkmr_hip_verify_multiproof_async", "vkmr_hip_multiproof_scratch_bytes", 16, _verify_multiproof),
    Row("vkmr_hip_reduce_forest_async", "vkmr_hip_forest_scratch_bytes", 16, _reduce_forest),
    Row("vkmr_hip_reduce_forest_mutated_async", "vkmr_hip_forest_scratch_bytes", 16, functools.partial(_reduce_forest, mutated=True)),
    Row("vkmr_hip_forest_multiproof_async", "vkmr_hip_forest_multiproof_scratch_bytes", 16, _forest_multiproof),
    Row("vkmr_hip_verify_forest_multiproof_async", "vkmr_hip_forest_multiproof_scratch_bytes", 16, _verify_forest_multiproof),
    Row("vkmr_hip_apply_multiproof_async", "vkmr_hip_apply_multiproof_scratch_bytes", 16, _apply_multiproof),
    Row("vkmr_hip_apply_forest_multiproof_async", "vkmr_hip_apply_multiproof_scratch_bytes", 16, _apply_forest_multiproof),
    Row("vkmr_hip_forest_find_async", "vkmr_hip_find_scratch_bytes", 8, _forest_find),
    Row("vkmr_hip_tree_find_async", "vkmr_hip_find_scratch_bytes", 8, _tree_find),
    Row("vkmr_hip_forest_sort_entries_async", "vkmr_hip_sort_entries_scratch_bytes", 16, _forest_sort_entries, UNSPECIFIED_BEHIND_N),
    Row("vkmr_hip_tree_sort_entries_async", "vkmr_hip_sort_entries_scratch_bytes", 16, _tree_sort_entries, UNSPECIFIED_BEHIND_N),
    Row("vkmr_hip_forest_diff_async", "vkmr_hip_diff_scratch_bytes", 16, _forest_diff),
    Row("vkmr_hip_tree_diff_async", "vkmr_hip_diff_scratch_bytes", 16, _tree_diff),
    Row("vkmr_hip_forest_audit_async", "vkmr_hip_audit_scratch_bytes", 16, _forest_audit),
    Row("vkmr_hip_tree_audit_async", "vkmr_hip_audit_scratch_bytes", 16, _tree_audit, fixed=(1,)),                 # (count, 1, capacity)
    Row("vkmr_hip_frontier_extend_async", "vkmr_hip_frontier_extend_scratch_bytes", 16, _frontier_extend),
    Row("vkmr_hip_forest_merkleblocks_async", "vkmr_hip_forest_merkleblocks_scratch_bytes", 16, _forest_merkleblocks),
    Row("vkmr_hip_tree_merkleblock_async", "vkmr_hip_forest_merkleblocks_scratch_bytes", 16, _tree_merkleblock),
    Row("vkmr_hip_forest_range_async", "vkmr_hip_range_scratch_bytes", 16, _forest_range, fixed=(0,)),            # (0, Q)
    Row("vkmr_hip_tree_range_async", "vkmr_hip_range_scratch_bytes", 16, _tree_range, fixed=(0,)),
    Row("vkmr_hip_verify_forest_range_async", "vkmr_hip_range_scratch_bytes", 16, _verify_forest_range),
    Row("vkmr_hip_verify_range_async", "vkmr_hip_range_scratch_bytes", 16, _verify_tree_range),
    Row("vkmr_hip_forest_sort_leaves_async", "vkmr_hip_sort_leaves_scratch_bytes", 16, _forest_sort_leaves),
    Row("vkmr_hip_tree_sort_leaves_async", "vkmr_hip_sort_leaves_scratch_bytes", 16, _tree_sort_leaves),
    Row("vkmr_hip_forest_merge_leaves_async", "vkmr_hip_merge_leaves_scratch_bytes", 16, _forest_merge),
    Row("vkmr_hip_tree_merge_leaves_async", "vkmr_hip_merge_leaves_scratch_bytes", 16, _tree_merge, fixed=(2,)),   # one tree a side
    Row("vkmr_hip_combine_async", "vkmr_hip_reduce_scratch_bytes", 16, _combine),
]
BY_NAME = {row.name: row for row in ROWS}


def scratch_bytes(row, variant):
    """What the ABI's own size function answers for the variant (host-only: no device is needed)."""
    from vk_merkle_roots_amd import _abi
    return int(getattr(_abi.lib(), row.size_fn)(*row.size(variant)))
