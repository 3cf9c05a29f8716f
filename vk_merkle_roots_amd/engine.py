"""Thin Python driver over the C ABI, used by tests/ and bench.py.

Mirrors, call for call, what the C++ stream processor (csrc/host/hip_sha256d.cpp) does
with the same ABI: upload a packed batch, map it into a slice of digests, reduce each
slice to `height` levels, combine the slice roots.  All hashing happens on the GPU.
"""
import ctypes as C
import math

import numpy as np

from . import _abi
from ._abi import check


NO_TREE = 0xFFFFFFFF                # trees[q] of a digest that is no leaf (vkmr_hip_forest_find_async)
NOT_FOUND = 0xFFFFFFFFFFFFFFFF      # its index


def tree_height(count):
    """Levels of the duplicate-last tree over `count` leaves; a lone leaf is still
    hashed with itself once (CpuSha256D::Root's do-while, reference
    src/vkmr/SHA-256plus.cpp:515-547)."""
    if count <= 0:
        raise ValueError("count must be positive")
    return max(1, int(count - 1).bit_length())


class PackedBatch:
    """Strings packed as the reference's Batch does (src/vkmr/Batches.cpp:64-121):
    `data` uint32 words, `meta` uint32 [count, 2] = {start word, size bytes}."""

    def __init__(self, data, meta, words, nbytes):
        self.data = data
        self.meta = meta
        self.count = int(meta.shape[0])
        self.words = int(words)
        self.nbytes = int(nbytes)

    def slice(self, lo, hi):
        """Strings [lo, hi) as their own batch (metadata rebased to word 0)."""
        meta = self.meta[lo:hi].copy()
        if hi <= lo:
            return PackedBatch(self.data[:0], meta, 0, 0)
        w0 = int(meta[0, 0])
        w1 = int(meta[-1, 0]) + (int(meta[-1, 1]) + 3) // 4
        meta[:, 0] -= np.uint32(w0)
        return PackedBatch(self.data[w0:w1], meta, w1 - w0, int(meta[:, 1].astype(np.uint64).sum()))


def pack_lines(stream, data_capacity_words=None):
    """Split `stream` (bytes) with the reference's line rules and pack the lines."""
    h = _abi.host_lib()
    buf = np.frombuffer(stream, dtype=np.uint8)
    n = len(stream)
    max_count = n // 2 + 2
    cap = data_capacity_words or (n // 4 + max_count + 4)
    data = np.zeros(cap, dtype=np.uint32)
    meta = np.zeros((max_count, 2), dtype=np.uint32)
    words = C.c_uint64(0)
    nbytes = C.c_uint64(0)
    cnt = h.vkmr_host_pack_lines(buf.ctypes.data if n else None, n, data.ctypes.data, cap, meta.ctypes.data, max_count,
                                 C.byref(words), C.byref(nbytes))
    if cnt < 0:
        raise RuntimeError("pack_lines: buffers too small")
    return PackedBatch(data[: words.value], meta[:cnt], words.value, nbytes.value)


def rndm_packed(seed, count, maxlen):
    """The strings of `rndm seed count maxlen`, generated straight into a packed batch."""
    h = _abi.host_lib()
    cap = int(count) * ((maxlen - 2) // 4 + 1) + 4
    data = np.empty(cap, dtype=np.uint32)           # untouched pages cost nothing
    meta = np.empty((count, 2), dtype=np.uint32)
    words = C.c_uint64(0)
    cnt = h.vkmr_host_rndm_pack(seed, count, maxlen, data.ctypes.data, cap, meta.ctypes.data, C.byref(words))
    if cnt != count:
        raise RuntimeError("rndm_packed: buffer too small")
    return PackedBatch(data[: words.value], meta, words.value, int(meta[:, 1].astype(np.uint64).sum()))


class RndmStream:
    """The stream of `rndm seed * maxlen`, handed out as consecutive packed batches."""

    def __init__(self, seed, maxlen):
        self.h = _abi.host_lib()
        self.maxlen = maxlen
        self.handle = self.h.vkmr_host_rndm_open(seed)

    def next(self, count):
        cap = int(count) * ((self.maxlen - 2) // 4 + 1) + 4
        data = np.empty(cap, dtype=np.uint32)
        meta = np.empty((count, 2), dtype=np.uint32)
        words = C.c_uint64(0)
        if self.h.vkmr_host_rndm_next(self.handle, count, self.maxlen, data.ctypes.data, cap, meta.ctypes.data, C.byref(words)) != count:
            raise RuntimeError("RndmStream.next: batch exceeds 2^32 words")
        return PackedBatch(data[: words.value], meta, words.value, int(meta[:, 1].astype(np.uint64).sum()))

    def close(self):
        if self.handle:
            self.h.vkmr_host_rndm_close(self.handle)
            self.handle = None


class DeviceBuffer:
    def __init__(self, dev, nbytes):
        self.dev = dev
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        check(dev.lib.vkmr_hip_device_alloc(dev.index, max(self.nbytes, 32), C.byref(p)), "vkmr_hip_device_alloc")
        self.ptr = p.value

    def at(self, byte_offset):
        return self.ptr + int(byte_offset)

    def free(self):
        if self.ptr:
            self.dev.lib.vkmr_hip_device_free(self.dev.index, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class BufferScope:
    """The temporary device buffers of one `with dev.scope() as tmp:` block, freed on every way out of it, an exception
    included.  release() takes out the ones the block hands on to their new owner."""

    def __init__(self, dev):
        self.dev, self.bufs = dev, []

    def keep(self, buf):
        if buf:
            self.bufs.append(buf)
        return buf

    def alloc(self, nbytes):
        return self.keep(self.dev.alloc(nbytes))

    def upload(self, arr):
        return self.keep(self.dev.upload(arr))

    def release(self, *bufs):
        self.bufs = [b for b in self.bufs if not any(b is x for x in bufs)]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for b in self.bufs:
            b.free()
        self.bufs = []


def _host(arr, dtype, *shape):
    """A host array as the device calls take it: contiguous, of `dtype`, reshaped."""
    return np.ascontiguousarray(arr, dtype=dtype).reshape(*shape)


def _as_uint64(values, what, noun, plural, below=None, range_error=IndexError):
    """`values` as a flat uint64 array.  ValueError when they are not integers, `range_error` for a negative one or, with
    `below`, for one outside [0, below); no device call."""
    raw = np.asarray(values).reshape(-1)
    if raw.dtype.kind == "O" and below is not None:            # Python ints numpy could not fit in one integer type
        vals = [int(x) for x in raw]
        if any(v < 0 or v >= below for v in vals):
            raise range_error(f"{what}: {noun} outside [0, {below})")
        return np.array(vals, dtype=np.uint64)
    if raw.size and raw.dtype.kind not in "iu":
        raise ValueError(f"{what}: {plural} must be integers")
    if raw.dtype.kind == "i" and (raw < 0).any():
        raise range_error(f"{what}: negative {noun}")
    out = raw.astype(np.uint64)
    if below is not None and (out >= np.uint64(below)).any():
        raise range_error(f"{what}: {noun} outside [0, {below})")
    return out


class HipDevice:
    """One GPU + one stream.  Every method is one or two ABI calls."""

    def __init__(self, index=0):
        self.lib = _abi.lib()
        self.index = index
        n = C.c_int(0)
        check(self.lib.vkmr_hip_device_count(C.byref(n)), "vkmr_hip_device_count")
        if index >= n.value:
            raise RuntimeError(f"HIP device {index} not present ({n.value} device(s)): {_abi.what_error()}")
        s = C.c_void_p()
        check(self.lib.vkmr_hip_stream_create(index, C.byref(s)), "vkmr_hip_stream_create")
        self.stream = s.value

    # -- plumbing -----------------------------------------------------------------
    def _call(self, name, *args, stream=None):
        """The C function `name` on this device and `stream` (the device's own when None): a buffer goes as its pointer,
        None as NULL, an integer as it is.  VkmrError, naming the function, when the ABI refuses the call."""
        check(getattr(self.lib, name)(self.index, stream or self.stream, *[getattr(a, "ptr", a) for a in args]), name)

    def name(self):
        buf = C.create_string_buffer(256)
        check(self.lib.vkmr_hip_device_name(self.index, buf, 256), "vkmr_hip_device_name")
        return buf.value.decode()

    def alloc(self, nbytes):
        return DeviceBuffer(self, nbytes)

    def scope(self):
        """`with dev.scope() as tmp:` -- tmp.alloc / tmp.upload / tmp.keep give buffers that are freed when the block ends."""
        return BufferScope(self)

    def upload(self, arr, stream=None):
        arr = np.ascontiguousarray(arr)
        buf = DeviceBuffer(self, arr.nbytes)
        if arr.nbytes:
            self._call("vkmr_hip_memcpy_h2d_async", buf, arr.ctypes.data, arr.nbytes, stream=stream)
            self.sync(stream)
        return buf

    def download(self, buf, nbytes, dtype=np.uint32, offset=0, stream=None):
        out = np.empty(nbytes // np.dtype(dtype).itemsize, dtype=dtype)
        if nbytes:
            self._call("vkmr_hip_memcpy_d2h_async", out.ctypes.data, buf.at(offset), nbytes, stream=stream)
            self.sync(stream)
        return out

    def sync(self, stream=None):
        self._call("vkmr_hip_stream_sync", stream=stream)

    def new_stream(self):
        s = C.c_void_p()
        check(self.lib.vkmr_hip_stream_create(self.index, C.byref(s)), "vkmr_hip_stream_create")
        return s.value

    def warm_up(self, kernels=True, copy_bytes=1 << 20, stream=None):
        """vkmr_hip_warm_up: the kernels loaded onto the device, the copy engine up -- what a caller does at start-up
        instead of inside its first copy and first launch (the reference builds its pipelines then: Devices.cpp:225-280)."""
        self._call("vkmr_hip_warm_up", (1 if kernels else 0) | (2 if copy_bytes else 0), copy_bytes or 0, stream=stream)

    def new_event(self):
        e = C.c_void_p()
        check(self.lib.vkmr_hip_event_create(self.index, C.byref(e)), "vkmr_hip_event_create")
        return e.value

    def record(self, event, stream=None):
        check(self.lib.vkmr_hip_event_record(self.index, event, stream or self.stream), "vkmr_hip_event_record")

    def wait(self, event):
        check(self.lib.vkmr_hip_event_wait(self.index, event), "vkmr_hip_event_wait")

    def elapsed_ms(self, e0, e1):
        ms = C.c_float(0)
        check(self.lib.vkmr_hip_event_elapsed_ms(self.index, e0, e1, C.byref(ms)), "vkmr_hip_event_elapsed_ms")
        return ms.value

    # -- the hot path -------------------------------------------------------------
    def map_async(self, data_buf, data_words, meta_buf, count, out_buf, out_offset_digests=0, meta_offset=0, stream=None):
        self._call("vkmr_hip_map_async", data_buf, data_words, meta_buf.at(8 * meta_offset), count, out_buf.at(32 * out_offset_digests), stream=stream)

    def map_packed(self, tmp, batch, out_buf=None, out_offset_digests=0, meta=None):
        """The strings of `batch` (those of `meta`, rows of batch.meta, when given) mapped to leaf digests in device memory:
        into out_buf from digest out_offset_digests on, or into a new buffer, which is returned.  Enqueued, not waited for:
        the uploaded strings, and a new buffer, belong to the scope `tmp`, which must outlive the map (end it behind a sync
        or a download; tmp.release() a new buffer that is handed on)."""
        meta = batch.meta if meta is None else meta
        d_data = tmp.upload(batch.data if batch.words else np.zeros(1, np.uint32))
        d_meta = tmp.upload(meta)
        out = out_buf or tmp.alloc(32 * int(meta.shape[0]))
        self.map_async(d_data, batch.words, d_meta, int(meta.shape[0]), out, out_offset_digests=out_offset_digests)
        return out

    def reduce_async(self, digests_buf, count, height, scratch_buf, root_buf, root_index=0, levels_variant=False, stream=None):
        self._call("vkmr_hip_reduce_levels_async" if levels_variant else "vkmr_hip_reduce_async", digests_buf, count, height, scratch_buf,
                   root_buf.at(32 * root_index), stream=stream)

    def reduce_slices_async(self, digests_buf, nslices, capacity, count_last, height, scratch_buf, roots_buf, stream=None):
        self._call("vkmr_hip_reduce_slices_async", digests_buf, nslices, capacity, count_last, height, scratch_buf, roots_buf, stream=stream)

    def proof(self, digests_buf, count, height, index):
        """(siblings [height, 8], root [8]) of leaf `index` in the tree reduce_async(count, height) computes."""
        with self.scope() as tmp:
            d_sib, d_root, d_scratch = tmp.alloc(32 * max(height, 1)), tmp.alloc(32), tmp.keep(self.reduce_scratch(count))
            self._call("vkmr_hip_proof_async", digests_buf, count, height, index, d_scratch, d_sib, d_root)
            sib = self.download(d_sib, 32 * height).reshape(-1, 8) if height else np.zeros((0, 8), np.uint32)
            return sib, self.download(d_root, 32)

    def reduce_with_proofs(self, digests_buf, count, height, indices):
        """(siblings [k, height, 8], root [8]): the reduction that writes the proofs of leaves `indices` while it runs
        (vkmr_hip_reduce_proofs_async; k <= 16)."""
        idx = np.ascontiguousarray(indices, dtype=np.uint64)
        k = int(idx.shape[0])
        with self.scope() as tmp:
            d_sib, d_root, d_scratch = tmp.alloc(32 * max(height, 1) * max(k, 1)), tmp.alloc(32), tmp.keep(self.reduce_scratch(count))
            self._call("vkmr_hip_reduce_proofs_async", digests_buf, count, height, d_scratch, d_root, idx.ctypes.data if k else None, k, d_sib)
            sib = self.download(d_sib, 32 * height * k).reshape(k, height, 8) if height and k else np.zeros((k, height, 8), np.uint32)
            return sib, self.download(d_root, 32)

    # -- stored tree: build, gather proofs, verify -----------------------------------
    def tree_bytes(self, count, height):
        return self.lib.vkmr_hip_tree_bytes(count, height)

    def reduce_tree_async(self, digests_buf, count, height, tree_buf, stream=None):
        self._call("vkmr_hip_reduce_tree_async", digests_buf, count, height, tree_buf, stream=stream)

    def tree_proofs_async(self, digests_buf, tree_buf, count, height, indices_buf, k, siblings_buf, stream=None):
        self._call("vkmr_hip_tree_proofs_async", digests_buf, tree_buf, count, height, indices_buf, k, siblings_buf, stream=stream)

    def verify_proofs_async(self, leaves_buf, indices_buf, siblings_buf, k, height, roots_buf, nroots, ok_buf, stream=None):
        self._call("vkmr_hip_verify_proofs_async", leaves_buf, indices_buf, siblings_buf, k, height, roots_buf, nroots, ok_buf, stream=stream)

    def tree_update_async(self, digests_buf, tree_buf, count, height, indices_buf, leaves_buf, k, status_buf, stream=None):
        self._call("vkmr_hip_tree_update_async", digests_buf, tree_buf, count, height, indices_buf, leaves_buf, k, status_buf, stream=stream)

    def tree_multiproof_async(self, digests_buf, tree_buf, count, height, indices_buf, k, scratch_buf, nodes_buf, nodes_capacity, info_buf,
                              stream=None):
        self._call("vkmr_hip_tree_multiproof_async", digests_buf, tree_buf, count, height, indices_buf, k, scratch_buf, nodes_buf, nodes_capacity,
                   info_buf, stream=stream)

    def verify_multiproof_async(self, leaves_buf, indices_buf, k, height, nodes_buf, m, root_buf, scratch_buf, ok_buf, stream=None):
        self._call("vkmr_hip_verify_multiproof_async", leaves_buf, indices_buf, k, height, nodes_buf, m, root_buf, scratch_buf, ok_buf, stream=stream)

    def verify_multiproof(self, leaves, indices, nodes, root, height):
        """bool: the multiproof `nodes` ([M, 8]) proves leaves ([k, 8]) at `indices` ([k], strictly increasing) under `root`
        in a tree of `height` levels (1..63).  Host arrays in, verified on the device; no leaf proves nothing: False."""
        leaves, idx, nodes, root = _host(leaves, np.uint32, -1, 8), _host(indices, np.uint64, -1), _host(nodes, np.uint32, -1, 8), _host(root, np.uint32, 8)
        k, m = int(idx.shape[0]), int(nodes.shape[0])
        if leaves.shape[0] != k:
            raise ValueError("verify_multiproof: one leaf per index")
        if k == 0:
            return False
        with self.scope() as tmp:
            d_leaves, d_idx, d_nodes, d_root = (tmp.upload(a) for a in (leaves, idx, nodes, root))
            d_scr, d_ok = tmp.alloc(self.lib.vkmr_hip_multiproof_scratch_bytes(k, height)), tmp.alloc(4)
            self.verify_multiproof_async(d_leaves, d_idx, k, height, d_nodes if m else None, m, d_root, d_scr, d_ok)
            return int(self.download(d_ok, 4)[0]) == 1

    def build_tree(self, digests_buf, count, height=None):
        """Every level of the tree over `count` digests in `digests_buf` (which stays level 0 and must outlive the tree),
        kept on the device: a MerkleTree."""
        height = tree_height(count) if height is None else height
        tree_buf = self.alloc(self.tree_bytes(count, height)) if height else None
        self.reduce_tree_async(digests_buf, count, height, tree_buf)
        return MerkleTree(self, digests_buf, count, height, tree_buf)

    def verify_proofs(self, leaves, indices, siblings, roots):
        """bool [k]: proof q (leaf [8], index, siblings [height, 8]) folds to roots[0] (roots [8] or [1, 8]) or roots[q]
        (roots [k, 8]), its index inside the tree.  Host arrays in, verified on the device."""
        leaves, idx, roots = _host(leaves, np.uint32, -1, 8), _host(indices, np.uint64, -1), _host(roots, np.uint32, -1, 8)
        k = int(idx.shape[0])
        siblings = _host(siblings, np.uint32, k, -1, 8)
        if leaves.shape[0] != k or roots.shape[0] not in (1, k):
            raise ValueError("verify_proofs: one leaf per index, and one root or one per proof")
        if k == 0:
            return np.zeros(0, dtype=bool)
        with self.scope() as tmp:
            d_leaves, d_idx, d_sib, d_roots = (tmp.upload(a) for a in (leaves, idx, siblings, roots))
            d_ok = tmp.alloc(4 * k)
            self.verify_proofs_async(d_leaves, d_idx, d_sib, k, siblings.shape[1], d_roots, roots.shape[0], d_ok)
            return self.download(d_ok, 4 * k) == 1

    # -- forest: the roots of many trees of unequal size in one call ----------------------
    def reduce_forest_async(self, digests_buf, total, offsets_buf, ntrees, max_count, scratch_buf, roots_buf, status_buf, stream=None):
        self._call("vkmr_hip_reduce_forest_async", digests_buf, total, offsets_buf, ntrees, max_count, scratch_buf, roots_buf, status_buf, stream=stream)

    def reduce_forest_mutated_async(self, digests_buf, total, offsets_buf, ntrees, max_count, scratch_buf, roots_buf, mutated_buf, status_buf,
                                    stream=None):
        self._call("vkmr_hip_reduce_forest_mutated_async", digests_buf, total, offsets_buf, ntrees, max_count, scratch_buf, roots_buf, mutated_buf,
                   status_buf, stream=stream)

    def _reduce_forest(self, tmp, d_leaves, total, offsets, ntrees, max_count, what, stored, d_mutated=None):
        """One forest call over checked offsets (ntrees >= 1), its buffers in the scope `tmp`: the roots alone, or with
        `stored` every level kept; with d_mutated (8 * ntrees bytes) the flagged build, which fills it.  (max_count, offsets
        buffer, level buffer, roots buffer); ValueError when the device refuses the forest."""
        if max_count is None:
            max_count = max(1, int(np.diff(offsets).max()))
        d_off, d_roots, d_status = tmp.upload(offsets), tmp.alloc(32 * ntrees), tmp.alloc(4)
        build = {(False, False): self.reduce_forest_async, (False, True): self.reduce_forest_mutated_async,
                 (True, False): self.reduce_forest_tree_async, (True, True): self.reduce_forest_tree_mutated_async}[stored, bool(d_mutated)]
        d_levels = tmp.alloc(self.forest_tree_bytes(total, ntrees, max_count) if stored else self.lib.vkmr_hip_forest_scratch_bytes(total, ntrees))
        build(d_leaves, total, d_off, ntrees, max_count, d_levels, d_roots, *([d_mutated] if d_mutated else []), d_status)
        status = int(self.download(d_status, 4)[0])
        if status:
            raise ValueError(f"{what}: the device refused the forest (status {status}: {forest_status_text(status)})")
        return max_count, d_off, d_levels, d_roots

    def _forest_of_buffer(self, d_leaves, total, counts, max_count, what, mutated=False):
        """[ntrees, 8] uint32: the roots of the trees of `counts` leaves each over the `total` cells of d_leaves; with
        `mutated` from the flagged build, and (roots, masks [ntrees] uint64)."""
        offsets, ntrees = _checked_offsets(counts, total, what)
        if ntrees == 0:
            roots, masks = np.zeros((0, 8), dtype=np.uint32), np.zeros(0, dtype=np.uint64)
            return (roots, masks) if mutated else roots
        with self.scope() as tmp:
            d_mut = tmp.alloc(8 * ntrees) if mutated else None
            d_roots = self._reduce_forest(tmp, d_leaves, total, offsets, ntrees, max_count, what, stored=False, d_mutated=d_mut)[3]
            roots = self.download(d_roots, 32 * ntrees).reshape(ntrees, 8)
            return (roots, self.download(d_mut, 8 * ntrees, dtype=np.uint64)) if mutated else roots

    def _forest_of_digests(self, digests, counts, max_count, what, mutated):
        digests = _host(digests, np.uint32, -1, 8)
        total = int(digests.shape[0])
        with self.scope() as tmp:
            return self._forest_of_buffer(tmp.upload(digests) if total else None, total, counts, max_count, what, mutated=mutated)

    def forest_roots(self, digests, counts, max_count=None):
        """[ntrees, 8] uint32: the root of every tree of a forest (vkmr_hip_reduce_forest_async).  `digests` [total, 8] holds the
        leaves of all trees back to back, tree t the next counts[t] of them; an empty tree gets an all-zero root.  max_count:
        an upper bound on every count (the largest count when None).  ValueError when the counts do not add up to the
        leaves, or when the device refuses the forest (a count above max_count)."""
        return self._forest_of_digests(digests, counts, max_count, "forest_roots", mutated=False)

    def forest_roots_mutated(self, digests, counts, max_count=None):
        """(roots, mutated): forest_roots, and uint64 [ntrees] whose bit l is set when level l of the tree holds two equal
        siblings that both exist (vkmr_hip_reduce_forest_mutated_async; CVE-2012-2459: such a tree shares its root with a
        shorter leaf list).  `mutated != 0` is Bitcoin Core's flag.  Same arguments and errors as forest_roots."""
        return self._forest_of_digests(digests, counts, max_count, "forest_roots_mutated", mutated=True)

    # -- stored forest: every level kept, proofs gathered from it, proofs of unequal height verified --
    def forest_tree_bytes(self, total, ntrees, max_count):
        return self.lib.vkmr_hip_forest_tree_bytes(total, ntrees, max_count)

    def reduce_forest_tree_async(self, digests_buf, total, offsets_buf, ntrees, max_count, forest_buf, roots_buf, status_buf, stream=None):
        self._call("vkmr_hip_reduce_forest_tree_async", digests_buf, total, offsets_buf, ntrees, max_count, forest_buf, roots_buf, status_buf,
                   stream=stream)

    def reduce_forest_tree_mutated_async(self, digests_buf, total, offsets_buf, ntrees, max_count, forest_buf, roots_buf, mutated_buf, status_buf,
                                         stream=None):
        self._call("vkmr_hip_reduce_forest_tree_mutated_async", digests_buf, total, offsets_buf, ntrees, max_count, forest_buf, roots_buf, mutated_buf,
                   status_buf, stream=stream)

    def forest_tree_mutated_async(self, digests_buf, forest_buf, total, offsets_buf, ntrees, max_count, mutated_buf, stream=None):
        self._call("vkmr_hip_forest_tree_mutated_async", digests_buf, forest_buf, total, offsets_buf, ntrees, max_count, mutated_buf, stream=stream)

    def forest_proofs_async(self, digests_buf, forest_buf, total, offsets_buf, ntrees, max_count, trees_buf, indices_buf, k, siblings_buf,
                            heights_buf, stream=None):
        self._call("vkmr_hip_forest_proofs_async", digests_buf, forest_buf, total, offsets_buf, ntrees, max_count, trees_buf, indices_buf, k,
                   siblings_buf, heights_buf, stream=stream)

    def verify_forest_proofs_async(self, leaves_buf, trees_buf, indices_buf, siblings_buf, heights_buf, k, stride, roots_buf, ntrees, ok_buf,
                                   stream=None):
        self._call("vkmr_hip_verify_forest_proofs_async", leaves_buf, trees_buf, indices_buf, siblings_buf, heights_buf, k, stride, roots_buf, ntrees,
                   ok_buf, stream=stream)

    def forest_update_async(self, digests_buf, forest_buf, total, offsets_buf, ntrees, max_count, trees_buf, indices_buf, leaves_buf, k, roots_buf,
                            status_buf, stream=None):
        self._call("vkmr_hip_forest_update_async", digests_buf, forest_buf, total, offsets_buf, ntrees, max_count, trees_buf, indices_buf, leaves_buf,
                   k, roots_buf, status_buf, stream=stream)

    def forest_multiproof_async(self, digests_buf, forest_buf, total, offsets_buf, ntrees, max_count, trees_buf, indices_buf, k, scratch_buf,
                                nodes_buf, nodes_capacity, heights_buf, info_buf, stream=None):
        self._call("vkmr_hip_forest_multiproof_async", digests_buf, forest_buf, total, offsets_buf, ntrees, max_count, trees_buf, indices_buf, k,
                   scratch_buf, nodes_buf, nodes_capacity, heights_buf, info_buf, stream=stream)

    def verify_forest_multiproof_async(self, leaves_buf, trees_buf, indices_buf, heights_buf, k, stride, nodes_buf, m, roots_buf, ntrees,
                                       scratch_buf, ok_buf, stream=None):
        self._call("vkmr_hip_verify_forest_multiproof_async", leaves_buf, trees_buf, indices_buf, heights_buf, k, stride, nodes_buf, m, roots_buf,
                   ntrees, scratch_buf, ok_buf, stream=stream)

    def verify_forest_multiproof(self, leaves, trees, indices, heights, nodes, roots):
        """bool: the forest multiproof `nodes` ([M, 8], level-major over the whole forest) proves leaves ([k, 8]) at the
        strictly increasing (trees[q], indices[q]) under roots[trees[q]] (roots [ntrees, 8]), heights[q] being the height of
        entry q's tree (vkmr_hip_verify_forest_multiproof_async).  Host arrays in, verified on the device; no leaf proves
        nothing: False."""
        leaves, trees, idx = _host(leaves, np.uint32, -1, 8), _host(trees, np.uint32, -1), _host(indices, np.uint64, -1)
        heights, nodes, roots = _host(heights, np.uint32, -1), _host(nodes, np.uint32, -1, 8), _host(roots, np.uint32, -1, 8)
        k, m = int(idx.shape[0]), int(nodes.shape[0])
        if leaves.shape[0] != k or trees.shape[0] != k or heights.shape[0] != k:
            raise ValueError("verify_forest_multiproof: one leaf, one tree and one height per index")
        if k == 0:
            return False
        if roots.shape[0] == 0:
            raise ValueError("verify_forest_multiproof: no root")
        stride = max(1, min(63, int(heights.max())))       # a height above 63 is refused by the device's check
        with self.scope() as tmp:
            d_leaves, d_trees, d_idx, d_h, d_nodes, d_roots = (tmp.upload(a) for a in (leaves, trees, idx, heights, nodes, roots))
            d_scr, d_ok = tmp.alloc(self.lib.vkmr_hip_forest_multiproof_scratch_bytes(k, stride)), tmp.alloc(4)
            self.verify_forest_multiproof_async(d_leaves, d_trees, d_idx, d_h, k, stride, d_nodes if m else None, m, d_roots, roots.shape[0],
                                                d_scr, d_ok)
            return int(self.download(d_ok, 4)[0]) == 1

    # -- applying a multiproof: a holder of the roots alone follows leaf updates ----------
    def apply_multiproof_scratch_bytes(self, k, levels):
        return self.lib.vkmr_hip_apply_multiproof_scratch_bytes(k, levels)

    def apply_multiproof_enqueue(self, old_leaves_buf, new_leaves_buf, indices_buf, k, count, height, nodes_buf, m, root_buf, scratch_buf, ok_buf,
                                 new_root_buf, stream=None):
        self._call("vkmr_hip_apply_multiproof_async", old_leaves_buf, new_leaves_buf, indices_buf, k, count, height, nodes_buf, m, root_buf,
                   scratch_buf, ok_buf, new_root_buf, stream=stream)

    def apply_forest_multiproof_enqueue(self, old_leaves_buf, new_leaves_buf, trees_buf, indices_buf, counts_buf, k, stride, nodes_buf, m,
                                        roots_buf, ntrees, scratch_buf, ok_buf, new_roots_buf, stream=None):
        self._call("vkmr_hip_apply_forest_multiproof_async", old_leaves_buf, new_leaves_buf, trees_buf, indices_buf, counts_buf, k, stride,
                   nodes_buf, m, roots_buf, ntrees, scratch_buf, ok_buf, new_roots_buf, stream=stream)

    def apply_multiproof(self, old_leaves, new_leaves, indices, nodes, root, count, height=None):
        """The new root [8] of a tree of `count` leaves (and `height` levels; None: the minimal height) after the leaves at
        `indices` ([k], strictly increasing) went from old_leaves to new_leaves ([k, 8] each), from the old `root` and the
        multiproof `nodes` ([M, 8]) gathered before the update alone; None when the proof is refused: the old leaves do not
        fold to `root`, or the indices and the count do not fit (vkmr_hip_apply_multiproof_async).  Host arrays in, folded
        on the device; no leaf changes nothing: None."""
        old, new = _digest_pairs(old_leaves, new_leaves, "apply_multiproof")
        idx, nodes, root = _host(indices, np.uint64, -1), _host(nodes, np.uint32, -1, 8), _host(root, np.uint32, 8)
        k, m = int(idx.shape[0]), int(nodes.shape[0])
        if old.shape[0] != k:
            raise ValueError("apply_multiproof: one old and one new leaf per index")
        height = (tree_height(int(count)) if int(count) > 0 else 1) if height is None else int(height)   # no leaf: the device answers 0
        if k == 0:
            return None
        with self.scope() as tmp:
            d_old, d_new, d_idx, d_nodes, d_root = (tmp.upload(a) for a in (old, new, idx, nodes, root))
            d_scr, d_ok, d_out = tmp.alloc(self.apply_multiproof_scratch_bytes(k, height)), tmp.alloc(4), tmp.alloc(32)
            self.apply_multiproof_enqueue(d_old, d_new, d_idx, k, int(count), height, d_nodes if m else None, m, d_root, d_scr, d_ok, d_out)
            return self.download(d_out, 32) if int(self.download(d_ok, 4)[0]) == 1 else None

    def apply_forest_multiproof(self, old_leaves, new_leaves, trees, indices, counts, nodes, roots):
        """The roots [ntrees, 8] of a forest after the leaves at the strictly increasing (trees[q], indices[q]) went from
        old_leaves to new_leaves ([k, 8] each) -- a copy of `roots` with the named trees advanced -- from the old roots, the
        forest multiproof `nodes` ([M, 8]) gathered before the update and counts[q], the leaf count of entry q's tree, alone;
        None when the proof is refused (vkmr_hip_apply_forest_multiproof_async).  Host arrays in, folded on the device; no
        leaf changes nothing: None."""
        old, new = _digest_pairs(old_leaves, new_leaves, "apply_forest_multiproof")
        trees, idx, counts = _host(trees, np.uint32, -1), _host(indices, np.uint64, -1), _host(counts, np.uint64, -1)
        nodes, roots = _host(nodes, np.uint32, -1, 8), _host(roots, np.uint32, -1, 8)
        k, m = int(idx.shape[0]), int(nodes.shape[0])
        if old.shape[0] != k or trees.shape[0] != k or counts.shape[0] != k:
            raise ValueError("apply_forest_multiproof: one old leaf, one new leaf, one tree and one count per index")
        if k == 0:
            return None
        if roots.shape[0] == 0:
            raise ValueError("apply_forest_multiproof: no root")
        # a count of 0 and a height above 63 are refused by the device's checks
        stride = min(63, max(tree_height(int(c)) if c else 1 for c in np.unique(counts)))
        with self.scope() as tmp:
            d_old, d_new, d_trees, d_idx, d_counts, d_nodes, d_roots = (tmp.upload(a) for a in (old, new, trees, idx, counts, nodes, roots))
            d_scr, d_ok = tmp.alloc(self.apply_multiproof_scratch_bytes(k, stride)), tmp.alloc(4)
            self.apply_forest_multiproof_enqueue(d_old, d_new, d_trees, d_idx, d_counts, k, stride, d_nodes if m else None, m, d_roots,
                                                 roots.shape[0], d_scr, d_ok, d_roots)      # in place: d_roots is this call's own copy
            if int(self.download(d_ok, 4)[0]) != 1:
                return None
            return self.download(d_roots, roots.nbytes).reshape(-1, 8)

    def _build_forest_of_buffer(self, d_leaves, total, counts, max_count, what, owned=(), mutated=False, reserve_trees=0, reserve_leaves=0):
        """A MerkleForest of the trees of `counts` leaves each over the `total` cells of d_leaves (its level 0); with `mutated`
        built by the flagged twin, whose masks it keeps.  The last reserve_leaves of the `total` cells stay free behind the
        last leaf, and reserve_trees empty trees follow the last tree: room for MerkleForest.append."""
        reserve_trees, reserve_leaves = _reserve(what, reserve_trees, reserve_leaves, max_count)
        offsets, used_trees = _checked_offsets(counts, total, what, slack=reserve_leaves)
        ntrees = used_trees + reserve_trees
        if reserve_trees:
            offsets = np.concatenate([offsets, np.full(reserve_trees, offsets[-1], dtype=np.uint64)])
        if ntrees == 0:
            raise ValueError(f"{what}: no tree")
        with self.scope() as tmp:
            d_mut = tmp.alloc(8 * ntrees) if mutated else None
            max_count, d_off, d_forest, d_roots = self._reduce_forest(tmp, d_leaves, total, offsets, ntrees, max_count, what, stored=True,
                                                                      d_mutated=d_mut)
            masks = self.download(d_mut, 8 * ntrees, dtype=np.uint64) if mutated else None
            tmp.release(d_off, d_forest, d_roots)      # the forest's from here on
        return MerkleForest(self, d_leaves, total, np.diff(offsets), d_off, max_count, d_forest, d_roots, owned=owned, built_mutated=masks,
                            used_trees=used_trees)

    def build_forest(self, digests, counts, max_count=None, mutated=False, reserve_trees=0, reserve_leaves=0):
        """Every level of every tree of a forest, kept on the device: a MerkleForest (vkmr_hip_reduce_forest_tree_async).
        `digests` [total, 8] (a host array) holds the leaves of all trees back to back, tree t the next counts[t] of them;
        max_count: an upper bound on every count (the largest count when None).  mutated=True builds with
        vkmr_hip_reduce_forest_tree_mutated_async -- the same forest -- and keeps the build's masks in `built_mutated`.
        reserve_trees, reserve_leaves: room for MerkleForest.append -- that many empty trees behind the last tree and spare
        cells behind the last leaf; max_count must then be given, it bounds the trees still to come.
        ValueError when the counts do not add up to the leaves, for no tree at all, for room reserved without a max_count, or
        when the device refuses the forest (a count above max_count)."""
        digests = _host(digests, np.uint32, -1, 8)
        reserve_trees, reserve_leaves = _reserve("build_forest", reserve_trees, reserve_leaves, max_count)
        used, total = int(digests.shape[0]), int(digests.shape[0]) + reserve_leaves
        with self.scope() as tmp:
            if reserve_leaves:
                d_in = tmp.alloc(32 * total)
                if used:
                    self._call("vkmr_hip_memcpy_h2d_async", d_in, digests.ctypes.data, digests.nbytes)
                    self.sync()
            else:
                d_in = tmp.upload(digests) if total else None
            forest = self._build_forest_of_buffer(d_in, total, counts, max_count, "build_forest", owned=[d_in] if d_in else [], mutated=mutated,
                                                  reserve_trees=reserve_trees, reserve_leaves=reserve_leaves)
            tmp.release(d_in)
        return forest

    def verify_forest_proofs(self, leaves, trees, indices, siblings, heights, roots):
        """bool [k]: proof q (leaf [8], tree, index, siblings [stride, 8] of which the first heights[q] count) folds to
        roots[trees[q]] (roots [ntrees, 8]), with 1 <= heights[q] <= stride, its index below 2^heights[q] and its tree below
        ntrees (vkmr_hip_verify_forest_proofs_async).  Host arrays in, verified on the device."""
        leaves, trees, idx = _host(leaves, np.uint32, -1, 8), _host(trees, np.uint32, -1), _host(indices, np.uint64, -1)
        heights, roots = _host(heights, np.uint32, -1), _host(roots, np.uint32, -1, 8)
        k = int(idx.shape[0])
        siblings = _host(siblings, np.uint32, k, -1, 8)
        if leaves.shape[0] != k or trees.shape[0] != k or heights.shape[0] != k:
            raise ValueError("verify_forest_proofs: one leaf, one tree and one height per index")
        if k == 0:
            return np.zeros(0, dtype=bool)
        if roots.shape[0] == 0:
            raise ValueError("verify_forest_proofs: no root")
        with self.scope() as tmp:
            d_leaves, d_trees, d_idx, d_sib, d_h, d_roots = (tmp.upload(a) for a in (leaves, trees, idx, siblings, heights, roots))
            d_ok = tmp.alloc(4 * k)
            self.verify_forest_proofs_async(d_leaves, d_trees, d_idx, d_sib, d_h, k, siblings.shape[1], d_roots, roots.shape[0], d_ok)
            return self.download(d_ok, 4 * k) == 1

    # -- leaves by digest: where in a tree or forest is this hash? ------------------------------
    def find_scratch_bytes(self, k):
        return self.lib.vkmr_hip_find_scratch_bytes(k)

    def forest_find_async(self, digests_buf, total, offsets_buf, ntrees, queries_buf, k, scratch_buf, trees_buf, indices_buf, stream=None):
        """trees_buf[q], indices_buf[q] = where queries_buf[q] (a digest) is a leaf of the forest: the lowest position wins; not
        found: 0xFFFFFFFF and 2^64 - 1.  All in device memory; scratch_buf: find_scratch_bytes(k).  include/vkmr_hip.h."""
        self._call("vkmr_hip_forest_find_async", digests_buf, total, offsets_buf, ntrees, queries_buf, k, scratch_buf, trees_buf, indices_buf,
                   stream=stream)

    def tree_find_async(self, digests_buf, count, queries_buf, k, scratch_buf, indices_buf, stream=None):
        """indices_buf[q] = the lowest index at which queries_buf[q] is a leaf of the tree over digests_buf[0 .. count), or
        2^64 - 1.  All in device memory; scratch_buf: find_scratch_bytes(k)."""
        self._call("vkmr_hip_tree_find_async", digests_buf, count, queries_buf, k, scratch_buf, indices_buf, stream=stream)

    # -- leaf entries sorted and deduplicated on the device: find -> update, find -> multiproof -----
    def sort_entries_scratch_bytes(self, total, k):
        return self.lib.vkmr_hip_sort_entries_scratch_bytes(total, k)

    def forest_sort_entries_async(self, total, offsets_buf, ntrees, trees_buf, indices_buf, k, scratch_buf, trees_out_buf, indices_out_buf,
                                  order_out_buf, info_buf, stream=None):
        """The k entries (trees_buf[q], indices_buf[q]), in any order, as the distinct valid pairs in strictly increasing order
        in cells [0, n) of trees_out_buf / indices_out_buf, order_out_buf[j] (uint32) the last q that holds pair j; info_buf:
        4 uint64 = n, "not found" markers, entries out of range, earlier repeats.  All in device memory; scratch_buf:
        sort_entries_scratch_bytes(total, k), 16-byte aligned.  include/vkmr_hip.h."""
        self._call("vkmr_hip_forest_sort_entries_async", total, offsets_buf, ntrees, trees_buf, indices_buf, k, scratch_buf, trees_out_buf,
                   indices_out_buf, order_out_buf, info_buf, stream=stream)

    def tree_sort_entries_async(self, count, indices_buf, k, scratch_buf, indices_out_buf, order_out_buf, info_buf, stream=None):
        """forest_sort_entries_async for one tree of `count` leaves: indices alone, the marker being 2^64 - 1."""
        self._call("vkmr_hip_tree_sort_entries_async", count, indices_buf, k, scratch_buf, indices_out_buf, order_out_buf, info_buf, stream=stream)

    def gather_digests_async(self, src_buf, order_buf, n, dst_buf, stream=None):
        """dst_buf[j] = src_buf[order_buf[j]], j < n: digests of 32 bytes, order uint32, all in device memory."""
        self._call("vkmr_hip_gather_digests_async", src_buf, order_buf, n, dst_buf, stream=stream)

    # -- two stored forests or trees of one shape: the leaves that differ, found from the roots down -----
    def diff_scratch_bytes(self, capacity):
        return self.lib.vkmr_hip_diff_scratch_bytes(capacity)

    def forest_diff_async(self, digests_a_buf, forest_a_buf, roots_a_buf, digests_b_buf, forest_b_buf, roots_b_buf, total, offsets_buf, ntrees,
                          max_count, scratch_buf, trees_buf, indices_buf, leaves_buf, capacity, info_buf, stream=None):
        """Cells [0, n) of trees_buf / indices_buf = the (tree, index) pairs, strictly increasing, of the leaves in which the
        stored forests A and B (same offsets, total, ntrees, max_count) differ; leaves_buf (or None): B's leaves there.
        info_buf: 4 uint64 = status (bit 2: more than `capacity` differ), n, trees whose roots differ, nodes whose children
        were compared.  All in device memory; scratch_buf: diff_scratch_bytes(capacity), 16-byte aligned.  include/vkmr_hip.h."""
        self._call("vkmr_hip_forest_diff_async", digests_a_buf, forest_a_buf, roots_a_buf, digests_b_buf, forest_b_buf, roots_b_buf, total, offsets_buf,
                   ntrees, max_count, scratch_buf, trees_buf, indices_buf, leaves_buf, capacity, info_buf, stream=stream)

    def tree_diff_async(self, digests_a_buf, tree_a_buf, digests_b_buf, tree_b_buf, count, height, scratch_buf, indices_buf, leaves_buf, capacity,
                        info_buf, stream=None):
        """forest_diff_async for two stored trees of one `count` and `height`: indices alone."""
        self._call("vkmr_hip_tree_diff_async", digests_a_buf, tree_a_buf, digests_b_buf, tree_b_buf, count, height, scratch_buf, indices_buf,
                   leaves_buf, capacity, info_buf, stream=stream)

    # -- a stored forest or tree audited in place: the nodes that are not the hash of their stored children -----
    def audit_scratch_bytes(self, total, ntrees, capacity):
        """Scratch of an audit with room for `capacity` listed nodes: 0 for capacity 0; a tree: (count, 1, capacity)."""
        return self.lib.vkmr_hip_audit_scratch_bytes(total, ntrees, capacity)

    # The *_enqueue wrappers, from here on, are asynchronous like every *_async wrapper above.  They do not carry that suffix
    # because the *_async wrappers of this class are a closed list, recorded call by call in tests/golden/engine_calls.json.
    # tests/test_engine_calls.py pins both families: those against the record, these against include/vkmr_hip.h.
    def forest_audit_enqueue(self, digests_buf, forest_buf, roots_buf, total, offsets_buf, ntrees, max_count, scratch_buf, masks_buf, trees_buf,
                             levels_buf, nodes_buf, capacity, info_buf, stream=None):
        """masks_buf[t] (uint64) bit l - 1 = level l of tree t holds a node that is not hash_pair of its two stored children;
        cells [0, min(n, capacity)) of trees_buf / levels_buf (uint32) and nodes_buf (uint64) = the bad nodes in increasing
        (level, tree, node) order; info_buf: 4 uint64 = status (bits 0, 1: the offsets check; bit 2: more than `capacity` > 0),
        n, trees with a nonzero mask, nodes checked.  capacity 0: masks and counters only, the lists and scratch_buf may be
        None.  Reads only.  All in device memory; scratch_buf: audit_scratch_bytes(total, ntrees, capacity).  include/vkmr_hip.h."""
        self._call("vkmr_hip_forest_audit_async", digests_buf, forest_buf, roots_buf, total, offsets_buf, ntrees, max_count, scratch_buf, masks_buf,
                   trees_buf, levels_buf, nodes_buf, capacity, info_buf, stream=stream)

    def tree_audit_enqueue(self, digests_buf, tree_buf, count, height, scratch_buf, levels_buf, nodes_buf, capacity, info_buf, stream=None):
        """forest_audit_enqueue for one stored tree of `count` leaves and `height` levels: levels and nodes alone, and
        info_buf[2] is the tree's own level mask.  scratch_buf: audit_scratch_bytes(count, 1, capacity)."""
        self._call("vkmr_hip_tree_audit_async", digests_buf, tree_buf, count, height, scratch_buf, levels_buf, nodes_buf, capacity, info_buf,
                   stream=stream)

    # -- stored forests that grow: trees appended into reserved room, the last trees dropped (named like the two above) -----
    def forest_append_enqueue(self, digests_buf, forest_buf, total, offsets_buf, ntrees, max_count, first_tree, used, leaves_buf, n_leaves,
                              new_offsets_buf, m, roots_buf, mutated_buf, status_buf, stream=None):
        """Trees first_tree .. first_tree + m - 1 of a stored forest built with room to spare (total, ntrees, max_count: the
        build's), empty at offset `used` until now, take the n_leaves digests of leaves_buf: new tree j those from
        new_offsets_buf[j] to new_offsets_buf[j + 1] (m + 1 uint64, from 0 to n_leaves).  leaves_buf at digests_buf.at(32 * used):
        the leaves are in place.  mutated_buf (ntrees uint64) or None: the masks of the new trees.  status_buf: one uint32,
        forest_append_status_text names its bits; nonzero: nothing changed.  All in device memory.  include/vkmr_hip.h."""
        self._call("vkmr_hip_forest_append_async", digests_buf, forest_buf, total, offsets_buf, ntrees, max_count, first_tree, used, leaves_buf,
                   n_leaves, new_offsets_buf, m, roots_buf, mutated_buf, status_buf, stream=stream)

    def forest_truncate_enqueue(self, offsets_buf, ntrees, keep_trees, roots_buf, stream=None):
        """Trees keep_trees .. ntrees - 1 of a stored forest emptied: their offsets end where tree keep_trees begins, their
        roots are zero; one launch, no hash."""
        self._call("vkmr_hip_forest_truncate_async", offsets_buf, ntrees, keep_trees, roots_buf, stream=stream)

    # -- forests that slide: the oldest trees dropped, stored trees copied into another forest; no hash in either ------------
    def forest_drop_front_enqueue(self, offsets_buf, ntrees, drop_trees, roots_buf, mutated_buf=None, stream=None):
        """Trees 0 .. drop_trees - 1 of a stored forest emptied where tree drop_trees begins: their offsets are its offset,
        their roots zero (and their masks in mutated_buf, ntrees uint64 or None); one launch, no hash, nothing else moves."""
        self._call("vkmr_hip_forest_drop_front_async", offsets_buf, ntrees, drop_trees, roots_buf, mutated_buf, stream=stream)

    def forest_copy_trees_enqueue(self, src_digests_buf, src_forest_buf, src_total, src_offsets_buf, src_ntrees, src_max_count, src_roots_buf,
                                  src_mutated_buf, sel_buf, m, n_leaves, new_offsets_buf, dst_digests_buf, dst_forest_buf, dst_total, dst_offsets_buf,
                                  dst_ntrees, dst_max_count, first_tree, used, dst_roots_buf, dst_mutated_buf, status_buf, stream=None):
        """Trees first_tree .. first_tree + m - 1 of the destination forest (dst_*: forest_append_enqueue's arguments), empty at
        offset `used` until now, become trees sel_buf[0 .. m) (uint32) of the stored source forest src_*, copied cell by
        cell and never hashed.  new_offsets_buf: m + 1 uint64 from 0 to n_leaves, the prefix sums of the chosen trees' counts.
        src_mutated_buf / dst_mutated_buf: the forests' masks or None (copied; zeroed without the source's).  status_buf: one
        uint32, forest_copy_status_text names its bits; nonzero: nothing changed.  All in device memory.  include/vkmr_hip.h."""
        self._call("vkmr_hip_forest_copy_trees_async", src_digests_buf, src_forest_buf, src_total, src_offsets_buf, src_ntrees, src_max_count,
                   src_roots_buf, src_mutated_buf, sel_buf, m, n_leaves, new_offsets_buf, dst_digests_buf, dst_forest_buf, dst_total, dst_offsets_buf,
                   dst_ntrees, dst_max_count, first_tree, used, dst_roots_buf, dst_mutated_buf, status_buf, stream=stream)

    def forest_extend_enqueue(self, digests_buf, forest_buf, total, offsets_buf, ntrees, max_count, tree, count, used, leaves_buf, n_leaves, roots_buf,
                              mutated_buf, status_buf, stream=None):
        """The open tree `tree` of a stored forest (total, ntrees, max_count: the build's) -- `count` leaves ending at cell
        `used`, every tree behind it empty -- takes the n_leaves digests of leaves_buf; only its right edge is hashed.
        leaves_buf at digests_buf.at(32 * used): the leaves are in place.  mutated_buf (ntrees uint64) or None: the open tree's
        mask formed again.  status_buf: one uint32, forest_append_status_text names its bits; nonzero: nothing changed.  All
        in device memory.  include/vkmr_hip.h."""
        self._call("vkmr_hip_forest_extend_async", digests_buf, forest_buf, total, offsets_buf, ntrees, max_count, tree, count, used, leaves_buf,
                   n_leaves, roots_buf, mutated_buf, status_buf, stream=stream)

    def forest_shrink_enqueue(self, digests_buf, forest_buf, total, offsets_buf, ntrees, max_count, tree, count, used, r, roots_buf, mutated_buf,
                              status_buf, stream=None):
        """The open tree drops its last r leaves; the other arguments as forest_extend_enqueue's."""
        self._call("vkmr_hip_forest_shrink_async", digests_buf, forest_buf, total, offsets_buf, ntrees, max_count, tree, count, used, r, roots_buf,
                   mutated_buf, status_buf, stream=stream)

    def forest_frontier_enqueue(self, digests_buf, forest_buf, total, offsets_buf, ntrees, max_count, roots_buf, stride, counts_out_buf, peaks_out_buf,
                                stream=None):
        """The frontier of every tree of a stored forest (total, ntrees, max_count: the build's; roots_buf its roots): ntrees
        uint64 counts and ntrees x stride digests, cell l of a tree the peak of bit l of its count, zero for a clear bit.  All
        in device memory.  include/vkmr_hip.h."""
        self._call("vkmr_hip_forest_frontier_async", digests_buf, forest_buf, total, offsets_buf, ntrees, max_count, roots_buf, stride, counts_out_buf,
                   peaks_out_buf, stream=stream)

    def frontier_roots_enqueue(self, counts_buf, peaks_buf, stride, T, roots_out_buf, stream=None):
        """roots_out_buf[q] = the root of frontier q (counts_buf[q], the stride cells of peaks_buf behind q * stride)."""
        self._call("vkmr_hip_frontier_roots_async", counts_buf, peaks_buf, stride, T, roots_out_buf, stream=stream)

    def verify_frontier_enqueue(self, counts_buf, peaks_buf, stride, T, roots_buf, ok_buf, stream=None):
        """ok_buf[q] (uint32) = 1 when frontier q has the root roots_buf[q], else 0."""
        self._call("vkmr_hip_verify_frontier_async", counts_buf, peaks_buf, stride, T, roots_buf, ok_buf, stream=stream)

    def frontier_extend_enqueue(self, counts_buf, peaks_buf, stride, T, leaves_buf, total_new, offsets_buf, max_new, scratch_buf, new_counts_buf,
                                new_peaks_buf, roots_buf, status_buf, stream=None):
        """T frontiers take the total_new digests of leaves_buf, tree q those from offsets_buf[q] to offsets_buf[q + 1] (T + 1
        uint64 from 0 to total_new, none more than max_new apart): the new counts and peaks (they may be the old buffers) and
        the T roots.  scratch_buf: frontier_extend_scratch(total_new, T).  status_buf: one uint32, frontier_status_text names
        its bits; nonzero: nothing written.  All in device memory.  include/vkmr_hip.h."""
        self._call("vkmr_hip_frontier_extend_async", counts_buf, peaks_buf, stride, T, leaves_buf, total_new, offsets_buf, max_new, scratch_buf,
                   new_counts_buf, new_peaks_buf, roots_buf, status_buf, stream=stream)

    def frontier_extend_scratch(self, total_new, T):
        return self.alloc(self.lib.vkmr_hip_frontier_extend_scratch_bytes(total_new, T))

    def forest_consistency_enqueue(self, digests_buf, forest_buf, total, offsets_buf, ntrees, max_count, roots_buf, trees_buf, old_counts_buf, Q, stride,
                                   new_counts_out_buf, peaks_out_buf, rights_out_buf, status_buf, stream=None):
        """The consistency proofs of Q queries (trees_buf uint32, old_counts_buf uint64) out of a stored forest (total, ntrees,
        max_count: the build's; roots_buf its roots): Q uint64 counts as they are now and two rows of Q x stride digests, every
        cell written.  status_buf: one uint32, consistency_status_text names its bits; nonzero: nothing written.  All in device
        memory.  include/vkmr_hip.h."""
        self._call("vkmr_hip_forest_consistency_async", digests_buf, forest_buf, total, offsets_buf, ntrees, max_count, roots_buf, trees_buf,
                   old_counts_buf, Q, stride, new_counts_out_buf, peaks_out_buf, rights_out_buf, status_buf, stream=stream)

    def verify_consistency_enqueue(self, old_counts_buf, new_counts_buf, peaks_buf, rights_buf, stride, Q, old_roots_buf, new_roots_buf, ok_buf,
                                   stream=None):
        """ok_buf[q] (uint32) = 1 when proof q shows that the tree of new_counts_buf[q] leaves under new_roots_buf[q] extends the
        one of old_counts_buf[q] leaves under old_roots_buf[q], else 0."""
        self._call("vkmr_hip_verify_consistency_async", old_counts_buf, new_counts_buf, peaks_buf, rights_buf, stride, Q, old_roots_buf, new_roots_buf,
                   ok_buf, stream=stream)

    def forest_proofs_at_enqueue(self, digests_buf, forest_buf, total, offsets_buf, ntrees, max_count, roots_buf, epoch_trees_buf, epoch_counts_buf, E,
                                 epochs_buf, indices_buf, k, stride, edges_out_buf, old_roots_out_buf, siblings_buf, heights_buf, status_buf, stream=None):
        """Inclusion proofs as of an earlier count out of a stored forest (total, ntrees, max_count: the build's; roots_buf its
        roots): E epochs (epoch_trees_buf uint32, epoch_counts_buf uint64) and k queries (epochs_buf uint32, indices_buf
        uint64) give E x stride edge cells, E old roots, k x stride sibling cells and k heights, every cell written; k == 0 (the
        four query buffers may be None): the edges and the old roots alone.  status_buf: one uint32,
        consistency_status_text names its bits; nonzero: nothing written.  What comes out is what verify_forest_proofs_async
        takes with the epochs as trees and the old roots as roots.  All in device memory.  include/vkmr_hip.h."""
        self._call("vkmr_hip_forest_proofs_at_async", digests_buf, forest_buf, total, offsets_buf, ntrees, max_count, roots_buf, epoch_trees_buf,
                   epoch_counts_buf, E, epochs_buf, indices_buf, k, stride, edges_out_buf, old_roots_out_buf, siblings_buf, heights_buf, status_buf,
                   stream=stream)

    def forest_merkleblocks_enqueue(self, digests_buf, forest_buf, total, offsets_buf, ntrees, max_count, trees_buf, indices_buf, k, scratch_buf,
                                    block_trees_buf, block_counts_buf, bit_counts_buf, hash_starts_buf, byte_starts_buf, hashes_buf, hash_capacity,
                                    flags_buf, flag_capacity, info_buf, stream=None):
        """One partial Merkle tree in BIP37 order per tree named by the k sorted (tree, index) entries in device memory
        (vkmr_hip_forest_merkleblocks_async): the per-block arrays (room for k entries, the two starts for k + 1), the hashes
        (hash_capacity cells), the flag bytes (flag_capacity bytes) and info_buf (4 uint64: status, blocks, hashes, flag
        bytes; merkleblocks_status_text names the status bits).  scratch_buf: merkleblocks_scratch_bytes(k, the forest's
        stride).  All in device memory.  include/vkmr_hip.h."""
        self._call("vkmr_hip_forest_merkleblocks_async", digests_buf, forest_buf, total, offsets_buf, ntrees, max_count, trees_buf, indices_buf, k,
                   scratch_buf, block_trees_buf, block_counts_buf, bit_counts_buf, hash_starts_buf, byte_starts_buf, hashes_buf, hash_capacity, flags_buf,
                   flag_capacity, info_buf, stream=stream)

    def tree_merkleblock_enqueue(self, digests_buf, tree_buf, count, height, indices_buf, k, scratch_buf, block_trees_buf, block_counts_buf,
                                 bit_counts_buf, hash_starts_buf, byte_starts_buf, hashes_buf, hash_capacity, flags_buf, flag_capacity, info_buf,
                                 stream=None):
        """forest_merkleblocks_enqueue for ONE stored tree of height max(1, ceil(log2 count)) and k strictly increasing indices
        (vkmr_hip_tree_merkleblock_async): one block, tree 0."""
        self._call("vkmr_hip_tree_merkleblock_async", digests_buf, tree_buf, count, height, indices_buf, k, scratch_buf, block_trees_buf,
                   block_counts_buf, bit_counts_buf, hash_starts_buf, byte_starts_buf, hashes_buf, hash_capacity, flags_buf, flag_capacity, info_buf,
                   stream=stream)

    def merkleblocks_scratch_bytes(self, k, stride):
        return self.lib.vkmr_hip_forest_merkleblocks_scratch_bytes(k, stride)

    # -- sorted trees: is a tree strictly increasing, where would a digest stand, the proof that it is no leaf ----------------
    def forest_sorted_enqueue(self, digests_buf, total, offsets_buf, ntrees, first_bad_buf, info_buf, stream=None):
        """first_bad_buf[t] (ntrees uint64) = the lowest index of tree t whose leaf is not above the one in front, or 2^64 - 1;
        info_buf: 4 uint64 (status, trees not sorted, of those the ones whose first offence is an equal pair, pairs compared).
        One pass over level 0; all in device memory.  include/vkmr_hip.h."""
        self._call("vkmr_hip_forest_sorted_async", digests_buf, total, offsets_buf, ntrees, first_bad_buf, info_buf, stream=stream)

    def tree_sorted_enqueue(self, digests_buf, count, first_bad_buf, info_buf, stream=None):
        """forest_sorted_enqueue for ONE tree over digests_buf[0 .. count): first_bad_buf is one uint64."""
        self._call("vkmr_hip_tree_sorted_async", digests_buf, count, first_bad_buf, info_buf, stream=stream)

    def forest_lower_bound_enqueue(self, digests_buf, total, offsets_buf, ntrees, trees_buf, queries_buf, Q, indices_buf, found_buf, stream=None):
        """indices_buf[q] (uint64) = the lower bound of the digest queries_buf[q] among the leaves of tree trees_buf[q], found_buf[q]
        (uint32) = 1 when the leaf there is the digest; 2^64 - 1 and 0 for a tree outside the forest.  All in device memory."""
        self._call("vkmr_hip_forest_lower_bound_async", digests_buf, total, offsets_buf, ntrees, trees_buf, queries_buf, Q, indices_buf, found_buf,
                   stream=stream)

    def tree_lower_bound_enqueue(self, digests_buf, count, queries_buf, Q, indices_buf, found_buf, stream=None):
        """forest_lower_bound_enqueue for ONE tree over digests_buf[0 .. count)."""
        self._call("vkmr_hip_tree_lower_bound_async", digests_buf, count, queries_buf, Q, indices_buf, found_buf, stream=stream)

    def forest_absence_enqueue(self, digests_buf, forest_buf, total, offsets_buf, ntrees, max_count, trees_buf, queries_buf, Q, stride, indices_buf,
                               neighbours_buf, main_buf, low_buf, heights_buf, stream=None):
        """The absence proofs of Q queries (trees_buf uint32, queries_buf digests) out of a stored forest (total, ntrees,
        max_count: the build's): Q uint64 indices, 2 Q neighbour cells (pred, succ), two rows of Q x stride cells and Q uint32
        heights, every cell written.  No hash.  All in device memory.  include/vkmr_hip.h."""
        self._call("vkmr_hip_forest_absence_async", digests_buf, forest_buf, total, offsets_buf, ntrees, max_count, trees_buf, queries_buf, Q, stride,
                   indices_buf, neighbours_buf, main_buf, low_buf, heights_buf, stream=stream)

    def tree_absence_enqueue(self, digests_buf, tree_buf, count, height, queries_buf, Q, indices_buf, neighbours_buf, main_buf, low_buf, stream=None):
        """forest_absence_enqueue for ONE stored tree of height max(1, ceil(log2 count)): rows of Q x height cells, no heights."""
        self._call("vkmr_hip_tree_absence_async", digests_buf, tree_buf, count, height, queries_buf, Q, indices_buf, neighbours_buf, main_buf, low_buf,
                   stream=stream)

    def verify_forest_absence_enqueue(self, queries_buf, trees_buf, indices_buf, neighbours_buf, main_buf, low_buf, heights_buf, Q, stride, roots_buf,
                                      counts_buf, ntrees, verdict_buf, stream=None):
        """verdict_buf[q] (uint32) = 0 not proven, 1 the digest queries_buf[q] is no leaf of tree trees_buf[q], 2 it is one: proof
        q checked against roots_buf[ntrees] and counts_buf[ntrees] (uint64).  All in device memory.  include/vkmr_hip.h."""
        self._call("vkmr_hip_verify_forest_absence_async", queries_buf, trees_buf, indices_buf, neighbours_buf, main_buf, low_buf, heights_buf, Q, stride,
                   roots_buf, counts_buf, ntrees, verdict_buf, stream=stream)

    def verify_absence_enqueue(self, queries_buf, indices_buf, neighbours_buf, main_buf, low_buf, Q, height, root_buf, count, verdict_buf, stream=None):
        """verify_forest_absence_enqueue against ONE root (root_buf, one cell) and one count: rows of Q x height cells."""
        self._call("vkmr_hip_verify_absence_async", queries_buf, indices_buf, neighbours_buf, main_buf, low_buf, Q, height, root_buf, count, verdict_buf,
                   stream=stream)

    def verify_forest_absence(self, queries, trees, indices, pred, succ, main, low, heights, roots, counts):
        """uint32 [Q] verdicts (0 not proven, 1 absent, 2 present) of Q absence proofs given as host arrays -- the fields of an
        AbsenceProofs -- against roots [ntrees, 8] and counts [ntrees]; verified on the device."""
        return AbsenceProofs(trees, queries, indices, pred, succ, main, low, heights).verify(self, roots, counts)

    def range_scratch_bytes(self, nleaves, Q):
        """Bytes of scratch_buf for the range calls on Q queries: the gathers take range_scratch_bytes(0, Q), the checks
        range_scratch_bytes(nleaves, Q) with nleaves the cells of their leaves."""
        return self.lib.vkmr_hip_range_scratch_bytes(nleaves, Q)

    def forest_range_enqueue(self, digests_buf, forest_buf, total, offsets_buf, ntrees, max_count, trees_buf, lo_buf, hi_buf, Q, stride, scratch_buf,
                             firsts_buf, leaf_starts_buf, leaves_buf, leaves_capacity, left_buf, right_buf, heights_buf, info_buf, stream=None):
        """The range proofs of Q queries (trees_buf uint32, lo_buf and hi_buf digests: closed intervals) out of a stored forest: Q
        uint64 firsts, Q + 1 uint64 leaf_starts, the carried leaves back to back (leaves_capacity cells; None with 0 only counts),
        two rows of Q x stride cells, Q uint32 heights and info_buf (4 uint64: status, leaves carried, queries refused, leaves in
        range; range_status_text names the status bits).  No hash.  All in device memory.  include/vkmr_hip.h."""
        self._call("vkmr_hip_forest_range_async", digests_buf, forest_buf, total, offsets_buf, ntrees, max_count, trees_buf, lo_buf, hi_buf, Q, stride,
                   scratch_buf, firsts_buf, leaf_starts_buf, leaves_buf, leaves_capacity, left_buf, right_buf, heights_buf, info_buf, stream=stream)

    def tree_range_enqueue(self, digests_buf, tree_buf, count, height, lo_buf, hi_buf, Q, scratch_buf, firsts_buf, leaf_starts_buf, leaves_buf,
                           leaves_capacity, left_buf, right_buf, info_buf, stream=None):
        """forest_range_enqueue for ONE stored tree of height max(1, ceil(log2 count)): rows of Q x height cells, no heights."""
        self._call("vkmr_hip_tree_range_async", digests_buf, tree_buf, count, height, lo_buf, hi_buf, Q, scratch_buf, firsts_buf, leaf_starts_buf,
                   leaves_buf, leaves_capacity, left_buf, right_buf, info_buf, stream=stream)

    def verify_forest_range_enqueue(self, trees_buf, lo_buf, hi_buf, firsts_buf, leaf_starts_buf, leaves_buf, nleaves, left_buf, right_buf, heights_buf,
                                    Q, stride, roots_buf, counts_buf, ntrees, scratch_buf, verdict_buf, in_first_buf, in_count_buf, stream=None):
        """verdict_buf[q] (uint32) = 1 when the leaves carried for query q are ALL the leaves of tree trees_buf[q] in [lo, hi] (and
        their fences) under roots_buf[ntrees] and counts_buf[ntrees] (uint64), 0 otherwise; in_first_buf / in_count_buf (uint64): the
        leaves inside the bounds.  scratch_buf: range_scratch_bytes(nleaves, Q).  All in device memory.  include/vkmr_hip.h."""
        self._call("vkmr_hip_verify_forest_range_async", trees_buf, lo_buf, hi_buf, firsts_buf, leaf_starts_buf, leaves_buf, nleaves, left_buf, right_buf,
                   heights_buf, Q, stride, roots_buf, counts_buf, ntrees, scratch_buf, verdict_buf, in_first_buf, in_count_buf, stream=stream)

    def verify_range_enqueue(self, lo_buf, hi_buf, firsts_buf, leaf_starts_buf, leaves_buf, nleaves, left_buf, right_buf, Q, height, root_buf, count,
                             scratch_buf, verdict_buf, in_first_buf, in_count_buf, stream=None):
        """verify_forest_range_enqueue against ONE root (root_buf, one cell) and one count: rows of Q x height cells."""
        self._call("vkmr_hip_verify_range_async", lo_buf, hi_buf, firsts_buf, leaf_starts_buf, leaves_buf, nleaves, left_buf, right_buf, Q, height,
                   root_buf, count, scratch_buf, verdict_buf, in_first_buf, in_count_buf, stream=stream)

    # -- the leaves of a forest sorted on the device, tree by tree, in the order an absence proof rests on -------------------------
    def sort_leaves_scratch_bytes(self, total):
        return self.lib.vkmr_hip_sort_leaves_scratch_bytes(total)

    def forest_sort_leaves_enqueue(self, digests_in_buf, total, offsets_buf, ntrees, max_count, scratch_buf, digests_out_buf, order_out_buf, info_buf,
                                   stream=None):
        """For every tree t the leaves at cells [offsets[t], offsets[t+1]) of digests_in_buf, in increasing digest order (word 0
        first, unsigned; equal digests in input order), at the same cells of digests_out_buf; order_out_buf[j] (uint32, may be
        None) the flat cell of digests_in_buf that lies at cell j; info_buf: 4 uint64 (status, leaves sorted, leaves tying on the
        sort key, leaves equal to an earlier one).  All in device memory; scratch_buf: sort_leaves_scratch_bytes(total), 16-byte
        aligned.  A nonzero status writes no cell.  include/vkmr_hip.h."""
        self._call("vkmr_hip_forest_sort_leaves_async", digests_in_buf, total, offsets_buf, ntrees, max_count, scratch_buf, digests_out_buf,
                   order_out_buf, info_buf, stream=stream)

    def tree_sort_leaves_enqueue(self, digests_in_buf, count, scratch_buf, digests_out_buf, order_out_buf, info_buf, stream=None):
        """forest_sort_leaves_enqueue for ONE tree over digests_in_buf[0 .. count)."""
        self._call("vkmr_hip_tree_sort_leaves_async", digests_in_buf, count, scratch_buf, digests_out_buf, order_out_buf, info_buf, stream=stream)

    def _sort_leaves_of_buffer(self, tmp, d_in, total, offsets, ntrees, max_count, what):
        """The leaves of the trees at `offsets` (ntrees >= 1) over the `total` cells of d_in, sorted into a new buffer of as many
        cells in the scope `tmp`: (sorted buffer, order buffer, info [4] uint64).  RuntimeError when the device refuses; nothing
        falls back to the host."""
        d_out, d_order, d_info = tmp.alloc(32 * total), tmp.alloc(4 * total), tmp.alloc(32)
        d_scratch = tmp.alloc(self.sort_leaves_scratch_bytes(total))
        self.forest_sort_leaves_enqueue(d_in, total, tmp.upload(offsets), ntrees, max_count, d_scratch, d_out, d_order, d_info)
        info = self.download(d_info, 32, dtype=np.uint64)
        tmp.release(d_scratch)
        d_scratch.free()
        status = int(info[0])
        if status & 4:
            raise RuntimeError(f"{what}: {int(info[2])} leaves tie on the sort key, above the limit of {LEAFSORT_MAX_TIES} "
                               f"(status {status}: {leafsort_status_text(status)}); such a batch is sorted on the host: vk.sort_digests")
        if status:
            raise RuntimeError(f"{what}: the device refused the forest (status {status}: {leafsort_status_text(status)})")
        return d_out, d_order, info

    def sort_leaves(self, digests, counts, max_count=None):
        """(sorted [n, 8] uint32, order [n] uint32, info [4] uint64): every tree's leaves (`digests` [n, 8], tree t the next
        counts[t] of them) sorted on the device in the order an absence proof rests on -- word 0 first, every word unsigned,
        equal digests in input order -- (vkmr_hip_forest_sort_leaves_async); sorted[j] = digests[order[j]].  info: status 0, n,
        the leaves that tied on the sort key, the leaves equal to an earlier leaf of their tree (a tree with one of those cannot
        be strictly increasing).  max_count: an upper bound on every count (the largest count when None).  ValueError when the
        counts do not add up; RuntimeError when the device refuses -- a count above max_count, or more ties than the sort takes,
        which names vk.sort_digests; it never falls back to the host by itself."""
        digests = _host(digests, np.uint32, -1, 8)
        total = int(digests.shape[0])
        offsets, ntrees = _checked_offsets(counts, total, "sort_leaves")
        if ntrees == 0 or total == 0:
            return np.zeros((0, 8), dtype=np.uint32), np.zeros(0, dtype=np.uint32), np.array([0, 0, 0, 0], dtype=np.uint64)
        if max_count is None:
            max_count = max(1, int(np.diff(offsets).max()))
        with self.scope() as tmp:
            d_out, d_order, info = self._sort_leaves_of_buffer(tmp, tmp.upload(digests), total, offsets, ntrees, max_count, "sort_leaves")
            return self.download(d_out, 32 * total).reshape(total, 8), self.download(d_order, 4 * total), info

    def _build_sorted_forest_of_buffer(self, tmp, d_in, total, counts, max_count, what, **build):
        """(MerkleForest, order [n] uint32) over the leaves in the first cells of d_in, sorted on the device: the sorted buffer
        is the forest's level 0."""
        reserve_leaves = int(build.get("reserve_leaves", 0))
        offsets, ntrees = _checked_offsets(counts, total, what, slack=reserve_leaves)
        if ntrees == 0:
            raise ValueError(f"{what}: no tree")
        if max_count is None:
            max_count = max(1, int(np.diff(offsets).max()))
        n = int(offsets[-1])
        if total == 0:
            d_out, order = None, np.zeros(0, dtype=np.uint32)
        else:
            d_out, d_order, _ = self._sort_leaves_of_buffer(tmp, d_in, total, offsets, ntrees, max_count, what)
            order = self.download(d_order, 4 * n)
        forest = self._build_forest_of_buffer(d_out, total, counts, max_count, what, owned=[d_out] if d_out else [], **build)
        if d_out:
            tmp.release(d_out)
        return forest, order

    def build_sorted_forest(self, digests, counts, max_count=None, mutated=False, reserve_trees=0, reserve_leaves=0):
        """(MerkleForest, order): build_forest over every tree's leaves SORTED on the device (sort_leaves' order), so that
        MerkleForest.is_sorted holds when no tree has a repeated leaf and MerkleForest.absence proves under its roots.  The
        leaves are uploaded once, sorted into the buffer that becomes the forest's level 0 and never come back; order [n] uint32
        says which input digest lies at each cell (leaf j of the forest is digests[order[j]]), for a payload to follow.  Same
        keywords and ValueErrors as build_forest; RuntimeError as sort_leaves."""
        digests = _host(digests, np.uint32, -1, 8)
        reserve_trees, reserve_leaves = _reserve("build_sorted_forest", reserve_trees, reserve_leaves, max_count)
        used, total = int(digests.shape[0]), int(digests.shape[0]) + reserve_leaves
        with self.scope() as tmp:
            d_in = tmp.alloc(32 * total) if total else None
            if used:
                self._call("vkmr_hip_memcpy_h2d_async", d_in, digests.ctypes.data, digests.nbytes)
                self.sync()
            return self._build_sorted_forest_of_buffer(tmp, d_in, total, counts, max_count, "build_sorted_forest", mutated=mutated,
                                                       reserve_trees=reserve_trees, reserve_leaves=reserve_leaves)

    # -- two sorted forests merged tree by tree on the device: insert, remove and intersect leaves ---------------------------------
    def merge_leaves_scratch_bytes(self, a_total, b_total, ntrees):
        return self.lib.vkmr_hip_merge_leaves_scratch_bytes(a_total, b_total, ntrees)

    def forest_merge_leaves_enqueue(self, a_buf, a_total, a_offsets_buf, b_buf, b_total, b_offsets_buf, ntrees, op, scratch_buf, out_buf, out_capacity,
                                    out_offsets_buf, origin_out_buf, info_buf, stream=None):
        """Tree t of the output = op (0 union, 1 difference, 2 intersection) of tree t of A (strictly increasing) and tree t of B
        (non-decreasing; equal neighbours count once): out_offsets_buf (ntrees + 1 uint64 from 0), the trees back to back in the
        first cells of out_buf (out_capacity cells), origin_out_buf (uint64 per output cell, bit 63: a cell of B; may be None),
        info_buf: 4 uint64 (status, n_out, matches, repeats).  All in device memory; scratch_buf:
        merge_leaves_scratch_bytes(a_total, b_total, ntrees), 16-byte aligned.  A nonzero status writes no cell and no offset.
        include/vkmr_hip.h."""
        self._call("vkmr_hip_forest_merge_leaves_async", a_buf, a_total, a_offsets_buf, b_buf, b_total, b_offsets_buf, ntrees, op, scratch_buf, out_buf,
                   out_capacity, out_offsets_buf, origin_out_buf, info_buf, stream=stream)

    def tree_merge_leaves_enqueue(self, a_buf, a_count, b_buf, b_count, op, scratch_buf, out_buf, out_capacity, origin_out_buf, info_buf, stream=None):
        """forest_merge_leaves_enqueue for ONE tree a side, a_buf[0 .. a_count) and b_buf[0 .. b_count): no offsets, n_out in
        info_buf[1]."""
        self._call("vkmr_hip_tree_merge_leaves_async", a_buf, a_count, b_buf, b_count, op, scratch_buf, out_buf, out_capacity, origin_out_buf, info_buf,
                   stream=stream)

    def _sorted_batch(self, tmp, rows, offsets, ntrees, what, stream=None):
        """The batch `rows` ([n, 8], n >= 1) uploaded and every tree's leaves sorted by forest_sort_leaves_enqueue on `stream`; the
        sort's info is NOT read here: (sorted buffer, info buffer).  The caller looks at the info once its own call is done."""
        n = int(rows.shape[0])
        d_in, d_sorted, d_info = tmp.upload(rows), tmp.alloc(32 * n), tmp.alloc(32)
        self.forest_sort_leaves_enqueue(d_in, n, tmp.upload(offsets), ntrees, max(1, int(np.diff(offsets).max())),
                                        tmp.alloc(self.sort_leaves_scratch_bytes(n)), d_sorted, None, d_info, stream=stream)
        return d_sorted, d_info

    def _raise_unless_sorted_batch(self, d_sort_info, what):
        if d_sort_info is not None:
            status = int(self.download(d_sort_info, 32, dtype=np.uint64)[0])
            if status:
                raise RuntimeError(f"{what}: the batch was not sorted (status {status}: {leafsort_status_text(status)}); sort it with vk.sort_digests "
                                   f"and pass sort_b=False")

    def merge_leaves(self, a, a_counts, b, b_counts, op="union", sort_b=True):
        """(digests [n_out, 8] uint32, counts [ntrees] uint64, origin [n_out] uint64, info [4] uint64): tree t of the result is
        the union, "difference" or "intersection" of tree t of `a` (the next a_counts[t] rows of it, strictly increasing in
        sort_leaves' order) and tree t of `b`, merged on the device (vkmr_hip_forest_merge_leaves_async).  With sort_b the
        batch `b` comes in any order and goes through forest_sort_leaves_enqueue first, on the same stream; without, every tree of
        it must not decrease.  A digest that `b` holds twice counts once; a digest in both is a's.  origin[j]: the row of `a`
        that lies at output row j, or (1 << 63) | the row of the batch as it was merged (sorted, with sort_b).  info: status 0,
        n_out, the distinct digests of b found in a, the repeats in b.  ValueError when the counts do not add up or name
        different numbers of trees, or for an unknown op; RuntimeError, carrying merge_status_text, when the device refuses --
        `a` not strictly increasing, `b` decreasing; nothing falls back to the host."""
        what = "merge_leaves"
        code = _merge_op(op, what)
        a, b = _host(a, np.uint32, -1, 8), _host(b, np.uint32, -1, 8)
        na, nb = int(a.shape[0]), int(b.shape[0])
        a_off, ntrees = _checked_offsets(a_counts, na, what)
        b_off, b_trees = _checked_offsets(b_counts, nb, what)
        if b_trees != ntrees:
            raise ValueError(f"{what}: {ntrees} trees of a, {b_trees} of b")
        if ntrees == 0:
            return np.zeros((0, 8), dtype=np.uint32), np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
        cap = na + nb if code == 0 else na
        with self.scope() as tmp:
            d_a = tmp.upload(a) if na else None
            d_b, d_sort_info = None, None
            if nb and sort_b:
                d_b, d_sort_info = self._sorted_batch(tmp, b, b_off, ntrees, what)
            elif nb:
                d_b = tmp.upload(b)
            d_out, d_origin, d_off, d_info = (tmp.alloc(32 * cap) if cap else None), (tmp.alloc(8 * cap) if cap else None), tmp.alloc(8 * (ntrees + 1)), tmp.alloc(32)
            self.forest_merge_leaves_enqueue(d_a, na, tmp.upload(a_off), d_b, nb, tmp.upload(b_off), ntrees, code,
                                             tmp.alloc(self.merge_leaves_scratch_bytes(na, nb, ntrees)), d_out, cap, d_off, d_origin, d_info)
            info = self.download(d_info, 32, dtype=np.uint64)
            self._raise_unless_sorted_batch(d_sort_info, what)
            _raise_merge_status(info, what)
            n = int(info[1])
            out = self.download(d_out, 32 * n).reshape(n, 8) if n else np.zeros((0, 8), dtype=np.uint32)
            origin = self.download(d_origin, 8 * n, dtype=np.uint64) if n else np.zeros(0, dtype=np.uint64)
            return out, np.diff(self.download(d_off, 8 * (ntrees + 1), dtype=np.uint64)), origin, info

    def reduce_scratch(self, count, levels_variant=False):
        fn = self.lib.vkmr_hip_reduce_levels_scratch_bytes if levels_variant else self.lib.vkmr_hip_reduce_scratch_bytes
        return self.alloc(fn(count))

    def combine_async(self, roots_buf, n, scratch_buf, root_buf, stream=None):
        self._call("vkmr_hip_combine_async", roots_buf, n, scratch_buf, root_buf, stream=stream)

    def combine(self, roots):
        """Root ([8] uint32) over slice roots given as a host array, in slice order."""
        roots = _host(roots, np.uint32, -1, 8)
        with self.scope() as tmp:
            d_in, d_root, d_scratch = tmp.upload(roots), tmp.alloc(32), tmp.keep(self.reduce_scratch(roots.shape[0]))
            self.combine_async(d_in, roots.shape[0], d_scratch, d_root)
            return self.download(d_root, 32)

    # -- conveniences used by tests ------------------------------------------------
    def leaf_digests(self, batch):
        """Digests of every string of `batch` as a [count, 8] uint32 array."""
        if batch.count == 0:
            return np.zeros((0, 8), dtype=np.uint32)
        with self.scope() as tmp:
            return self.download(self.map_packed(tmp, batch), 32 * batch.count).reshape(-1, 8)

    def reduce_digests(self, digests, height=None, levels_variant=False):
        """Sub-tree root ([8] uint32) of a [count, 8] uint32 array of digests."""
        digests = _host(digests, np.uint32, -1, 8)
        count = digests.shape[0]
        if height is None:
            height = tree_height(count)
        with self.scope() as tmp:
            d_in, d_scratch, d_root = tmp.upload(digests), tmp.keep(self.reduce_scratch(count, levels_variant)), tmp.alloc(32)
            self.reduce_async(d_in, count, height, d_scratch, d_root, levels_variant=levels_variant)
            return self.download(d_root, 32)


DIFF_FIRST_CAPACITY = 65536      # diff(capacity=None) starts here and grows DIFF_GROWTH-fold while more leaves differ
DIFF_GROWTH = 16
DIFF_MAX_CAPACITY = 2**32 - 1


class DiffOverflow(RuntimeError):
    """More leaves differ than the capacity a diff was given."""


def _digest_pairs(old_digests, new_digests, what):
    old, new = _host(old_digests, np.uint32, -1, 8), _host(new_digests, np.uint32, -1, 8)
    if old.shape[0] != new.shape[0]:
        raise ValueError(f"{what}: one new digest per old digest")
    return old, new


class Multiproof:
    """One proof for several leaves of one tree (vkmr_hip_tree_multiproof_async): `indices` uint64 [k] sorted and unique,
    `nodes` uint32 [M, 8] in level-major order, `level_counts` uint64 [height] (nodes per level), `height`.  With the leaves
    at `indices` and the root it is what HipDevice.verify_multiproof and vkmr_host_cpu_verify_multiproof take."""

    def __init__(self, indices, nodes, level_counts, height):
        self.indices, self.nodes, self.level_counts, self.height = indices, nodes, level_counts, int(height)


def _multiproof_level_counts(indices, height):
    """[height] ints: the nodes a multiproof of the sorted unique `indices` holds per level.  Index arithmetic only."""
    cur = np.asarray(indices, dtype=np.uint64)
    counts = []
    for _ in range(height):
        have_next = np.zeros(cur.shape[0], dtype=bool)
        have_next[:-1] = (cur[1:] == cur[:-1] + np.uint64(1)) & ((cur[:-1] & np.uint64(1)) == 0)   # an even node with its odd sibling behind it
        pairs = int(have_next.sum())
        counts.append(int(cur.shape[0]) - 2 * pairs)
        cur = np.unique(cur >> np.uint64(1))
    return counts


class ForestMultiproof:
    """One proof for leaves of many trees of a forest (vkmr_hip_forest_multiproof_async): `trees` uint32 [k] and `indices`
    uint64 [k], the (tree, index) pairs sorted and unique; `heights` uint32 [k], the height of each entry's tree; `nodes`
    uint32 [M, 8] in level-major order over the whole forest; `level_counts` uint64 [stride] (nodes per level); `stride`.
    With the leaves at those positions and the forest's roots it is what HipDevice.verify_forest_multiproof and
    vkmr_host_cpu_verify_forest_multiproof take."""

    def __init__(self, trees, indices, heights, nodes, level_counts, stride):
        self.trees, self.indices, self.heights, self.nodes, self.level_counts, self.stride = trees, indices, heights, nodes, level_counts, int(stride)

    def split(self):
        """{tree: Multiproof}: the level-major nodes regrouped per tree, from the indices and heights alone.  Each tree's
        proof can be forwarded by itself and checked with HipDevice.verify_multiproof or vkmr_host_cpu_verify_multiproof."""
        trees = np.asarray(self.trees)
        starts = np.flatnonzero(np.concatenate([[True], trees[1:] != trees[:-1]])) if trees.shape[0] else np.zeros(0, dtype=np.int64)
        ends = np.concatenate([starts[1:], [trees.shape[0]]]).astype(np.int64)
        runs = [(int(trees[a]), self.indices[a:b], int(self.heights[a])) for a, b in zip(starts, ends)]
        counts = [_multiproof_level_counts(idx, h) for _, idx, h in runs]
        parts = [[] for _ in runs]
        at = 0
        for l in range(self.stride):               # level-major: level l of every tree that has one, tree by tree
            for r, (_, _, h) in enumerate(runs):
                if l < h:
                    parts[r].append(self.nodes[at: at + counts[r][l]])
                    at += counts[r][l]
        if at != self.nodes.shape[0]:
            raise ValueError(f"ForestMultiproof.split: the entries imply {at} nodes, the proof holds {self.nodes.shape[0]}")
        return {t: Multiproof(idx, np.concatenate(parts[r]).reshape(-1, 8), np.array(counts[r], dtype=np.uint64), h)
                for r, (t, idx, h) in enumerate(runs)}


def _compact_size(n):
    """Bitcoin's CompactSize of n < 2^64."""
    if n < 253:
        return bytes([n])
    for tag, width in ((253, 2), (254, 4), (255, 8)):
        if n < 1 << (8 * width):
            return bytes([tag]) + int(n).to_bytes(width, "little")
    raise ValueError("CompactSize: a length of 2^64 or more")


def _read_compact_size(data, at, what):
    """(n, the position behind it); any encoding of a length is read, the shortest is not insisted on."""
    if at >= len(data):
        raise ValueError(f"PartialMerkleTree.parse: the bytes end in front of {what}")
    tag = data[at]
    if tag < 253:
        return tag, at + 1
    width = {253: 2, 254: 4, 255: 8}[tag]
    if at + 1 + width > len(data):
        raise ValueError(f"PartialMerkleTree.parse: the bytes end inside {what}")
    return int.from_bytes(data[at + 1: at + 1 + width], "little"), at + 1 + width


class PartialMerkleTree:
    """One tree's partial Merkle tree in BIP37 order: `count`, the tree's leaves; `hashes` uint32 [n, 8], word-valued digests in
    the walk's order; `flags`, the flag bytes (uint8 [m], flag i in bit i & 7 of byte i >> 3).  One block of
    vkmr_hip_forest_merkleblocks_async."""

    def __init__(self, count, hashes, flags):
        self.count = int(count)
        self.hashes = _host(hashes, np.uint32, -1, 8)
        self.flags = np.frombuffer(bytes(flags), dtype=np.uint8) if isinstance(flags, (bytes, bytearray)) else _host(flags, np.uint8, -1)

    def serialize(self):
        """Bitcoin's CPartialMerkleTree bytes: uint32 LE count, CompactSize, the hashes -- each as the big-endian bytes of its
        eight words, the byte order of vkmr_hip_digest_hex --, CompactSize, the flag bytes.  ValueError for a count above
        2^32 - 1, which the wire form cannot say."""
        if not 0 <= self.count <= 0xFFFFFFFF:
            raise ValueError(f"PartialMerkleTree.serialize: a count of {self.count} does not fit the wire form's 32 bits")
        return (self.count.to_bytes(4, "little") + _compact_size(self.hashes.shape[0]) + self.hashes.astype(">u4").tobytes() +
                _compact_size(self.flags.shape[0]) + self.flags.tobytes())

    @classmethod
    def parse(cls, data):
        """The inverse of serialize().  ValueError for bytes that end early or go on behind the flags."""
        data = bytes(data)
        if len(data) < 4:
            raise ValueError("PartialMerkleTree.parse: the bytes end inside the count")
        count = int.from_bytes(data[:4], "little")
        n, at = _read_compact_size(data, 4, "the number of hashes")
        if at + 32 * n > len(data):
            raise ValueError("PartialMerkleTree.parse: the bytes end inside the hashes")
        hashes = np.frombuffer(data[at: at + 32 * n], dtype=">u4").astype(np.uint32).reshape(n, 8)
        m, at = _read_compact_size(data, at + 32 * n, "the number of flag bytes")
        if at + m != len(data):
            raise ValueError("PartialMerkleTree.parse: " + ("the bytes end inside the flags" if at + m > len(data) else "bytes behind the flags"))
        return cls(count, hashes, np.frombuffer(data[at:], dtype=np.uint8))

    def extract(self):
        """(root [8] uint32, indices uint64 [n], leaves uint32 [n, 8]): the root the hashes fold to and the matched leaves, by
        vkmr_host_cpu_merkleblock_extract -- Bitcoin Core's TraverseAndExtract under this project's height.  The caller compares
        the root with the one it trusts.  ValueError, naming the reason, when the tree is refused."""
        n = int(self.hashes.shape[0])
        hashes, flags = np.ascontiguousarray(self.hashes), np.ascontiguousarray(self.flags)
        root, idx, leaves, found = np.zeros(8, np.uint32), np.zeros(max(n, 1), np.uint64), np.zeros((max(n, 1), 8), np.uint32), np.zeros(1, np.uint64)
        rc = _abi.host_lib().vkmr_host_cpu_merkleblock_extract(self.count, hashes.ctypes.data if n else None, n, flags.ctypes.data if flags.size else None,
                                                               int(flags.shape[0]), root.ctypes.data, idx.ctypes.data, leaves.ctypes.data, found.ctypes.data)
        if rc != 0:
            raise ValueError(f"PartialMerkleTree.extract: refused ({rc}: {MERKLEBLOCK_EXTRACT_REFUSALS.get(rc, 'unknown')})")
        m = int(found[0])
        return root, idx[:m].copy(), leaves[:m].copy()


MERKLEBLOCK_EXTRACT_REFUSALS = {-1: "a missing pointer", -2: "a count of 0", -3: "more hashes than leaves", -4: "fewer flag bits than hashes",
                                -5: "a flag or a hash read past the end", -6: "not all hashes used", -7: "the flags used do not end in the last byte",
                                -8: "a right child equal to its left (CVE-2012-2459)"}


class PartialMerkleTrees:
    """What merkleblocks() gives: one partial Merkle tree per named tree, side by side as the device wrote them.  `trees` uint32
    [B] ascending, `counts` uint64 [B], `bit_counts` uint64 [B] (flags per block), `hash_starts` and `byte_starts` uint64 [B + 1],
    `hashes` uint32 [N, 8] tree-major, `flags` uint8 [bytes] (every block starts on a byte).  len() is B; [b] is block b as a
    PartialMerkleTree."""

    def __init__(self, trees, counts, bit_counts, hash_starts, byte_starts, hashes, flags):
        self.trees, self.counts, self.bit_counts, self.hash_starts, self.byte_starts = trees, counts, bit_counts, hash_starts, byte_starts
        self.hashes, self.flags = hashes, flags

    def __len__(self):
        return int(self.trees.shape[0])

    def __getitem__(self, b):
        b = int(b)
        if not -len(self) <= b < len(self):
            raise IndexError(f"block {b} of {len(self)}")
        b %= len(self)
        return PartialMerkleTree(int(self.counts[b]), self.hashes[int(self.hash_starts[b]): int(self.hash_starts[b + 1])],
                                 self.flags[int(self.byte_starts[b]): int(self.byte_starts[b + 1])])


class UpdateWitness:
    """What a primary sends beside an update so that a holder of the roots alone can follow it (update_with_witness):
    `proof`, the Multiproof or ForestMultiproof of the updated positions gathered BEFORE the update; `counts` uint64 [k], the
    leaf count of each entry's tree; `old_leaves` and `new_leaves` uint32 [k, 8], the leaves there before and after."""

    def __init__(self, proof, counts, old_leaves, new_leaves):
        self.proof, self.counts, self.old_leaves, self.new_leaves = proof, counts, old_leaves, new_leaves

    def apply(self, dev, roots):
        """The follower's step on `dev`: a forest's old `roots` [ntrees, 8] give the new roots [ntrees, 8], a tree's old root
        [8] its new root [8]; None when the witness does not fit them (HipDevice.apply_forest_multiproof / apply_multiproof)."""
        p = self.proof
        if isinstance(p, ForestMultiproof):
            return dev.apply_forest_multiproof(self.old_leaves, self.new_leaves, p.trees, p.indices, self.counts, p.nodes, roots)
        return dev.apply_multiproof(self.old_leaves, self.new_leaves, p.indices, p.nodes, roots, int(self.counts[0]), p.height)


AUDIT_MAX_CAPACITY = 2**32 - 1


class AuditReport:
    """What an audit of a stored tree or forest found.  `clean`: no node differs from the hash of its stored children -- the
    levels and roots are what a rebuild from the current leaves would write.  n_bad: the bad nodes; trees / levels uint32 [m],
    nodes uint64 [m]: the first m = min(n_bad, capacity) of them in increasing (level, tree, node) order (a tree: trees all
    0); masks uint64 [ntrees]: bit l - 1 = level l of that tree holds a bad node; flagged: trees with a nonzero mask; checked:
    the nodes that were hashed and compared; status: bit 2 (value 4) when the lists were cut at the capacity."""

    def __init__(self, status, n_bad, flagged, checked, trees, levels, nodes, masks):
        self.status, self.n_bad, self.flagged, self.checked = int(status), int(n_bad), int(flagged), int(checked)
        self.trees, self.levels, self.nodes, self.masks = trees, levels, nodes, masks
        self.clean = self.n_bad == 0

    def __repr__(self):
        listed = ", ".join(f"(t={t}, l={l}, j={j})" for t, l, j in zip(self.trees.tolist(), self.levels.tolist(), self.nodes.tolist()))
        return f"AuditReport(clean={self.clean}, n_bad={self.n_bad}, checked={self.checked}, bad=[{listed}])"


def _empty(columns):
    return tuple(np.zeros(0, dtype=t) for t in columns)


def _bare(parts):
    """A tuple of one as the thing itself: a tree's `indices` where a forest gives `(trees, indices)`."""
    return parts[0] if len(parts) == 1 else parts


class _Stored:
    """What MerkleTree and MerkleForest share: every operation over host arrays, written once.  A leaf is named by an ENTRY,
    one cell of each entry column -- (index) in a tree, (tree, index) in a forest -- and the `*_async` methods of both classes
    take their entry buffers side by side, so the bodies here hand them on as one splatted tuple.  A subclass supplies
      _columns         the dtypes of the entry columns
      _proof_columns   the dtypes of what a proof call writes per entry besides its cells (a forest: the heights)
      _Proof           the class of its multiproofs: _Proof(*entry columns, *proof columns, nodes, level counts, stride)
      ntrees, cells, stride            its trees, its leaf cells, the cells of one proof
      _multiproof_sizes, _status_text, _same_shape, _update_order
      _lower_bound_of, _absence_of     its lower_bound_async / absence_async over host trees and a device buffer of digests
    the thin *_async methods, and the public methods whose signature names the entry columns."""

    @staticmethod
    def _alloc(tmp, columns, k):
        return tuple(tmp.alloc(np.dtype(t).itemsize * k) for t in columns)

    def _read(self, bufs, columns, n):
        return tuple(self.dev.download(b, np.dtype(t).itemsize * n, dtype=t) for b, t in zip(bufs, columns))

    def _refuse(self, method, status, whose):
        """RuntimeError when a status word the device wrote is not 0: it refused entries (`whose`) that were checked or made here."""
        if status:
            text = self._status_text(status)
            raise RuntimeError(f"{type(self).__name__}.{method}: the device refused {whose} (status {status}{': ' + text if text else ''})")

    def _find(self, tmp, queries, k):
        """find_async of the k digests `queries` (a host array) enqueued, its buffers in the scope `tmp`: the entry buffers it fills."""
        d_entries = self._alloc(tmp, self._columns, k)
        self.find_async(tmp.upload(queries), k, tmp.alloc(self.dev.find_scratch_bytes(k)), *d_entries)
        return d_entries

    def find(self, digests):
        """For each digest ([k, 8] uint32, a host array) the lowest position at which it is a leaf: a tree gives indices
        uint64 [k], NOT_FOUND (2^64 - 1) for none; a forest (trees [k] uint32, indices [k] uint64), NO_TREE and NOT_FOUND for
        none.  Inner nodes and roots are not leaves."""
        q = _host(digests, np.uint32, -1, 8)
        k = int(q.shape[0])
        if k == 0:
            return _bare(_empty(self._columns))
        with self.dev.scope() as tmp:
            return _bare(self._read(self._find(tmp, q, k), self._columns, k))

    def proofs_of(self, digests):
        """hash -> position -> proof on the device, nothing downloaded in between.  A tree gives (siblings [k, height, 8]
        uint32, indices [k] uint64); a forest (siblings [k, levels, 8], heights [k] uint32, trees [k] uint32, indices [k]
        uint64): what proofs() returns for those positions, and the positions.  A digest that is no leaf gets find's markers
        and zero cells (a forest: height 0), as proofs() gives for a bad position."""
        q = _host(digests, np.uint32, -1, 8)
        k = int(q.shape[0])
        if k == 0:
            return (*self._no_proofs(0), *_empty(self._columns))
        with self.dev.scope() as tmp:
            d_entries = self._find(tmp, q, k)
            return (*self._gather_proofs(tmp, d_entries, k), *self._read(d_entries, self._columns, k))

    def first_unsorted(self):
        """uint64 [ntrees]: per tree the lowest index whose leaf is not above the leaf in front of it (an equal one offends as
        well), NOT_FOUND (2^64 - 1) for a tree that is strictly increasing -- the order being that of the digests' bytes.  One
        pass over the leaves on the device; a descent from one tree into the next is no offence."""
        return self._sorted()[0]

    def is_sorted(self):
        """Every tree strictly increasing: what an absence proof's verdict rests on."""
        return int(self._sorted()[1][1]) == 0

    def _sorted(self):
        """(first_bad uint64 [ntrees], info uint64 [4]) of sorted_async; RuntimeError when the device found the offsets broken."""
        if self.ntrees == 0:
            return np.zeros(0, np.uint64), np.zeros(4, np.uint64)
        with self.dev.scope() as tmp:
            d_bad, d_info = tmp.alloc(8 * self.ntrees), tmp.alloc(32)
            self.sorted_async(d_bad, d_info)
            bad, info = self.dev.download(d_bad, 8 * self.ntrees, dtype=np.uint64), self.dev.download(d_info, 32, dtype=np.uint64)
        if int(info[0]):
            raise RuntimeError(f"{type(self).__name__}.first_unsorted: the offsets are not a forest's (status {int(info[0])})")
        return bad, info

    def _queries(self, trees, digests, what):
        """(trees uint32 [Q], digests uint32 [Q, 8]) of a call that names a tree per digest."""
        q = _host(digests, np.uint32, -1, 8)
        t = np.zeros(q.shape[0], np.uint32) if trees is None else _host(trees, np.uint32, -1)
        if t.shape[0] != q.shape[0]:
            raise ValueError(f"{what}: one tree per digest")
        return t, q

    def _lower_bound(self, trees, digests):
        t, q = self._queries(trees, digests, "lower_bound")
        Q = int(q.shape[0])
        if Q == 0:
            return np.zeros(0, np.uint64), np.zeros(0, bool)
        with self.dev.scope() as tmp:
            d_idx, d_found = tmp.alloc(8 * Q), tmp.alloc(4 * Q)
            self._lower_bound_of(tmp, t, tmp.upload(q), Q, d_idx, d_found)
            return self.dev.download(d_idx, 8 * Q, dtype=np.uint64), self.dev.download(d_found, 4 * Q) == 1

    def _absence(self, trees, digests, stride):
        t, q = self._queries(trees, digests, "absence")
        Q = int(q.shape[0])
        if Q == 0:
            return AbsenceProofs(t, q, np.zeros(0, np.uint64), *(np.zeros((0, 8), np.uint32),) * 2, *(np.zeros((0, stride, 8), np.uint32),) * 2,
                                 np.zeros(0, np.uint32))
        with self.dev.scope() as tmp:
            d_idx, d_nb, d_main, d_low = tmp.alloc(8 * Q), tmp.alloc(64 * Q), tmp.alloc(32 * Q * stride), tmp.alloc(32 * Q * stride)
            heights = self._absence_of(tmp, t, tmp.upload(q), Q, stride, d_idx, d_nb, d_main, d_low)
            nb = self.dev.download(d_nb, 64 * Q).reshape(Q, 2, 8)
            return AbsenceProofs(t, q, self.dev.download(d_idx, 8 * Q, dtype=np.uint64), nb[:, 0], nb[:, 1],
                                 self.dev.download(d_main, 32 * Q * stride).reshape(Q, stride, 8),
                                 self.dev.download(d_low, 32 * Q * stride).reshape(Q, stride, 8), heights)

    def _ranges(self, trees, lo, hi, stride):
        t, x = self._queries(trees, lo, "ranges")
        y = _host(hi, np.uint32, -1, 8)
        if y.shape[0] != x.shape[0]:
            raise ValueError("ranges: one upper bound per lower bound")
        if not 1 <= stride <= 63:
            raise ValueError("ranges: stride in 1..63")
        Q = int(x.shape[0])
        if Q == 0:
            return RangeProofs(t, x, y, np.zeros(0, np.uint64), np.zeros(1, np.uint64), np.zeros((0, 8), np.uint32),
                               *(np.zeros((0, stride, 8), np.uint32),) * 2, np.zeros(0, np.uint32), np.zeros(4, np.uint64))
        dev = self.dev
        with dev.scope() as tmp:
            d_first, d_starts, d_left, d_right, d_info = tmp.alloc(8 * Q), tmp.alloc(8 * (Q + 1)), tmp.alloc(32 * Q * stride), tmp.alloc(32 * Q * stride), tmp.alloc(32)
            call = self._range_call(tmp, t, tmp.upload(x), tmp.upload(y), Q, stride, tmp.alloc(dev.range_scratch_bytes(0, Q)), d_first, d_starts, d_left,
                                    d_right, d_info)
            heights = call(None, 0)                  # the counting call: info[1] is what the leaves need
            n = int(dev.download(d_info, 32, dtype=np.uint64)[1])
            leaves = np.zeros((0, 8), np.uint32)
            if n:
                d_leaves = tmp.alloc(32 * n)
                heights = call(d_leaves, n)
                leaves = dev.download(d_leaves, 32 * n).reshape(n, 8)
            info = dev.download(d_info, 32, dtype=np.uint64)
            if int(info[0]):
                raise RuntimeError(f"{type(self).__name__}.ranges: status {int(info[0])}: {range_status_text(int(info[0]))}")
            return RangeProofs(t, x, y, dev.download(d_first, 8 * Q, dtype=np.uint64), dev.download(d_starts, 8 * (Q + 1), dtype=np.uint64), leaves,
                               dev.download(d_left, 32 * Q * stride).reshape(Q, stride, 8), dev.download(d_right, 32 * Q * stride).reshape(Q, stride, 8),
                               heights, info)

    def _no_proofs(self, k):
        """What k proofs without a cell are: (siblings [k, stride, 8], *the proof columns), all zero."""
        return (np.zeros((k, self.stride, 8), dtype=np.uint32), *(np.zeros(k, dtype=t) for t in self._proof_columns))

    def _gather_proofs(self, tmp, d_entries, k):
        """proofs_async of the k entries in d_entries and its results read back: (siblings [k, stride, 8], *the proof columns).
        A tree of one leaf has no level and no sibling: zero cells, no device call."""
        if self.stride == 0:
            return self._no_proofs(k)
        d_sib, d_extra = tmp.alloc(32 * k * self.stride), self._alloc(tmp, self._proof_columns, k)
        self.proofs_async(*d_entries, k, d_sib, *d_extra)
        return (self.dev.download(d_sib, 32 * k * self.stride).reshape(k, self.stride, 8), *self._read(d_extra, self._proof_columns, k))

    def _proofs(self, cols):
        k = int(cols[-1].shape[0])
        if k == 0 or self.stride == 0:
            return _bare(self._no_proofs(k))
        with self.dev.scope() as tmp:
            return _bare(self._gather_proofs(tmp, [tmp.upload(c) for c in cols], k))

    def _gather_multiproof(self, tmp, d_entries, k, method, whose):
        """multiproof_async over the k sorted entries in d_entries and its results read back, status and counts in one
        download: (nodes [M, 8], the proof columns, the level counts)."""
        cap, scratch_bytes = self._multiproof_sizes(k)
        d_scr = tmp.alloc(scratch_bytes) if self.stride else None
        d_nodes = tmp.alloc(32 * cap) if cap else None
        d_extra, d_info = self._alloc(tmp, self._proof_columns, k), tmp.alloc(8 * (2 + self.stride))
        self.multiproof_async(*d_entries, k, d_scr, d_nodes, cap, *d_extra, d_info)
        info = self.dev.download(d_info, 8 * (2 + self.stride), dtype=np.uint64)
        self._refuse(method, int(info[0]), whose)      # M and the counts are only written without a status
        m = int(info[1]) if self.stride else 0
        nodes = self.dev.download(d_nodes, 32 * m).reshape(m, 8) if m else np.zeros((0, 8), dtype=np.uint32)
        return nodes, self._read(d_extra, self._proof_columns, k), info[2:].copy()

    def _multiproof(self, entries):
        *cols, _ = self._update_order(*entries, "multiproof")
        k = int(cols[-1].shape[0])
        if k == 0:
            raise ValueError("multiproof: no entry")
        with self.dev.scope() as tmp:
            nodes, extra, counts = self._gather_multiproof(tmp, [tmp.upload(c) for c in cols], k, "multiproof", "sorted in-range entries")
        return self._Proof(*cols, *extra, nodes, counts, self.stride)

    def multiproof_of(self, digests):
        """(Multiproof or ForestMultiproof, order): ONE proof for the leaves that hold `digests` (a host array [k, 8]): find ->
        sort -> multiproof on the device.  digests[order[j]] is the leaf of entry j; digests that are no leaf are left out,
        repeats count once.  ValueError when none is found."""
        q = _host(digests, np.uint32, -1, 8)
        k = int(q.shape[0])
        if k == 0:
            raise ValueError("multiproof_of: no digest")
        with self.dev.scope() as tmp:
            d_sorted, d_order, (n, _, _, _) = self._sort(tmp, self._find(tmp, q, k), k)
            if n == 0:
                raise ValueError("multiproof_of: none of the digests is a leaf")
            nodes, extra, counts = self._gather_multiproof(tmp, d_sorted, n, "multiproof_of", "its own sorted entries")
            cols, order = self._read(d_sorted, self._columns, n), self.dev.download(d_order, 4 * n)
        return self._Proof(*cols, *extra, nodes, counts, self.stride), order

    def _gather_merkleblocks(self, tmp, d_entries, k, method, whose):
        """merkleblocks_async over the k sorted entries in d_entries with buffers of the bounds' sizes, read back as far as they
        are used: a PartialMerkleTrees."""
        cap_h, cap_b, scratch_bytes = self._merkleblocks_sizes(k)
        cols = (np.uint32, np.uint64, np.uint64)
        d_rows, d_hs, d_bs = self._alloc(tmp, cols, k), tmp.alloc(8 * (k + 1)), tmp.alloc(8 * (k + 1))
        d_hashes, d_flags, d_info = tmp.alloc(32 * cap_h), tmp.alloc(cap_b), tmp.alloc(32)
        self.merkleblocks_async(*d_entries, k, tmp.alloc(scratch_bytes), *d_rows, d_hs, d_bs, d_hashes, cap_h, d_flags, cap_b, d_info)
        status, B, n, m = (int(x) for x in self.dev.download(d_info, 32, dtype=np.uint64))
        if status:
            text = merkleblocks_status_text(status)
            raise RuntimeError(f"{type(self).__name__}.{method}: the device refused {whose} (status {status}{': ' + text if text else ''})")
        trees, counts, bits = self._read(d_rows, cols, B)
        return PartialMerkleTrees(trees, counts, bits, self.dev.download(d_hs, 8 * (B + 1), dtype=np.uint64), self.dev.download(d_bs, 8 * (B + 1), dtype=np.uint64),
                                  self.dev.download(d_hashes, 32 * n).reshape(n, 8), self.dev.download(d_flags, m, dtype=np.uint8))

    def _merkleblocks(self, entries, what):
        self._merkleblock_height(what)
        *cols, _ = self._update_order(*entries, what)
        k = int(cols[-1].shape[0])
        if k == 0:
            raise ValueError(f"{what}: no entry")
        with self.dev.scope() as tmp:
            return self._gather_merkleblocks(tmp, [tmp.upload(c) for c in cols], k, what, "sorted in-range entries")

    def _merkleblocks_of(self, digests, what):
        self._merkleblock_height(what)
        q = _host(digests, np.uint32, -1, 8)
        k = int(q.shape[0])
        if k == 0:
            raise ValueError(f"{what}: no digest")
        with self.dev.scope() as tmp:
            d_sorted, d_order, (n, _, _, _) = self._sort(tmp, self._find(tmp, q, k), k)
            if n == 0:
                raise ValueError(f"{what}: none of the digests is a leaf")
            return self._gather_merkleblocks(tmp, d_sorted, n, what, "its own sorted entries"), self.dev.download(d_order, 4 * n)

    def _apply(self, tmp, method, whose, d_entries, d_leaves, n):
        """update_async of the n sorted entries in d_entries to the digests in d_leaves, and its status word read back."""
        d_status = tmp.alloc(4)
        self.update_async(*d_entries, d_leaves, n, d_status)
        self._refuse(method, int(self.dev.download(d_status, 4)[0]), whose)

    def _update(self, entries, leaves):
        lv = np.asarray(leaves)
        k = int(np.asarray(entries[-1]).size)
        if lv.shape != (k, 8):
            raise ValueError(f"update: leaves must be [{k}, 8], not {list(lv.shape)}")
        *cols, pos = self._update_order(*entries, "update")
        with self.dev.scope() as tmp:
            if pos.shape[0]:
                d_leaves = tmp.upload(np.ascontiguousarray(lv[pos], dtype=np.uint32))
                self._apply(tmp, "update", "sorted in-range entries", [tmp.upload(c) for c in cols], d_leaves, pos.shape[0])

    def _update_with_witness(self, entries, leaves):
        """update() that also returns what a holder of the roots needs to follow it: the old leaves and the multiproof of the
        sorted entries gathered, then the update, enqueued back to back on the device's stream and read back at the end."""
        what = "update_with_witness"
        lv = np.asarray(leaves)
        k = int(np.asarray(entries[-1]).size)
        if lv.shape != (k, 8):
            raise ValueError(f"{what}: leaves must be [{k}, 8], not {list(lv.shape)}")
        *cols, pos = self._update_order(*entries, what)
        n = int(pos.shape[0])
        if n == 0:
            raise ValueError(f"{what}: no entry")
        if self.stride == 0:
            raise ValueError(f"{what}: a tree of one leaf and no level has no path to fold")
        cells, counts = self._entry_cells(*cols)
        if int(cells.max()) >= 2**32:
            raise ValueError(f"{what}: a leaf at cell 2^32 or beyond")      # gather_digests_async takes uint32 positions
        new = np.ascontiguousarray(lv[pos], dtype=np.uint32)
        cap, scratch_bytes = self._multiproof_sizes(n)
        with self.dev.scope() as tmp:
            d_entries, d_new, d_cells = [tmp.upload(c) for c in cols], tmp.upload(new), tmp.upload(cells.astype(np.uint32))
            d_old, d_scr, d_nodes = tmp.alloc(32 * n), tmp.alloc(scratch_bytes), tmp.alloc(32 * cap) if cap else None
            d_extra, d_info, d_status = self._alloc(tmp, self._proof_columns, n), tmp.alloc(8 * (2 + self.stride)), tmp.alloc(4)
            self.dev.gather_digests_async(self.digests, d_cells, n, d_old)
            self.multiproof_async(*d_entries, n, d_scr, d_nodes, cap, *d_extra, d_info)
            self.update_async(*d_entries, d_new, n, d_status)
            info = self.dev.download(d_info, 8 * (2 + self.stride), dtype=np.uint64)
            self._refuse(what, int(info[0]), "sorted in-range entries")
            self._refuse(what, int(self.dev.download(d_status, 4)[0]), "sorted in-range entries")
            m = int(info[1])
            nodes = self.dev.download(d_nodes, 32 * m).reshape(m, 8) if m else np.zeros((0, 8), dtype=np.uint32)
            extra, old = self._read(d_extra, self._proof_columns, n), self.dev.download(d_old, 32 * n).reshape(n, 8)
        return UpdateWitness(self._Proof(*cols, *extra, nodes, info[2:].copy(), self.stride), counts, old, new)

    def _update_packed(self, entries, batch):
        k = int(np.asarray(entries[-1]).size)
        if batch.count != k:
            raise ValueError(f"update_packed: {batch.count} strings for {k} indices")
        *cols, pos = self._update_order(*entries, "update_packed")
        with self.dev.scope() as tmp:
            if pos.shape[0]:      # map's entries are independent: the strings in sorted-entry order
                d_leaves = self.dev.map_packed(tmp, batch, meta=np.ascontiguousarray(batch.meta[pos]))
                self._apply(tmp, "update_packed", "sorted in-range entries", [tmp.upload(c) for c in cols], d_leaves, pos.shape[0])

    def _sort(self, tmp, d_entries, k):
        """sort_entries_async of the k entries in d_entries, its buffers in the scope `tmp`, and the one read-back of a sort,
        32 bytes: (sorted entry buffers, order buffer, (n, not found, out of range, repeats))."""
        d_sorted, d_order, d_info = self._alloc(tmp, self._columns, k), tmp.alloc(4 * k), tmp.alloc(32)
        self.sort_entries_async(*d_entries, k, tmp.alloc(self.dev.sort_entries_scratch_bytes(self.cells, k)), *d_sorted, d_order, d_info)
        return d_sorted, d_order, tuple(int(x) for x in self.dev.download(d_info, 32, dtype=np.uint64))

    def _update_entries(self, d_entries, leaves_buf, k):
        k = int(k)
        if k <= 0:
            return 0, 0, 0
        with self.dev.scope() as tmp:
            d_sorted, d_order, (n, missing, outside, repeats) = self._sort(tmp, d_entries, k)
            if outside:
                raise IndexError(f"update_entries: {outside} entries name no leaf (and are no marker)")
            if n:
                d_leaves = tmp.alloc(32 * n)
                self.dev.gather_digests_async(leaves_buf, d_order, n, d_leaves)
                self._apply(tmp, "update_entries", "its own sorted entries", d_sorted, d_leaves, n)
            return n, missing, repeats

    def replace(self, old_digests, new_digests):
        """The leaves that hold old_digests[q] become new_digests[q] (host arrays [k, 8]): find -> sort -> gather -> update on
        the device, no position and no digest coming back.  (replaced, missing): leaves written, and old digests that are no
        leaf.  Two equal old digests take the last new value.  A digest held by several leaves replaces the LOWEST position
        only: that is find's rule."""
        old, new = _digest_pairs(old_digests, new_digests, "replace")
        k = int(old.shape[0])
        if k == 0:
            return 0, 0
        with self.dev.scope() as tmp:
            applied, missing, _ = self._update_entries(self._find(tmp, old, k), tmp.upload(new), k)
            return applied, missing

    def _diff(self, tmp, other, capacity, leaves, what):
        """One diff against `other` in the scope `tmp`, the 32 bytes of its info read back: (n, entry buffers, leaves buffer or
        None).  capacity None: from min(cells, DIFF_FIRST_CAPACITY), DIFF_GROWTH times more while the device reports more, up
        to `cells`; an integer: DiffOverflow when more leaves differ."""
        self._same_shape(other, what)
        nothing = (None,) * len(self._columns)
        if self.ntrees == 0:                      # the call does nothing and writes no counters
            return 0, nothing, None
        grow = capacity is None
        cap = min(self.cells, DIFF_FIRST_CAPACITY) if grow else int(capacity)
        if not 0 <= cap <= DIFF_MAX_CAPACITY:
            raise ValueError(f"{what}: capacity outside [0, 2^32)")
        while True:
            d_scr, d_info = tmp.alloc(self.dev.diff_scratch_bytes(cap)), tmp.alloc(32)
            d_entries = self._alloc(tmp, self._columns, cap) if cap else nothing
            d_leaves = tmp.alloc(32 * cap) if leaves and cap else None
            self.diff_async(other, d_scr, *d_entries, d_leaves, cap, d_info)
            status, n = (int(x) for x in self.dev.download(d_info, 32, dtype=np.uint64)[:2])
            if status == 0:
                return n, d_entries, d_leaves
            if status != 4:
                raise RuntimeError(f"{what}: the device reports status {status}")
            if not grow or cap >= min(self.cells, DIFF_MAX_CAPACITY):
                raise DiffOverflow(f"{what}: more than {cap} leaves differ (a frontier of {n} on the way down)")
            for b in (d_scr, d_info, *d_entries, d_leaves):
                if b:
                    b.free()
                    tmp.release(b)
            cap = min(self.cells, DIFF_MAX_CAPACITY, cap * DIFF_GROWTH)

    def diff(self, other, capacity=None):
        """The leaves in which this tree or forest and `other` differ, in increasing order: a tree gives indices uint64 [n],
        a forest (trees uint32 [n], indices uint64 [n]).  capacity None: room for min(cells, 65536) answers first, 16 times
        more while more differ; an integer: DiffOverflow when more differ.  ValueError for another device or another shape
        (a tree's count and height; a forest's counts, dropped front and max_count), before any device call."""
        with self.dev.scope() as tmp:
            n, d_entries, _ = self._diff(tmp, other, capacity, False, "diff")
            return _bare(self._read(d_entries, self._columns, n) if n else _empty(self._columns))

    def sync_from(self, other):
        """Make this tree or forest equal to `other`: the diff with other's leaves at the differing positions, then the update
        of exactly those, all on the device; the 32 bytes of counters are what comes back.  The number of leaves written."""
        with self.dev.scope() as tmp:
            n, d_entries, d_leaves = self._diff(tmp, other, None, True, "sync_from")
            if n:
                self._apply(tmp, "sync_from", "the diff's own entries", d_entries, d_leaves, n)
            return n

    def _audit(self, tmp, cap):
        """One audit with room for `cap` listed nodes in the scope `tmp`, the 32 bytes of its info read back: the report."""
        columns = self._audit_columns
        nothing = (None,) * len(columns)
        d_masks = tmp.alloc(8 * self.ntrees) if self._audit_masks else None
        d_lists = self._alloc(tmp, columns, cap) if cap else nothing
        d_scr = tmp.alloc(self.dev.audit_scratch_bytes(self.cells, self.ntrees, cap)) if cap else None
        d_info = tmp.alloc(32)
        self.audit_async(d_scr, *((d_masks,) if self._audit_masks else ()), *d_lists, cap, d_info)
        status, n_bad, third, checked = (int(x) for x in self.dev.download(d_info, 32, dtype=np.uint64))
        if status & 3:
            raise RuntimeError(f"{type(self).__name__}.audit: the device refused the shape (status {status}: {forest_status_text(status & 3)})")
        m = min(n_bad, cap)
        lists = self._read(d_lists, columns, m) if m else _empty(columns)
        if self._audit_masks:
            masks, flagged, trees = self.dev.download(d_masks, 8 * self.ntrees, dtype=np.uint64), third, lists[0]
        else:
            masks, flagged, trees = np.array([third], dtype=np.uint64), int(third != 0), np.zeros(m, dtype=np.uint32)
        return AuditReport(status, n_bad, flagged, checked, trees, lists[-2], lists[-1], masks)

    def audit(self, capacity=None):
        """Which nodes are not the hash of their two stored children?  An AuditReport; nothing of the structure is written.
        capacity None: the masks-only form first, and the list only when there is a bad node, sized from their number; an
        integer: one call with room for that many (0: masks and counters alone), status bit 2 in the report when there are more."""
        cap = 0 if capacity is None else int(capacity)
        if not 0 <= cap <= AUDIT_MAX_CAPACITY:
            raise ValueError("audit: capacity outside [0, 2^32)")
        if self.ntrees == 0 or self.cells == 0 and not self._audit_masks:     # the call does nothing and writes no counters
            return AuditReport(0, 0, 0, 0, *_empty((np.uint32, np.uint32, np.uint64)), np.zeros(self.ntrees, dtype=np.uint64))
        with self.dev.scope() as tmp:
            report = self._audit(tmp, cap)
            if capacity is None and report.n_bad:
                report = self._audit(tmp, min(report.n_bad, AUDIT_MAX_CAPACITY))
            return report


class MerkleTree(_Stored):
    """Every level of a duplicate-last tree, resident on the device (vkmr_hip_reduce_tree_async): level 0 is the digests
    buffer it was built from, levels 1..height one buffer laid out as include/vkmr_hip.h describes."""

    _columns, _proof_columns, _Proof = (np.uint64,), (), Multiproof
    ntrees = 1
    cells = property(lambda self: self.count)
    stride = property(lambda self: self.height)

    def __init__(self, dev, digests_buf, count, height, tree_buf, owned=()):
        self.dev, self.digests, self.count, self.height, self.tree = dev, digests_buf, int(count), int(height), tree_buf
        self._owned = list(owned)

    def level_size(self, l):
        return -(-self.count >> l)

    def level_offset(self, l):
        """Start cell of level l >= 1 inside the tree buffer."""
        return sum(self.level_size(j) for j in range(1, l))

    def level(self, l):
        """[n_l, 8] uint32: the cells of level l (0 = the leaves, height = the root)."""
        if not 0 <= l <= self.height:
            raise IndexError(f"level {l} of a tree of height {self.height}")
        n = self.level_size(l)
        if l == 0:
            return self.dev.download(self.digests, 32 * n).reshape(n, 8)
        return self.dev.download(self.tree, 32 * n, offset=32 * self.level_offset(l)).reshape(n, 8)

    def root(self):
        """[8] uint32; equals what reduce_async(count, height) writes."""
        if self.height == 0:
            return self.dev.download(self.digests, 32)
        return self.dev.download(self.tree, 32, offset=self.dev.tree_bytes(self.count, self.height) - 32)

    def proofs_async(self, indices_buf, k, siblings_buf, stream=None):
        """Siblings of k leaves whose indices are in device memory, written to siblings_buf [k, height] on the device."""
        self.dev.tree_proofs_async(self.digests, self.tree, self.count, self.height, indices_buf, k, siblings_buf, stream=stream)

    def proofs(self, indices):
        """[k, height, 8] uint32: the proofs of leaves `indices` (a host array); an index >= count gets zero cells."""
        return self._proofs((_host(indices, np.uint64, -1),))

    def find_async(self, queries_buf, k, scratch_buf, indices_buf, stream=None):
        """indices_buf[q] = the lowest index whose leaf equals the digest queries_buf[q], or 2^64 - 1 (NOT_FOUND): device
        memory throughout, scratch_buf of dev.find_scratch_bytes(k) bytes; ordered on `stream` behind earlier updates."""
        self.dev.tree_find_async(self.digests, self.count, queries_buf, k, scratch_buf, indices_buf, stream=stream)

    def sorted_async(self, first_bad_buf, info_buf, stream=None):
        """first_bad_buf (one uint64) = the lowest index whose leaf is not above the one in front, or 2^64 - 1; info_buf: 4 uint64.
        Device memory; ordered on `stream` behind earlier updates.  HipDevice.tree_sorted_enqueue."""
        self.dev.tree_sorted_enqueue(self.digests, self.count, first_bad_buf, info_buf, stream=stream)

    def lower_bound_async(self, queries_buf, Q, indices_buf, found_buf, stream=None):
        """indices_buf[q] = the lower bound of the digest queries_buf[q] among the leaves, found_buf[q] = 1 when it is a leaf."""
        self.dev.tree_lower_bound_enqueue(self.digests, self.count, queries_buf, Q, indices_buf, found_buf, stream=stream)

    def lower_bound(self, digests):
        """(indices uint64 [Q], found bool [Q]): where each digest ([Q, 8], a host array) would stand among the leaves -- on a
        sorted tree the number of leaves below it -- and whether it is the leaf there.  The number of leaves in [x, y) is the
        difference of two answers."""
        return self._lower_bound(None, digests)

    def _lower_bound_of(self, tmp, trees, d_queries, Q, d_idx, d_found):
        self.lower_bound_async(d_queries, Q, d_idx, d_found)

    def _absence_of(self, tmp, trees, d_queries, Q, stride, d_idx, d_nb, d_main, d_low):
        """absence_async enqueued; the heights of the Q proofs: the tree's, it writes none."""
        self.absence_async(d_queries, Q, d_idx, d_nb, d_main, d_low)
        return np.full(Q, stride, np.uint32)

    def _absence_height(self):
        if self.height != tree_height(self.count):
            raise ValueError(f"absence: a tree of {self.count} leaves stored with height {self.height}; the proofs need height {tree_height(self.count)}")

    def absence_async(self, queries_buf, Q, indices_buf, neighbours_buf, main_buf, low_buf, stream=None):
        """The absence proofs of the Q digests in queries_buf: Q indices, 2 Q neighbour cells and two rows of Q x height cells, all
        in device memory.  HipDevice.tree_absence_enqueue; a tree stored with height max(1, ceil(log2 count)) only."""
        self._absence_height()
        self.dev.tree_absence_enqueue(self.digests, self.tree, self.count, self.height, queries_buf, Q, indices_buf, neighbours_buf, main_buf, low_buf,
                                      stream=stream)

    def absence(self, digests):
        """The AbsenceProofs (tree 0 throughout) that show, to a holder of the root and the count, that each digest ([Q, 8]) is no
        leaf of this tree -- or that it is one.  The verdict binds when the tree is sorted: is_sorted()."""
        self._absence_height()
        return self._absence(None, digests, self.height)

    def range_async(self, lo_buf, hi_buf, Q, scratch_buf, firsts_buf, leaf_starts_buf, leaves_buf, leaves_capacity, left_buf, right_buf, info_buf,
                    stream=None):
        """The range proofs of the Q closed intervals [lo_buf[q], hi_buf[q]], all in device memory.  HipDevice.tree_range_enqueue; a
        tree stored with height max(1, ceil(log2 count)) only."""
        self._absence_height()
        self.dev.tree_range_enqueue(self.digests, self.tree, self.count, self.height, lo_buf, hi_buf, Q, scratch_buf, firsts_buf, leaf_starts_buf,
                                    leaves_buf, leaves_capacity, left_buf, right_buf, info_buf, stream=stream)

    def _range_call(self, tmp, trees, d_lo, d_hi, Q, stride, d_scr, d_first, d_starts, d_left, d_right, d_info):
        def call(d_leaves, capacity):
            self.range_async(d_lo, d_hi, Q, d_scr, d_first, d_starts, d_leaves, capacity, d_left, d_right, d_info)
            return np.full(Q, stride, np.uint32)     # the tree's: the call writes none
        return call

    def range(self, lo, hi):
        """The RangeProofs (tree 0 throughout) that show, to a holder of the root and the count, EVERY leaf in each closed interval
        [lo[q], hi[q]] ([Q, 8] each, or one digest each).  The verdict binds when the tree is sorted: is_sorted()."""
        self._absence_height()
        return self._ranges(None, lo, hi, self.height)

    def multiproof_async(self, indices_buf, k, scratch_buf, nodes_buf, nodes_capacity, info_buf, stream=None):
        """ONE proof for the k leaves whose strictly increasing indices are in device memory, written to nodes_buf
        (nodes_capacity cells); info_buf: 2 + height uint64 (status, M, the per-level counts).  include/vkmr_hip.h."""
        self.dev.tree_multiproof_async(self.digests, self.tree, self.count, self.height, indices_buf, k, scratch_buf, nodes_buf, nodes_capacity,
                                       info_buf, stream=stream)

    def _multiproof_sizes(self, k):
        """(the most nodes a multiproof of k leaves holds, the bytes of its scratch)."""
        lib = self.dev.lib
        return lib.vkmr_hip_multiproof_max_nodes(self.count, self.height, k), lib.vkmr_hip_multiproof_scratch_bytes(k, self.height)

    def multiproof(self, indices):
        """A Multiproof of leaves `indices` (a host array; sorted and deduplicated here).  IndexError for an index < 0 or
        >= count, ValueError for indices that are not integers or for none at all, before any device call."""
        return self._multiproof((indices,))

    def merkleblocks_async(self, indices_buf, k, scratch_buf, block_trees_buf, block_counts_buf, bit_counts_buf, hash_starts_buf, byte_starts_buf,
                           hashes_buf, hash_capacity, flags_buf, flag_capacity, info_buf, stream=None):
        """The tree's partial Merkle tree in BIP37 order for the k strictly increasing indices in device memory: one block.
        HipDevice.tree_merkleblock_enqueue; include/vkmr_hip.h."""
        self.dev.tree_merkleblock_enqueue(self.digests, self.tree, self.count, self.height, indices_buf, k, scratch_buf, block_trees_buf, block_counts_buf,
                                          bit_counts_buf, hash_starts_buf, byte_starts_buf, hashes_buf, hash_capacity, flags_buf, flag_capacity, info_buf,
                                          stream=stream)

    def _merkleblocks_sizes(self, k):
        """(the most hashes, the most flag bytes, the bytes of the scratch) of k entries: the forest's bounds for one tree."""
        lib = self.dev.lib
        return (lib.vkmr_hip_forest_merkleblocks_max_hashes(self.count, 1, self.count, k),
                lib.vkmr_hip_forest_merkleblocks_max_flag_bytes(self.count, 1, self.count, k), lib.vkmr_hip_forest_merkleblocks_scratch_bytes(k, self.height))

    def _merkleblock_height(self, what):
        if self.height != tree_height(self.count):
            raise ValueError(f"{what}: a tree of {self.count} leaves stored with height {self.height}; the walk needs height {tree_height(self.count)}")

    def merkleblock(self, indices):
        """The PartialMerkleTree (BIP37 order, Bitcoin's CPartialMerkleTree) that shows leaves `indices` (a host array; sorted
        and deduplicated here) to be in this tree.  IndexError for an index < 0 or >= count, ValueError for none at all or for
        a tree stored with another height than max(1, ceil(log2 count)), before any device call."""
        return self._merkleblocks((indices,), "merkleblock")[0]

    def merkleblock_of(self, digests):
        """(PartialMerkleTree, order): find -> sort -> merkleblock on the device for the leaves that hold `digests` ([k, 8], any
        order); digests[order[j]] is the j-th matched leaf, digests that are no leaf are left out, repeats count once.
        ValueError when none is found."""
        blocks, order = self._merkleblocks_of(digests, "merkleblock_of")
        return blocks[0], order

    def update_async(self, indices_buf, leaves_buf, k, status_buf, stream=None):
        """Leaves indices[q] = leaves[q], q < k, and every ancestor rehashed, on the device: indices [k] uint64 strictly
        increasing and < count, leaves [k, 8], status one uint32 (0: applied; bit 0: an index >= count, bit 1: not strictly
        increasing; nonzero: nothing changed).  All in device memory; ordered on `stream` like the proof gather."""
        self.dev.tree_update_async(self.digests, self.tree, self.count, self.height, indices_buf, leaves_buf, k, status_buf, stream=stream)

    def _status_text(self, status):
        return ""

    def _update_order(self, indices, what="update"):
        """(sorted unique uint64 indices, positions in `indices` they come from): the last occurrence of a repeated index
        wins.  IndexError for an index < 0 or >= count; no device call."""
        idx = _as_uint64(indices, what, "index", "indices", below=self.count)
        order = np.argsort(idx, kind="stable")
        s = idx[order]
        last = np.ones(s.shape[0], dtype=bool)
        last[:-1] = s[1:] != s[:-1]        # a stable sort keeps repeats in call order: the last of each run is the last occurrence
        return s[last], order[last]

    def update(self, indices, leaves):
        """Set leaf indices[q] to leaves[q] ([k, 8] uint32; host arrays) and rehash every ancestor, on the device; a repeated
        index takes its last value.  A tree built over a caller's digests buffer updates that buffer (it is level 0).
        IndexError for an index < 0 or >= count, ValueError when leaves is not [k, 8], both before any device call."""
        self._update((indices,), leaves)

    def _entry_cells(self, indices):
        """(each entry's cell in the digests buffer, the leaf count of its tree)."""
        return indices, np.full(indices.shape[0], self.count, dtype=np.uint64)

    def update_with_witness(self, indices, leaves):
        """update(), returning the UpdateWitness of it: the Multiproof of the sorted unique indices gathered before the update,
        the count, and the leaves there before and after.  witness.apply(dev, old root) gives a holder of the root alone
        the root after the update.  update()'s rules; ValueError also for no index at all or a tree of height 0."""
        return self._update_with_witness((indices,), leaves)

    def update_packed(self, indices, batch):
        """Set leaf indices[q] to the digest of string q of `batch` (batch.count == len(indices)): the strings are mapped on
        the device and the tree updated there, no digest goes through the host.  Same index rules as update()."""
        self._update_packed((indices,), batch)

    def sort_entries_async(self, indices_buf, k, scratch_buf, indices_out_buf, order_out_buf, info_buf, stream=None):
        """The k indices in device memory, in any order, sorted and deduplicated for update_async / multiproof_async:
        HipDevice.tree_sort_entries_async with this tree's count; scratch_buf of dev.sort_entries_scratch_bytes(count, k)."""
        self.dev.tree_sort_entries_async(self.count, indices_buf, k, scratch_buf, indices_out_buf, order_out_buf, info_buf, stream=stream)

    def update_entries(self, indices_buf, leaves_buf, k):
        """Set leaf indices[q] to leaves[q], q < k, both in DEVICE memory and in any order: sorted and deduplicated on the
        device (a repeated index takes its last value, NOT_FOUND markers are left out), the leaves gathered into that order,
        the tree updated; only the sort's 32 bytes of counters come back.  (applied, not_found, repeats).  IndexError when an
        index is >= count (and no marker), before anything of the tree changes."""
        return self._update_entries((indices_buf,), leaves_buf, k)

    def _same_shape(self, other, what):
        """ValueError unless `other` is a MerkleTree of this tree's device, count and height; no device call."""
        if not isinstance(other, MerkleTree):
            raise ValueError(f"{what}: the other side is no MerkleTree")
        if other.dev.index != self.dev.index:
            raise ValueError(f"{what}: the trees live on devices {self.dev.index} and {other.dev.index}")
        if other.count != self.count or other.height != self.height:
            raise ValueError(f"{what}: a tree of {self.count} leaves and height {self.height} against one of {other.count} and {other.height}")

    def diff_async(self, other, scratch_buf, indices_buf, leaves_buf, capacity, info_buf, stream=None):
        """Cells [0, n) of indices_buf = the strictly increasing indices of the leaves in which this tree (A) and `other` (B,
        same count and height) differ, found from the roots down; leaves_buf (or None): B's leaves there; info_buf: 4 uint64
        (status, n, roots differing, nodes compared).  Device memory throughout, scratch_buf of dev.diff_scratch_bytes(capacity)
        bytes; ordered on `stream` behind earlier updates of either tree.  include/vkmr_hip.h."""
        self._same_shape(other, "diff_async")
        self.dev.tree_diff_async(self.digests, self.tree, other.digests, other.tree, self.count, self.height, scratch_buf, indices_buf, leaves_buf,
                                 capacity, info_buf, stream=stream)

    _audit_masks = False          # the tree's one level mask comes back in info_buf[2]
    _audit_columns = (np.uint32, np.uint64)                  # what the list holds per bad node: level, node

    def audit_async(self, scratch_buf, levels_buf, nodes_buf, capacity, info_buf, stream=None):
        """Cells [0, min(n, capacity)) of levels_buf (uint32) / nodes_buf (uint64) = the nodes (level, node) that are not
        hash_pair of their two stored children, in increasing order; info_buf: 4 uint64 (status, n, the level mask, nodes
        checked).  capacity 0: counters only, the other buffers may be None.  Reads only; device memory throughout, scratch_buf
        of dev.audit_scratch_bytes(count, 1, capacity) bytes; ordered on `stream` behind earlier updates.  include/vkmr_hip.h."""
        self.dev.tree_audit_enqueue(self.digests, self.tree, self.count, self.height, scratch_buf, levels_buf, nodes_buf, capacity, info_buf,
                                    stream=stream)

    # -- a sorted tree that changes: a NEW tree whose level 0 is the output of vkmr_hip_tree_merge_leaves_async ---------------------
    def _merged(self, what, op, digests):
        """(MerkleTree, info): this tree's leaves merged with the batch (`digests` [n, 8] in any order: sorted on the device
        first) into a new stored tree that owns its leaves; this one is only read."""
        dev = self.dev
        what = f"MerkleTree.{what}"
        rows = _host(digests, np.uint32, -1, 8)
        nb = int(rows.shape[0])
        cap = self.count + nb if op == 0 else self.count
        d_out = dev.alloc(32 * cap)
        try:
            with dev.scope() as tmp:
                d_b, d_sort_info = dev._sorted_batch(tmp, rows, np.array([0, nb], dtype=np.uint64), 1, what) if nb else (None, None)
                d_info = tmp.alloc(32)
                dev.tree_merge_leaves_enqueue(self.digests, self.count, d_b, nb, op, tmp.alloc(dev.merge_leaves_scratch_bytes(self.count, nb, 1)), d_out, cap,
                                              None, d_info)
                info = dev.download(d_info, 32, dtype=np.uint64)
                dev._raise_unless_sorted_batch(d_sort_info, what)
                _raise_merge_status(info, what)
            n = int(info[1])
            if n == 0:
                raise ValueError(f"{what}: no leaf is left, and a stored tree has at least one")
            tree = dev.build_tree(d_out, n)
            dev.sync()
            tree._owned.append(d_out)
            return tree, info
        except BaseException:
            d_out.free()
            raise

    def inserted(self, digests):
        """(MerkleTree, info): a NEW stored tree over this tree's leaves and `digests` ([n, 8], in any order), increasing and
        each once (vkmr_hip_tree_merge_leaves_async, union); it owns its leaves, this tree is not touched and must be sorted:
        one that is not is refused (status bit 2).  info: 0, the leaves of the result, the distinct digests of the batch that
        were leaves already, the repeats in the batch.  RuntimeError with merge_status_text when the device refuses."""
        return self._merged("inserted", 0, digests)

    def removed(self, digests):
        """(MerkleTree, info) as inserted(): without the leaves that equal a digest of the batch.  ValueError when none is left."""
        return self._merged("removed", 1, digests)

    def common(self, digests):
        """(MerkleTree, info) as inserted(): the leaves that equal a digest of the batch.  ValueError when there is none."""
        return self._merged("common", 2, digests)

    def free(self):
        if self.tree:
            self.tree.free()
            self.tree = None
        for b in self._owned:
            b.free()
        self._owned = []


class MerkleForest(_Stored):
    """Every level of every tree of a forest, resident on the device (vkmr_hip_reduce_forest_tree_async): level 0 is the
    leaves buffer it was built from, levels 1..`levels` one buffer laid out as include/vkmr_hip.h describes, the roots a
    buffer of their own.  `levels` is also the stride of its proofs.  `built_mutated`: the mutation masks of the build
    (uint64 [ntrees]) when it was a flagged one, else None; mutated() gives those of the forest as it is now.  `front`: the
    cells of level 0 in front of the first tree that are no tree's (offsets_buf[0]), for a forest laid into a larger buffer."""

    _columns, _proof_columns, _Proof = (np.uint32, np.uint64), (np.uint32,), ForestMultiproof
    cells = property(lambda self: self.total)
    stride = property(lambda self: self.levels)

    def __init__(self, dev, digests_buf, total, counts, offsets_buf, max_count, forest_buf, roots_buf, owned=(), built_mutated=None, used_trees=None,
                 front=0):
        self.built_mutated = built_mutated
        self.dev, self.digests, self.total, self.offsets, self.max_count = dev, digests_buf, int(total), offsets_buf, int(max_count)
        self.counts = np.array(counts, dtype=np.uint64)      # one entry per tree of the capacity; a copy, append() writes into it
        self.ntrees = int(self.counts.shape[0])
        self.levels = tree_height(min(self.max_count, self.total)) if self.total else 1
        self.forest, self.roots_buf = forest_buf, roots_buf
        self._owned = list(owned)
        self.used_trees = self.ntrees if used_trees is None else int(used_trees)
        self.dropped_trees = 0                               # drop_front(): trees emptied at the front
        self.dropped_leaves = int(front)                     # cells in front that are no tree's: dropped ones, behind the `front` it was laid at
        if not 0 <= self.dropped_leaves <= self.total:
            raise ValueError(f"MerkleForest: {front} cells in front of the first tree, {self.total} cells in all")

    # -- room to grow: `total` and `ntrees` are the capacity the level buffers are laid out for; the trees in use are the first
    # used_trees, their leaves end at cell used_leaves; the trees behind them are empty and the cells behind them free.  After
    # drop_front() the first dropped_leaves cells belong to no tree: used_leaves still is the cell behind the last leaf in
    # use, where append and extend go on, and live_leaves counts the leaves that trees hold.  A forest laid into a larger
    # buffer (offsets_buf[0] > 0: a handle made with front=offsets_buf[0]) starts with dropped_leaves == front, the cells in
    # front of its first tree that are no tree's, and `total` counts them: everything above holds as after a drop_front()
    used_leaves = property(lambda self: self.dropped_leaves + int(self.counts.sum()))
    live_leaves = property(lambda self: int(self.counts.sum()))
    free_trees = property(lambda self: self.ntrees - self.used_trees)
    free_leaves = property(lambda self: self.total - self.used_leaves)

    def append_async(self, leaves_buf, n_leaves, new_offsets_buf, m, status_buf, mutated_buf=None, stream=None):
        """The next m free trees take the n_leaves digests of leaves_buf, new tree j those from new_offsets_buf[j] to
        new_offsets_buf[j + 1] (m + 1 uint64 from 0 to n_leaves, none above max_count apart); all in device memory.
        leaves_buf at digests.at(32 * used_leaves): they are in place.  status_buf: one uint32, 0 when appended
        (forest_append_status_text names the bits; nonzero: nothing changed); mutated_buf: ntrees uint64 or None, the masks
        of the new trees.  Ordered on `stream`: a proof gather behind it sees the new trees.  Only enqueues: the caller who
        has seen status 0 tells the handle with appended(counts)."""
        self.dev.forest_append_enqueue(self.digests, self.forest, self.total, self.offsets, self.ntrees, self.max_count, self.used_trees,
                                       self.used_leaves, leaves_buf, n_leaves, new_offsets_buf, m, self.roots_buf, mutated_buf, status_buf,
                                       stream=stream)

    def appended(self, counts):
        """The host's view after an append_async that reported status 0: the next len(counts) trees are in use with these counts."""
        m = len(counts)
        self.counts[self.used_trees: self.used_trees + m] = np.asarray(counts, dtype=np.uint64)
        self.used_trees += m

    def _append_counts(self, counts, n, what, cells="digests"):
        """The new trees' offsets relative to used_leaves (uint64 [m + 1]) and the counts (uint64 [m]), refused here -- before
        any device call -- when they do not add up to the n digests, do not fit the free trees or leaves, or exceed max_count."""
        offsets, m = _checked_offsets(counts, n, what, cells)
        new = np.diff(offsets)
        if m > self.free_trees:
            raise ValueError(f"{what}: {m} trees, room for {self.free_trees}")
        if n > self.free_leaves:
            raise ValueError(f"{what}: {n} leaves, room for {self.free_leaves}")
        if m and int(new.max()) > self.max_count:
            raise ValueError(f"{what}: a tree of {int(new.max())} leaves, max_count is {self.max_count}")
        return offsets, new

    def _append(self, tmp, leaves_buf, offsets, new, mutated, what):
        """append_async of leaves in device memory with its buffers in the scope `tmp`, waited for: the numbers of the new
        trees, with `mutated` (numbers, their masks).  RuntimeError when the device refuses what was checked here."""
        first, m = self.used_trees, int(new.shape[0])
        trees = np.arange(first, first + m, dtype=np.uint32)
        masks = np.zeros(m, dtype=np.uint64)
        if m:
            d_status, d_mut = tmp.alloc(4), tmp.alloc(8 * self.ntrees) if mutated else None
            self.append_async(leaves_buf, int(offsets[-1]), tmp.upload(offsets), m, d_status, d_mut)
            status = int(self.dev.download(d_status, 4)[0])
            if status:
                raise RuntimeError(f"MerkleForest.{what}: the device refused the trees (status {status}: {forest_append_status_text(status)})")
            if mutated:
                masks = self.dev.download(d_mut, 8 * m, dtype=np.uint64, offset=8 * first)
            self.appended(new)
        return (trees, masks) if mutated else trees

    def append(self, digests, counts, mutated=False):
        """New trees behind the last one in use, into the room reserved at the build (build_forest(reserve_trees=,
        reserve_leaves=)): `digests` [n, 8] (a host array) holds their leaves back to back, new tree j the next counts[j] of
        them.  Only the new trees are hashed; nothing of an earlier tree moves, and the forest is afterwards what a build over
        all its trees gives.  The numbers of the new trees (uint32 [m]); mutated=True: (numbers, their mutation masks uint64
        [m], what forest_roots_mutated gives for them).  ValueError, before any device call, when the counts do not add up
        to the digests, when there is no room for the trees or the leaves, or for a count above max_count."""
        digests = _host(digests, np.uint32, -1, 8)
        offsets, new = self._append_counts(counts, int(digests.shape[0]), "append")
        if new.shape[0] == 0:
            return self._append(None, None, offsets, new, mutated, "append")
        with self.dev.scope() as tmp:
            return self._append(tmp, tmp.upload(digests) if digests.shape[0] else None, offsets, new, mutated, "append")

    def append_packed(self, batch, counts):
        """append() of the digests of the strings of `batch`, new tree j over the next counts[j] of them: the strings are
        mapped on the device straight into level 0 behind the last leaf and the trees appended in place; no digest goes
        through the host.  append()'s refusals; the numbers of the new trees."""
        offsets, new = self._append_counts(counts, batch.count, "append_packed", "strings")
        if new.shape[0] == 0:
            return self._append(None, None, offsets, new, False, "append_packed")
        with self.dev.scope() as tmp:
            if batch.count:
                self.dev.map_packed(tmp, batch, out_buf=self.digests, out_offset_digests=self.used_leaves)
            return self._append(tmp, self.digests.at(32 * self.used_leaves) if batch.count else None, offsets, new, False, "append_packed")

    def truncate_async(self, keep_trees, stream=None):
        """Trees keep_trees .. ntrees - 1 emptied on the device (their roots zero, their leaves' cells free again) and in the
        host's view; one launch on `stream`.  ValueError for keep_trees above used_trees."""
        keep_trees = int(keep_trees)
        if not 0 <= keep_trees <= self.used_trees:
            raise ValueError(f"truncate: {keep_trees} trees to keep, {self.used_trees} in use")
        if keep_trees < self.dropped_trees:
            raise ValueError(f"truncate: {keep_trees} trees to keep, the first {self.dropped_trees} were dropped from the front")
        self.dev.forest_truncate_enqueue(self.offsets, self.ntrees, keep_trees, self.roots_buf, stream=stream)
        self.counts[keep_trees:] = 0
        self.used_trees = keep_trees

    def truncate(self, keep_trees):
        """Drop the last trees in use, all from number keep_trees on: the inverse of append(), for appending others in their
        place.  drop_front() is its counterpart for the oldest trees.  ValueError for keep_trees above used_trees, or below
        the trees dropped from the front."""
        self.truncate_async(keep_trees)
        self.dev.sync()

    # -- forests that slide: the oldest trees dropped where they lie, the rest copied into a forest with fresh room ----------
    def drop_front_async(self, k, stream=None):
        """Trees 0 .. k - 1 emptied on the device and in the host's view; one launch on `stream`, no hash.  They become empty
        trees where tree k begins, so every tree from k on keeps its NUMBER, its cells and its proofs.  ValueError for k
        above used_trees; k at or below dropped_trees does nothing."""
        k = int(k)
        if not 0 <= k <= self.used_trees:
            raise ValueError(f"drop_front: {k} trees to drop, {self.used_trees} in use")
        if k <= self.dropped_trees:
            return
        self.dev.forest_drop_front_enqueue(self.offsets, self.ntrees, k, self.roots_buf, None, stream=stream)
        self.dropped_leaves += int(self.counts[:k].sum())
        self.counts[:k] = 0
        self.dropped_trees = k

    def drop_front(self, k):
        """Drop the oldest trees, all below number k: a window that slides (a chain keeps the last N blocks, an index expires
        files, a log is pruned).  Nothing moves and nothing is hashed; the dropped trees stay in the numbering as empty trees
        (roots zero, counts 0), find() no longer answers with their leaves, an update naming one is refused.  Their cells are
        not free again -- dropped_leaves counts them, used_leaves and free_leaves are where append() goes on -- until
        repacked() copies the live trees into a forest with fresh room.  A dropped tree is never the open tree: after
        drop_front(used_trees) extend() and shrink() find no tree in use, and the next leaves come by append().  ValueError
        for k above used_trees."""
        self.drop_front_async(k)
        self.dev.sync()

    def append_from_async(self, src, sel_buf, m, n_leaves, new_offsets_buf, status_buf, src_mutated_buf=None, mutated_buf=None, stream=None):
        """The next m free trees become trees sel_buf[0 .. m) (uint32) of the stored forest `src`, another MerkleForest of this
        device: copied cell by cell, never hashed.  new_offsets_buf: m + 1 uint64 from 0 to n_leaves, the prefix sums of their
        counts; status_buf: one uint32, 0 when copied (forest_copy_status_text names the bits; nonzero: nothing changed);
        src_mutated_buf / mutated_buf: the masks of `src` and of this forest (uint64 per tree) or None.  All in device
        memory; ordered on `stream`.  Only enqueues: the caller who has seen status 0 tells the handle with appended(counts)."""
        self.dev.forest_copy_trees_enqueue(src.digests, src.forest, src.total, src.offsets, src.ntrees, src.max_count, src.roots_buf,
                                           src_mutated_buf, sel_buf, m, n_leaves, new_offsets_buf, self.digests, self.forest, self.total,
                                           self.offsets, self.ntrees, self.max_count, self.used_trees, self.used_leaves, self.roots_buf,
                                           mutated_buf, status_buf, stream=stream)

    def _chosen(self, src, trees, what):
        """(sel uint32 [m], the new offsets, the counts) of trees `trees` of `src`, with append's host refusals."""
        if not isinstance(src, MerkleForest):
            raise ValueError(f"{what}: the source is no MerkleForest")
        if src is self:
            raise ValueError(f"{what}: a copy inside one forest is not offered")
        sel = _as_uint64(trees, what, "tree", "trees", below=src.ntrees).astype(np.uint32)
        counts = src.counts[sel.astype(np.int64)]
        offsets, new = self._append_counts(counts, int(counts.sum()), what, "leaves")
        return sel, offsets, new

    def append_from(self, src, trees, mutated=False):
        """New trees behind the last one in use, copied from the stored forest `src` (same device): its trees `trees`, in
        any order, with repeats and empty trees.  Every level is copied from src's, nothing is hashed and no leaf goes through
        the host: two forests merged, one split, trees moved.  The numbers of the new trees; mutated=True: (numbers, their
        mutation masks, from a scan of src).  append()'s ValueErrors for room and max_count, taken from src.counts, before
        any device call; IndexError for a tree src does not have; RuntimeError when the device refuses."""
        sel, offsets, new = self._chosen(src, trees, "append_from")
        first, m = self.used_trees, int(sel.shape[0])
        numbers = np.arange(first, first + m, dtype=np.uint32)
        masks = np.zeros(m, dtype=np.uint64)
        if m:
            with self.dev.scope() as tmp:
                d_status, d_src_mut, d_mut = tmp.alloc(4), None, None
                if mutated:
                    d_src_mut, d_mut = tmp.alloc(8 * src.ntrees), tmp.alloc(8 * self.ntrees)
                    src.mutated_async(d_src_mut)
                self.append_from_async(src, tmp.upload(sel), m, int(offsets[-1]), tmp.upload(offsets), d_status, d_src_mut, d_mut)
                status = int(self.dev.download(d_status, 4)[0])
                if status:
                    raise RuntimeError(f"MerkleForest.append_from: the device refused the trees (status {status}: {forest_copy_status_text(status)})")
                if mutated:
                    masks = self.dev.download(d_mut, 8 * m, dtype=np.uint64, offset=8 * first)
                self.appended(new)
        return (numbers, masks) if mutated else numbers

    def repacked(self, trees=None, max_count=None, reserve_trees=0, reserve_leaves=0, mutated=False):
        """A new MerkleForest, owning all its buffers, that holds trees `trees` of this one -- by default the trees in use that
        were not dropped, in order -- as its trees 0 .. m - 1, with reserve_trees empty trees and reserve_leaves free cells
        behind them: the room in front that drop_front() left is reclaimed, a used-up reserve renewed, trees deleted from the
        middle.  Allocation plus one copy call: no leaf goes through the host and nothing is hashed.  max_count: that of the
        new forest (this forest's when None).  mutated=True keeps the copied trees' masks in built_mutated.  This forest is
        left as it is.  ValueError for no tree at all or a chosen tree above max_count, IndexError for a tree not there."""
        what = "repacked"
        reserve_trees, reserve_leaves = _reserve(what, reserve_trees, reserve_leaves, self.max_count)
        if trees is None:
            trees = np.arange(self.dropped_trees, self.used_trees, dtype=np.uint32)
        sel = _as_uint64(trees, what, "tree", "trees", below=self.ntrees).astype(np.uint32)
        counts = self.counts[sel.astype(np.int64)]
        m, n = int(sel.shape[0]), int(counts.sum())
        max_count = self.max_count if max_count is None else int(max_count)
        if m + reserve_trees == 0:
            raise ValueError(f"{what}: no tree")
        if max_count < 1 or (m and int(counts.max()) > max_count):
            raise ValueError(f"{what}: a tree of {int(counts.max()) if m else 0} leaves, max_count is {max_count}")
        ntrees, total = m + reserve_trees, n + reserve_leaves
        dev = self.dev
        with dev.scope() as tmp:
            d_leaves = tmp.alloc(32 * total) if total else None
            d_forest = tmp.alloc(dev.forest_tree_bytes(total, ntrees, max_count))
            d_off, d_roots = tmp.upload(np.zeros(ntrees + 1, dtype=np.uint64)), tmp.upload(np.zeros((ntrees, 8), dtype=np.uint32))
            new = MerkleForest(dev, d_leaves, total, np.zeros(ntrees, dtype=np.uint64), d_off, max_count, d_forest, d_roots, used_trees=0)
            got = new.append_from(self, sel, mutated=mutated)
            if mutated:
                new.built_mutated = np.concatenate([got[1], np.zeros(reserve_trees, dtype=np.uint64)])
            new._owned = [d_leaves] if d_leaves else []
            tmp.release(d_leaves, d_forest, d_off, d_roots)      # the new forest's from here on
        return new

    # -- the open tree: the last tree in use takes more leaves, or drops its last, at its right edge ------------------------
    @property
    def open_tree(self):
        """The number of the last tree in use, the one extend() and shrink() work on; None when no tree is in use.  A tree
        dropped from the front is never the open tree: after drop_front(used_trees) -- or a truncate() down to the dropped
        trees -- there is none until append() brings the next."""
        return self.used_trees - 1 if self.used_trees > self.dropped_trees else None

    def _open(self, what, more=0, fewer=0):
        """(the open tree, its count, the leaves in use); ValueError -- before any device call -- when no tree is in use, when
        `more` leaves do not fit the free cells or take the tree past max_count, or for more than its count to drop."""
        tree = self.open_tree
        if tree is None:
            raise ValueError(f"{what}: no tree in use")
        count = int(self.counts[tree])
        if more < 0 or fewer < 0:
            raise ValueError(f"{what}: a negative number of leaves")
        if more > self.free_leaves:
            raise ValueError(f"{what}: {more} leaves, room for {self.free_leaves}")
        if count + more > self.max_count:
            raise ValueError(f"{what}: a tree of {count + more} leaves, max_count is {self.max_count}")
        if fewer > count:
            raise ValueError(f"{what}: {fewer} leaves to drop, the open tree has {count}")
        return tree, count, self.used_leaves

    def extend_async(self, leaves_buf, n, status_buf, mutated_buf=None, stream=None):
        """The open tree takes the n digests of leaves_buf (device memory) behind its last leaf; only the nodes of its right
        edge are hashed.  leaves_buf at digests.at(32 * used_leaves): they are in place.  status_buf: one uint32, 0 when done
        (forest_append_status_text names the bits; nonzero: nothing changed); mutated_buf: ntrees uint64 or None, the open
        tree's mask formed again.  Ordered on `stream`.  Only enqueues: the caller who has seen status 0 tells the handle
        with extended(n).  ValueError as extend()."""
        n = int(n)
        tree, count, used = self._open("extend_async", more=n)
        self.dev.forest_extend_enqueue(self.digests, self.forest, self.total, self.offsets, self.ntrees, self.max_count, tree, count, used,
                                       leaves_buf, n, self.roots_buf, mutated_buf, status_buf, stream=stream)

    def extended(self, n):
        """The host's view after an extend_async that reported status 0: the open tree holds n more leaves."""
        self.counts[self.open_tree] += np.uint64(n)

    def shrink_async(self, r, status_buf, mutated_buf=None, stream=None):
        """The open tree drops its last r leaves; status_buf and mutated_buf as extend_async's.  Only enqueues: the caller who
        has seen status 0 tells the handle with shrunk(r).  ValueError as shrink()."""
        r = int(r)
        tree, count, used = self._open("shrink_async", fewer=r)
        self.dev.forest_shrink_enqueue(self.digests, self.forest, self.total, self.offsets, self.ntrees, self.max_count, tree, count, used, r,
                                       self.roots_buf, mutated_buf, status_buf, stream=stream)

    def shrunk(self, r):
        """The host's view after a shrink_async that reported status 0: the open tree holds r leaves fewer."""
        self.counts[self.open_tree] -= np.uint64(r)

    def _edge(self, tmp, enqueue, done, n, mutated, what):
        """enqueue(status_buf, mutated_buf) of n leaves with its buffers in the scope `tmp`, waited for, then done(n): the open
        tree's count, with `mutated` (count, its mask).  RuntimeError when the device refuses what was checked here."""
        tree = self.open_tree
        mask = np.uint64(0)
        if n:
            d_status, d_mut = tmp.alloc(4), tmp.alloc(8 * self.ntrees) if mutated else None
            enqueue(d_status, d_mut)
            status = int(self.dev.download(d_status, 4)[0])
            if status:
                raise RuntimeError(f"MerkleForest.{what}: the device refused (status {status}: {forest_append_status_text(status)})")
            done(n)
            if mutated:
                mask = self.dev.download(d_mut, 8, dtype=np.uint64, offset=8 * tree)[0]
        elif mutated:
            mask = self.mutated()[tree]
        count = int(self.counts[tree])
        return (count, mask) if mutated else count

    def extend(self, digests, mutated=False):
        """More leaves for the open tree (the last tree in use), into the cells reserved at the build (reserve_leaves):
        `digests` [n, 8] (a host array) go behind its last leaf and only the nodes of its right edge are hashed, at most
        (n >> l) + 2 at level l; the forest is afterwards what a build over the new counts gives.  The open tree's count;
        mutated=True: (count, its mutation mask, what forest_roots_mutated gives for it).  ValueError, before any device call,
        when no tree is in use -- none at all, or every one dropped from the front: a dropped tree takes no leaf, growth goes
        on by append() -- when there is no room for the leaves or the tree would pass max_count."""
        digests = _host(digests, np.uint32, -1, 8)
        n = int(digests.shape[0])
        self._open("extend", more=n)
        if n == 0 and not mutated:
            return self._edge(None, None, None, 0, False, "extend")
        with self.dev.scope() as tmp:
            d_new = tmp.upload(digests) if n else None
            return self._edge(tmp, lambda d_status, d_mut: self.extend_async(d_new, n, d_status, d_mut), self.extended, n, mutated, "extend")

    def extend_packed(self, batch):
        """extend() by the digests of the strings of `batch`: mapped on the device straight into level 0 behind the last leaf,
        then the tree extended in place; no digest goes through the host.  extend()'s refusals; the open tree's count."""
        n = int(batch.count)
        self._open("extend_packed", more=n)
        if n == 0:
            return self._edge(None, None, None, 0, False, "extend_packed")
        with self.dev.scope() as tmp:
            self.dev.map_packed(tmp, batch, out_buf=self.digests, out_offset_digests=self.used_leaves)
            place = self.digests.at(32 * self.used_leaves)
            return self._edge(tmp, lambda d_status, d_mut: self.extend_async(place, n, d_status, d_mut), self.extended, n, False, "extend_packed")

    def shrink(self, r, mutated=False):
        """The open tree drops its last r leaves: the inverse of extend(); their cells are free again.  Only the nodes of the
        new right edge are hashed.  The open tree's count (it may reach 0: the tree stays in use, empty); mutated=True:
        (count, its mask).  ValueError, before any device call, when no tree is in use (a tree dropped from the front is not:
        open_tree) or r is above the open tree's count."""
        r = int(r)
        self._open("shrink", fewer=r)
        if r == 0 and not mutated:
            return self._edge(None, None, None, 0, False, "shrink")
        with self.dev.scope() as tmp:
            return self._edge(tmp, lambda d_status, d_mut: self.shrink_async(r, d_status, d_mut), self.shrunk, r, mutated, "shrink")

    def frontier(self, stride=None):
        """The Frontier of every tree as it is now, read out of the stored levels (no hash): what a follower adopts
        (Frontier.verify under the roots it trusts) and then advances by Frontier.extend with the leaves the primary appends
        or extends by.  stride: cells per tree, by default the bits of min(max_count, total), the least that holds every
        tree the forest allows."""
        stride = max(1, min(self.max_count, self.total).bit_length()) if stride is None else int(stride)
        if self.ntrees == 0:
            return Frontier.empty(0, stride)
        with self.dev.scope() as tmp:
            d_counts, d_peaks = tmp.alloc(8 * self.ntrees), tmp.alloc(32 * self.ntrees * stride)
            self.dev.forest_frontier_enqueue(self.digests, self.forest, self.total, self.offsets, self.ntrees, self.max_count, self.roots_buf, stride,
                                             d_counts, d_peaks)
            return Frontier(self.dev.download(d_counts, 8 * self.ntrees, dtype=np.uint64),
                            self.dev.download(d_peaks, 32 * self.ntrees * stride).reshape(self.ntrees, stride, 8))

    def consistency(self, old_counts, trees=None, stride=None):
        """The ConsistencyProof that tree trees[q] as it is now extends what it was at old_counts[q] leaves, read out of the
        stored levels (no hash): what a holder of the old root and of the root now checks (ConsistencyProof.verify) without the
        leaves between.  trees None: one query per tree, old_counts one per tree; else any trees in any order, as often as
        wanted.  stride: cells per row, by default that of frontier().  RuntimeError, with consistency_status_text, when the
        device refuses: a tree outside the forest, an old count above the tree's count (a tree that shrank or was dropped)."""
        stride = max(1, min(self.max_count, self.total).bit_length()) if stride is None else int(stride)
        old_counts = np.array(old_counts, dtype=np.uint64).reshape(-1)
        trees = np.arange(self.ntrees, dtype=np.uint32) if trees is None else np.array(trees, dtype=np.uint32).reshape(-1)
        Q = int(trees.shape[0])
        if int(old_counts.shape[0]) != Q:
            raise ValueError(f"consistency: {int(old_counts.shape[0])} old counts for {Q} queries")
        if Q == 0:
            return ConsistencyProof(trees, old_counts, np.zeros(0, np.uint64), np.zeros((0, stride, 8), np.uint32), np.zeros((0, stride, 8), np.uint32))
        with self.dev.scope() as tmp:
            d_counts, d_peaks, d_rights, d_status = tmp.alloc(8 * Q), tmp.alloc(32 * Q * stride), tmp.alloc(32 * Q * stride), tmp.alloc(4)
            self.dev.forest_consistency_enqueue(self.digests, self.forest, self.total, self.offsets, self.ntrees, self.max_count, self.roots_buf,
                                                tmp.upload(trees), tmp.upload(old_counts), Q, stride, d_counts, d_peaks, d_rights, d_status)
            status = int(self.dev.download(d_status, 4)[0])
            if status:
                raise RuntimeError(f"MerkleForest.consistency: the device refused (status {status}: {consistency_status_text(status)})")
            return ConsistencyProof(trees, old_counts, self.dev.download(d_counts, 8 * Q, dtype=np.uint64),
                                    self.dev.download(d_peaks, 32 * Q * stride).reshape(Q, stride, 8),
                                    self.dev.download(d_rights, 32 * Q * stride).reshape(Q, stride, 8))

    def proofs_at(self, old_counts, epochs, indices, trees=None, stride=None):
        """(siblings [k, stride, 8], heights [k], old_roots [E, 8]): the proof of leaf indices[q] of epoch epochs[q] under the
        root that epoch's tree had at old_counts[epoch] leaves, out of the levels stored now; the right edge of every old tree
        is hashed once per epoch, a query hashes nothing.  trees None: one epoch per tree, so an epoch's number is its tree's,
        as in consistency(); else epoch e is tree trees[e] as of old_counts[e], any trees as often as wanted.  heights[q] is
        the old tree's height; a query into an epoch outside the list or with an index at or above its old count gets height 0
        and zero cells.  stride: cells per proof, by default that of frontier().  Verified by
        HipDevice.verify_forest_proofs(leaves, epochs, indices, siblings, heights, old_roots) -- or under the roots the asker
        holds in place of old_roots.  RuntimeError, with consistency_status_text, when the device refuses: a tree outside the
        forest, an old count above the tree's count (a tree that shrank or was dropped)."""
        stride = max(1, min(self.max_count, self.total).bit_length()) if stride is None else int(stride)
        old_counts = np.array(old_counts, dtype=np.uint64).reshape(-1)
        trees = np.arange(self.ntrees, dtype=np.uint32) if trees is None else np.array(trees, dtype=np.uint32).reshape(-1)
        epochs, indices = np.array(epochs, dtype=np.uint32).reshape(-1), np.array(indices, dtype=np.uint64).reshape(-1)
        E, k = int(trees.shape[0]), int(epochs.shape[0])
        if int(old_counts.shape[0]) != E:
            raise ValueError(f"proofs_at: {int(old_counts.shape[0])} old counts for {E} epochs")
        if int(indices.shape[0]) != k:
            raise ValueError("proofs_at: one epoch per index")
        if E == 0:
            return np.zeros((k, stride, 8), np.uint32), np.zeros(k, np.uint32), np.zeros((0, 8), np.uint32)
        with self.dev.scope() as tmp:
            d_edges, d_roots, d_status = tmp.alloc(32 * E * stride), tmp.alloc(32 * E), tmp.alloc(4)
            d_sib, d_heights = (tmp.alloc(32 * k * stride), tmp.alloc(4 * k)) if k else (None, None)
            self.dev.forest_proofs_at_enqueue(self.digests, self.forest, self.total, self.offsets, self.ntrees, self.max_count, self.roots_buf,
                                              tmp.upload(trees), tmp.upload(old_counts), E, tmp.upload(epochs) if k else None,
                                              tmp.upload(indices) if k else None, k, stride, d_edges, d_roots, d_sib, d_heights, d_status)
            status = int(self.dev.download(d_status, 4)[0])
            if status:
                raise RuntimeError(f"MerkleForest.proofs_at: the device refused (status {status}: {consistency_status_text(status)})")
            old_roots = self.dev.download(d_roots, 32 * E).reshape(E, 8)
            if k == 0:
                return np.zeros((0, stride, 8), np.uint32), np.zeros(0, np.uint32), old_roots
            return self.dev.download(d_sib, 32 * k * stride).reshape(k, stride, 8), self.dev.download(d_heights, 4 * k), old_roots

    def roots_at(self, old_counts, trees=None):
        """[E, 8] uint32: the root tree trees[e] had at old_counts[e] leaves (all zero for a count of 0), from the levels stored
        now: proofs_at without a query.  trees None: one count per tree."""
        return self.proofs_at(old_counts, [], [], trees=trees)[2]

    def roots(self):
        """[ntrees, 8] uint32: what forest_roots gives for the same leaves (an all-zero root for an empty tree)."""
        return self.dev.download(self.roots_buf, 32 * self.ntrees).reshape(self.ntrees, 8)

    def mutated_async(self, mutated_buf, stream=None):
        """The mutation masks of the forest as it is now, written to mutated_buf (ntrees uint64 in device memory): a scan of
        the stored levels, ordered on `stream` behind earlier updates (vkmr_hip_forest_tree_mutated_async)."""
        self.dev.forest_tree_mutated_async(self.digests, self.forest, self.total, self.offsets, self.ntrees, self.max_count, mutated_buf,
                                           stream=stream)

    def mutated(self):
        """uint64 [ntrees]: bit l set when level l of the tree holds two equal siblings that both exist (CVE-2012-2459), for
        the leaves as they are now -- after update() and update_packed() too.  What forest_roots_mutated gives for them."""
        with self.dev.scope() as tmp:
            d_mut = tmp.alloc(8 * self.ntrees)
            self.mutated_async(d_mut)
            return self.dev.download(d_mut, 8 * self.ntrees, dtype=np.uint64)

    def proofs_async(self, trees_buf, indices_buf, k, siblings_buf, heights_buf, stream=None):
        """Proofs of k (tree, index) queries in device memory, written to siblings_buf [k, levels] and heights_buf [k]."""
        self.dev.forest_proofs_async(self.digests, self.forest, self.total, self.offsets, self.ntrees, self.max_count, trees_buf, indices_buf, k,
                                     siblings_buf, heights_buf, stream=stream)

    def proofs(self, trees, indices):
        """(siblings [k, levels, 8] uint32, heights [k] uint32) of leaves `indices` of trees `trees` (host arrays): the
        first heights[q] cells of proof q count, the rest are zero; a tree >= ntrees or an index >= its tree's count gets
        height 0 and zero cells."""
        trees, idx = _host(trees, np.uint32, -1), _host(indices, np.uint64, -1)
        if trees.shape[0] != idx.shape[0]:
            raise ValueError("proofs: one tree per index")
        return self._proofs((trees, idx))

    def find_async(self, queries_buf, k, scratch_buf, trees_buf, indices_buf, stream=None):
        """trees_buf[q], indices_buf[q] = where the digest queries_buf[q] is a leaf: the lowest position of the forest wins;
        NO_TREE (0xFFFFFFFF) and NOT_FOUND (2^64 - 1) when it is none.  Device memory throughout, scratch_buf of
        dev.find_scratch_bytes(k) bytes; ordered on `stream` behind earlier updates.  The two outputs are what proofs_async takes."""
        self.dev.forest_find_async(self.digests, self.total, self.offsets, self.ntrees, queries_buf, k, scratch_buf, trees_buf, indices_buf,
                                   stream=stream)

    def sorted_async(self, first_bad_buf, info_buf, stream=None):
        """first_bad_buf[t] (ntrees uint64) = the lowest index of tree t whose leaf is not above the one in front, or 2^64 - 1;
        info_buf: 4 uint64.  Device memory; ordered on `stream` behind earlier updates.  HipDevice.forest_sorted_enqueue."""
        self.dev.forest_sorted_enqueue(self.digests, self.total, self.offsets, self.ntrees, first_bad_buf, info_buf, stream=stream)

    def lower_bound_async(self, trees_buf, queries_buf, Q, indices_buf, found_buf, stream=None):
        """indices_buf[q] = the lower bound of the digest queries_buf[q] among the leaves of tree trees_buf[q], found_buf[q] = 1
        when it is a leaf of it; 2^64 - 1 and 0 for a tree outside the forest."""
        self.dev.forest_lower_bound_enqueue(self.digests, self.total, self.offsets, self.ntrees, trees_buf, queries_buf, Q, indices_buf, found_buf,
                                            stream=stream)

    def lower_bound(self, trees, digests):
        """(indices uint64 [Q], found bool [Q]): where digest q ([Q, 8], host arrays) would stand among the leaves of tree
        trees[q] -- on a sorted tree the number of leaves below it -- and whether it is the leaf there; NOT_FOUND and False for
        a tree outside the forest.  The number of leaves in [x, y) is the difference of two answers."""
        return self._lower_bound(trees, digests)

    def absence_async(self, trees_buf, queries_buf, Q, stride, indices_buf, neighbours_buf, main_buf, low_buf, heights_buf, stream=None):
        """The absence proofs of Q (tree, digest) queries in device memory: Q indices, 2 Q neighbour cells, two rows of Q x stride
        cells and Q heights.  HipDevice.forest_absence_enqueue."""
        self.dev.forest_absence_enqueue(self.digests, self.forest, self.total, self.offsets, self.ntrees, self.max_count, trees_buf, queries_buf, Q,
                                        stride, indices_buf, neighbours_buf, main_buf, low_buf, heights_buf, stream=stream)

    def _lower_bound_of(self, tmp, trees, d_queries, Q, d_idx, d_found):
        self.lower_bound_async(tmp.upload(trees), d_queries, Q, d_idx, d_found)

    def _absence_of(self, tmp, trees, d_queries, Q, stride, d_idx, d_nb, d_main, d_low):
        """absence_async enqueued; the heights it wrote, read back."""
        d_h = tmp.alloc(4 * Q)
        self.absence_async(tmp.upload(trees), d_queries, Q, stride, d_idx, d_nb, d_main, d_low, d_h)
        return self.dev.download(d_h, 4 * Q)

    def absence(self, trees, digests, stride=None):
        """The AbsenceProofs that show, to a holder of the roots and the counts, that digest q ([Q, 8]) is no leaf of tree
        trees[q] -- or that it is one: the two leaves that straddle it and their proofs in the compact form, read out of the
        stored levels (no hash).  stride: cells per row, by default the forest's.  The verdict binds when the trees are
        sorted: is_sorted()."""
        return self._absence(trees, digests, self.levels if stride is None else int(stride))

    def range_async(self, trees_buf, lo_buf, hi_buf, Q, stride, scratch_buf, firsts_buf, leaf_starts_buf, leaves_buf, leaves_capacity, left_buf,
                    right_buf, heights_buf, info_buf, stream=None):
        """The range proofs of Q (tree, lo, hi) queries in device memory.  HipDevice.forest_range_enqueue."""
        self.dev.forest_range_enqueue(self.digests, self.forest, self.total, self.offsets, self.ntrees, self.max_count, trees_buf, lo_buf, hi_buf, Q,
                                      stride, scratch_buf, firsts_buf, leaf_starts_buf, leaves_buf, leaves_capacity, left_buf, right_buf, heights_buf,
                                      info_buf, stream=stream)

    def _range_call(self, tmp, trees, d_lo, d_hi, Q, stride, d_scr, d_first, d_starts, d_left, d_right, d_info):
        d_trees, d_h = tmp.upload(trees), tmp.alloc(4 * Q)

        def call(d_leaves, capacity):
            self.range_async(d_trees, d_lo, d_hi, Q, stride, d_scr, d_first, d_starts, d_leaves, capacity, d_left, d_right, d_h, d_info)
            return self.dev.download(d_h, 4 * Q)
        return call

    def ranges(self, trees, lo, hi, stride=None):
        """The RangeProofs that show, to a holder of the roots and the counts, EVERY leaf of tree trees[q] in the closed interval
        [lo[q], hi[q]] ([Q, 8] each): the leaves in range with the neighbour on either side that fences them, and the two rows of
        nodes that close the run, read out of the stored levels (no hash).  A first call counts the leaves, a second carries them.
        stride: cells per row, by default the forest's.  The verdict binds when the trees are sorted: is_sorted()."""
        return self._ranges(trees, lo, hi, self.levels if stride is None else int(stride))

    def multiproof_async(self, trees_buf, indices_buf, k, scratch_buf, nodes_buf, nodes_capacity, heights_buf, info_buf, stream=None):
        """ONE proof for the k (tree, index) entries in device memory (strictly increasing pairs), written to nodes_buf
        (nodes_capacity cells) and heights_buf [k]; info_buf: 2 + levels uint64 (status, M, the per-level counts).
        include/vkmr_hip.h."""
        self.dev.forest_multiproof_async(self.digests, self.forest, self.total, self.offsets, self.ntrees, self.max_count, trees_buf, indices_buf,
                                         k, scratch_buf, nodes_buf, nodes_capacity, heights_buf, info_buf, stream=stream)

    def _multiproof_sizes(self, k):
        """(the most nodes a multiproof of k entries holds, the bytes of its scratch)."""
        lib = self.dev.lib
        return (lib.vkmr_hip_forest_multiproof_max_nodes(self.total, self.ntrees, self.max_count, k),
                lib.vkmr_hip_forest_multiproof_scratch_bytes(k, self.levels))

    def multiproof(self, trees, indices):
        """A ForestMultiproof of leaves `indices` of trees `trees` (host arrays; the pairs sorted and deduplicated here).
        ValueError when there is not one tree per index or for no entry at all, IndexError for a tree outside [0, ntrees) or an
        index outside [0, counts[tree]), all before any device call."""
        return self._multiproof((trees, indices))

    def merkleblocks_async(self, trees_buf, indices_buf, k, scratch_buf, block_trees_buf, block_counts_buf, bit_counts_buf, hash_starts_buf,
                           byte_starts_buf, hashes_buf, hash_capacity, flags_buf, flag_capacity, info_buf, stream=None):
        """One partial Merkle tree in BIP37 order per tree named by the k (tree, index) entries in device memory (strictly
        increasing pairs).  HipDevice.forest_merkleblocks_enqueue; include/vkmr_hip.h."""
        self.dev.forest_merkleblocks_enqueue(self.digests, self.forest, self.total, self.offsets, self.ntrees, self.max_count, trees_buf, indices_buf, k,
                                             scratch_buf, block_trees_buf, block_counts_buf, bit_counts_buf, hash_starts_buf, byte_starts_buf, hashes_buf,
                                             hash_capacity, flags_buf, flag_capacity, info_buf, stream=stream)

    def _merkleblocks_sizes(self, k):
        """(the most hashes, the most flag bytes, the bytes of the scratch) of k entries."""
        lib = self.dev.lib
        return (lib.vkmr_hip_forest_merkleblocks_max_hashes(self.total, self.ntrees, self.max_count, k),
                lib.vkmr_hip_forest_merkleblocks_max_flag_bytes(self.total, self.ntrees, self.max_count, k),
                lib.vkmr_hip_forest_merkleblocks_scratch_bytes(k, self.levels))

    def _merkleblock_height(self, what):
        pass                                   # a forest's trees have the height the walk needs

    def merkleblocks(self, trees, indices):
        """PartialMerkleTrees: one partial Merkle tree in BIP37 order (Bitcoin's CPartialMerkleTree) per tree named, showing
        leaves `indices` of trees `trees` (host arrays; the pairs sorted and deduplicated here) -- the `merkleblock` answers of
        a rescan over many blocks, one device call.  ValueError when there is not one tree per index or for no entry at all,
        IndexError for a tree outside [0, ntrees) or an index outside [0, counts[tree]), all before any device call."""
        return self._merkleblocks((trees, indices), "merkleblocks")

    def merkleblocks_of(self, digests):
        """(PartialMerkleTrees, order): find -> sort -> merkleblocks on the device for the leaves that hold `digests` ([k, 8],
        txids in any order); digests[order[j]] is the leaf of the j-th sorted entry, digests that are no leaf are left out,
        repeats count once.  ValueError when none is found."""
        return self._merkleblocks_of(digests, "merkleblocks_of")

    def update_async(self, trees_buf, indices_buf, leaves_buf, k, status_buf, stream=None):
        """Leaf indices[q] of tree trees[q] = leaves[q], q < k, and every ancestor rehashed, on the device: trees [k] uint32 and
        indices [k] uint64 strictly increasing as (tree, index) pairs with index < counts[tree], leaves [k, 8], status one
        uint32 (0: applied; forest_update_status_text names the bits; nonzero: nothing changed).  All in device memory; ordered
        on `stream` like the proof gather."""
        self.dev.forest_update_async(self.digests, self.forest, self.total, self.offsets, self.ntrees, self.max_count, trees_buf, indices_buf,
                                     leaves_buf, k, self.roots_buf, status_buf, stream=stream)

    def _status_text(self, status):
        return forest_multiproof_status_text(status)      # the update's bits, and the multiproof's bit 2 that an update never sets

    def _update_order(self, trees, indices, what="update"):
        """(trees uint32, indices uint64, positions in the call they come from): the (tree, index) pairs sorted
        lexicographically, each once; the last occurrence of a repeated pair wins.  ValueError when there is not one tree per
        index, IndexError for a tree outside [0, ntrees) or an index outside [0, counts[tree]); no device call."""
        if np.asarray(trees).size != np.asarray(indices).size:
            raise ValueError(f"{what}: one tree per index")
        t = _as_uint64(trees, what, "tree", "trees", below=self.ntrees)
        idx = _as_uint64(indices, what, "index", "indices", below=int(self.counts.max()) if self.ntrees else 0)
        if (idx >= self.counts[t.astype(np.int64)]).any():
            raise IndexError(f"{what}: index outside its tree")
        order = np.lexsort((idx, t))           # stable: repeats stay in call order, so the last of each run is the last occurrence
        st, si = t[order], idx[order]
        last = np.ones(st.shape[0], dtype=bool)
        last[:-1] = (st[1:] != st[:-1]) | (si[1:] != si[:-1])
        return st[last].astype(np.uint32), si[last], order[last]

    def update(self, trees, indices, leaves):
        """Set leaf indices[q] of tree trees[q] to leaves[q] ([k, 8] uint32; host arrays) and rehash every ancestor, on the
        device; a repeated (tree, index) pair takes its last value.  A forest built over a caller's leaves buffer updates that
        buffer (it is level 0).  ValueError when leaves is not [k, 8] or there is not one tree per index, IndexError for a tree
        outside [0, ntrees) or an index outside [0, counts[tree]), all before any device call."""
        self._update((trees, indices), leaves)

    def _entry_cells(self, trees, indices):
        """(each entry's cell in the leaves buffer, the leaf count of its tree)."""
        t = trees.astype(np.int64)
        offsets = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.uint64) + np.uint64(self.dropped_leaves)
        return offsets[t] + indices, self.counts[t]

    def update_with_witness(self, trees, indices, leaves):
        """update(), returning the UpdateWitness of it: the ForestMultiproof of the sorted unique entries gathered before the
        update, the count of each entry's tree, and the leaves there before and after.  witness.apply(dev, old roots) gives a
        holder of the roots alone the roots after the update.  update()'s rules; ValueError also for no entry at all."""
        return self._update_with_witness((trees, indices), leaves)

    def update_packed(self, trees, indices, batch):
        """Set leaf indices[q] of tree trees[q] to the digest of string q of `batch` (batch.count == len(indices)): the strings
        are mapped on the device and the forest updated there, no digest goes through the host.  Same rules as update()."""
        self._update_packed((trees, indices), batch)

    def sort_entries_async(self, trees_buf, indices_buf, k, scratch_buf, trees_out_buf, indices_out_buf, order_out_buf, info_buf, stream=None):
        """The k (tree, index) entries in device memory, in any order -- find_async's outputs as they are -- sorted and
        deduplicated for update_async / multiproof_async: HipDevice.forest_sort_entries_async with this forest's offsets;
        scratch_buf of dev.sort_entries_scratch_bytes(total, k)."""
        self.dev.forest_sort_entries_async(self.total, self.offsets, self.ntrees, trees_buf, indices_buf, k, scratch_buf, trees_out_buf,
                                           indices_out_buf, order_out_buf, info_buf, stream=stream)

    def update_entries(self, trees_buf, indices_buf, leaves_buf, k):
        """Set leaf indices[q] of tree trees[q] to leaves[q], q < k, all three in DEVICE memory and in any order: sorted and
        deduplicated on the device (a repeated pair takes its last value, find's NO_TREE markers are left out), the leaves
        gathered into that order, the forest updated; only the sort's 32 bytes of counters come back.  (applied, not_found,
        repeats).  IndexError when an entry is out of range (and no marker), before anything of the forest changes."""
        return self._update_entries((trees_buf, indices_buf), leaves_buf, k)

    def _same_shape(self, other, what):
        """ValueError unless `other` is a MerkleForest of this forest's device, counts, capacity (cells and trees, room to grow
        included), front and max_count; no device call.  With equal counts, equal dropped_leaves put every tree of the two at
        the same offset: one forest's offsets then serve for both."""
        if not isinstance(other, MerkleForest):
            raise ValueError(f"{what}: the other side is no MerkleForest")
        if other.dev.index != self.dev.index:
            raise ValueError(f"{what}: the forests live on devices {self.dev.index} and {other.dev.index}")
        if other.ntrees != self.ntrees or other.total != self.total or not np.array_equal(other.counts, self.counts):
            raise ValueError(f"{what}: the forests do not have the same counts")
        if other.dropped_leaves != self.dropped_leaves:
            raise ValueError(f"{what}: {self.dropped_leaves} cells dropped in front against {other.dropped_leaves}: the trees lie at other offsets")
        if other.max_count != self.max_count:
            raise ValueError(f"{what}: max_count {self.max_count} against {other.max_count}")

    def diff_async(self, other, scratch_buf, trees_buf, indices_buf, leaves_buf, capacity, info_buf, stream=None):
        """Cells [0, n) of trees_buf / indices_buf = the strictly increasing (tree, index) pairs of the leaves in which this
        forest (A) and `other` (B, same counts and max_count, laid out at the same offsets) differ, found from the roots down --
        what update_async and multiproof_async take; leaves_buf (or None): B's leaves there; info_buf: 4 uint64 (status, n,
        trees whose roots differ, nodes compared).  Device memory throughout, scratch_buf of dev.diff_scratch_bytes(capacity)
        bytes; ordered on `stream` behind earlier updates of either forest.  include/vkmr_hip.h."""
        self._same_shape(other, "diff_async")
        self.dev.forest_diff_async(self.digests, self.forest, self.roots_buf, other.digests, other.forest, other.roots_buf, self.total, self.offsets,
                                   self.ntrees, self.max_count, scratch_buf, trees_buf, indices_buf, leaves_buf, capacity, info_buf, stream=stream)

    _audit_masks = True
    _audit_columns = (np.uint32, np.uint32, np.uint64)       # what the list holds per bad node: tree, level, node

    def audit_async(self, scratch_buf, masks_buf, trees_buf, levels_buf, nodes_buf, capacity, info_buf, stream=None):
        """masks_buf[t] (uint64) bit l - 1 = level l of tree t holds a node that is not hash_pair of its two stored children;
        cells [0, min(n, capacity)) of trees_buf / levels_buf (uint32) / nodes_buf (uint64) = those nodes in increasing (level,
        tree, node) order; info_buf: 4 uint64 (status, n, trees with a nonzero mask, nodes checked).  capacity 0: masks and
        counters only, the lists and the scratch may be None.  Reads only; device memory throughout, scratch_buf of
        dev.audit_scratch_bytes(total, ntrees, capacity) bytes; ordered on `stream` behind earlier updates.  include/vkmr_hip.h."""
        self.dev.forest_audit_enqueue(self.digests, self.forest, self.roots_buf, self.total, self.offsets, self.ntrees, self.max_count, scratch_buf,
                                      masks_buf, trees_buf, levels_buf, nodes_buf, capacity, info_buf, stream=stream)

    # -- a sorted forest that changes: a NEW forest whose level 0 is the output of vkmr_hip_forest_merge_leaves_async ---------------
    def _merged(self, what, op, digests, counts, max_count=None, mutated=False, reserve_trees=0, reserve_leaves=0):
        """(MerkleForest, info): the trees in use merged with the batch (`digests` [n, 8], tree t the next counts[t] of them, in
        any order: sorted on the device first) into a new stored forest; this one is only read."""
        dev = self.dev
        what = f"MerkleForest.{what}"
        rows = _host(digests, np.uint32, -1, 8)
        nb, used = int(rows.shape[0]), self.used_trees
        b_off, b_trees = _checked_offsets(counts, nb, what)
        if b_trees != used:
            raise ValueError(f"{what}: {b_trees} counts for the {used} trees in use")
        if used == 0:
            raise ValueError(f"{what}: no tree")
        reserve_trees, reserve_leaves = _reserve(what, reserve_trees, reserve_leaves, max_count)
        a_counts = self.counts[:used]
        if max_count is None:
            max_count = max(1, int((a_counts + np.diff(b_off)).max())) if op == 0 else self.max_count
        na = self.live_leaves
        cap, ntrees = (na + nb if op == 0 else na), used + reserve_trees
        total = cap + reserve_leaves
        d_out = d_off = d_forest = d_roots = None
        try:
            with dev.scope() as tmp:
                d_b, d_sort_info = dev._sorted_batch(tmp, rows, b_off, used, what) if nb else (None, None)
                d_out, d_off = (dev.alloc(32 * total) if total else None), dev.alloc(8 * (ntrees + 1))
                d_forest, d_roots = dev.alloc(dev.forest_tree_bytes(total, ntrees, max_count)), dev.alloc(32 * ntrees)
                d_info, d_status, d_mut = tmp.alloc(32), tmp.alloc(4), (tmp.alloc(8 * ntrees) if mutated else None)
                dev._call("vkmr_hip_memset_async", d_off, 0xFF, 8 * (ntrees + 1))     # offsets no build accepts, should the merge refuse
                dev.forest_merge_leaves_enqueue(self.digests, self.total, self.offsets, d_b, nb, tmp.upload(b_off), used, op,
                                                tmp.alloc(dev.merge_leaves_scratch_bytes(self.total, nb, used)), d_out, cap, d_off, None, d_info)

                def build():
                    if mutated:
                        dev.reduce_forest_tree_mutated_async(d_out, total, d_off, ntrees, max_count, d_forest, d_roots, d_mut, d_status)
                    else:
                        dev.reduce_forest_tree_async(d_out, total, d_off, ntrees, max_count, d_forest, d_roots, d_status)
                if not reserve_trees:
                    build()                                  # from out_offsets on the same stream: nothing was read in between
                info = dev.download(d_info, 32, dtype=np.uint64)
                dev._raise_unless_sorted_batch(d_sort_info, what)
                _raise_merge_status(info, what)
                offsets = dev.download(d_off, 8 * (used + 1), dtype=np.uint64)
                if reserve_trees:                            # the empty trees behind: their offsets are the host's to write
                    tail = np.full(reserve_trees, offsets[-1], dtype=np.uint64)
                    dev._call("vkmr_hip_memcpy_h2d_async", d_off.at(8 * (used + 1)), tail.ctypes.data, tail.nbytes)
                    dev.sync()
                    build()
                status = int(dev.download(d_status, 4)[0])
                if status:
                    raise ValueError(f"{what}: the device refused the forest (status {status}: {forest_status_text(status)})")
                masks = dev.download(d_mut, 8 * ntrees, dtype=np.uint64) if mutated else None
            new_counts = np.concatenate([np.diff(offsets), np.zeros(reserve_trees, dtype=np.uint64)])
            return MerkleForest(dev, d_out, total, new_counts, d_off, max_count, d_forest, d_roots, owned=[d_out] if d_out else [],
                                built_mutated=masks, used_trees=used), info
        except BaseException:
            for b in (d_out, d_off, d_forest, d_roots):
                if b:
                    b.free()
            raise

    def inserted(self, digests, counts, **build):
        """(MerkleForest, info): a NEW stored forest whose tree t holds this forest's leaves and the next counts[t] rows of
        `digests` ([n, 8], in any order: they are sorted on the device first), increasing and each once -- the union by
        vkmr_hip_forest_merge_leaves_async; its level 0 IS the merge's output buffer, and it is built from the merge's
        offsets on the same stream.  This forest must be sorted (is_sorted()) and is not touched: one that is not is refused
        (status bit 2), not trusted.  info: 0, the leaves of the result, the distinct digests of the batch that were leaves
        already, the repeats in the batch.  Keywords as build_forest's (max_count, mutated, reserve_trees, reserve_leaves);
        max_count None: the largest count the result can have.  ValueError for counts that do not add up or are not one per
        tree in use; RuntimeError with merge_status_text when the device refuses."""
        return self._merged("inserted", 0, digests, counts, **build)

    def removed(self, digests, counts, **build):
        """(MerkleForest, info) as inserted(): tree t without the leaves that equal one of its rows of the batch (the
        difference); info[2] says how many were there to remove."""
        return self._merged("removed", 1, digests, counts, **build)

    def common(self, digests, counts, **build):
        """(MerkleForest, info) as inserted(): tree t holds the leaves that equal one of its rows of the batch (the
        intersection)."""
        return self._merged("common", 2, digests, counts, **build)

    def free(self):
        for b in [self.forest, self.roots_buf, self.offsets] + self._owned:
            if b:
                b.free()
        self.forest = self.roots_buf = self.offsets = None
        self._owned = []


def merkle_tree_packed(dev, batch, height=None):
    """The strings of `batch` mapped to leaf digests and the whole tree over them built, all on the device (a MerkleTree
    that owns its leaves)."""
    if batch.count == 0:
        raise ValueError("merkle_tree_packed: empty batch")
    with dev.scope() as tmp:
        d_leaves = dev.map_packed(tmp, batch)
        tree = dev.build_tree(d_leaves, batch.count, height)
        dev.sync()
        tree._owned.append(d_leaves)
        tmp.release(d_leaves)
    return tree


def forest_offsets(counts):
    """(offsets uint64 [ntrees + 1], ntrees) of trees of `counts` leaves laid back to back from cell 0."""
    raw = _as_uint64(counts, "forest", "count", "counts", range_error=ValueError)
    offsets = np.zeros(raw.size + 1, dtype=np.uint64)
    np.cumsum(raw, out=offsets[1:])
    return offsets, int(raw.size)


def _checked_offsets(counts, total, what, cells="leaves", slack=0):
    """forest_offsets(counts); ValueError when they do not add up to the leaves (or strings) at hand: the `total` cells less
    the `slack` kept free behind the last of them."""
    offsets, ntrees = forest_offsets(counts)
    if int(offsets[-1]) + slack != total:
        raise ValueError(f"{what}: the counts add up to {int(offsets[-1])}, not to the {total - slack} {cells}")
    return offsets, ntrees


def _reserve(what, reserve_trees, reserve_leaves, max_count):
    """(reserve_trees, reserve_leaves) as non-negative ints; ValueError for a negative one, or when room is reserved and
    max_count is left open: the largest count of today's trees would bound the trees still to come."""
    reserve_trees, reserve_leaves = int(reserve_trees), int(reserve_leaves)
    if reserve_trees < 0 or reserve_leaves < 0:
        raise ValueError(f"{what}: negative reserve")
    if (reserve_trees or reserve_leaves) and max_count is None:
        raise ValueError(f"{what}: a forest with room to grow needs an explicit max_count")
    return reserve_trees, reserve_leaves


def forest_status_text(status):
    """The bits of vkmr_hip_reduce_forest_async's status word, named."""
    names = []
    if status & 1:
        names.append("bit 0: the offsets decrease or end past the leaves")
    if status & 2:
        names.append("bit 1: a tree holds more than max_count leaves")
    if status & ~3:
        names.append("unknown bits")
    return "; ".join(names) if names else "ok"


def forest_update_status_text(status):
    """The bits of vkmr_hip_forest_update_async's status word, named."""
    names = []
    if status & 1:
        names.append("bit 0: a tree outside the forest or an index outside its tree")
    if status & 2:
        names.append("bit 1: the (tree, index) pairs are not strictly increasing")
    if status & ~3:
        names.append("unknown bits")
    return "; ".join(names) if names else "ok"


class Frontier:
    """What a holder of the roots alone keeps of T trees that grow: `counts` (uint64 [T]) and `peaks` (uint32 [T, stride, 8]),
    cell l of a tree the root of the complete subtree of 2^l leaves that ends at its last leaf, for every set bit l of its
    count, zero for a clear bit (include/vkmr_hip.h).  Host arrays; every method is one ABI call on `dev` around them.  The
    roots and every later frontier follow from it and the leaves that arrive: no stored level, no witness."""

    MAX_COUNT = 1 << 58

    def __init__(self, counts, peaks):
        self.counts = np.array(counts, dtype=np.uint64).reshape(-1)
        T = int(self.counts.shape[0])
        peaks = np.array(peaks, dtype=np.uint32)
        self.peaks = peaks if peaks.ndim == 3 else peaks.reshape(T, -1, 8)
        if self.peaks.shape[0] != T or self.peaks.shape[2] != 8 or not 1 <= self.stride <= 64:
            raise ValueError("Frontier: peaks must be [T, stride, 8] with stride in 1..64")

    T = property(lambda self: int(self.counts.shape[0]))
    stride = property(lambda self: int(self.peaks.shape[1]))

    @classmethod
    def empty(cls, T, stride=64):
        """T trees not yet begun."""
        return cls(np.zeros(int(T), np.uint64), np.zeros((int(T), int(stride), 8), np.uint32))

    def same_as(self, other):
        """Byte for byte: equal counts and equal cells, the zero ones included."""
        return (self.counts.shape == other.counts.shape and self.peaks.shape == other.peaks.shape and bool((self.counts == other.counts).all())
                and bool((self.peaks == other.peaks).all()))

    def _walk(self, dev, want):
        """The root walk over the frontiers on `dev`: the roots [T, 8], or with `want` (roots [T, 8]) the answers uint32 [T]."""
        T = self.T
        if T == 0:
            return np.zeros((0, 8), np.uint32) if want is None else np.zeros(0, np.uint32)
        with dev.scope() as tmp:
            d_counts, d_peaks = tmp.upload(self.counts), tmp.upload(self.peaks)
            if want is None:
                d_roots = tmp.alloc(32 * T)
                dev.frontier_roots_enqueue(d_counts, d_peaks, self.stride, T, d_roots)
                return dev.download(d_roots, 32 * T).reshape(T, 8)
            d_ok = tmp.alloc(4 * T)
            dev.verify_frontier_enqueue(d_counts, d_peaks, self.stride, T, tmp.upload(_host(want, np.uint32, T, 8)), d_ok)
            return dev.download(d_ok, 4 * T)

    def roots(self, dev):
        """[T, 8] uint32: the root of every tree (all zero for one not yet begun)."""
        return self._walk(dev, None)

    def verify(self, dev, roots):
        """uint32 [T]: 1 where the frontier has the root roots[q], else 0 -- how a frontier that was sent is adopted under
        roots already trusted."""
        return self._walk(dev, roots)

    def _new_offsets(self, counts, n, what):
        """The offsets of the new leaves (uint64 [T + 1]); ValueError, before any device call, when the counts are not one per
        tree, do not add up to the n leaves, or take a tree past 2^58 leaves or past the bits a frontier of this stride holds."""
        offsets, m = _checked_offsets(counts, n, what)
        if m != self.T:
            raise ValueError(f"{what}: {m} counts for {self.T} trees")
        after = [int(c) + int(k) for c, k in zip(self.counts, np.diff(offsets))]
        if any(c > self.MAX_COUNT or c.bit_length() > self.stride for c in after):
            raise ValueError(f"{what}: a tree of {max(after)} leaves does not fit a frontier of stride {self.stride}")
        return offsets

    def _extend(self, dev, tmp, leaves_buf, offsets, what):
        """The one extend: the leaves in device memory, the frontier up and back, in place on the device.  The new roots."""
        T, n = self.T, int(offsets[-1])
        if T == 0:
            return np.zeros((0, 8), np.uint32)
        d_counts, d_peaks, d_roots, d_status = tmp.upload(self.counts), tmp.upload(self.peaks), tmp.alloc(32 * T), tmp.alloc(4)
        scratch = tmp.keep(dev.frontier_extend_scratch(n, T))
        dev.frontier_extend_enqueue(d_counts, d_peaks, self.stride, T, leaves_buf, n, tmp.upload(offsets), int(np.diff(offsets).max()), scratch,
                                    d_counts, d_peaks, d_roots, d_status)
        status = int(dev.download(d_status, 4)[0])
        if status:
            raise RuntimeError(f"Frontier.{what}: the device refused (status {status}: {frontier_status_text(status)})")
        self.counts = dev.download(d_counts, 8 * T, dtype=np.uint64)
        self.peaks = dev.download(d_peaks, 32 * T * self.stride).reshape(T, self.stride, 8)
        return dev.download(d_roots, 32 * T).reshape(T, 8)

    def extend(self, dev, digests, counts):
        """Tree q takes the next counts[q] rows of `digests` [n, 8] (a host array; 0 for a tree that takes none): the frontier
        advances and the new roots [T, 8] are returned -- what the primary's trees have after the same leaves.  ValueError
        as _new_offsets says."""
        digests = _host(digests, np.uint32, -1, 8)
        offsets = self._new_offsets(counts, int(digests.shape[0]), "extend")
        with dev.scope() as tmp:
            return self._extend(dev, tmp, tmp.upload(digests) if digests.shape[0] else None, offsets, "extend")

    def extend_packed(self, dev, batch, counts):
        """extend() by the digests of the strings of `batch`, mapped on the device; no digest goes through the host."""
        offsets = self._new_offsets(counts, int(batch.count), "extend_packed")
        with dev.scope() as tmp:
            return self._extend(dev, tmp, dev.map_packed(tmp, batch) if batch.count else None, offsets, "extend_packed")


class ConsistencyProof:
    """Q proofs that a tree only grew (include/vkmr_hip.h, CONSISTENCY PROOFS): query q says that tree `trees[q]`, which has
    `new_counts[q]` leaves, extends what it was at `old_counts[q]` leaves.  `peaks` (uint32 [Q, stride, 8]) are the peaks of the
    OLD count, `rights` the right neighbours of the walk from them to the root now; cells the check does not read are zero.
    Host arrays, as Frontier's; MerkleForest.consistency gathers one, a holder of the two roots verifies it."""

    def __init__(self, trees, old_counts, new_counts, peaks, rights):
        self.trees = np.array(trees, dtype=np.uint32).reshape(-1)
        self.old_counts = np.array(old_counts, dtype=np.uint64).reshape(-1)
        self.new_counts = np.array(new_counts, dtype=np.uint64).reshape(-1)
        Q = int(self.trees.shape[0])
        self.peaks, self.rights = (np.array(x, dtype=np.uint32) for x in (peaks, rights))
        if (self.old_counts.shape[0] != Q or self.new_counts.shape[0] != Q or self.peaks.ndim != 3 or self.peaks.shape != self.rights.shape
                or self.peaks.shape[0] != Q or self.peaks.shape[2] != 8 or not 1 <= self.stride <= 64):
            raise ValueError("ConsistencyProof: one tree, old count and new count per query; peaks and rights [Q, stride, 8] with stride in 1..64")

    Q = property(lambda self: int(self.trees.shape[0]))
    stride = property(lambda self: int(self.peaks.shape[1]))

    def same_as(self, other):
        """Byte for byte: equal queries, counts and cells, the zero ones included."""
        mine, theirs = ((p.trees, p.old_counts, p.new_counts, p.peaks, p.rights) for p in (self, other))
        return all(a.shape == b.shape and bool((a == b).all()) for a, b in zip(mine, theirs))

    def frontier(self):
        """Frontier(old_counts, peaks): frontier().roots(dev) is the root every queried tree had at its old count, and a
        follower that fell behind adopts it under the old root it trusts and goes on with Frontier.extend."""
        return Frontier(self.old_counts, self.peaks)

    def verify(self, dev, old_roots, new_roots):
        """uint32 [Q]: 1 where proof q holds under old_roots[q] and new_roots[q] ([Q, 8] each, per QUERY: the caller indexes
        its own root tables by `trees`), else 0."""
        Q = self.Q
        if Q == 0:
            return np.zeros(0, np.uint32)
        with dev.scope() as tmp:
            d_ok = tmp.alloc(4 * Q)
            dev.verify_consistency_enqueue(tmp.upload(self.old_counts), tmp.upload(self.new_counts), tmp.upload(self.peaks), tmp.upload(self.rights),
                                           self.stride, Q, tmp.upload(_host(old_roots, np.uint32, Q, 8)), tmp.upload(_host(new_roots, np.uint32, Q, 8)), d_ok)
            return dev.download(d_ok, 4 * Q)


class AbsenceProofs:
    """Q proofs that a digest is no leaf of a sorted tree (include/vkmr_hip.h, SORTED TREES): `queries[q]` ([Q, 8]) would stand at
    index `indices[q]` of tree `trees[q]`, between `pred[q]` and `succ[q]` (zero cells where there is none); `main` ([Q, stride, 8])
    is the inclusion proof of the anchor -- succ, or the last leaf behind which the digest lies -- and `low` the siblings of pred
    below the level at which the two paths meet.  `heights[q]` is the tree's.  Host arrays; MerkleForest.absence gathers one, a
    holder of the roots and the counts verifies it."""

    def __init__(self, trees, queries, indices, pred, succ, main, low, heights):
        self.trees, self.heights = (np.array(x, dtype=np.uint32).reshape(-1) for x in (trees, heights))
        self.indices = np.array(indices, dtype=np.uint64).reshape(-1)
        Q = int(self.trees.shape[0])
        self.queries, self.pred, self.succ = (np.array(x, dtype=np.uint32).reshape(-1, 8) for x in (queries, pred, succ))
        self.main, self.low = (np.array(x, dtype=np.uint32) for x in (main, low))
        if (any(a.shape[0] != Q for a in (self.heights, self.indices, self.queries, self.pred, self.succ)) or self.main.ndim != 3
                or self.main.shape != self.low.shape or self.main.shape[0] != Q or self.main.shape[2] != 8 or not 1 <= self.stride <= 63):
            raise ValueError("AbsenceProofs: one tree, digest, index, pred, succ and height per query; main and low [Q, stride, 8] with stride in 1..63")

    Q = property(lambda self: int(self.trees.shape[0]))
    stride = property(lambda self: int(self.main.shape[1]))
    neighbours = property(lambda self: np.ascontiguousarray(np.stack([self.pred, self.succ], axis=1)))   # [Q, 2, 8]: as the ABI takes them

    def same_as(self, other):
        """Byte for byte: equal queries, indices, neighbours, heights and cells, the zero ones included."""
        names = ("trees", "queries", "indices", "pred", "succ", "main", "low", "heights")
        return all(getattr(self, n).shape == getattr(other, n).shape and bool((getattr(self, n) == getattr(other, n)).all()) for n in names)

    def verify(self, dev, roots, counts):
        """uint32 [Q]: 0 not proven, 1 absent, 2 present -- proof q under roots[trees[q]] and counts[trees[q]] (roots [ntrees, 8],
        counts [ntrees]: the verifier's own tables)."""
        Q = self.Q
        if Q == 0:
            return np.zeros(0, np.uint32)
        roots, counts = _host(roots, np.uint32, -1, 8), _host(counts, np.uint64, -1)
        if roots.shape[0] != counts.shape[0]:
            raise ValueError("AbsenceProofs.verify: one count per root")
        with dev.scope() as tmp:
            d_verdict = tmp.alloc(4 * Q)
            dev.verify_forest_absence_enqueue(tmp.upload(self.queries), tmp.upload(self.trees), tmp.upload(self.indices), tmp.upload(self.neighbours),
                                              tmp.upload(self.main), tmp.upload(self.low), tmp.upload(self.heights), Q, self.stride,
                                              tmp.upload(roots) if roots.shape[0] else None, tmp.upload(counts) if roots.shape[0] else None,
                                              int(roots.shape[0]), d_verdict)
            return dev.download(d_verdict, 4 * Q)


def _digests_below(rows, x):
    """bool [n]: rows[i] < x in the order of the digests' bytes (word 0 first, every word unsigned); rows [n, 8], x [8]."""
    differs = rows != x
    first = np.argmax(differs, axis=1)
    at = np.arange(rows.shape[0])
    return differs.any(axis=1) & (rows[at, first] < x[first])


def _digests_above(rows, x):
    """bool [n]: rows[i] > x, as _digests_below."""
    differs = rows != x
    first = np.argmax(differs, axis=1)
    at = np.arange(rows.shape[0])
    return differs.any(axis=1) & (rows[at, first] > x[first])


class RangeProofs:
    """Q proofs that the leaves carried are ALL the leaves of a sorted tree in a closed interval (include/vkmr_hip.h, RANGE PROOFS):
    query q is (`trees[q]`, `lo[q]`, `hi[q]`); its run, leaves `firsts[q]` onwards of the tree, lies at `leaves[leaf_starts[q] :
    leaf_starts[q + 1]]` -- the leaves in range and the neighbour on either side that fences them --, `left` and `right` ([Q, stride,
    8]) are the nodes that close the run at every level, `heights[q]` is the tree's and `info` the gather's four words.  Host arrays;
    MerkleForest.ranges gathers one, a holder of the roots and the counts verifies it.  proofs[q] is query q's part as a dict."""

    def __init__(self, trees, lo, hi, firsts, leaf_starts, leaves, left, right, heights, info=None):
        self.trees, self.heights = (np.array(x, dtype=np.uint32).reshape(-1) for x in (trees, heights))
        self.firsts, self.leaf_starts = (np.array(x, dtype=np.uint64).reshape(-1) for x in (firsts, leaf_starts))
        Q = int(self.trees.shape[0])
        self.lo, self.hi, self.leaves = (np.array(x, dtype=np.uint32).reshape(-1, 8) for x in (lo, hi, leaves))
        self.left, self.right = (np.array(x, dtype=np.uint32) for x in (left, right))
        self.info = np.zeros(4, np.uint64) if info is None else np.array(info, dtype=np.uint64).reshape(4)
        if (any(a.shape[0] != Q for a in (self.heights, self.firsts, self.lo, self.hi)) or self.leaf_starts.shape[0] != Q + 1 or self.left.ndim != 3
                or self.left.shape != self.right.shape or self.left.shape[0] != Q or self.left.shape[2] != 8 or not 1 <= self.stride <= 63):
            raise ValueError("RangeProofs: one tree, lo, hi, first and height per query, Q + 1 leaf_starts; left and right [Q, stride, 8] with stride in 1..63")

    Q = property(lambda self: int(self.trees.shape[0]))
    stride = property(lambda self: int(self.left.shape[1]))

    def __len__(self):
        return self.Q

    def _run(self, q):
        q = int(q)
        if not 0 <= q < self.Q:
            raise IndexError(f"RangeProofs: query {q} of {self.Q}")
        a, b = int(self.leaf_starts[q]), int(self.leaf_starts[q + 1])
        if not a <= b <= self.leaves.shape[0]:
            raise ValueError(f"RangeProofs: leaf_starts[{q}] and the one behind it do not lie in the leaves")
        return self.leaves[a:b]

    def __getitem__(self, q):
        run = self._run(q)
        q = int(q)
        return {"tree": int(self.trees[q]), "lo": self.lo[q], "hi": self.hi[q], "first": int(self.firsts[q]), "leaves": run, "left": self.left[q],
                "right": self.right[q], "height": int(self.heights[q])}

    def in_range(self, q):
        """The carried leaves of query q that lie in [lo[q], hi[q]] ([n, 8]); what verify() counts in in_count when it proves q."""
        run = self._run(q)
        if run.shape[0] == 0:
            return run
        keep = ~_digests_below(run, self.lo[int(q)]) & ~_digests_above(run, self.hi[int(q)])
        return run[keep]

    def same_as(self, other):
        """Byte for byte: equal queries, firsts, leaf_starts, leaves, heights and cells, the zero ones included."""
        names = ("trees", "lo", "hi", "firsts", "leaf_starts", "leaves", "left", "right", "heights")
        return all(getattr(self, n).shape == getattr(other, n).shape and bool((getattr(self, n) == getattr(other, n)).all()) for n in names)

    def verify(self, dev, roots, counts):
        """(verdict uint32 [Q], in_first uint64 [Q], in_count uint64 [Q]): verdict 1 when the run of query q is proven complete under
        roots[trees[q]] and counts[trees[q]] (roots [ntrees, 8], counts [ntrees]: the verifier's own tables), and then the leaves
        inside the bounds as an index into the tree and a number; zeros otherwise."""
        Q = self.Q
        if Q == 0:
            return np.zeros(0, np.uint32), np.zeros(0, np.uint64), np.zeros(0, np.uint64)
        roots, counts = _host(roots, np.uint32, -1, 8), _host(counts, np.uint64, -1)
        if roots.shape[0] != counts.shape[0]:
            raise ValueError("RangeProofs.verify: one count per root")
        n = int(self.leaves.shape[0])
        with dev.scope() as tmp:
            d_verdict, d_first, d_count = tmp.alloc(4 * Q), tmp.alloc(8 * Q), tmp.alloc(8 * Q)
            dev.verify_forest_range_enqueue(tmp.upload(self.trees), tmp.upload(self.lo), tmp.upload(self.hi), tmp.upload(self.firsts),
                                            tmp.upload(self.leaf_starts), tmp.upload(self.leaves) if n else None, n, tmp.upload(self.left),
                                            tmp.upload(self.right), tmp.upload(self.heights), Q, self.stride,
                                            tmp.upload(roots) if roots.shape[0] else None, tmp.upload(counts) if roots.shape[0] else None,
                                            int(roots.shape[0]), tmp.alloc(dev.range_scratch_bytes(n, Q)), d_verdict, d_first, d_count)
            return dev.download(d_verdict, 4 * Q), dev.download(d_first, 8 * Q, dtype=np.uint64), dev.download(d_count, 8 * Q, dtype=np.uint64)


def range_status_text(status):
    """The bits of vkmr_hip_forest_range_async's status word (info[0]), named."""
    names = ["bit 0: more leaves are carried than the leaves buffer has cells (info[1] is the number)"] if status & 1 else []
    if status & ~1:
        names.append("unknown bits")
    return "; ".join(names) if names else "ok"


def sort_digests(digests, counts):
    """A HOST helper, numpy on the CPU, for tests and small callers: the digests ([n, 8] uint32) with every tree's leaves
    (counts[t] of them, in order) sorted by the order an absence proof rests on -- word 0 first, every word unsigned.  The device's
    sort is HipDevice.sort_leaves / build_sorted_forest; this one has no tie limit and takes the batches that one refuses."""
    d = _host(digests, np.uint32, -1, 8).copy()
    at = 0
    for c in (int(c) for c in counts):
        part = d[at: at + c]
        d[at: at + c] = part[np.lexsort(tuple(part[:, w] for w in range(7, -1, -1)))]
        at += c
    if at != d.shape[0]:
        raise ValueError(f"sort_digests: the counts sum to {at}, {d.shape[0]} digests given")
    return d


LEAFSORT_MAX_TIES = 1 << 14     # VKMR_LEAFSORT_MAX_TIES of csrc/leafsort_plan.hpp (tests/test_leafsort_abi.py holds the two together)


def leafsort_status_text(status):
    """The bits of vkmr_hip_forest_sort_leaves_async's status word (info[0]), named."""
    names = []
    if status & 3:
        names.append(forest_status_text(status & 3))
    if status & 4:
        names.append("bit 2: more leaves tie on the sort key than one sort places")
    if status & ~7:
        names.append("unknown bits")
    return "; ".join(names) if names else "ok"


MERGE_OPS = {"union": 0, "difference": 1, "intersection": 2}     # VKMR_MERGE_* of csrc/merge_plan.hpp


def _merge_op(op, what):
    if op in MERGE_OPS:
        return MERGE_OPS[op]
    if isinstance(op, (int, np.integer)) and not isinstance(op, bool) and int(op) in MERGE_OPS.values():
        return int(op)
    raise ValueError(f"{what}: op is one of {', '.join(MERGE_OPS)}, not {op!r}")


def merge_status_text(status):
    """The bits of vkmr_hip_forest_merge_leaves_async's status word (info[0]), named."""
    names = [text for bit, text in ((1, "bit 0: the offsets of A decrease or end past its cells"), (2, "bit 1: the offsets of B decrease or end past its cells"),
                                    (4, "bit 2: a tree of A is not strictly increasing"), (8, "bit 3: a tree of B decreases"),
                                    (16, "bit 4: the output has more leaves than cells")) if status & bit]
    if status & ~31:
        names.append("unknown bits")
    return "; ".join(names) if names else "ok"


def _raise_merge_status(info, what):
    status = int(info[0])
    if status:
        raise RuntimeError(f"{what}: the device refused the merge (status {status}: {merge_status_text(status)})")


def sorted_forest_packed(dev, batch, counts, max_count=None, reserve_trees=0, reserve_leaves=0):
    """(MerkleForest, order): merkle_forest_packed over SORTED leaves -- the strings of `batch` mapped to leaf digests once, every
    tree's digests (tree t the next counts[t] of them) sorted on the device and the stored forest built over the sorted buffer,
    with no trip through the host.  order [n] uint32: leaf j of the forest is the digest of string order[j].  Keywords and
    errors as HipDevice.build_sorted_forest."""
    what = "sorted_forest_packed"
    _checked_offsets(counts, batch.count, what, "strings")
    reserve_trees, reserve_leaves = _reserve(what, reserve_trees, reserve_leaves, max_count)
    total = batch.count + reserve_leaves
    with dev.scope() as tmp:
        d_leaves = tmp.alloc(32 * total) if total else None
        if batch.count:
            dev.map_packed(tmp, batch, out_buf=d_leaves)
        return dev._build_sorted_forest_of_buffer(tmp, d_leaves, total, counts, max_count, what, reserve_trees=reserve_trees,
                                                  reserve_leaves=reserve_leaves)


def consistency_status_text(status):
    """The bits of vkmr_hip_forest_consistency_async's status word, named."""
    names = []
    if status & 1:
        names.append("bit 0: a tree index outside the forest")
    if status & 2:
        names.append("bit 1: an old count above the count the tree has now")
    if status & 4:
        names.append("bit 2: a tree's count has more bits than a row has cells")
    if status & ~7:
        names.append("unknown bits")
    return "; ".join(names) if names else "ok"


def frontier_status_text(status):
    """The bits of vkmr_hip_frontier_extend_async's status word, named."""
    names = []
    if status & 1:
        names.append("bit 0: the offsets decrease, do not start at 0 or do not end at the new leaves")
    if status & 2:
        names.append("bit 1: a tree takes more than max_new leaves")
    if status & 4:
        names.append("bit 2: a tree would hold more than 2^58 leaves")
    if status & 8:
        names.append("bit 3: a new count has more bits than the frontier has cells")
    if status & ~15:
        names.append("unknown bits")
    return "; ".join(names) if names else "ok"


def forest_append_status_text(status):
    """The bits of vkmr_hip_forest_append_async's status word, named."""
    names = []
    if status & 1:
        names.append("bit 0: the new offsets decrease, do not start at 0 or do not end at the new leaves")
    if status & 2:
        names.append("bit 1: a new tree holds more than max_count leaves")
    if status & 4:
        names.append("bit 2: the forest's free trees do not begin where the caller says")
    if status & ~7:
        names.append("unknown bits")
    return "; ".join(names) if names else "ok"


def forest_copy_status_text(status):
    """The bits of vkmr_hip_forest_copy_trees_async's status word, named: append's three and bit 3."""
    names = [] if not status & 7 else [forest_append_status_text(status & 7)]
    if status & 8:
        names.append("bit 3: a chosen tree is not in the source forest, or a new count is not that tree's count")
    if status & ~15:
        names.append("unknown bits")
    return "; ".join(names) if names else "ok"


def merkleblocks_status_text(status):
    """The bits of vkmr_hip_forest_merkleblocks_async's status word (info[0]), named."""
    names = ["bit 0: a tree outside the forest or an index outside its tree", "bit 1: the entries are not strictly increasing",
             "bit 2: more hashes or flag bytes than the buffers hold"]
    return "; ".join(n for b, n in enumerate(names) if status >> b & 1)


def forest_multiproof_status_text(status):
    """The bits of vkmr_hip_forest_multiproof_async's status word (info[0]), named."""
    names = []
    if status & 3:
        names.append(forest_update_status_text(status & 3))
    if status & 4:
        names.append("bit 2: more nodes than the node buffer holds")
    if status & ~7:
        names.append("unknown bits")
    return "; ".join(names) if names else "ok"


def _forest_packed(dev, batch, counts, max_count, what, stored, mutated=False, reserve_trees=0, reserve_leaves=0):
    """`batch` mapped to leaf digests ONCE and one forest call over them: the roots (with `mutated`: and the masks), or with
    `stored` a MerkleForest that owns its leaves, with room to grow when some is reserved."""
    _checked_offsets(counts, batch.count, what, "strings")
    reserve_trees, reserve_leaves = _reserve(what, reserve_trees, reserve_leaves, max_count)
    with dev.scope() as tmp:
        if reserve_leaves:                       # the leaves buffer with spare cells behind the last leaf
            d_leaves = tmp.alloc(32 * (batch.count + reserve_leaves))
            if batch.count:
                dev.map_packed(tmp, batch, out_buf=d_leaves)
        else:
            d_leaves = dev.map_packed(tmp, batch) if batch.count else None
        if not stored:
            return dev._forest_of_buffer(d_leaves, batch.count, counts, max_count, what, mutated=mutated)
        forest = dev._build_forest_of_buffer(d_leaves, batch.count + reserve_leaves, counts, max_count, what, owned=[d_leaves] if d_leaves else [],
                                             reserve_trees=reserve_trees, reserve_leaves=reserve_leaves)
        tmp.release(d_leaves)
    return forest


def merkle_forest_packed(dev, batch, counts, max_count=None, reserve_trees=0, reserve_leaves=0):
    """The strings of `batch` mapped to leaf digests ONCE and the stored forest built over them, tree t over the next
    counts[t] of them, all on the device (a MerkleForest that owns its leaves).  reserve_trees, reserve_leaves: room for
    MerkleForest.append and append_packed, as HipDevice.build_forest reserves it; max_count must then be given."""
    return _forest_packed(dev, batch, counts, max_count, "merkle_forest_packed", stored=True, reserve_trees=reserve_trees,
                          reserve_leaves=reserve_leaves)


def merkle_roots_packed_forest(dev, batch, counts, max_count=None):
    """One root per block from a stream of strings: `batch` is mapped to leaf digests ONCE and ONE forest call reduces tree t
    over the next counts[t] of them.  [ntrees, 8] uint32 (digest_hex gives the canonical text); no digest goes through
    the host."""
    return _forest_packed(dev, batch, counts, max_count, "merkle_roots_packed_forest", stored=False)


def merkle_roots_packed_forest_mutated(dev, batch, counts, max_count=None):
    """merkle_roots_packed_forest with the verdict on every block: (roots [ntrees, 8] uint32, mutated [ntrees] uint64), bit l
    of mutated[t] set when level l of tree t holds two equal siblings that both exist (HipDevice.forest_roots_mutated).  The
    strings are mapped ONCE and ONE flagged forest call reduces them; no digest goes through the host."""
    return _forest_packed(dev, batch, counts, max_count, "merkle_roots_packed_forest_mutated", stored=False, mutated=True)


def digest_hex(words):
    """Canonical hex of a word-valued digest (big-endian bytes of H[0..7])."""
    return np.ascontiguousarray(words, dtype=np.uint32).astype(">u4").tobytes().hex()


def merkle_root_packed_batched(dev, batch, slice_capacity, batch_strings=None):
    """Same tree as merkle_root_packed, all slices resident and reduced by ONE
    vkmr_hip_reduce_slices_async, slice roots combined on the device."""
    n = batch.count
    if n == 0:
        return ""
    nslices = (n + slice_capacity - 1) // slice_capacity
    batch_strings = batch_strings or n
    with dev.scope() as tmp:
        d_slices = tmp.alloc(32 * nslices * slice_capacity)
        for b0 in range(0, n, batch_strings):
            with dev.scope() as up:
                dev.map_packed(up, batch.slice(b0, min(n, b0 + batch_strings)), d_slices, out_offset_digests=b0)
                dev.sync()
        count_last = n - (nslices - 1) * slice_capacity
        height = int(math.log2(slice_capacity)) if nslices > 1 else tree_height(n)
        d_scratch = tmp.alloc(dev.lib.vkmr_hip_reduce_slices_scratch_bytes(slice_capacity, nslices))
        d_roots = tmp.alloc(32 * nslices)
        dev.reduce_slices_async(d_slices, nslices, slice_capacity, count_last, height, d_scratch, d_roots)
        if nslices > 1:
            d_top, d_final = tmp.keep(dev.reduce_scratch(nslices)), tmp.alloc(32)
            dev.reduce_async(d_roots, nslices, tree_height(nslices), d_top, d_final)
            return digest_hex(dev.download(d_final, 32))
        return digest_hex(dev.download(d_roots, 32))


def merkle_root_packed(dev, batch, slice_capacity=None, batch_strings=None, levels_variant=False):
    """Root (hex) of all strings of `batch`: map in sub-batches of `batch_strings`,
    slices of `slice_capacity` digests (a power of two), per-slice reduce, combine.
    Same decomposition as the reference's stream processor (src/vkmr/SHA-256vk.cpp:288-429);
    by SURVEY.md 8a Q6 the result equals the single global duplicate-last tree."""
    n = batch.count
    if n == 0:
        return ""
    if slice_capacity is None:
        slice_capacity = 1 << max(1, (n - 1).bit_length())
    if slice_capacity & (slice_capacity - 1):
        raise ValueError("slice capacity must be a power of two")
    batch_strings = batch_strings or n
    nslices = (n + slice_capacity - 1) // slice_capacity
    cap_height = int(math.log2(slice_capacity))
    with dev.scope() as run:
        d_roots = run.alloc(32 * nslices)
        for s in range(nslices):
            lo, hi = s * slice_capacity, min(n, (s + 1) * slice_capacity)
            with dev.scope() as tmp:
                d_slice = tmp.alloc(32 * (hi - lo))
                for b0 in range(lo, hi, batch_strings):
                    with dev.scope() as up:
                        dev.map_packed(up, batch.slice(b0, min(hi, b0 + batch_strings)), d_slice, out_offset_digests=b0 - lo)
                        dev.sync()
                height = cap_height if nslices > 1 else tree_height(hi - lo)
                d_scratch = tmp.keep(dev.reduce_scratch(hi - lo, levels_variant))
                dev.reduce_async(d_slice, hi - lo, height, d_scratch, d_roots, root_index=s, levels_variant=levels_variant)
                dev.sync()
        roots = dev.download(d_roots, 32 * nslices).reshape(-1, 8)
    root = roots[0] if nslices == 1 else dev.combine(roots)
    return digest_hex(root)
