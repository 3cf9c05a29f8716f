"""Stored forests and packed batches that lie above 4 GiB: cell indices of 2^27 and more (2^27 cells x 32 B = 4 GiB), byte
offsets of 2^32 and more, packed-word indices of 2^30 and more.  A plain module: no fixtures, no GPU of its own.

A forest at a shift.  What a stored forest answers -- roots, proofs, masks, frontiers, find, diff, audit -- does not depend on
where it lies, so a SMALL forest laid into a LARGE buffer (offsets[0] = D > 0, the handle made with front=D) is checked by the
models the suite already has, at cell indices no other test reaches.  The gigabytes in front are allocated and never touched; a
kernel with one lane per cell of a level buffer leaves them through its tree search within a few loads.  Shifted is the view
of a forest_life_cases.ModelForest at such a shift: the same state, trees and digests, the cells TRUE cells.  The device's
`total` is D + the model's, so the stride (`levels`) is taken from that total: it differs from the model's own only while the
model's total is below max_count.

Canaries.  A store whose address lost its upper bits lands low in the same buffer: cells [0, HEAD) of each big buffer and FENCE
cells on either side of the level-0 window hold CANARY words, and are read again after every step of a walk and when a test ends.

No host array here is ever sized by D or by a batch's data_words: readers download the covering runs of a list of cells."""
import numpy as np
import pytest

import forest_life_cases as fl
import forest_multiproof_cases as fm
from merkle_model import stored_level_base, stored_node_cell, tree_height

LINE = 1 << 27              # cells: the first cell whose byte offset needs 33 bits
HEAD, FENCE = 4096, 64      # canary cells at the start of a big buffer, and on either side of the level-0 window
CANARY = 0xCA9A57E5
GAP = 4096                  # cells: two cells further apart than this are downloaded in separate runs

# (placement level, config, seed) of the life walks above the line: tests/test_forest_life_model.py asserts that they straddle it
HIGH_WALKS = [(0, "roomy", 7), (0, "tight", 1), (1, "roomy", 7), (3, "roomy", 4)]


def shift_for(level, total, ntrees):
    """The cells D in front of a forest of (total, ntrees) that put cell 2^27 of the buffer of `level` at a quarter of the
    forest's window there: level 0 lives in the digests buffer, level l >= 1 at stored_level_base(total + D, ntrees, l) of the
    level buffers, a tree at offset o at (o >> l) + t behind it.  For l >= 1 the smallest such D, never rounded to a
    power of two on purpose: (offset >> l) does not commute with a shift (copy_step's remark in forest_plan.hpp), and the
    trees' cells of the upper levels then lie where no forest at offset 0 puts them."""
    total, ntrees = int(total), int(ntrees)
    if level == 0:
        return LINE - total // 4

    def reach(d):
        return stored_level_base(total + d, ntrees, level) + ((d + total // 4) >> level) + ntrees // 2

    lo, hi = 0, LINE << level                       # reach(hi) >= ((2^27 << l) >> l)
    while lo < hi:
        mid = (lo + hi) // 2
        if reach(mid) >= LINE:
            hi = mid
        else:
            lo = mid + 1
    return lo


class Shifted:
    """A ModelForest as it lies `D` cells into a larger buffer; level None: where it is (D = 0), and then everything here is
    the model's own.  D is a function of the model's shape, so a forest and its twin share it and a repack chooses it again.
    Whatever is not overridden here -- trees, counts, roots(), masks(), find(), entries(), leaves_at(), checked(), `image` -- is
    the model's: `image` stays local, index it with local_live_cells()."""

    def __init__(self, model, level=None):
        self.local, self.level = model, level
        self.D = 0 if level is None else shift_for(level, model.total, model.ntrees)

    def __getattr__(self, name):
        return getattr(self.local, name)

    total = property(lambda self: self.local.total + self.D)
    dropped_leaves = property(lambda self: self.local.dropped_leaves + self.D)
    used_leaves = property(lambda self: self.local.used_leaves + self.D)
    levels = property(lambda self: tree_height(min(self.max_count, self.total)) if self.total else 1)
    frontier_stride = property(lambda self: max(1, min(self.max_count, self.total).bit_length()))

    def books(self):
        out = dict(self.local.books())
        out.update(total=self.total, levels=self.levels, dropped_leaves=self.dropped_leaves, used_leaves=self.used_leaves)
        return out

    def offsets(self):
        return self.local.offsets() + np.uint64(self.D)

    def live_cells(self):
        return self.local.live_cells() + self.D

    def local_live_cells(self):
        return self.local.live_cells()

    def nodes(self, with_levels=False):
        """(cells, digests[, levels]): ModelForest.nodes() at the true cells, through stored_node_cell with total + D and
        D + offset."""
        m = self.local
        off = self.offsets()
        cells, digests, levels = [], [], []
        for t, leaves in enumerate(m.trees):
            if leaves.shape[0]:
                lv = m.tree_levels(t)
                for l in range(1, len(lv) - 1):
                    for j in range(lv[l].shape[0]):
                        cells.append(stored_node_cell(self.total, m.ntrees, off[t], t, l, j))
                        digests.append(lv[l][j])
                        levels.append(l)
        assert len(set(cells)) == len(cells)
        out = (np.array(cells, dtype=np.int64), np.array(digests, dtype=np.uint32).reshape(-1, 8))
        return out + (np.array(levels, dtype=np.int64),) if with_levels else out

    def cells_of_level(self, level):
        """The true cells that hold something live at `level`: leaves of level 0, stored nodes of a level above."""
        if level == 0:
            return self.live_cells()
        cells, _, levels = self.nodes(with_levels=True)
        return cells[levels == level]

    def proofs(self, trees, indices):
        sib, heights = self.local.proofs(trees, indices)
        out = np.zeros((sib.shape[0], self.levels, 8), dtype=np.uint32)
        out[:, : sib.shape[1]] = sib
        return out, heights

    def multiproof(self, trees, indices):
        nodes, heights, level_counts, _ = fm.make(self.local.image, self.local.offsets(), trees, indices, self.levels)
        return nodes, heights, level_counts

    def frontier(self, stride=None):
        return self.local.frontier(self.frontier_stride if stride is None else stride)


def straddles(view):
    """Do the live cells of the view's placement level lie on both sides of cell 2^27?"""
    cells = view.cells_of_level(view.level)
    return bool(cells.shape[0]) and int(cells.min()) < LINE <= int(cells.max())


def straddling_steps(name, seed, level):
    """(steps after which the forest under test straddles the line, the kinds performed in such a step) over one walk, D chosen
    again after each repack.  A step counts when the forest it worked on -- for a repack the new one -- straddles."""
    life = fl.Life(seed, fl.CONFIGS[name])
    n, kinds = 0, set()
    for _, kind, p in life.steps():
        life.apply(kind, p)
        if straddles(Shifted(life.a, level)):
            n += 1
            kinds.add(kind)
    return n, kinds


# ---- the device side ---------------------------------------------------------------------------------------------------------

def alloc(gpu, nbytes, what):
    """gpu.alloc, or a skip that names the size: the tests here need tens of GiB of (untouched) device memory."""
    import vk_merkle_roots_amd as vk
    try:
        return gpu.alloc(nbytes)
    except vk.VkmrError as e:
        pytest.skip(f"no {nbytes} bytes of device memory for {what}: {e}")


def put(gpu, buf, byte_offset, arr):
    """Host array -> buf at a byte offset."""
    arr = np.ascontiguousarray(arr)
    if arr.nbytes:
        gpu._call("vkmr_hip_memcpy_h2d_async", buf.at(byte_offset), arr.ctypes.data, arr.nbytes)
        gpu.sync()


def zero(gpu, buf, byte_offset, nbytes):
    if nbytes:
        gpu._call("vkmr_hip_memset_async", buf.at(byte_offset), 0, nbytes)
        gpu.sync()


def write_canary(gpu, buf, first_cell, ncells, words_per_cell=8):
    put(gpu, buf, 4 * words_per_cell * first_cell, np.full(ncells * words_per_cell, CANARY, dtype=np.uint32))
    return (buf, 4 * words_per_cell * first_cell, 4 * words_per_cell * ncells)


def canaries_intact(gpu, canaries):
    """Every canary range, (buffer, byte offset, bytes), still holds nothing but CANARY words; the first that does not."""
    for n, (buf, at, nbytes) in enumerate(canaries):
        got = gpu.download(buf, nbytes, offset=at)
        assert (got == CANARY).all(), ("canary", n, "byte", at + 4 * int(np.flatnonzero(got != CANARY)[0]))
    return True


def read_cells(gpu, buf, cells, words_per_cell=8):
    """[len(cells), words_per_cell]: the cells of `buf` named, by downloading the covering range of every run of cells that lie
    within GAP of each other -- never a whole buffer."""
    cells = np.asarray(cells, dtype=np.int64).reshape(-1)
    out = np.zeros((cells.shape[0], words_per_cell), dtype=np.uint32)
    if cells.shape[0] == 0:
        return out
    order = np.argsort(cells, kind="stable")
    ranked = cells[order]
    starts = np.concatenate([[0], np.flatnonzero(np.diff(ranked) > GAP) + 1, [ranked.shape[0]]])
    for a, b in zip(starts, starts[1:]):
        lo, hi = int(ranked[a]), int(ranked[b - 1]) + 1
        run = gpu.download(buf, 4 * words_per_cell * (hi - lo), offset=4 * words_per_cell * lo).reshape(-1, words_per_cell)
        out[order[a:b]] = run[ranked[a:b] - lo]
    return out


def _shell(gpu, view, counts, offsets, used_trees):
    """The buffers of a forest of the view's shape at its shift and the handle over them: the digests buffer (FENCE cells
    longer than the forest's `total`, for the canary behind the window), the level buffers, offsets and roots.  Only the
    window [D, D + total) of level 0 is zero-filled, as the model's image is; the handle owns everything and carries the
    canary ranges in `canaries`."""
    import vk_merkle_roots_amd as vk
    D, T, m = view.D, view.total, view.local
    assert D >= HEAD + FENCE
    bufs = []
    try:
        d_leaves = alloc(gpu, 32 * (T + FENCE), "level 0")
        bufs.append(d_leaves)
        forest_bytes = gpu.forest_tree_bytes(T, m.ntrees, m.max_count)
        assert forest_bytes == 32 * stored_level_base(T, m.ntrees, view.levels + 1) >= 32 * HEAD
        d_forest = alloc(gpu, forest_bytes, "the level buffers")
        bufs.append(d_forest)
        d_off = gpu.upload(np.asarray(offsets, dtype=np.uint64))
        bufs.append(d_off)
        d_roots = gpu.upload(np.zeros((m.ntrees, 8), dtype=np.uint32))
        bufs.append(d_roots)
        zero(gpu, d_leaves, 32 * D, 32 * m.total)
        canaries = [write_canary(gpu, d_leaves, 0, HEAD), write_canary(gpu, d_forest, 0, HEAD), write_canary(gpu, d_leaves, D - FENCE, FENCE),
                    write_canary(gpu, d_leaves, T, FENCE)]
    except BaseException:
        for b in bufs:
            b.free()
        raise
    handle = vk.MerkleForest(gpu, d_leaves, T, counts, d_off, m.max_count, d_forest, d_roots, owned=[d_leaves], used_trees=used_trees, front=D)
    handle.canaries = canaries
    return handle


def build(gpu, view):
    """The MerkleForest of a model that has dropped nothing yet, at the view's shift: only the window's leaves are uploaded, at
    an offset, and the forest is built through the raw call, as forest_update_cases.RawForest builds."""
    m = view.local
    assert m.dropped_trees == 0 and m.dropped_leaves == 0
    handle = _shell(gpu, view, m.counts, view.offsets(), m.used_trees)
    try:
        put(gpu, handle.digests, 32 * view.D, m.image[: m.used_leaves])
        with gpu.scope() as tmp:
            d_status = tmp.upload(np.full(1, 0xDEADBEEF, dtype=np.uint32))
            gpu.reduce_forest_tree_async(handle.digests, view.total, handle.offsets, m.ntrees, m.max_count, handle.forest, handle.roots_buf, d_status)
            assert int(gpu.download(d_status, 4)[0]) == 0
    except BaseException:
        handle.free()
        raise
    return handle


def empty_shell(gpu, view):
    """A forest of the view's shape at its shift with no tree in use: counts all 0, every offset D, used_trees 0."""
    m = view.local
    return _shell(gpu, view, np.zeros(m.ntrees, dtype=np.uint64), np.full(m.ntrees + 1, view.D, dtype=np.uint64), 0)


def repacked_at(gpu, forest, level, trees=None, reserve_trees=0, reserve_leaves=0, mutated=False):
    """MerkleForest.repacked() with the new forest at a shift: an empty shell of the new shape, D chosen again for it, then
    append_from -- the two steps repacked() itself performs."""
    sel = np.arange(forest.dropped_trees, forest.used_trees, dtype=np.uint32) if trees is None else np.array(trees, dtype=np.uint32).reshape(-1)
    counts = forest.counts[sel.astype(np.int64)]
    shape = fl.ModelForest(int(sel.shape[0]) + reserve_trees, int(counts.sum()) + reserve_leaves, forest.max_count)
    new = empty_shell(gpu, Shifted(shape, level))
    try:
        got = new.append_from(forest, sel, mutated=mutated)
    except BaseException:
        new.free()
        raise
    if mutated:
        new.built_mutated = np.concatenate([got[1], np.zeros(reserve_trees, dtype=np.uint64)])
    return new


# ---- packed batches at high word indices ---------------------------------------------------------------------------------------
#
# A batch for vkmr_hip_map_async whose data buffer is mostly untouched: the real strings sit in CLUSTERS uploaded at an offset,
# and around them lies a long list of filler entries of size 0 whose `start` is the first word of the cluster in front of them
# (of the first cluster, for those in front of it) -- so a tile's extent never leaves its cluster.  The number of entries is
# what makes vkmr_map::plan (csrc/map_plan.hpp) choose the wanted mode.

MAP_KERNELS = {"STAGED": "map_kernel<512, 1024, 17664, 0, false, 0>", "DIRECT512": "map_kernel<512, 2048, 64, 2, true, 0>",
               "DIRECT256": "map_kernel<256, 2048, 64, 2, true, 0>", "LONG512": "map_kernel<512, 2048, 64, 5, true, 0>",
               "LONG256": "map_kernel<256, 2048, 64, 5, true, 0>"}
STAGE_WORDS = 17664


def map_mode(data_words, count):
    """The mode vkmr_map::plan gives a batch: by the average packed string in words, and by whether the launch is short."""
    avg = (data_words + count - 1) // count
    big = ((count // 1024) & ~63) >= 1024
    if avg >= 128:
        return "LONG512" if big else "LONG256"
    if avg >= 32:
        return "DIRECT512" if big else "DIRECT256"
    return "STAGED"


class Cluster:
    """About 600 strings of 0 - 100 bytes (a few of 200 - 5000 with `long_ones`) packed back to back so that they lie across
    word `across` of the data buffer -- or, with across None, so that they end with the buffer of data_words words, followed by
    one string the end of the buffer cuts (the kernel hashes the bytes that are there) and one entry wholly outside it (hashed
    as the empty string).  words: what is uploaded at word `first`; meta [n, 2]: {start word, size in bytes} as the entries
    declare them; want [n, 8]: oracle.leaf of what each entry must hash."""

    def __init__(self, oracle, seed, data_words, across=None, long_ones=False):
        rng = np.random.default_rng(seed)
        sizes = [int(x) for x in rng.integers(0, 101, size=600)]
        sizes[5], sizes[77], sizes[300] = 0, 55, 64                           # an empty one, one that fills a block but for the length, a whole block
        if long_ones:
            for at, size in ((40, 200), (199, 5000), (333, 1021), (580, 512)):
                sizes[at] = size
        strings = [rng.integers(0, 256, size=n, dtype=np.uint8).tobytes() for n in sizes]
        packed = b"".join(s + b"\0" * (-len(s) % 4) for s in strings)
        nwords = len(packed) // 4
        starts = np.concatenate([[0], np.cumsum([(n + 3) // 4 for n in sizes])])[:-1]
        hashed = list(strings)
        if across is None:
            cut = rng.integers(0, 256, size=50, dtype=np.uint8).tobytes()     # 50 bytes declared, 3 words of them inside the buffer
            packed += cut[:12]
            self.first = data_words - 3 - nwords
            starts = np.concatenate([starts, [nwords, nwords + 3 + 4]])      # the last entry begins 4 words behind the buffer's end
            sizes += [50, 40]
            hashed += [cut[:12], b""]
        else:
            self.first = across - int(starts[300])                            # string 300, a whole block, begins at the word itself
            assert self.first < across < self.first + nwords
        self.words = np.frombuffer(packed, dtype="<u4").astype(np.uint32)
        assert 0 <= self.first and self.first + self.words.shape[0] <= data_words
        self.meta = np.stack([starts + self.first, np.array(sizes)], axis=1).astype(np.uint32)
        assert int(self.meta[:, 0].astype(np.int64).max()) == int((starts + self.first).max()) < 2**32
        self.want = np.stack([oracle.leaf(s) for s in hashed])
        self.n = self.meta.shape[0]
        self.span = self.first + nwords - (self.first & ~3)                   # the words a tile that holds all of it stages


def map_case(gpu, oracle, d_data, data_words, count, clusters, mode):
    """One vkmr_hip_map_async over `count` entries -- the clusters' (already uploaded) strings, fillers around them -- that must
    run as `mode`: the kernel's name afterwards, every real entry and 10 000 sampled fillers (all of them, where there are fewer) against the oracle, the canaries
    in front of the output, behind it and in [count, count + 64).  Metadata and output are built and read piecewise: no host
    array is sized by data_words, nor by count."""
    import vk_merkle_roots_amd as vk
    assert map_mode(data_words, count) == mode and count + FENCE < 2**32
    k = len(clusters)
    at = [(j + 1) * count // (k + 1) - c.n // 2 + 37 for j, c in enumerate(clusters)]           # where cluster j's entries begin: no tile's edge
    assert at[0] > 0 and all(a + c.n < b for a, c, b in zip(at, clusters, at[1:] + [count]))
    if mode == "STAGED":                                                       # a tile that holds real strings is staged, not the fallback:
        assert k == 1 and clusters[0].span <= STAGE_WORDS - 4                   # any run of entries spans at most its one cluster
    rng = np.random.default_rng(count)
    empty = oracle.leaf(b"")
    d_meta = d_out = None
    try:
        d_meta = alloc(gpu, 8 * count, "the metadata")
        d_out = alloc(gpu, 32 * (FENCE + count + FENCE), "the digests")
        chunk = 1 << 20
        for j, c in enumerate(clusters):                                       # fillers [lo, hi) begin at cluster j's first word
            lo, hi = (0 if j == 0 else at[j]), (at[j + 1] if j + 1 < k else count)
            fill = np.tile(np.array([c.first, 0], dtype=np.uint32), (min(chunk, hi - lo), 1))
            for a in range(lo, hi, chunk):
                put(gpu, d_meta, 8 * a, fill[: min(chunk, hi - a)])
        for a, c in zip(at, clusters):
            put(gpu, d_meta, 8 * a, c.meta)
        canaries = [write_canary(gpu, d_out, 0, FENCE), write_canary(gpu, d_out, FENCE + count, FENCE)]
        gpu.map_async(d_data, data_words, d_meta, count, d_out, out_offset_digests=FENCE)
        gpu.sync()
        info = vk.lib().vkmr_hip_kernel_info().decode()
        assert MAP_KERNELS[mode] in info, info
        for j, (a, c) in enumerate(zip(at, clusters)):
            got = read_cells(gpu, d_out, FENCE + a + np.arange(c.n))
            bad = np.flatnonzero((got != c.want).any(axis=1))
            assert bad.shape[0] == 0, (mode, "cluster", j, "at word", c.first, "entries", bad[:8].tolist(), "of", c.n)
        if count <= 20000:                                                     # a short launch: every filler there is
            cells = np.arange(count)
        else:
            cells = (rng.integers(0, count - 100, size=110)[:, None] + np.arange(100)[None, :]).reshape(-1)
        edges = np.array([0, count - 1] + [a - 1 for a in at] + [a + c.n for a, c in zip(at, clusters)])
        cells = np.concatenate([cells, edges])
        real = np.zeros(cells.shape[0], dtype=bool)
        for a, c in zip(at, clusters):
            real |= (cells >= a) & (cells < a + c.n)
        cells = cells[~real]
        assert cells.shape[0] >= min(10000, count - sum(c.n for c in clusters))
        got = read_cells(gpu, d_out, FENCE + cells)
        bad = np.flatnonzero((got != empty).any(axis=1))
        assert bad.shape[0] == 0, (mode, "fillers", cells[bad[:8]].tolist())
        assert canaries_intact(gpu, canaries)
    finally:
        for b in (d_meta, d_out):
            if b:
                b.free()
