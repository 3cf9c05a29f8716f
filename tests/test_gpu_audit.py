"""The audit of a stored forest or tree on the GPU (vkmr_hip_forest_audit_async and vkmr_hip_tree_audit_async, raw and through
MerkleForest / MerkleTree): a fresh build audits clean, then single cells are written and every output -- the four counters, the
masks, the list up to the capacity -- is compared exactly with the rule restated in tests/audit_cases.py; the words around the
outputs and behind the list keep their pattern, and the structure is read back byte for byte after every call."""
import numpy as np
import pytest

import audit_cases as ac
from merkle_model import At

pytestmark = pytest.mark.gpu

GUARD = 512                                       # words in front of and behind each output: more than one workgroup's lanes
FULL_SCAN_NODES = 1500                            # above this the model looks only at the nodes a write can change


def write_cells(gpu, buf, mirror, last):
    """Every cell of `mirror` that differs from `last` written to the device buffer by itself, 32 bytes each; `last` follows."""
    rows = np.flatnonzero((mirror != last).any(axis=1))
    for i in rows:
        row = np.ascontiguousarray(mirror[i])
        gpu._call("vkmr_hip_memcpy_h2d_async", At(buf, 32 * int(i)), row.ctypes.data, 32)
        gpu.sync()
    last[rows] = mirror[rows]
    return len(rows)


class Outputs:
    """masks [n] uint64, trees / levels [cap] uint32, nodes [cap] uint64 and info [4] on the device, each between GUARD words of
    audit_cases' fill pattern."""

    def __init__(self, gpu, nmasks, cap):
        self.gpu, self.nmasks, self.cap = gpu, nmasks, cap
        self.shapes = [(nmasks, np.uint64, ac.FILL64), (cap, np.uint32, ac.FILL32), (cap, np.uint32, ac.FILL32), (cap, np.uint64, ac.FILL64), (4, np.uint64, ac.FILL64)]
        self.bufs = [gpu.upload(np.full(2 * GUARD + n, fill, dtype=t)) for n, t, fill in self.shapes]
        self.at = [At(b, GUARD * np.dtype(t).itemsize) for b, (_, t, _) in zip(self.bufs, self.shapes)]

    def read(self):
        """(info, masks, trees, levels, nodes), the guards checked."""
        out = []
        for b, (n, t, fill) in zip(self.bufs, self.shapes):
            a = self.gpu.download(b, np.dtype(t).itemsize * (2 * GUARD + n), dtype=t)
            assert (a[:GUARD] == fill).all() and (a[GUARD + n:] == fill).all(), "guard words"
            out.append(a[GUARD: GUARD + n])
            b.free()
        masks, trees, levels, nodes, info = out
        return info, masks, trees, levels, nodes


def scratch(gpu, total, ntrees, capacity):
    return gpu.upload(np.full(gpu.audit_scratch_bytes(total, ntrees, capacity) // 4, ac.FILL32, dtype=np.uint32)) if capacity else None


class DevForest:
    """The mirror `f` (audit_cases.Forest) as a stored forest on the device, BUILT there into buffers prefilled with the
    mirror's padding, so that the two can be compared cell for cell."""

    def __init__(self, gpu, f, offsets=None):
        import vk_merkle_roots_amd as vk
        self.gpu, self.f = gpu, f
        self.d_leaves = gpu.upload(f.leaves) if f.total else None
        self.d_off = gpu.upload(f.offsets if offsets is None else np.asarray(offsets, dtype=np.uint64))
        assert gpu.forest_tree_bytes(f.total, f.ntrees, f.max_count) == 32 * f.forest.shape[0]
        self.d_forest = gpu.upload(np.full_like(f.forest, ac.PADDING))
        self.d_roots = gpu.upload(np.full_like(f.roots, ac.PADDING))
        d_status = gpu.upload(np.full(1, 0xDEADBEEF, dtype=np.uint32))
        gpu.reduce_forest_tree_async(self.d_leaves, f.total, self.d_off, f.ntrees, f.max_count, self.d_forest, self.d_roots, d_status)
        self.build_status = int(gpu.download(d_status, 4)[0])
        d_status.free()
        self.handle = vk.MerkleForest(gpu, self.d_leaves, f.total, f.counts, self.d_off, f.max_count, self.d_forest, self.d_roots)
        self.last = [a.copy() for a in f.arrays()]

    def state(self):
        gpu, f = self.gpu, self.f
        return (gpu.download(self.d_leaves, 32 * f.total).reshape(-1, 8) if f.total else np.zeros((0, 8), dtype=np.uint32),
                gpu.download(self.d_forest, 32 * f.forest.shape[0]).reshape(-1, 8), gpu.download(self.d_roots, 32 * f.ntrees).reshape(-1, 8))

    def push(self):
        """The mirror's changed cells written to the device, one cell at a time."""
        return sum(write_cells(self.gpu, b, m, l) for b, m, l in zip((self.d_leaves, self.d_forest, self.d_roots), self.f.arrays(), self.last) if b)

    def audit(self, capacity):
        f, gpu = self.f, self.gpu
        out, d_scr = Outputs(gpu, f.ntrees, capacity), scratch(gpu, f.total, f.ntrees, capacity)
        lists = out.at[1:4] if capacity else (None, None, None)
        self.handle.audit_async(d_scr, out.at[0], *lists, capacity, out.at[4])
        got = out.read()
        if d_scr:
            d_scr.free()
        return got

    def free(self):
        for b in (self.d_leaves, self.d_off, self.d_forest, self.d_roots):
            if b:
                b.free()


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def rounds(struct, dev, corruptions, mirror_arrays, what, capacities=lambda n: sorted({n, max(n - 1, 0), 0})):
    """A clean audit, then every corruption by itself: written cell by cell, audited at capacity n, n - 1 and 0, compared with
    the model, the structure read back unchanged, the cells put back."""
    base = [a.copy() for a in mirror_arrays()]
    clean = struct.audit(4)
    assert clean.n_bad == 0
    before = dev.state()
    for capacity in (0, 4):
        ac.assert_matches(clean if capacity else struct.audit(0), *dev.audit(capacity), (what, "fresh", capacity))
    assert same(dev.state(), before)
    full = clean.checked <= FULL_SCAN_NODES
    for name, ids, write, n in corruptions:
        write()
        assert dev.push() >= 1, (what, name)
        before = dev.state()
        for capacity in capacities(n):
            want = struct.audit(capacity, only=None if full else ac.touched(ids))
            assert want.n_bad == n, (what, name, want.n_bad)
            ac.assert_matches(want, *dev.audit(capacity), (what, name, capacity))
        assert same(dev.state(), before), (what, name, "the audit wrote to the structure")
        for a, b in zip(mirror_arrays(), base):
            a[:] = b
        dev.push()
    ac.assert_matches(clean, *dev.audit(4), (what, "put back"))


@pytest.mark.parametrize("name,counts,first,slack", ac.FORESTS, ids=[c[0] for c in ac.FORESTS])
def test_forests_fresh_then_every_corruption(gpu, name, counts, first, slack):
    f = ac.Forest(counts, seed=len(counts), first=first, slack=slack)
    dev = DevForest(gpu, f)
    assert dev.build_status == 0
    assert same(dev.state(), f.arrays()), "the build and the mirror disagree"       # cell for cell, the padding included
    assert f.audit().checked == sum(ac.level_count(c, l) for c in counts for l in range(1, ac.tree_height(c) + 1) if c) + counts.count(0)
    rounds(f, dev, ac.forest_corruptions(f), f.arrays, name)
    dev.free()


class DevTree:
    def __init__(self, gpu, tr):
        self.gpu, self.tr = gpu, tr
        self.d_leaves = gpu.upload(tr.leaves)
        self.handle = gpu.build_tree(self.d_leaves, tr.count, tr.height)
        self.last = [tr.leaves.copy(), None]

    def state(self):
        tr = self.tr
        return (self.gpu.download(self.d_leaves, 32 * tr.count).reshape(-1, 8), self.gpu.download(self.handle.tree, 32 * tr.tree.shape[0]).reshape(-1, 8))

    def push(self):
        return sum(write_cells(self.gpu, b, m, l) for b, m, l in zip((self.d_leaves, self.handle.tree), (self.tr.leaves, self.tr.tree), self.last))

    def audit(self, capacity):
        tr, gpu = self.tr, self.gpu
        out, d_scr = Outputs(gpu, 0, capacity), scratch(gpu, tr.count, 1, capacity)
        self.handle.audit_async(d_scr, *(out.at[2:4] if capacity else (None, None)), capacity, out.at[4])
        info, _, trees, levels, nodes = out.read()
        assert (trees == ac.FILL32).all()          # the tree call has no such output
        if d_scr:
            d_scr.free()
        return info, None, None, levels, nodes

    def free(self):
        self.handle.free()
        self.d_leaves.free()


@pytest.mark.parametrize("count,height", ac.TREES)
def test_trees_fresh_then_every_corruption(gpu, count, height):
    tr = ac.Tree(count, height, seed=count)
    dev = DevTree(gpu, tr)
    dev.last[1] = tr.tree.copy()
    assert same(dev.state(), (tr.leaves, tr.tree)), "the build and the mirror disagree"
    assert tr.audit().checked == sum(-(-count >> l) for l in range(1, tr.height + 1))
    rounds(tr, dev, ac.tree_corruptions(tr), lambda: (tr.leaves, tr.tree), (count, height))
    dev.free()


def test_a_tree_of_600001_leaves(gpu):
    """Past every threshold of the level kernels and ragged on most levels.  The mirror takes the levels the device built (their
    root checked against the CPU backend) and the model looks at the nodes a write can change: a verdict depends on the node's
    own cell and its two children alone."""
    import vk_merkle_roots_amd as vk
    count, _ = ac.BIG_TREE
    leaves = np.random.default_rng(600001).integers(0, 2**32, size=(count, 8), dtype=np.uint32)
    tr = ac.Tree(count, leaves=leaves)
    dev = DevTree(gpu, tr)
    tr.tree[:] = dev.state()[1]
    dev.last[1] = tr.tree.copy()
    root = np.zeros(8, dtype=np.uint32)
    assert vk.host_lib().vkmr_host_cpu_reduce(leaves.ctypes.data, count, tr.height, root.ctypes.data) == 0 and np.array_equal(root, tr.tree[-1])
    for capacity in (0, 3):
        info, _, _, levels, nodes = dev.audit(capacity)
        assert list(info) == [0, 0, 0, tr.node_count()] and (levels == ac.FILL32).all() and (nodes == ac.FILL64).all()
    every = ac.tree_corruptions(tr)
    picked = [c for c in every if c[0] in ("first_leaf", "last_leaf", "the_root", "siblings", "consistent_forgery", "inner_l1", "inner_l7", "inner_l19")]
    picked += [c for c in every if c[0].startswith("ragged_edge")][:2]
    base = tr.leaves.copy(), tr.tree.copy()
    before_all = dev.state()
    for name, ids, write, n in picked:
        write()
        dev.push()
        for capacity in (n, n - 1):
            want = tr.audit(capacity, only=ac.touched(ids))
            assert want.n_bad == n, (name, want.n_bad)
            ac.assert_matches(want, *dev.audit(capacity), (name, capacity))
        tr.leaves[:], tr.tree[:] = base
        dev.push()
    assert same(dev.state(), before_all)
    # all of them at once: the list is in (level, node) order across levels, cut at the capacity
    ids_all = []
    for name, ids, write, n in picked:
        write()
        ids_all += ids
    dev.push()
    want = tr.audit(1000, only=ac.touched(ids_all))
    assert want.n_bad > 7 and list(zip(want.levels, want.nodes)) == sorted(zip(want.levels, want.nodes))
    ac.assert_matches(want, *dev.audit(1000), "all at once")
    ac.assert_matches(tr.audit(7, only=ac.touched(ids_all)), *dev.audit(7), "all at once, cut at 7")
    dev.free()


def test_a_refused_forest_reports_the_check_and_audits_nothing(gpu):
    f = ac.Forest([5, 0, 9], seed=3)
    good = DevForest(gpu, f)
    bad = DevForest(gpu, f, offsets=[0, 5, 4, 13])          # decreasing: the build refuses it, and so does the audit
    assert bad.build_status & 1
    import vk_merkle_roots_amd as vk
    bad.handle = vk.MerkleForest(gpu, bad.d_leaves, f.total, f.counts, bad.d_off, f.max_count, good.d_forest, good.d_roots)
    for capacity in (0, 4):
        info, masks, trees, levels, nodes = bad.audit(capacity)
        assert list(info) == [1, 0, 0, 0] and not masks.any()
        assert (trees == ac.FILL32).all() and (levels == ac.FILL32).all() and (nodes == ac.FILL64).all()
    too_small = vk.MerkleForest(gpu, good.d_leaves, f.total, f.counts, good.d_off, 8, good.d_forest, good.d_roots)       # a tree above max_count
    good.handle = too_small
    info, masks, *_ = good.audit(4)
    assert list(info) == [2, 0, 0, 0] and not masks.any()
    bad.free()
    good.free()


def test_the_python_layer_after_every_way_of_rewriting_a_forest(gpu):
    """update, update_entries, replace and sync_from leave a forest that audits clean; a cell overwritten behind their back is
    found by audit() at its position, with the list sized from the masks-only pass."""
    rng = np.random.default_rng(9)
    counts = [70, 0, 1, 200, 9, 33]
    leaves = rng.integers(0, 2**32, size=(sum(counts), 8), dtype=np.uint32)
    forest, other = gpu.build_forest(leaves, counts), gpu.build_forest(leaves, counts)
    want_checked = ac.Forest(counts).audit().checked
    fresh = forest.audit()
    assert fresh.clean and fresh.n_bad == 0 and fresh.checked == want_checked and not fresh.masks.any() and fresh.nodes.shape == (0,)
    new = rng.integers(0, 2**32, size=(5, 8), dtype=np.uint32)
    forest.update([0, 0, 3, 3, 5], [0, 69, 7, 199, 32], new)
    assert forest.audit().clean
    with gpu.scope() as tmp:
        d_t, d_i = tmp.upload(np.array([4, 3, 3], dtype=np.uint32)), tmp.upload(np.array([8, 100, 100], dtype=np.uint64))
        forest.update_entries(d_t, d_i, tmp.upload(new[:3]), 3)
    assert forest.audit().clean
    assert forest.replace(new[:2], new[2:4])[0] == 2 and forest.audit().clean
    assert other.sync_from(forest) > 0 and other.audit().clean and other.audit(capacity=0).clean
    # one inner cell of tree 3 (level 2, node 5) set to 0xFF bytes: the cell and its parent
    cell = sum((sum(counts) >> j) + len(counts) for j in range(1, 2)) + ((70 + 0 + 1) >> 2) + 3 + 5
    gpu._call("vkmr_hip_memset_async", At(forest.forest, 32 * cell), 0xFF, 32)
    r = forest.audit()
    assert not r.clean and r.n_bad == 2 and r.flagged == 1 and r.checked == want_checked and r.status == 0
    assert list(zip(r.trees, r.levels, r.nodes)) == [(3, 2, 5), (3, 3, 2)] and list(r.masks) == [0, 0, 0, 0b110, 0, 0]
    cut = forest.audit(capacity=1)
    assert cut.status == 4 and cut.n_bad == 2 and list(zip(cut.trees, cut.levels, cut.nodes)) == [(3, 2, 5)]
    assert forest.audit(capacity=0).n_bad == 2 and forest.audit(capacity=0).nodes.shape == (0,)
    forest.free()
    other.free()


def test_the_tree_and_the_forest_of_one_tree_agree(gpu):
    rng = np.random.default_rng(77)
    leaves = rng.integers(0, 2**32, size=(77, 8), dtype=np.uint32)
    forest = gpu.build_forest(leaves, [77])
    d_leaves = gpu.upload(leaves)
    tree = gpu.build_tree(d_leaves, 77)
    assert tree.height == forest.levels == 7
    a, b = tree.audit(), forest.audit()
    assert a.clean and b.clean and a.checked == b.checked == 39 + 20 + 10 + 5 + 3 + 2 + 1
    # level 3, node 4, and a leaf: the same cells in both layouts
    gpu._call("vkmr_hip_memset_async", At(tree.tree, 32 * (tree.level_offset(3) + 4)), 0x11, 32)
    gpu._call("vkmr_hip_memset_async", At(forest.forest, 32 * ((77 >> 1) + 1 + (77 >> 2) + 1 + 4)), 0x11, 32)
    for buf in (d_leaves, forest.digests):
        gpu._call("vkmr_hip_memset_async", At(buf, 32 * 76), 0x22, 32)
    a, b = tree.audit(), forest.audit()
    assert a.n_bad == b.n_bad == 3 and a.checked == b.checked
    assert list(zip(a.levels, a.nodes)) == list(zip(b.levels, b.nodes)) == [(1, 38), (3, 4), (4, 2)]
    assert int(a.masks[0]) == int(b.masks[0]) == 0b1101 and not a.trees.any() and not b.trees.any()
    tree.free()
    forest.free()
    d_leaves.free()
