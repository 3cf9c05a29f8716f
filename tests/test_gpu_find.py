"""The lookup by digest on the GPU (vkmr_hip_forest_find_async and vkmr_hip_tree_find_async, raw and through MerkleForest /
MerkleTree): every answer against the dict of first occurrences in tests/find_cases.py, the words around the outputs, the
edge arguments, the scratch reused, and the chain hash -> position -> proof -> verify with nothing downloaded in between."""
import numpy as np
import pytest

import find_cases as fd
import forest_cases as fc
import merkle_model
from merkle_model import At

pytestmark = pytest.mark.gpu

PATTERN = 0xC3C3C3C3
PATTERN64 = PATTERN * 0x100000001
GUARD = 512                                   # words in front of and behind each output: more than one workgroup's lanes


class Outputs:
    """trees [k] uint32 and indices [k] uint64 on the device, each between GUARD words of PATTERN."""

    def __init__(self, gpu, k):
        self.gpu, self.k = gpu, k
        self.d_trees = gpu.upload(np.full(2 * GUARD + k, PATTERN, dtype=np.uint32))
        self.d_idx = gpu.upload(np.full(2 * GUARD + k, PATTERN64, dtype=np.uint64))
        self.trees_at, self.idx_at = At(self.d_trees, 4 * GUARD), At(self.d_idx, 8 * GUARD)

    def read(self, stream=None):
        """(trees, indices), the guards checked."""
        t = self.gpu.download(self.d_trees, 4 * (2 * GUARD + self.k), stream=stream)
        i = self.gpu.download(self.d_idx, 8 * (2 * GUARD + self.k), dtype=np.uint64, stream=stream)
        assert (t[:GUARD] == PATTERN).all() and (t[GUARD + self.k:] == PATTERN).all()
        assert (i[:GUARD] == PATTERN64).all() and (i[GUARD + self.k:] == PATTERN64).all()
        return t[GUARD: GUARD + self.k], i[GUARD: GUARD + self.k]

    def free(self):
        self.d_trees.free()
        self.d_idx.free()


def forest_find(gpu, case, d_cells=None):
    """(trees, indices) of one raw vkmr_hip_forest_find_async over the case."""
    mine = d_cells is None and case.total > 0
    d_cells = gpu.upload(case.cells) if mine else d_cells
    d_off, d_q, d_scr = gpu.upload(case.offsets), gpu.upload(case.queries), gpu.alloc(gpu.find_scratch_bytes(case.k))
    out = Outputs(gpu, case.k)
    gpu.forest_find_async(d_cells, case.total, d_off, case.ntrees, d_q, case.k, d_scr, out.trees_at, out.idx_at)
    got = out.read()
    for b in (d_off, d_q, d_scr, out) + ((d_cells,) if mine else ()):
        b.free()
    return got


def tree_find(gpu, cells, queries):
    """indices of one raw vkmr_hip_tree_find_async over all of `cells` as one tree."""
    count, k = int(cells.shape[0]), int(queries.shape[0])
    d_cells = gpu.upload(cells) if count else None
    d_q, d_scr = gpu.upload(queries), gpu.alloc(gpu.find_scratch_bytes(k))
    out = Outputs(gpu, k)
    gpu.tree_find_async(d_cells, count, d_q, k, d_scr, out.idx_at)
    trees, got = out.read()
    assert (trees == PATTERN).all()           # the tree call has no such output
    for b in (d_q, d_scr, out) + ((d_cells,) if d_cells else ()):
        b.free()
    return got


def assert_equals_the_model(case, trees, indices, what):
    assert (indices == case.indices).all(), (what, np.nonzero(indices != case.indices)[0][:10])
    assert (trees == case.trees).all(), (what, np.nonzero(trees != case.trees)[0][:10])


@pytest.mark.parametrize("variant", fd.VARIANTS)
@pytest.mark.parametrize("name", sorted(fd.FORESTS))
def test_the_query_sets_give_the_models_answers(gpu, name, variant):
    case = fd.forest_case(name, variant)
    trees, indices = forest_find(gpu, case)
    assert_equals_the_model(case, trees, indices, (name, variant))
    flat = tree_find(gpu, case.cells, case.queries)                     # the same cells as one tree: the window's walls are leaves now
    assert (flat == fd.model(case.cells, [0, case.total], case.queries)[1]).all()


@pytest.mark.parametrize("name", sorted(n for n, (first, slack, _) in fd.FORESTS.items() if first == 0 and slack == 0))
def test_the_python_layer_gives_the_models_answers(gpu, name):
    case = fd.forest_case(name, "zero_is_a_leaf")
    forest = gpu.build_forest(case.cells, case.counts)
    trees, indices = forest.find(case.queries)
    assert trees.dtype == np.uint32 and indices.dtype == np.uint64
    assert_equals_the_model(case, trees, indices, name)
    sib, heights, trees2, indices2 = forest.proofs_of(case.queries)
    assert_equals_the_model(case, trees2, indices2, name)
    want_sib, want_h = forest.proofs(case.trees, case.indices)          # NO_TREE is a tree >= ntrees: height 0, zero cells
    assert (sib == want_sib).all() and (heights == want_h).all()
    assert (heights[~case.found()] == 0).all() and (heights[case.found()] > 0).all()
    roots = forest.roots()
    for q in np.nonzero(case.found())[0][:6]:
        assert (merkle_model.fold(case.queries[q], indices[q], sib[q], heights[q]) == roots[trees[q]]).all()
    empty_t, empty_i = forest.find(np.zeros((0, 8), dtype=np.uint32))
    assert empty_t.shape == (0,) and empty_i.shape == (0,)
    forest.free()
    if case.total <= 5000:                                              # one tree over the same cells
        tree = gpu.build_tree(gpu.upload(case.cells), case.total)
        want = fd.model(case.cells, [0, case.total], case.queries)[1]
        got = tree.find(case.queries)
        assert got.dtype == np.uint64 and (got == want).all()
        sib, got2 = tree.proofs_of(case.queries)
        assert (got2 == want).all() and (sib == tree.proofs(want)).all()
        assert not sib[want == fd.NOT_FOUND].any()
        root = tree.root()
        for q in np.nonzero(want != fd.NOT_FOUND)[0][:6]:
            assert (merkle_model.fold(case.queries[q], want[q], sib[q], tree.height) == root).all()
        tree.digests.free()
        tree.free()


@pytest.mark.parametrize("k", fd.CHAIN_K)
def test_one_chain_of_k_queries(gpu, k):
    """Every query starts at one slot: the insert and every leaf that shares the word walk the whole chain, round the table's
    end with `wrap`; k = 32 fills half of 64 slots, k = 33 is the first in 128."""
    for wrap in (False, True):
        for parity in (0, 1):
            case = fd.chain_case(k, wrap, parity)
            trees, indices = forest_find(gpu, case)
            assert_equals_the_model(case, trees, indices, (k, wrap, parity))


def test_all_leaves_equal(gpu):
    """Every lane of the scan hits one best position; the first leaf of the first tree that has one is the answer."""
    case = fd.all_equal_case()
    trees, indices = forest_find(gpu, case)
    assert_equals_the_model(case, trees, indices, "all equal")
    assert list(trees) == [2, fd.NO_TREE, 2] and list(indices) == [0, fd.NOT_FOUND, 0]


@pytest.mark.parametrize("total", fd.TOTALS)
def test_every_size(gpu, total):
    for k in fd.KS:
        case = fd.size_case(total, k)
        trees, indices = forest_find(gpu, case)
        assert_equals_the_model(case, trees, indices, (total, k))
        assert (tree_find(gpu, case.cells, case.queries) == fd.model(case.cells, [0, total], case.queries)[1]).all()


def test_the_second_trip_of_the_scans_loop(gpu):
    """The scan's grid is capped by the device's compute units: one leaf more than the capped grid covers in one trip, so that
    workgroup 0 takes a second one, and queries for the last leaves of the first trip and the lone leaf of the second."""
    import ctypes as C
    cus = C.c_int(0)
    assert gpu.lib.vkmr_hip_device_geometry(gpu.index, C.byref(cus), None) == 0 and cus.value > 0
    total = fd.second_trip_total(cus.value)
    rng = np.random.default_rng(fd.seed_of("second trip"))
    cells = merkle_model.random_leaves(rng, total)
    cells[total - 1] = cells[total - 2]                                 # the second trip's leaf is there twice: the first trip's wins
    picks = np.concatenate([[0, total - 1, total - 2, total - 3, total - 600], rng.integers(0, total, size=2000)])
    queries = np.concatenate([cells[picks], merkle_model.random_leaves(rng, 2092)])
    last = merkle_model.random_leaves(rng, 1)[0]                        # and a digest that only the second trip's tile holds
    case = fd.Case(cells, fc.offsets_of([total // 2, 0, total - total // 2]), np.concatenate([queries, [last]]))
    assert case.k == 4098 and not case.found()[-1]
    d_cells = gpu.upload(case.cells)
    trees, indices = forest_find(gpu, case, d_cells)
    assert_equals_the_model(case, trees, indices, "second trip")
    assert int(indices[1]) == total - 2 - total // 2 and int(trees[1]) == 2
    case.cells[total - 1] = last                                        # now the lone leaf of the second trip is the only answer
    d_cells.free()
    moved = fd.Case(case.cells, case.offsets, case.queries)
    assert moved.found()[-1] and int(moved.indices[-1]) == total - 1 - total // 2
    trees, indices = forest_find(gpu, moved)
    assert_equals_the_model(moved, trees, indices, "second trip, last leaf")


def test_no_query_writes_nothing_and_no_leaf_finds_nothing(gpu):
    case = fd.size_case(65, 63)
    d_cells, d_off, d_q = gpu.upload(case.cells), gpu.upload(case.offsets), gpu.upload(case.queries)
    d_scr = gpu.upload(np.full(gpu.find_scratch_bytes(case.k) // 4, PATTERN, dtype=np.uint32))
    out = Outputs(gpu, case.k)
    gpu.forest_find_async(d_cells, case.total, d_off, case.ntrees, d_q, 0, d_scr, out.trees_at, out.idx_at)          # k == 0
    gpu.tree_find_async(d_cells, case.total, d_q, 0, d_scr, out.idx_at)
    trees, indices = out.read()
    assert (trees == PATTERN).all() and (indices == PATTERN64).all()
    assert (gpu.download(d_scr, gpu.find_scratch_bytes(case.k)) == PATTERN).all()
    # no leaf: a forest of empty trees, no cell at all, no tree at all (then without offsets), a tree of no leaf
    d_empty = gpu.upload(np.array([3, 3, 3], dtype=np.uint64))
    for d_c, total, d_o, ntrees in ((d_cells, case.total, d_empty, 2), (None, 0, gpu.upload(np.zeros(3, dtype=np.uint64)), 2),
                                    (None, case.total, None, 0), (None, 0, None, 0)):
        gpu.forest_find_async(d_c, total, d_o, ntrees, d_q, case.k, d_scr, out.trees_at, out.idx_at)
        trees, indices = out.read()
        assert (trees == fd.NO_TREE).all() and (indices == fd.NOT_FOUND).all(), (total, ntrees)
    gpu.forest_find_async(d_cells, case.total, d_off, case.ntrees, d_q, case.k, d_scr, out.trees_at, out.idx_at)     # the buffers were good
    assert_equals_the_model(case, *out.read(), "after the empty ones")
    gpu.tree_find_async(None, 0, d_q, case.k, d_scr, out.idx_at)
    assert (out.read()[1] == fd.NOT_FOUND).all()
    for b in (d_cells, d_off, d_q, d_scr, d_empty, out):
        b.free()


def test_two_calls_on_one_scratch_back_to_back(gpu):
    """The second call's answers, whatever the first left in the scratch: the reset is part of the launch sequence.  The first
    call's table is the larger one, and holds every query of the second at other slots' worth of stale entries."""
    a, b = fd.size_case(5000, 4097), fd.size_case(5000, 65)
    d_cells_a, d_cells_b, d_off = gpu.upload(a.cells), gpu.upload(b.cells), gpu.upload(a.offsets)
    d_qa, d_qb = gpu.upload(a.queries), gpu.upload(b.queries)
    d_scr = gpu.alloc(gpu.find_scratch_bytes(a.k))
    out_a, out_b = Outputs(gpu, a.k), Outputs(gpu, b.k)
    s = gpu.new_stream()
    gpu.forest_find_async(d_cells_a, a.total, d_off, a.ntrees, d_qa, a.k, d_scr, out_a.trees_at, out_a.idx_at, stream=s)
    gpu.forest_find_async(d_cells_b, b.total, d_off, b.ntrees, d_qb, b.k, d_scr, out_b.trees_at, out_b.idx_at, stream=s)
    gpu.forest_find_async(d_cells_a, a.total, d_off, a.ntrees, d_qb, b.k, d_scr, out_a.trees_at, out_a.idx_at, stream=s)      # b's queries, a's leaves
    assert_equals_the_model(b, *out_b.read(stream=s), "second call")
    trees, indices = out_a.read(stream=s)
    cross = fd.Case(a.cells, a.offsets, b.queries)
    assert (trees[: b.k] == cross.trees).all() and (indices[: b.k] == cross.indices).all()
    assert (trees[b.k:] == a.trees[b.k:]).all() and (indices[b.k:] == a.indices[b.k:]).all()       # cells past k keep the first call's answers
    gpu.lib.vkmr_hip_stream_destroy(gpu.index, s)
    for x in (d_cells_a, d_cells_b, d_off, d_qa, d_qb, d_scr, out_a, out_b):
        x.free()


def test_hash_to_position_to_proof_to_verdict_in_a_forest_with_nothing_downloaded_in_between(gpu):
    case = fd.forest_case("empties_everywhere", "ones_is_a_leaf")
    forest = gpu.build_forest(case.cells, case.counts)
    k, H = case.k, forest.levels
    d_q, d_scr = gpu.upload(case.queries), gpu.alloc(gpu.find_scratch_bytes(k))
    d_trees, d_idx, d_sib, d_h, d_ok = gpu.alloc(4 * k), gpu.alloc(8 * k), gpu.alloc(32 * k * H), gpu.alloc(4 * k), gpu.alloc(4 * k)
    s = gpu.new_stream()
    forest.find_async(d_q, k, d_scr, d_trees, d_idx, stream=s)
    forest.proofs_async(d_trees, d_idx, k, d_sib, d_h, stream=s)
    gpu.verify_forest_proofs_async(d_q, d_trees, d_idx, d_sib, d_h, k, H, forest.roots_buf, forest.ntrees, d_ok, stream=s)    # the query IS the leaf
    ok = gpu.download(d_ok, 4 * k, stream=s)
    heights = gpu.download(d_h, 4 * k, stream=s)
    assert case.found().any() and not case.found().all()
    assert (ok == case.found().astype(np.uint32)).all()
    assert (heights[~case.found()] == 0).all() and (heights[case.found()] > 0).all()
    assert not gpu.download(d_sib, 32 * k * H, stream=s).reshape(k, H, 8)[~case.found()].any()
    assert_equals_the_model(case, gpu.download(d_trees, 4 * k, stream=s), gpu.download(d_idx, 8 * k, dtype=np.uint64, stream=s), "chain")
    gpu.lib.vkmr_hip_stream_destroy(gpu.index, s)
    for b in (d_q, d_scr, d_trees, d_idx, d_sib, d_h, d_ok):
        b.free()
    forest.free()


def test_hash_to_position_to_proof_to_verdict_in_one_tree_with_nothing_downloaded_in_between(gpu):
    case = fd.forest_case("window", "zero_is_a_leaf")                    # its cells as one tree of 302 leaves
    want = fd.model(case.cells, [0, case.total], case.queries)[1]
    found = want != fd.NOT_FOUND
    d_cells = gpu.upload(case.cells)
    tree = gpu.build_tree(d_cells, case.total)
    k, h = case.k, tree.height
    d_q, d_scr = gpu.upload(case.queries), gpu.alloc(gpu.find_scratch_bytes(k))
    d_idx, d_sib, d_ok = gpu.alloc(8 * k), gpu.alloc(32 * k * h), gpu.alloc(4 * k)
    s = gpu.new_stream()
    tree.find_async(d_q, k, d_scr, d_idx, stream=s)
    tree.proofs_async(d_idx, k, d_sib, stream=s)
    gpu.verify_proofs_async(d_q, d_idx, d_sib, k, h, At(tree.tree, gpu.tree_bytes(tree.count, h) - 32), 1, d_ok, stream=s)
    ok = gpu.download(d_ok, 4 * k, stream=s)
    assert found.any() and not found.all()
    assert (ok == found.astype(np.uint32)).all()
    assert (gpu.download(d_idx, 8 * k, dtype=np.uint64, stream=s) == want).all()
    gpu.lib.vkmr_hip_stream_destroy(gpu.index, s)
    for b in (d_q, d_scr, d_idx, d_sib, d_ok, d_cells):
        b.free()
    tree.free()


def test_a_find_behind_an_update_on_one_stream_sees_the_new_leaf(gpu):
    counts = [77, 0, 130, 64]
    host = fc.random_leaves(sum(counts), seed=2718)
    forest = gpu.build_forest(host, counts)
    new = fc.random_leaves(1, seed=2719)
    old = host[77 + 100].copy()
    queries = np.stack([old, new[0], host[0]])
    trees, indices = forest.find(queries)
    assert list(trees) == [2, fd.NO_TREE, 0] and list(indices) == [100, fd.NOT_FOUND, 0]
    s = gpu.new_stream()
    d_t, d_i, d_new, d_status = gpu.upload(np.array([2], dtype=np.uint32)), gpu.upload(np.array([100], dtype=np.uint64)), gpu.upload(new), gpu.alloc(4)
    d_q, d_scr = gpu.upload(queries), gpu.alloc(gpu.find_scratch_bytes(3))
    out = Outputs(gpu, 3)
    forest.update_async(d_t, d_i, d_new, 1, d_status, stream=s)
    forest.find_async(d_q, 3, d_scr, out.trees_at, out.idx_at, stream=s)
    trees, indices = out.read(stream=s)
    assert int(gpu.download(d_status, 4, stream=s)[0]) == 0
    assert list(trees) == [fd.NO_TREE, 2, 0] and list(indices) == [fd.NOT_FOUND, 100, 0]
    forest.update([2], [100], old.reshape(1, 8))                        # MerkleForest.update, then the method
    trees, indices = forest.find(queries)
    assert list(trees) == [2, fd.NO_TREE, 0] and list(indices) == [100, fd.NOT_FOUND, 0]
    gpu.lib.vkmr_hip_stream_destroy(gpu.index, s)
    for b in (d_t, d_i, d_new, d_status, d_q, d_scr, out):
        b.free()
    forest.free()
