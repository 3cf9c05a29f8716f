"""Inclusion proofs as of an earlier count on the GPU (vkmr_hip_forest_proofs_at_async through HipDevice,
MerkleForest.proofs_at / roots_at): byte for byte what the CPU twin gives, between guard words, for the shapes of
tests/proofs_at_cases.py; the same batch verified by the existing vkmr_hip_verify_forest_proofs_async under the old roots; the old
roots and the proofs by independent device paths (the consistency proof's frontier; a forest built from the prefix leaves); one
large tree; the shapes of the call; forests that grew, slid, were repacked, shrank and forked; the refusals; the code object."""
import numpy as np
import pytest

import forest_update_cases as fu
import proofs_at_cases as pc
from abi_support import assert_no_spills, isa_record
from merkle_model import At, random_leaves

pytestmark = pytest.mark.gpu

GUARD = 4                                                    # guard cells (and heights) on either side of every output


def device_proofs_at(gpu, forest, epoch_trees, epoch_counts, epochs, indices, stride, max_count=None):
    """One raw call on the MerkleForest `forest`: (status, edges, old roots, siblings, heights).  The status word starts as
    0xDEADBEEF, every output as the canary, with GUARD canary cells in front of and behind it that must still be there afterwards."""
    epoch_trees, epoch_counts = np.ascontiguousarray(epoch_trees, dtype=np.uint32), np.ascontiguousarray(epoch_counts, dtype=np.uint64)
    epochs, indices = np.ascontiguousarray(epochs, dtype=np.uint32), np.ascontiguousarray(indices, dtype=np.uint64)
    E, k = int(epoch_trees.shape[0]), int(epochs.shape[0])
    with gpu.scope() as tmp:
        d_edges, d_roots, d_sib = (tmp.upload(np.full((n + 2 * GUARD, 8), pc.CANARY, np.uint32)) for n in (E * stride, E, k * stride))
        d_heights = tmp.upload(np.full(k + 2 * GUARD, pc.HEIGHT_FILL, np.uint32))
        d_status = tmp.upload(np.full(1, 0xDEADBEEF, np.uint32))
        gpu.forest_proofs_at_enqueue(forest.digests, forest.forest, forest.total, forest.offsets, forest.ntrees,
                                     forest.max_count if max_count is None else max_count, forest.roots_buf, tmp.upload(epoch_trees), tmp.upload(epoch_counts),
                                     E, tmp.upload(epochs) if k else None, tmp.upload(indices) if k else None, k, stride, At(d_edges, 32 * GUARD),
                                     At(d_roots, 32 * GUARD), At(d_sib, 32 * GUARD), At(d_heights, 4 * GUARD), d_status)
        edges, roots, sib = (gpu.download(d, 32 * (n + 2 * GUARD)).reshape(-1, 8) for d, n in ((d_edges, E * stride), (d_roots, E), (d_sib, k * stride)))
        heights = gpu.download(d_heights, 4 * (k + 2 * GUARD))
        status = int(gpu.download(d_status, 4)[0])
    for a, fill in ((edges, pc.CANARY), (roots, pc.CANARY), (sib, pc.CANARY), (heights, pc.HEIGHT_FILL)):
        assert (a[:GUARD] == fill).all() and (a[-GUARD:] == fill).all()
    return status, edges[GUARD:-GUARD].reshape(E, stride, 8), roots[GUARD:-GUARD], sib[GUARD:-GUARD].reshape(k, stride, 8), heights[GUARD:-GUARD]


def same(got, want, note):
    for what, a, b in zip(("edges", "old roots", "siblings", "heights"), got, want):
        assert a.shape == b.shape and (a == b).all(), (note, what, np.nonzero((a != b).reshape(a.shape[0], -1).any(axis=1))[0][:8])


def leaves_of(model, epoch_trees, epoch_counts, epochs, indices):
    """(leaves [k, 8], good [k]): the leaf every good query proves; zero for a query outside the epochs or at or above its count."""
    E = len(epoch_trees)
    leaves, good = np.zeros((len(epochs), 8), np.uint32), np.zeros(len(epochs), bool)
    for q, (e, i) in enumerate(zip(np.asarray(epochs).tolist(), np.asarray(indices).tolist())):
        if e < E and i < int(epoch_counts[e]):
            leaves[q], good[q] = model.leaves[int(model.offsets[int(epoch_trees[e])]) + i], True
    return leaves, good


@pytest.fixture(scope="module")
def mixed():
    """The forest of every walk length, the issue's epochs and queries and what the CPU twin gives for them, computed once."""
    model = pc.Forest(pc.GPU_COUNTS, seed=521, first=3)
    epoch_trees, epoch_counts, epochs, indices = pc.gpu_epochs_and_queries()
    twin = pc.host_proofs_at(model.leaves, model.offsets, epoch_trees, epoch_counts, epochs, indices, stride=12)
    assert twin[0] == 0 and 30000 < epochs.shape[0] < 40000 and 650 < epoch_trees.shape[0] < 1000
    leaves, good = leaves_of(model, epoch_trees, epoch_counts, epochs, indices)
    assert int((~good).sum()) == 128 and (twin[4][~good] == 0).all() and (twin[4][good] > 0).all()
    return model, epoch_trees, epoch_counts, epochs, indices, twin, leaves, good


@pytest.fixture(scope="module")
def mixed_device(gpu, mixed):
    """The same batch out of a stored forest on the device, in ONE call."""
    model, epoch_trees, epoch_counts, epochs, indices = mixed[:5]
    raw = fu.RawForest(gpu, model.leaves, model.counts, 2048, first=model.first)
    got = device_proofs_at(gpu, raw.handle, epoch_trees, epoch_counts, epochs, indices, 12)
    yield raw, got
    raw.free()


def test_the_device_is_the_cpu_twin_byte_for_byte(gpu, mixed, mixed_device):
    model, epoch_trees, epoch_counts, epochs, indices, twin = mixed[:6]
    raw, got = mixed_device
    assert int(model.offsets[0]) > 0 and got[0] == 0
    same(got[1:], twin[1:], "mixed")
    siblings, heights, old_roots = raw.handle.proofs_at(epoch_counts, epochs, indices, trees=epoch_trees)          # the handle: the same call
    assert siblings.shape[1] == 12 and (siblings == got[3]).all() and (heights == got[4]).all() and (old_roots == got[2]).all()
    assert all((old_roots[e] == model.old_root(int(epoch_trees[e]), int(epoch_counts[e]))).all() for e in range(0, len(epoch_trees), 5))


def test_the_same_batch_verifies_on_the_device_under_the_old_roots(gpu, mixed, mixed_device):
    _, epoch_trees, epoch_counts, epochs, indices, _, leaves, good = mixed
    _, (_, _, old_roots, siblings, heights) = mixed_device
    ok = gpu.verify_forest_proofs(leaves, epochs, indices, siblings, heights, old_roots)
    assert ok[good].all(), np.nonzero(good & ~ok)[0][:8]
    assert not ok[~good].any()                                                                    # height 0: nothing to fold
    rng = np.random.default_rng(522)                                                               # one flipped bit in a cell below the height: 0
    flipped = siblings.copy()
    rows = np.nonzero(good)[0]
    flipped[rows, rng.integers(0, heights[rows]), rng.integers(0, 8, size=rows.shape[0])] ^= (np.uint32(1) << rng.integers(0, 32, size=rows.shape[0]).astype(np.uint32))
    assert not gpu.verify_forest_proofs(leaves, epochs, indices, flipped, heights, old_roots).any()


def test_the_old_roots_and_the_proofs_by_independent_device_paths(gpu, mixed, mixed_device):
    model, epoch_trees, epoch_counts, epochs, indices = mixed[:5]
    raw, (_, _, old_roots, siblings, heights) = mixed_device
    assert (old_roots == raw.handle.consistency(epoch_counts, trees=epoch_trees).frontier().roots(gpu)).all()      # the peaks of the old count, walked
    assert (raw.handle.roots_at(epoch_counts, trees=epoch_trees) == old_roots).all()
    # a forest BUILT FROM the prefix leaves, a tree per epoch: the existing gather's proofs, cell for cell (and its bad-index rule)
    prefix = np.concatenate([model.tree(int(t))[: int(c)] for t, c in zip(epoch_trees, epoch_counts)])
    built = gpu.build_forest(prefix, [int(c) for c in epoch_counts], max_count=2048)
    assert (built.roots() == old_roots).all()
    want_siblings, want_heights = built.proofs(epochs, indices)
    width = want_siblings.shape[1]
    assert width <= 12 and (want_heights == heights).all() and (want_siblings == siblings[:, :width]).all() and not siblings[:, width:].any()
    built.free()


def test_one_large_tree(gpu):
    n = 600001
    rng = np.random.default_rng(523)
    leaves = random_leaves(rng, n)
    forest = gpu.build_forest(leaves, [n])
    epoch_counts = [1, 1 << 19, (1 << 19) + 1, n - 2, n]
    epochs = np.repeat(np.arange(5, dtype=np.uint32), 3000)
    indices = np.concatenate([rng.integers(0, c, size=3000) for c in epoch_counts]).astype(np.uint64)
    indices[[3000, 3001, 6000, 6001, 9000, 12000]] = [0, (1 << 19) - 1, 1 << 19, (1 << 19) - 1, n - 3, n - 1]
    order = rng.permutation(epochs.shape[0])
    epochs, indices = epochs[order], indices[order]
    twin = pc.host_proofs_at(leaves, [0, n], [0] * 5, epoch_counts, epochs, indices, stride=20)
    got = device_proofs_at(gpu, forest, [0] * 5, epoch_counts, epochs, indices, 20)
    assert twin[0] == 0 and got[0] == 0
    same(got[1:], twin[1:], "large")
    assert got[4].tolist() == [[1, 19, 20, 20, 20][e] for e in epochs.tolist()] and (got[2][4] == forest.roots()[0]).all()
    assert [[l for l in range(20) if got[1][e, l].any()] for e in range(5)] == [pc.edge_levels(c) for c in epoch_counts]
    assert gpu.verify_forest_proofs(leaves[indices.astype(np.int64)], epochs, indices, got[3], got[4], got[2]).all()
    forest.free()


def test_a_tight_stride_a_wide_one_and_no_query(gpu, mixed):
    from vk_merkle_roots_amd._abi import VkmrError
    model, epoch_trees, epoch_counts, epochs, indices, twin, leaves, good = mixed
    forest = gpu.build_forest(model.leaves[model.first:], model.counts)
    tight = forest.proofs_at(epoch_counts, epochs, indices, trees=epoch_trees)
    wide = forest.proofs_at(epoch_counts, epochs, indices, trees=epoch_trees, stride=63)
    assert tight[0].shape[1] == 12 and (tight[0] == twin[3]).all() and (tight[1] == twin[4]).all() and (tight[2] == twin[2]).all()
    assert wide[0].shape[1] == 63 and (wide[0][:, :12] == twin[3]).all() and not wide[0][:, 12:].any() and (wide[1] == twin[4]).all() and (wide[2] == twin[2]).all()
    assert (gpu.verify_forest_proofs(leaves, epochs, indices, wide[0], wide[1], wide[2]) == good).all()
    raw = device_proofs_at(gpu, forest, epoch_trees, epoch_counts, [], [], 63)                    # k == 0: the edges and the old roots alone
    assert raw[0] == 0 and (raw[1][:, :12] == twin[1]).all() and not raw[1][:, 12:].any() and (raw[2] == twin[2]).all()
    assert (forest.roots_at(epoch_counts, trees=epoch_trees) == twin[2]).all()
    assert (forest.roots_at(model.counts) == forest.roots()).all()                                 # one epoch per tree, as of now
    with pytest.raises(VkmrError):
        forest.proofs_at(epoch_counts, epochs, indices, trees=epoch_trees, stride=11)              # a tree of 2 048 leaves has twelve bits
    forest.free()


def every_leaf_verifies(gpu, forest, leaves_of_tree, counts, roots):
    """Every leaf of every tree as of `counts` verifies under `roots` (the roots taken then), one epoch per tree."""
    epochs, indices = pc.every_leaf(counts)
    siblings, heights, old_roots = forest.proofs_at(counts, epochs, indices)
    assert (old_roots == roots).all(), np.nonzero((old_roots != roots).any(axis=1))[0]
    leaves = np.stack([leaves_of_tree[int(e)][int(i)] for e, i in zip(epochs, indices)])
    assert gpu.verify_forest_proofs(leaves, epochs, indices, siblings, heights, roots).all()
    return siblings, heights


def test_after_the_forest_has_changed(gpu):
    rng = np.random.default_rng(524)
    leaves = random_leaves(rng, 400)
    f = gpu.build_forest(leaves[:70], [5, 65], max_count=130, reserve_trees=3, reserve_leaves=330)
    trees = {0: leaves[:5], 1: leaves[5:70], 2: leaves[70:73], 3: leaves[73:200], 4: np.zeros((0, 8), np.uint32)}
    counts0, roots0 = f.counts.copy(), f.roots()
    assert f.append(leaves[70:80], [3, 7]).tolist() == [2, 3]
    counts1, roots1 = f.counts.copy(), f.roots()
    assert f.extend(leaves[80:200]) == 127                                                       # tree 3: 7 -> 127
    for counts, roots in ((counts0, roots0), (counts1, roots1), (f.counts.copy(), f.roots())):
        every_leaf_verifies(gpu, f, trees, counts, roots)
    f.drop_front(1)
    with pytest.raises(RuntimeError, match="bit 1"):
        f.proofs_at(counts1, [1], [0])                                                             # tree 0 holds no leaf: nothing above 0 as of it
    kept = counts1.copy()
    kept[0] = 0
    every_leaf_verifies(gpu, f, trees, kept, np.concatenate([np.zeros((1, 8), np.uint32), roots1[1:]]))
    g = f.repacked(trees=[3, 1], reserve_trees=1, reserve_leaves=10)                             # trees 3 and 1 of f as trees 0 and 1
    assert g.counts.tolist()[:2] == [127, 65]
    copied = every_leaf_verifies(gpu, g, {0: trees[3], 1: trees[1], 2: trees[4]}, [7, 65, 0], np.stack([roots1[3], roots1[1], np.zeros(8, np.uint32)]))
    source = f.proofs_at([7, 65], *pc.every_leaf([7, 65]), trees=[3, 1], stride=copied[0].shape[1])
    assert (copied[0] == source[0]).all() and (copied[1] == source[1]).all()                       # cell for cell what the source proves
    g.free()
    f.free()


def test_a_tree_that_shrank_is_refused_and_a_fork_is_caught_by_the_root(gpu):
    rng = np.random.default_rng(525)
    leaves, other = random_leaves(rng, 200), random_leaves(rng, 200)
    f = gpu.build_forest(leaves[:100], [5, 65, 30], max_count=256, reserve_trees=1, reserve_leaves=150)
    monitor_roots, monitor_counts = f.roots(), f.counts.copy()                                   # what a monitor trusts: [5, 65, 30, 0]
    assert f.extend(leaves[100:170]) == 100                                                      # the open tree, tree 2: 30 -> 100
    epochs, indices = pc.every_leaf(monitor_counts)
    mine = np.concatenate([leaves[:5], leaves[5:70], leaves[70:100]])
    siblings, heights, old_roots = f.proofs_at(monitor_counts, epochs, indices)
    assert (old_roots == monitor_roots).all() and gpu.verify_forest_proofs(mine, epochs, indices, siblings, heights, monitor_roots).all()
    assert f.shrink(71) == 29                                                                    # below the old count
    with pytest.raises(RuntimeError, match="bit 1"):
        f.proofs_at(monitor_counts, epochs, indices)
    with pytest.raises(RuntimeError, match="bit 1"):
        f.roots_at(monitor_counts)
    assert f.shrink(9) == 20 and f.extend(other[:80]) == 100                                     # and back up with other leaves: 20 trusted, 80 others
    siblings, heights, old_roots = f.proofs_at(monitor_counts, epochs, indices)
    forked = np.concatenate([leaves[:5], leaves[5:70], leaves[70:90], other[:10]])               # the first 30 leaves of tree 2 as they are now
    assert gpu.verify_forest_proofs(forked, epochs, indices, siblings, heights, old_roots).all()  # the proofs are those of the returned root,
    assert (old_roots[[0, 1, 3]] == monitor_roots[[0, 1, 3]]).all() and (old_roots[2] != monitor_roots[2]).any()   # which is not the monitor's
    assert (gpu.verify_forest_proofs(forked, epochs, indices, siblings, heights, monitor_roots) == (epochs != 2)).all()   # so nothing of tree 2 verifies under it
    f.free()


@pytest.mark.parametrize("what,status,trees,old,stride,max_count", pc.REFUSALS, ids=[r[0] for r in pc.REFUSALS])
def test_a_refused_call_writes_nothing(gpu, what, status, trees, old, stride, max_count):
    import vk_merkle_roots_amd as vk
    model = pc.Forest(pc.REFUSAL_COUNTS, seed=414)
    queries = ([0, 0, len(trees)], [0, 1, 0])
    assert pc.host_proofs_at(model.leaves, model.offsets, trees, old, *queries, stride=stride)[0] == status
    raw = fu.RawForest(gpu, model.leaves, model.counts, 129, first=model.first)
    got = device_proofs_at(gpu, raw.handle, trees, old, *queries, stride, max_count=max_count)
    assert got[0] == status, what
    assert all((a == pc.CANARY).all() for a in got[1:4]) and (got[4] == pc.HEIGHT_FILL).all()
    for bit in range(3):
        assert (f"bit {bit}:" in vk.consistency_status_text(got[0])) == bool(status >> bit & 1)
    fine = device_proofs_at(gpu, raw.handle, [0, 3, 2], [5, 100, 9], [0, 1, 3], [4, 99, 0], 8)     # the fault taken out: it goes through
    assert fine[0] == 0 and fine[4].tolist() == [3, 7, 0]
    if status == 2:
        with pytest.raises(RuntimeError, match="bit 1"):
            raw.handle.proofs_at(old, [0], [0], trees=trees)
    raw.free()


def test_the_code_object(native):
    from vk_merkle_roots_amd import isa_prio_pass
    rec = isa_record(native)                                                                     # the record the build writes beside the library
    assert rec is not None
    mine = {k: len(v) for k, v in rec["hash_blocks"].items() if "proofs_at_edge_kernel" in k}
    assert list(mine.values()) == [isa_prio_pass.EXPECTED_HASH_BLOCKS["proofs_at_edge_kernel"]] == [1]
    assert rec["audit"]["block_count_errors"] == [] and {v for k, v in rec["audit"]["blocks"].items() if "proofs_at" in k} == {1}
    assert not any("proofs_at_check" in k or "proofs_at_gather" in k for k in rec["hash_blocks"])
    # returns where the library came built, without the assembly it was made from
    assert_no_spills(native, ("proofs_at_check_kernel", "proofs_at_edge_kernel", "proofs_at_gather_kernel"))
