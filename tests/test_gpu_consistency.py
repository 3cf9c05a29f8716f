"""Consistency proofs on the GPU (vkmr_hip_forest_consistency_async, vkmr_hip_verify_consistency_async through HipDevice,
MerkleForest.consistency and vk.ConsistencyProof): byte for byte what the CPU twin gives, between guard words, for the shapes of
tests/consistency_cases.py; the verifier against the roots of the trees built from the first c leaves; the read set flip by
flip; a primary that forks; forests that grew, slid and were repacked; the refusals; and the code object."""
import numpy as np
import pytest

import consistency_cases as cc
import forest_update_cases as fu
from abi_support import assert_no_spills, isa_record
from merkle_model import At, random_leaves

pytestmark = pytest.mark.gpu

GUARD = 4                                                    # guard cells (and counts) on either side of every output


def device_gather(gpu, forest, trees, old, stride, max_count=None):
    """One raw gather out of the MerkleForest `forest`: (status, new counts, peaks, rights).  The status word starts as 0xDEADBEEF,
    every output as the canary, with GUARD canary cells in front of and behind it that must still be there afterwards."""
    trees, old = np.ascontiguousarray(trees, dtype=np.uint32), np.ascontiguousarray(old, dtype=np.uint64)
    Q = int(trees.shape[0])
    with gpu.scope() as tmp:
        d_counts = tmp.upload(np.full(Q + 2 * GUARD, cc.COUNT_FILL, np.uint64))
        d_peaks, d_rights = (tmp.upload(np.full((Q * stride + 2 * GUARD, 8), cc.CANARY, np.uint32)) for _ in range(2))
        d_status = tmp.upload(np.full(1, 0xDEADBEEF, np.uint32))
        gpu.forest_consistency_enqueue(forest.digests, forest.forest, forest.total, forest.offsets, forest.ntrees,
                                       forest.max_count if max_count is None else max_count, forest.roots_buf, tmp.upload(trees), tmp.upload(old), Q, stride,
                                       At(d_counts, 8 * GUARD), At(d_peaks, 32 * GUARD), At(d_rights, 32 * GUARD), d_status)
        counts = gpu.download(d_counts, 8 * (Q + 2 * GUARD), dtype=np.uint64)
        peaks, rights = (gpu.download(d, 32 * (Q * stride + 2 * GUARD)).reshape(-1, 8) for d in (d_peaks, d_rights))
        status = int(gpu.download(d_status, 4)[0])
    for a, fill in ((counts, cc.COUNT_FILL), (peaks, cc.CANARY), (rights, cc.CANARY)):
        assert (a[:GUARD] == fill).all() and (a[-GUARD:] == fill).all()
    return status, counts[GUARD:-GUARD], peaks[GUARD:-GUARD].reshape(Q, stride, 8), rights[GUARD:-GUARD].reshape(Q, stride, 8)


def same(got, want, note):
    for what, a, b in zip(("new counts", "peaks", "rights"), got, want):
        assert a.shape == b.shape and (a == b).all(), (note, what, np.nonzero((a != b).reshape(a.shape[0], -1).any(axis=1))[0][:8])


@pytest.fixture(scope="module")
def mixed():
    """The forest of every walk length, its queries and what the CPU twin gives for them, computed once."""
    model = cc.Forest(cc.GPU_COUNTS, seed=421, first=3)
    trees, old = cc.gpu_queries()
    twin = cc.host_gather(model.leaves, model.offsets, trees, old, stride=12)
    assert twin[0] == 0 and 650 < trees.shape[0] < 1000
    return model, trees, old, twin


def test_the_device_is_the_cpu_twin_byte_for_byte(gpu, mixed):
    import vk_merkle_roots_amd as vk
    model, trees, old, twin = mixed
    assert int(model.offsets[0]) > 0
    raw = fu.RawForest(gpu, model.leaves, model.counts, 2048, first=model.first)
    got = device_gather(gpu, raw.handle, trees, old, 12)
    assert got[0] == 0
    same(got[1:], twin[1:], "mixed")
    assert (got[1] == [model.counts[t] for t in trees]).all()
    proof = raw.handle.consistency(old, trees=trees)                                             # the handle: the same call
    assert proof.stride == 12 and proof.same_as(vk.ConsistencyProof(trees, old, *got[1:]))
    old_roots, new_roots = model.query_roots(trees, old)                                         # the trees built from the first c leaves
    now = raw.handle.roots()
    assert (now == model.roots()).all() and (now[trees.astype(np.int64)] == new_roots).all()
    ok = proof.verify(gpu, old_roots, now[trees.astype(np.int64)])
    assert (ok == 1).all(), [(int(trees[q]), int(old[q])) for q in np.nonzero(ok != 1)[0][:8]]
    assert (ok == cc.host_verify(old, proof.new_counts, proof.peaks, proof.rights, old_roots, new_roots)).all()
    assert (proof.frontier().roots(gpu) == old_roots).all()                                      # the root every tree had at its old count
    swapped = proof.verify(gpu, new_roots, old_roots)
    assert (swapped == (old == proof.new_counts)).all()
    raw.free()


def test_one_large_tree(gpu):
    n = 600001
    leaves = random_leaves(np.random.default_rng(422), n)
    forest = gpu.build_forest(leaves, [n])
    old = [1, 1 << 19, (1 << 19) + 1, n - 1, n]
    twin = cc.host_gather(leaves, [0, n], [0] * len(old), old, stride=20)
    got = device_gather(gpu, forest, [0] * len(old), old, 20)
    assert twin[0] == 0 and got[0] == 0
    same(got[1:], twin[1:], "large")
    proof = forest.consistency(old, trees=[0] * len(old))
    assert proof.stride == 20 and (proof.peaks == twin[2]).all() and (proof.rights == twin[3]).all()
    old_roots = proof.frontier().roots(gpu)
    now = np.repeat(forest.roots(), len(old), axis=0)
    assert (old_roots[-1] == now[0]).all() and (proof.verify(gpu, old_roots, now) == 1).all()
    assert (cc.host_verify(old, proof.new_counts, proof.peaks, proof.rights, old_roots, now) == 1).all()
    forest.free()


def test_a_tight_stride_and_a_wide_one(gpu, mixed):
    from vk_merkle_roots_amd._abi import VkmrError
    model, trees, old, twin = mixed
    forest = gpu.build_forest(model.leaves[model.first:], model.counts)
    tight, wide = forest.consistency(old, trees=trees), forest.consistency(old, trees=trees, stride=64)
    assert tight.stride == 12 and (tight.peaks == twin[2]).all() and (tight.rights == twin[3]).all()
    assert (wide.peaks[:, :12] == twin[2]).all() and (wide.rights[:, :12] == twin[3]).all() and not wide.peaks[:, 12:].any() and not wide.rights[:, 12:].any()
    old_roots, new_roots = model.query_roots(trees, old)
    assert (wide.verify(gpu, old_roots, new_roots) == 1).all()
    with pytest.raises(VkmrError):
        forest.consistency(old, trees=trees, stride=11)                                          # a tree of 2 048 leaves has twelve bits
    forest.free()


def test_the_read_set_on_the_device(gpu):
    import vk_merkle_roots_amd as vk
    f = cc.flips(20)
    assert f.stride == 5 and len(f.rows) == 210 * 11
    proof = vk.ConsistencyProof(np.zeros(len(f.rows), np.uint32), f.old_counts, f.new_counts, f.peaks, f.rights)
    ok = proof.verify(gpu, f.old_roots, f.new_roots)
    wrong = np.nonzero(ok != f.want)[0]
    assert wrong.size == 0, [(f.rows[i][0], f.rows[i][1], f.rows[i][5], int(ok[i])) for i in wrong[:8]]
    assert (ok == cc.host_verify(f.old_counts, f.new_counts, f.peaks, f.rights, f.old_roots, f.new_roots)).all()


def test_a_primary_that_forks_is_caught(gpu):
    rng = np.random.default_rng(423)
    leaves, other = random_leaves(rng, 200), random_leaves(rng, 200)
    f = gpu.build_forest(leaves[:100], [5, 65, 30], max_count=256, reserve_trees=1, reserve_leaves=150)
    old_roots, old_counts = f.roots(), f.counts.copy()
    assert old_counts.tolist() == [5, 65, 30, 0]
    assert f.extend(leaves[100:170]) == 100                                                      # the open tree, tree 2: 30 -> 100
    honest, honest_roots = f.consistency(old_counts), f.roots()
    assert honest.new_counts.tolist() == [5, 65, 100, 0] and (honest.verify(gpu, old_roots, honest_roots) == 1).all()
    assert f.shrink(80) == 20                                                                    # below the old count
    assert f.extend(other[:80]) == 100                                                           # and back up with other leaves
    forked_roots = f.roots()
    assert (forked_roots[[0, 1, 3]] == honest_roots[[0, 1, 3]]).all() and (forked_roots[2] != honest_roots[2]).any()
    forked = f.consistency(old_counts)
    assert forked.new_counts.tolist() == [5, 65, 100, 0]
    assert forked.verify(gpu, old_roots, forked_roots).tolist() == [1, 1, 0, 1]                  # the first 30 leaves are not the trusted ones
    assert honest.verify(gpu, old_roots, forked_roots).tolist() == [1, 1, 0, 1]                  # and the honest proof does not reach the forked root
    assert f.shrink(70) == 30 and f.consistency(old_counts).verify(gpu, old_roots, f.roots()).tolist() == [1, 1, 0, 1]   # 20 trusted leaves, 10 others
    assert f.shrink(1) == 29
    with pytest.raises(RuntimeError, match="bit 1"):
        f.consistency(old_counts)                                                                # 29 leaves: tree 2 no longer reaches its old count
    f.free()


def test_after_append_drop_front_and_repacked(gpu):
    rng = np.random.default_rng(424)
    leaves = random_leaves(rng, 400)
    f = gpu.build_forest(leaves[:70], [5, 65], max_count=130, reserve_trees=3, reserve_leaves=330)
    counts0, roots0 = f.counts.copy(), f.roots()
    assert f.append(leaves[70:80], [3, 7]).tolist() == [2, 3]
    counts1, roots1 = f.counts.copy(), f.roots()
    assert f.extend(leaves[80:200]) == 127                                                       # tree 3: 7 -> 127
    now = f.roots()
    for counts, roots in ((counts0, roots0), (counts1, roots1), (f.counts, now)):
        assert (f.consistency(counts).verify(gpu, roots, now) == 1).all()
    assert f.consistency(counts1).verify(gpu, roots0, now).tolist() == [1, 1, 0, 0, 1]           # the roots of another moment
    f.drop_front(1)
    with pytest.raises(RuntimeError, match="bit 1"):
        f.consistency(counts1)                                                                   # tree 0 holds no leaf: it proves nothing above 0
    kept = f.consistency(counts1[1:], trees=[1, 2, 3, 4])
    assert (kept.verify(gpu, roots1[1:], f.roots()[1:]) == 1).all()
    assert f.consistency([0], trees=[0]).verify(gpu, np.zeros((1, 8), np.uint32), f.roots()[:1]).tolist() == [1]
    g = f.repacked(trees=[3, 1], reserve_trees=1, reserve_leaves=10)                             # trees 3 and 1 of f as trees 0 and 1
    assert g.counts.tolist()[:2] == [127, 65]
    copied = g.consistency([7, 65, 0])                                                           # the counts they had in the source
    assert copied.verify(gpu, np.stack([roots1[3], roots1[1], np.zeros(8, np.uint32)]), g.roots()).tolist() == [1, 1, 1]
    source = f.consistency([7, 65], trees=[3, 1], stride=copied.stride)                          # cell for cell what the source proves
    assert (copied.peaks[:2] == source.peaks).all() and (copied.rights[:2] == source.rights).all() and copied.rights[0].any()
    g.free()
    f.free()


@pytest.mark.parametrize("what,status,trees,old,stride,max_count", cc.REFUSALS, ids=[r[0] for r in cc.REFUSALS])
def test_a_refused_gather_writes_nothing(gpu, what, status, trees, old, stride, max_count):
    import vk_merkle_roots_amd as vk
    model = cc.Forest(cc.REFUSAL_COUNTS, seed=414)
    assert cc.host_gather(model.leaves, model.offsets, trees, old, stride=stride)[0] == status
    raw = fu.RawForest(gpu, model.leaves, model.counts, 129, first=model.first)
    got = device_gather(gpu, raw.handle, trees, old, stride, max_count=max_count)
    assert got[0] == status, what
    assert (got[1] == cc.COUNT_FILL).all() and (got[2] == cc.CANARY).all() and (got[3] == cc.CANARY).all()
    for bit in range(3):
        assert (f"bit {bit}:" in vk.consistency_status_text(got[0])) == bool(status >> bit & 1)
    fine = device_gather(gpu, raw.handle, [0, 3, 2], [5, 100, 9], 8)                             # the fault taken out: it goes through
    assert fine[0] == 0 and fine[1].tolist() == [5, 129, 9]
    if status == 2:
        with pytest.raises(RuntimeError, match="bit 1"):
            raw.handle.consistency(old, trees=trees)
    raw.free()


def test_the_code_object(native):
    from vk_merkle_roots_amd import isa_prio_pass
    rec = isa_record(native)                                                                     # the record the build writes beside the library
    assert rec is not None
    mine = {k: len(v) for k, v in rec["hash_blocks"].items() if "consistency_fold_kernel" in k}
    assert list(mine.values()) == [isa_prio_pass.EXPECTED_HASH_BLOCKS["consistency_fold_kernel"]] == [1]
    assert rec["audit"]["block_count_errors"] == [] and {v for k, v in rec["audit"]["blocks"].items() if "consistency" in k} == {1}
    assert not any("consistency_check" in k or "consistency_gather" in k for k in rec["hash_blocks"])
    # returns where the library came built, without the assembly it was made from
    assert_no_spills(native, ("consistency_check_kernel", "consistency_gather_kernel", "consistency_fold_kernel"))
