"""The life of a stored forest on the GPU: every operation of MerkleForest directly after every other (the walks of
tests/forest_life_cases.py), and after EVERY step everything the forest answers compared with one model of it, never one device
result with another: the handle's books, the offsets, the roots, every live cell of level 0 and of the level buffers, the audit
and its count, the masks, the proofs of every live leaf, find, a multiproof, the frontier.  Beside the forest under test (A) walk
its twin (B: the structural steps alone, so that diff and sync_from always have the same shape in front of them), a follower that
holds only the roots and one that holds only a Frontier.  Every fourth step one call that must be refused, and is, without a
trace.  A failure prints (config, seed, step, kind, parameters): the walk can be replayed on the model alone.

The same walks above 4 GiB (test_the_walk_above_4_gib): the forests laid into large, mostly untouched buffers so that the live
cells of one level straddle cell 2^27 -- byte 2^32 -- of that level's buffer (tests/high_cases.py).  Every helper here takes the
model as a high_cases.Shifted view (level None: the forest where it is) and reads cells through high_cases.read_cells, so the
low and the high walks make the same checks against the same model; the high ones also find their canaries intact after every
step, looked at before anything else so that a store that lost its upper bits is named by where it landed."""
import numpy as np
import pytest

import forest_life_cases as fl
import forest_multiproof_cases as fm
import high_cases as hc
from merkle_model import stored_level_base

pytestmark = pytest.mark.gpu

WALKS = [(name, seed) for name in sorted(fl.CONFIGS) for seed in fl.SEEDS[name]]


def u32(values):
    return np.array(values, dtype=np.uint32).reshape(-1)


def u64(values):
    return np.array(values, dtype=np.uint64).reshape(-1)


def batch_of(vk, strings):
    return vk.pack_lines(b"".join(s + b"\n" for s in strings))


def built(gpu, model, level=None):
    """build_forest of a model that has dropped nothing yet; with a level, the same forest built at that placement's shift."""
    assert model.dropped_trees == 0
    if level is not None:
        return hc.build(gpu, hc.Shifted(model, level))
    leaves = np.concatenate(model.trees + [np.zeros((0, 8), dtype=np.uint32)])
    return gpu.build_forest(leaves, model.counts[: model.used_trees], max_count=model.max_count, reserve_trees=model.free_trees,
                            reserve_leaves=model.free_leaves)


def state_equals_model(gpu, forest, m):
    """Checks 2 - 4: the offsets, the roots, every live leaf and every live node at the model's cell (m: a Shifted view).  A
    forest with canaries has them looked at first: a store that lost its upper bits is then named by where it landed."""
    assert hc.canaries_intact(gpu, getattr(forest, "canaries", ()))
    assert (gpu.download(forest.offsets, 8 * (m.ntrees + 1), dtype=np.uint64) == m.offsets()).all(), "offsets"
    assert (forest.roots() == m.roots()).all(), "roots"
    assert (hc.read_cells(gpu, forest.digests, m.live_cells()) == m.image[m.local_live_cells()]).all(), "level 0"
    assert gpu.forest_tree_bytes(forest.total, forest.ntrees, forest.max_count) == 32 * stored_level_base(m.total, m.ntrees, m.levels + 1)
    cells, digests = m.nodes()
    assert (hc.read_cells(gpu, forest.forest, cells) == digests).all(), "the level buffers"


def everything_equals_model(gpu, vk, forest, life, level=None):
    m = hc.Shifted(life.a, level)
    roots = m.roots()
    # 1: the books
    for name, want in m.books().items():
        got = getattr(forest, name)
        assert (got.tolist() if name == "counts" else got) == want, name
    state_equals_model(gpu, forest, m)
    # 5: the audit
    report = forest.audit()
    assert report.clean and report.checked == m.checked(), "audit"
    # 6: the masks
    assert (forest.mutated() == m.masks()).all(), "masks"
    # 7: the proofs of every live leaf and of three entries that name none
    live = m.entries()
    bad = [(0 if m.dropped_trees else m.ntrees + 1, 0), (m.used_trees - 1 if m.used_trees else 0, m.counts[max(m.used_trees - 1, 0)]), (m.ntrees, 0)]
    trees, indices = u32([t for t, _ in live + bad]), u64([i for _, i in live + bad])
    sib, heights = forest.proofs(trees, indices)
    want_sib, want_heights = m.proofs(trees, indices)
    assert (sib == want_sib).all() and (heights == want_heights).all(), "proofs"
    assert not heights[len(live):].any() and not sib[len(live):].any(), "entries that name no leaf"
    if live:
        k = len(live)
        leaves = m.leaves_at(trees[:k], indices[:k])
        assert (gpu.verify_forest_proofs(leaves, trees[:k], indices[:k], sib[:k], heights[:k], roots) == 1).all(), "verify"
        q = int(life.ask.integers(0, k))
        flipped = sib[:k].copy()
        flipped[q, int(life.ask.integers(0, heights[q])), int(life.ask.integers(0, 8))] ^= np.uint32(1 << int(life.ask.integers(0, 32)))
        ok = gpu.verify_forest_proofs(leaves, trees[:k], indices[:k], flipped, heights[:k], roots)
        assert ok[q] == 0 and ok.sum() == k - 1, "a proof with one bit flipped"
    # 8: find
    queries = life.find_queries()
    got, want = forest.find(queries), m.find(queries)
    assert (got[0] == want[0]).all() and (got[1] == want[1]).all(), "find"
    # 9: one multiproof
    trees, indices = life.entry_set()
    if trees.shape[0]:
        proof = forest.multiproof(trees, indices)
        nodes, heights, level_counts = m.multiproof(trees, indices)
        assert (proof.trees == trees).all() and (proof.indices == indices).all() and (proof.heights == heights).all(), "multiproof entries"
        assert proof.nodes.shape == nodes.shape and (proof.nodes == nodes).all() and [int(x) for x in proof.level_counts] == list(level_counts)
        leaves = m.leaves_at(trees, indices)
        assert gpu.verify_forest_multiproof(leaves, proof.trees, proof.indices, proof.heights, proof.nodes, roots), "verify multiproof"
        assert fm.host_verify(leaves, proof.trees, proof.indices, proof.heights, m.levels, proof.nodes, roots), "the host verifier"
    # 10: the frontier
    frontier = forest.frontier()
    counts, peaks = m.frontier()
    assert frontier.stride == m.frontier_stride and (frontier.counts == counts).all() and (frontier.peaks == peaks).all(), "frontier"
    return frontier


def refused_call(gpu, forest, life, number, level=None):
    """One call that must be refused, in turn: an update of a leaf that is none through the handle, the same entry through the
    raw call, a raw extend with a wrong count, a diff against a fresh build of the same counts that has no dropped front (its
    trees lie at other offsets; above the line it is built at the forest's own shift).  Each is a refusal the device or the
    handle documents; none touches anything."""
    m = hc.Shifted(life.a, level)
    tree, index = (0, 0) if m.dropped_trees else (0, m.counts[0])        # a dropped tree, or index == count
    leaf = life.ask.integers(0, 2**32, size=(1, 8), dtype=np.uint32)
    which = (number // 4) % 4
    if which == 3 and m.local.dropped_leaves == 0:
        which = 0                                                        # nothing dropped in front: a fresh build lies where the forest lies
    last = m.used_trees - 1
    if which == 2 and (last < 0 or m.free_leaves == 0 or (m.counts[last] == 0 and m.local.used_leaves == 0)):
        which = 1                                                        # no argument set the host lets through: the raw update instead
    if which == 0:
        with pytest.raises(IndexError):
            forest.update([tree], [index], leaf)
        return
    if which == 3:
        if level is None:
            fresh = gpu.build_forest(m.image[m.live_cells()], m.counts[: m.used_trees], max_count=m.max_count, reserve_trees=m.free_trees,
                                     reserve_leaves=m.total - m.live_leaves)
        else:
            fresh = built(gpu, fl.ModelForest(m.ntrees, m.local.total, m.max_count, m.trees), level)
        assert fresh.counts.tolist() == forest.counts.tolist() and (fresh.total, fresh.ntrees) == (forest.total, forest.ntrees)
        for call in (lambda: forest.diff(fresh), lambda: fresh.diff(forest)):
            with pytest.raises(ValueError, match="dropped in front"):
                call()
        assert hc.canaries_intact(gpu, getattr(fresh, "canaries", ()))
        fresh.free()
        return
    with gpu.scope() as tmp:
        d_status = tmp.upload(np.full(1, 0xDEADBEEF, dtype=np.uint32))
        if which == 1:
            gpu.forest_update_async(forest.digests, forest.forest, forest.total, forest.offsets, forest.ntrees, forest.max_count, tmp.upload(u32([tree])),
                                    tmp.upload(u64([index])), tmp.upload(leaf), 1, forest.roots_buf, d_status)
        else:
            count = m.counts[last]
            wrong = count - 1 if count else 1                            # offsets[tree] + count != used: status bit 2
            gpu.forest_extend_enqueue(forest.digests, forest.forest, forest.total, forest.offsets, forest.ntrees, forest.max_count, last, wrong,
                                      m.used_leaves, tmp.upload(leaf), 1, forest.roots_buf, None, d_status)
        status = int(gpu.download(d_status, 4)[0])
        assert status not in (0, 0xDEADBEEF), (which, status)


def perform(gpu, vk, kind, p, a, b, src, life, level=None):
    """The step on the device: on A, and on B where it is structural.  (A, B, what the calls returned)."""
    got = {}
    if kind == "update":
        trees, indices = u32(p["trees"]), u64(p["indices"])
        if p["form"] == "update":
            a.update(trees, indices, p["values"])
        elif p["form"] == "update_packed":
            a.update_packed(trees, indices, batch_of(vk, p["strings"]))
        elif trees.shape[0]:
            with gpu.scope() as tmp:
                got["counted"] = a.update_entries(tmp.upload(trees), tmp.upload(indices), tmp.upload(p["values"]), trees.shape[0])
        else:
            got["counted"] = a.update_entries(None, None, None, 0)
    elif kind == "replace":
        got["counted"] = a.replace(p["old"], p["new"])
    elif kind == "witness":
        if not p["degenerate"]:
            got["witness"] = a.update_with_witness(u32(p["trees"]), u64(p["indices"]), p["values"])
    elif kind == "append":
        if p["form"] == "append":
            ret = a.append(p["leaves"], p["counts"], mutated=p["mutated"])
            got["numbers"], got["new_masks"] = ret if p["mutated"] else (ret, None)
            b.append(p["leaves"], p["counts"])
        else:
            got["numbers"] = a.append_packed(batch_of(vk, p["strings"]), p["counts"])
            b.append_packed(batch_of(vk, p["strings"]), p["counts"])
    elif kind == "truncate":
        a.truncate(p["keep"])
        b.truncate(p["keep"])
    elif kind == "extend":
        if p["refused"]:
            for f in (a, b):
                with pytest.raises(ValueError, match="no tree in use"):
                    f.extend(p["leaves"])
        elif p["form"] == "extend":
            ret = a.extend(p["leaves"], mutated=p["mutated"])
            got["count"], got["open_mask"] = ret if p["mutated"] else (ret, None)
            b.extend(p["leaves"])
        else:
            got["count"] = a.extend_packed(batch_of(vk, p["strings"]))
            b.extend_packed(batch_of(vk, p["strings"]))
    elif kind == "shrink":
        if p["refused"]:
            for f in (a, b):
                with pytest.raises(ValueError, match="no tree in use"):
                    f.shrink(p["r"])
        else:
            ret = a.shrink(p["r"], mutated=p["mutated"])
            got["count"], got["open_mask"] = ret if p["mutated"] else (ret, None)
            b.shrink(p["r"])
    elif kind == "drop_front":
        a.drop_front(p["k"])
        b.drop_front(p["k"])
    elif kind == "repack":
        old_roots = (life.a.roots(), life.b.roots())
        room = dict(trees=p["trees"], reserve_trees=p["reserve_trees"], reserve_leaves=p["reserve_leaves"], mutated=p["mutated"])
        new = []
        try:
            for f in (a, b):
                new.append(f.repacked(**room) if level is None else hc.repacked_at(gpu, f, level, **room))
            for f, roots in zip((a, b), old_roots):                      # the old handle is left as it is, until it is freed
                assert f.audit().clean and (f.roots() == roots).all(), "the forest repacked() was called on"
                assert hc.canaries_intact(gpu, getattr(f, "canaries", ()))
        except BaseException:
            for f in new:
                f.free()
            raise
        for f in (a, b):
            f.free()
        a, b = new
        got["built_mutated"] = a.built_mutated
    elif kind == "append_from":
        ret = a.append_from(src, u32(p["sel"]), mutated=p["mutated"])
        got["numbers"], got["new_masks"] = ret if p["mutated"] else (ret, None)
        b.append_from(src, u32(p["sel"]))
    elif kind == "sync":
        got["diff"] = a.diff(b)
        got["n"] = b.sync_from(a)
    return a, b, got


def returns_equal_model(gpu, kind, p, a, b, got, want, life, level=None):
    m, mb = hc.Shifted(life.a, level), hc.Shifted(life.b, level)
    masks = want["masks"]
    if "counted" in got:
        assert tuple(got["counted"]) == tuple(want["counted"]), "the counters returned"
    if "numbers" in got:
        assert got["numbers"].tolist() == want["numbers"], "the numbers of the new trees"
        if got.get("new_masks") is not None:
            assert (got["new_masks"] == masks[want["numbers"]]).all(), "the masks of the new trees"
    if "count" in got:
        assert got["count"] == want["count"], "the open tree's count"
        if got.get("open_mask") is not None:
            assert got["open_mask"] == masks[m.open_tree], "the open tree's mask"
    if kind == "repack":
        assert (got["built_mutated"] is None) == (not p["mutated"])
        if p["mutated"]:
            assert (got["built_mutated"] == masks).all(), "the masks repacked() kept"
    if "witness" in got:                                                 # 11: the holder of the roots alone follows
        assert (got["witness"].apply(gpu, want["roots_before"]) == m.roots()).all(), "the roots-only follower"
    if kind == "sync":                                                   # 12
        assert (got["diff"][0] == want["diff"][0]).all() and (got["diff"][1] == want["diff"][1]).all(), "diff"
        assert got["diff"][0].shape == want["diff"][0].shape and got["n"] == want["n"], "sync_from"
        again = a.diff(b)
        assert again[0].shape == (0,) and again[1].shape == (0,), "a second diff"
    if kind in fl.STRUCTURAL or kind == "sync":                          # the twin: its books and its cells are its model's
        assert b.counts.tolist() == mb.counts and b.dropped_leaves == mb.dropped_leaves and b.used_trees == mb.used_trees
        state_equals_model(gpu, b, mb)


def follow(gpu, vk, follower, frontier, kind, p, life, level=None):
    """The Frontier-only follower: advanced by the new leaves on append and extend steps, adopted again -- the forest's frontier
    verified under the model's roots -- after any other step; then the model's, byte for byte."""
    m = hc.Shifted(life.a, level)
    if kind in ("append", "extend") and not p["degenerate"] and p["leaves"].shape[0]:
        new = np.zeros(m.ntrees, dtype=np.int64)
        if kind == "append":
            new[m.used_trees - len(p["counts"]): m.used_trees] = p["counts"]
        else:
            new[m.open_tree] = p["leaves"].shape[0]
        assert (follower.extend(gpu, p["leaves"], new) == m.roots()).all(), "the frontier follower's roots"
    elif kind not in ("append", "extend") or kind == "append" and not p["degenerate"]:
        assert (frontier.verify(gpu, m.roots()) == 1).all(), "the frontier adopted under the model's roots"
        follower = frontier
    assert follower.same_as(vk.Frontier(*m.frontier())), "the frontier follower"
    return follower


def the_walk(gpu, name, seed, level=None):
    """One walk, the forests where build_forest puts them (level None) or at the shift of that placement level: every step
    performed, every check made after it, every fourth step a refused call; at the end every pair of kinds has been performed
    and the canaries of the forests that have them are intact."""
    import vk_merkle_roots_amd as vk
    life = fl.Life(seed, fl.CONFIGS[name])
    forests = []
    try:
        for model, low in ((life.a, False), (life.b, False), (life.src, True)):       # src may stay low
            forests.append(built(gpu, model, None if low else level))
        a, b, src = forests
        try:
            follower = everything_equals_model(gpu, vk, a, life, level)
            state_equals_model(gpu, b, hc.Shifted(life.b, level))
            assert (follower.verify(gpu, life.a.roots()) == 1).all()
        except BaseException:
            print("failed at", (level, name, seed, "the build, before step 0"))
            raise
        for number, kind, p in life.steps():
            try:
                a, b, got = perform(gpu, vk, kind, p, a, b, src, life, level)
                forests[:2] = [a, b]
                want = life.apply(kind, p)
                returns_equal_model(gpu, kind, p, a, b, got, want, life, level)
                frontier = everything_equals_model(gpu, vk, a, life, level)
                follower = follow(gpu, vk, follower, frontier, kind, p, life, level)
                if number % 4 == 3:
                    refused_call(gpu, a, life, number, level)
                    state_equals_model(gpu, a, hc.Shifted(life.a, level))
            except BaseException:
                print("failed at", (level, name, seed, number, kind, p))
                raise
        assert life.pairs == {(x, y) for x in fl.KINDS for y in fl.KINDS}
        for f in (a, b):
            assert hc.canaries_intact(gpu, getattr(f, "canaries", ()))
    finally:
        for f in forests:
            f.free()


@pytest.mark.parametrize("name,seed", WALKS)
def test_every_operation_after_every_other_against_the_model(gpu, name, seed):
    the_walk(gpu, name, seed)


@pytest.mark.parametrize("level,name,seed", hc.HIGH_WALKS)
def test_the_walk_above_4_gib(gpu, level, name, seed):
    """The walk with A, B and both followers, the live cells of `level` on both sides of cell 2^27 of that level's buffer in
    most steps: level 0, the leaves straddle byte 2^32 of the digests buffer; level 1, the level-1 nodes straddle byte 2^32 of
    the level buffers while level 0 straddles byte 2^33; level 3 likewise.  The tight walks reach level 3 in two or three
    steps only, so none is placed there.  Peak device memory: four forests of about 16 GiB in a repack step of level 1."""
    the_walk(gpu, name, seed, level)


def test_a_twin_that_kept_its_front_is_refused_then_diffed_after_it_dropped_it_too(gpu):
    rng = np.random.default_rng(7)
    leaves = rng.integers(0, 2**32, size=(7, 8), dtype=np.uint32)
    a = gpu.build_forest(leaves, [3, 4], max_count=4)
    a.drop_front(1)                                                      # counts [0, 4], offsets [3, 3, 7]
    b = gpu.build_forest(leaves[3:], [0, 4], max_count=4, reserve_leaves=3)      # counts [0, 4], offsets [0, 0, 4]
    assert a.counts.tolist() == b.counts.tolist() == [0, 4] and (a.total, a.ntrees, a.max_count) == (b.total, b.ntrees, b.max_count)
    for call in (lambda: a.diff(b), lambda: b.diff(a), lambda: b.sync_from(a), lambda: a.sync_from(b)):
        with pytest.raises(ValueError, match="dropped in front"):
            call()
    assert (a.roots() == b.roots()).all() and a.audit().clean and b.audit().clean
    twin = gpu.build_forest(leaves, [3, 4], max_count=4)
    changed = leaves[3:].copy()
    changed[2, 5] ^= np.uint32(1)
    twin.update([1, 1, 0], [2, 0, 1], np.concatenate([changed[2:3], leaves[3:4], changed[:1]]))     # tree 1: leaf 2 differs, leaf 0 does not
    twin.drop_front(1)
    trees, indices = a.diff(twin)
    assert trees.tolist() == [1] and indices.tolist() == [2]
    assert twin.sync_from(a) == 1 and a.diff(twin)[0].shape == (0,) and (twin.roots() == a.roots()).all() and twin.audit().clean
    for f in (a, b, twin):
        f.free()
