"""Applying a multiproof on the GPU (vkmr_hip_apply_forest_multiproof_async, vkmr_hip_apply_multiproof_async through HipDevice,
MerkleForest / MerkleTree.update_with_witness and UpdateWitness): the new roots against the host CPU counterpart and against a
rebuild of the updated leaves on every case table and entry set (tests/apply_cases.py), the ballot-word and prefix-block edges
of the ranking, the verdict one corruption at a time with exact buffers between canaries, roots advanced in place, and a
primary and a follower end to end."""
import numpy as np
import pytest

import apply_cases as ac
import forest_cases as fc
import forest_multiproof_cases as fm
from merkle_model import At, random_leaves, tree_height

pytestmark = pytest.mark.gpu

PATTERN = 0xC3C3C3C3
GUARD = 4096


def device_apply_forest(gpu, old, new, trees, indices, counts, stride, nodes, roots, in_place=False):
    """vkmr_hip_apply_forest_multiproof_async at `stride` with a scratch of exactly the size function, one ok word and ntrees
    new-root cells, each between two canary pages that are checked here: (ok, new roots [ntrees, 8] as the call left them).
    ok and the new roots start as PATTERN; in_place passes the roots buffer as new_roots (its pages are checked as well)."""
    k, m, ntrees = int(np.asarray(trees).shape[0]), int(np.asarray(nodes).reshape(-1, 8).shape[0]), int(roots.shape[0])
    sizes = [gpu.apply_multiproof_scratch_bytes(k, stride), 4, 32 * ntrees]
    assert sizes[0] % 16 == 0 and sizes[0] > 0
    bufs = [gpu.upload(np.full((GUARD + n + GUARD) // 4, PATTERN, dtype=np.uint32)) for n in sizes]
    if in_place:
        framed = np.full((GUARD + 32 * ntrees + GUARD) // 4, PATTERN, dtype=np.uint32)
        framed[GUARD // 4: GUARD // 4 + 8 * ntrees] = np.ascontiguousarray(roots, dtype=np.uint32).reshape(-1)
        bufs[2].free()
        bufs[2] = gpu.upload(framed)
    d_scr, d_ok, d_out = (At(b, GUARD) for b in bufs)
    with gpu.scope() as tmp:
        d_old, d_new, d_nodes, d_roots = (tmp.upload(np.ascontiguousarray(a, dtype=np.uint32)) for a in (old, new, nodes, roots))
        d_trees = tmp.upload(np.ascontiguousarray(trees, dtype=np.uint32))
        d_idx, d_counts = tmp.upload(np.ascontiguousarray(indices, dtype=np.uint64)), tmp.upload(np.ascontiguousarray(counts, dtype=np.uint64))
        gpu.apply_forest_multiproof_enqueue(d_old, d_new, d_trees, d_idx, d_counts, k, stride, d_nodes if m else None, m, d_out if in_place else d_roots,
                                            ntrees, d_scr, d_ok, d_out)
        out = []
        for b, n in zip(bufs, sizes):
            after = gpu.download(b, GUARD + n + GUARD)
            assert (after[: GUARD // 4] == PATTERN).all() and (after[-(GUARD // 4):] == PATTERN).all(), n
            out.append(after[GUARD // 4: GUARD // 4 + n // 4])
    for b in bufs:
        b.free()
    ok = int(out[1][0])
    assert ok in (0, 1)
    return ok, out[2].reshape(-1, 8)


def device_apply_tree(gpu, old, new, indices, count, height, nodes, root):
    """vkmr_hip_apply_multiproof_async the same way: (ok, new root [8] as the call left it)."""
    k, m = int(np.asarray(indices).shape[0]), int(np.asarray(nodes).reshape(-1, 8).shape[0])
    sizes = [gpu.apply_multiproof_scratch_bytes(k, height), 4, 32]
    bufs = [gpu.upload(np.full((GUARD + n + GUARD) // 4, PATTERN, dtype=np.uint32)) for n in sizes]
    d_scr, d_ok, d_out = (At(b, GUARD) for b in bufs)
    with gpu.scope() as tmp:
        d_old, d_new, d_nodes, d_root = (tmp.upload(np.ascontiguousarray(a, dtype=np.uint32)) for a in (old, new, nodes, root))
        d_idx = tmp.upload(np.ascontiguousarray(indices, dtype=np.uint64))
        gpu.apply_multiproof_enqueue(d_old, d_new, d_idx, k, int(count), int(height), d_nodes if m else None, m, d_root, d_scr, d_ok, d_out)
        out = []
        for b, n in zip(bufs, sizes):
            after = gpu.download(b, GUARD + n + GUARD)
            assert (after[: GUARD // 4] == PATTERN).all() and (after[-(GUARD // 4):] == PATTERN).all(), n
            out.append(after[GUARD // 4: GUARD // 4 + n // 4])
    for b in bufs:
        b.free()
    ok = int(out[1][0])
    assert ok in (0, 1)
    return ok, out[2]


@pytest.mark.parametrize("pattern", ac.LEAF_PATTERNS)
@pytest.mark.parametrize("name", ac.NON_EMPTY)
def test_new_roots_equal_the_host_cpu_s_and_a_rebuild_on_every_case_table(gpu, name, pattern):
    counts = fc.CASES[name]
    leaves = ac.case_leaves(name, pattern)
    off = fc.offsets_of(counts)
    forest = gpu.build_forest(leaves, counts)
    H, roots = forest.levels, forest.roots()
    rng = np.random.default_rng(len(name) * 131 + len(pattern))
    taller = None
    for set_name, (trees, indices) in ac.entry_sets(counts, rng).items():
        proof = forest.multiproof(trees, indices)
        old, new, cs = fm.leaves_at(leaves, off, trees, indices), random_leaves(rng, len(trees)), ac.counts_of(counts, trees)
        ok, got = device_apply_forest(gpu, old, new, trees, indices, cs, H, proof.nodes, roots)
        assert ok == 1, set_name
        r, cpu = ac.host_apply_forest(old, new, trees, indices, cs, H, proof.nodes, roots)
        assert r == 1 and (got == cpu).all(), (set_name, np.flatnonzero((got != cpu).any(axis=1))[:10])     # the canaries of unnamed trees included
        after = ac.updated(leaves, counts, trees, indices, new)
        rebuilt = gpu.build_forest(after, counts)
        want = rebuilt.roots()
        rebuilt.free()
        named = np.unique(trees).astype(np.int64)
        assert (got[named] == want[named]).all(), (set_name, [int(t) for t in named if (got[t] != want[t]).any()][:10])
        others = np.ones(len(counts), dtype=bool)
        others[named] = False
        assert (got[others] == PATTERN).all(), set_name                     # cells of unnamed trees are never written
        through = gpu.apply_forest_multiproof(old, new, trees, indices, cs, proof.nodes, roots)
        assert through is not None and (through[named] == want[named]).all() and (through[others] == roots[others]).all(), set_name
        parts = proof.split()
        for t in sorted(parts)[:: max(1, len(parts) // 20)][:20]:          # up to 20 trees, spread over the forest
            rows = np.flatnonzero(trees == t)
            ok, root = device_apply_tree(gpu, old[rows], new[rows], parts[t].indices, counts[t], parts[t].height, parts[t].nodes, roots[t])
            assert ok == 1 and (root == want[t]).all(), (set_name, t)
            one = gpu.apply_multiproof(old[rows], new[rows], parts[t].indices, parts[t].nodes, roots[t], counts[t])
            assert one is not None and (one == want[t]).all(), (set_name, t)
            taller = t if taller is None and counts[t] > 1 else taller
        if taller is not None and set_name == "first and last":
            # one tree built with a height above its minimal one: its own stored tree gives the multiproof and the root
            t = taller
            height = tree_height(counts[t]) + 2
            d_slice = gpu.upload(leaves[int(off[t]): int(off[t + 1])])
            tree = gpu.build_tree(d_slice, counts[t], height)
            idx = np.array(sorted(set([0, counts[t] - 1])), dtype=np.uint64)
            mine, fresh = tree.multiproof(idx), random_leaves(rng, idx.shape[0])
            root = tree.root()
            ok, got_root = device_apply_tree(gpu, leaves[int(off[t]) + idx.astype(np.int64)], fresh, idx, counts[t], height, mine.nodes, root)
            r, cpu_root = ac.host_apply_tree(leaves[int(off[t]) + idx.astype(np.int64)], fresh, idx, counts[t], height, mine.nodes, root)
            tree.update(idx, fresh)
            assert ok == 1 and r == 1 and (got_root == cpu_root).all() and (got_root == tree.root()).all(), (t, height)
            tree.free()
            d_slice.free()
    forest.free()


def test_ballot_word_and_prefix_block_edges(gpu):
    """k = 1, 63, 64, 65 (a mask word and its successor), 16384, 16385 (a block of 256 words and its successor) and every leaf,
    each a prefix of the sorted every-leaf set of one forest of 186 trees, checked against a rebuild."""
    counts = fc.CASES["sizes_1_to_130"] + fc.CASES["power_of_two_edges"]
    total = sum(counts)
    leaves = fc.random_leaves(total, seed=191)
    forest = gpu.build_forest(leaves, counts)
    H, roots = forest.levels, forest.roots()
    every_t, every_i = fm.fp.all_queries(counts, sample_above=1 << 30)
    assert every_t.shape[0] == total > 16385 and H == 14      # every prefix length below exists
    rng = np.random.default_rng(192)
    for k in ac.EDGE_KS + (total,):
        trees, indices = every_t[:k], every_i[:k]
        proof = forest.multiproof(trees, indices)
        old, new, cs = leaves[:k], random_leaves(rng, k), ac.counts_of(counts, trees)     # the prefix of the sorted every-leaf set is the first k leaves
        ok, got = device_apply_forest(gpu, old, new, trees, indices, cs, H, proof.nodes, roots)
        assert ok == 1, k
        after = leaves.copy()
        after[:k] = new
        rebuilt = gpu.build_forest(after, counts)
        want = rebuilt.roots()
        rebuilt.free()
        named = np.unique(trees).astype(np.int64)
        assert (got[named] == want[named]).all(), k
        assert (np.delete(got, named, axis=0) == PATTERN).all(), k
        r, cpu = ac.host_apply_forest(old, new, trees, indices, cs, H, proof.nodes, roots)
        assert r == 1 and (cpu == got).all(), k
    forest.free()


def test_the_verdict_one_corruption_at_a_time_equals_the_host_s_and_a_refusal_writes_nothing(gpu):
    """Every mutation of forest_multiproof_cases.MUTATIONS, told in counts, and the refusals only the counts can cause.  The
    canary pages around the scratch, ok and the new roots are checked inside device_apply_forest on every call."""
    ran = set()
    for name in ac.NON_EMPTY:
        counts = fc.CASES[name]
        leaves = ac.case_leaves(name)
        off = fc.offsets_of(counts)
        forest = gpu.build_forest(leaves, counts)
        H, roots = forest.levels, forest.roots()
        rng = np.random.default_rng(len(name) * 19 + 7)
        for set_name, (trees, indices) in ac.entry_sets(counts, rng).items():
            if set_name == "every leaf" and trees.shape[0] > 3000:
                continue                   # the same rule at every size: the other four sets of the large tables run
            heights = np.array([tree_height(counts[int(t)]) for t in trees], dtype=np.uint32)
            proof = forest.multiproof(trees, indices)
            old, new, cs = fm.leaves_at(leaves, off, trees, indices), random_leaves(rng, len(trees)), ac.counts_of(counts, trees)
            cases = [(m[0], m[1], m[2], m[3], ac.counts_for_heights(m[4], m[2], counts), m[5], m[6])
                     for m in fm.mutations(old, trees, indices, heights, H, proof.nodes, roots, rng)]
            q = int(rng.integers(0, len(trees)))
            whole = trees == trees[q]
            cases.append(("count 0", old, trees, indices, np.where(whole, np.uint64(0), cs), proof.nodes, roots))
            c = int(cs[q])
            if c > 1 and tree_height(c - 1) == tree_height(c):
                last = int(np.flatnonzero(whole)[-1])
                lie, ix = cs.copy(), indices.copy()
                lie[whole], ix[last] = c - 1, c - 1                            # in order, inside 2^h, at the count
                cases.append(("index >= count but < 2^h", old, trees, ix, lie, proof.nodes, roots))
            if int(whole.sum()) >= 2 and c > 1 and tree_height(c - 1) == tree_height(c):
                lie = cs.copy()
                lie[int(np.flatnonzero(whole)[0])] = c - 1
                if int(indices[int(np.flatnonzero(whole)[0])]) < c - 1:
                    cases.append(("one entry of a tree with another count", old, trees, indices, lie, proof.nodes, roots))
            for mname, lv, tr, ix, mcs, nd, rt in cases:
                r, cpu = ac.host_apply_forest(lv, new, tr, ix, mcs, H, nd, rt)
                ok, got = device_apply_forest(gpu, lv, new, tr, ix, mcs, H, nd, rt)
                assert ok == r, (name, set_name, mname)
                assert r == (1 if mname == fm.STILL_ACCEPTED else 0), (name, set_name, mname)
                assert (got == cpu).all(), (name, set_name, mname)
                if ok == 0:
                    assert (got == PATTERN).all(), (name, set_name, mname)
                ran.add(mname)
        forest.free()
    assert ran == set(fm.MUTATIONS) | {fm.STILL_ACCEPTED, "count 0", "index >= count but < 2^h", "one entry of a tree with another count"}


def test_the_tree_call_refuses_what_the_host_refuses(gpu):
    rng = np.random.default_rng(41)
    count, height = 130, 8
    leaves = random_leaves(rng, count)
    d_leaves = gpu.upload(leaves)
    tree = gpu.build_tree(d_leaves, count)
    idx = np.array([0, 64, 128, 129], dtype=np.uint64)
    proof, root, new = tree.multiproof(idx), tree.root(), random_leaves(rng, 4)
    old = leaves[idx.astype(np.int64)]
    changed = old.copy()
    changed[2, 5] ^= np.uint32(4)
    for what, args in (("as made", (old, new, idx, count, height, proof.nodes, root)),
                       ("count 0", (old, new, idx, 0, height, proof.nodes, root)),
                       ("index at the count", (old, new, idx, 129, height, proof.nodes, root)),
                       ("a count above 2^height", (old, new, idx, 257, height, proof.nodes, root)),
                       ("leaf changed", (changed, new, idx, count, height, proof.nodes, root)),
                       ("node dropped", (old, new, idx, count, height, proof.nodes[:-1], root)),
                       ("another root", (old, new, idx, count, height, proof.nodes, new[0]))):
        r, cpu = ac.host_apply_tree(*args)
        ok, got = device_apply_tree(gpu, *args)
        assert ok == r == (1 if what == "as made" else 0), what
        assert (got == cpu).all(), what
        if ok == 0:
            assert (got == PATTERN).all(), what
    tree.update(idx, new)
    assert (device_apply_tree(gpu, old, new, idx, count, height, proof.nodes, root)[1] == tree.root()).all()
    tree.free()
    d_leaves.free()


def test_roots_advance_in_place(gpu):
    counts = fc.CASES["sizes_1_to_130"] + [0, 4097]
    leaves = fc.random_leaves(sum(counts), seed=193)
    off = fc.offsets_of(counts)
    forest = gpu.build_forest(leaves, counts)
    H, roots = forest.levels, forest.roots()
    rng = np.random.default_rng(194)
    for set_name, (trees, indices) in ac.entry_sets(counts, rng).items():
        if set_name == "every leaf":
            trees, indices = trees[::3], indices[::3]          # leave some trees unnamed
        proof = forest.multiproof(trees, indices)
        old, new, cs = fm.leaves_at(leaves, off, trees, indices), random_leaves(rng, len(trees)), ac.counts_of(counts, trees)
        ok, apart = device_apply_forest(gpu, old, new, trees, indices, cs, H, proof.nodes, roots)
        ok2, in_place = device_apply_forest(gpu, old, new, trees, indices, cs, H, proof.nodes, roots, in_place=True)
        assert ok == ok2 == 1, set_name
        named = np.unique(trees).astype(np.int64)
        others = np.ones(len(counts), dtype=bool)
        others[named] = False
        assert (in_place[named] == apart[named]).all() and (in_place[others] == roots[others]).all(), set_name
        bad = old.copy()
        bad[0, 0] ^= np.uint32(1)
        ok3, kept = device_apply_forest(gpu, bad, new, trees, indices, cs, H, proof.nodes, roots, in_place=True)
        assert ok3 == 0 and (kept == roots).all(), set_name    # refused: the roots stay as they were
    forest.free()


def test_a_follower_with_the_roots_alone_follows_the_primary(gpu):
    """update_with_witness on a forest and on a tree; the witness applied to the old roots gives the structure's roots after
    the update, and a second witness on top of the first does again."""
    import vk_merkle_roots_amd as vk
    counts = fc.CASES["sizes_1_to_130"] + [0, 1, 2048, 2049]
    leaves = fc.random_leaves(sum(counts), seed=195)
    forest = gpu.build_forest(leaves, counts)
    follower = forest.roots()
    rng = np.random.default_rng(196)
    for round_ in range(2):
        trees, indices = ac.entry_sets(counts, rng)[("7 random per tree", "left of the last pair")[round_]]
        order = rng.permutation(trees.shape[0])                # any order, with a repeat: the last value wins
        t, i = np.concatenate([trees[order], trees[:1]]), np.concatenate([indices[order], indices[:1]])
        fresh = random_leaves(rng, t.shape[0])
        witness = forest.update_with_witness(t, i, fresh)
        assert isinstance(witness, vk.UpdateWitness) and isinstance(witness.proof, vk.ForestMultiproof)
        assert (witness.proof.trees == trees).all() and (witness.proof.indices == indices).all()
        assert (witness.counts == ac.counts_of(counts, trees)).all() and witness.old_leaves.shape == witness.new_leaves.shape == (trees.shape[0], 8)
        assert (witness.new_leaves[0] == fresh[-1]).all()
        assert gpu.verify_forest_multiproof(witness.old_leaves, trees, indices, witness.proof.heights, witness.proof.nodes, follower)
        follower = witness.apply(gpu, follower)
        assert follower is not None and (follower == forest.roots()).all(), round_
        assert witness.apply(gpu, follower) is None            # the witness is of the roots before, not of these
    rebuilt = gpu.build_forest(forest.dev.download(forest.digests, 32 * sum(counts)).reshape(-1, 8), counts)
    assert (rebuilt.roots() == follower).all()
    rebuilt.free()
    forest.free()

    for count, height in ((1000, None), (77, 9)):
        d_leaves = gpu.upload(random_leaves(rng, count))
        tree = gpu.build_tree(d_leaves, count, height)
        root = tree.root()
        for idx in ([count - 1, 0, 500 % count], [(count - 1) & ~1, 3, 3]):
            witness = tree.update_with_witness(idx, random_leaves(rng, len(idx)))
            assert isinstance(witness.proof, vk.Multiproof) and (witness.counts == count).all()
            root = witness.apply(gpu, root)
            assert root is not None and (root == tree.root()).all(), (count, idx)
        tree.free()
        d_leaves.free()
