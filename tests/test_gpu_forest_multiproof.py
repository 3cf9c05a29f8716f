"""Multiproofs inside a stored forest on the GPU (vkmr_hip_forest_multiproof_async, vkmr_hip_verify_forest_multiproof_async
through HipDevice, MerkleForest and ForestMultiproof): the gather against the host CPU counterpart, a hashlib restatement
(tests/forest_multiproof_cases.py) and the stored tree of each tree alone; the ballot-word and prefix-block edges of the
ranking; the verifier's acceptance rule one corruption at a time; statuses, exact buffers and canaries; stream order behind an
update; and a ranking over more than 256 (level, block) pairs."""
import numpy as np
import pytest

import forest_cases as fc
import forest_multiproof_cases as fm
from merkle_model import At

pytestmark = pytest.mark.gpu

PATTERN = 0xC3C3C3C3
NON_EMPTY = sorted(name for name, counts in fc.CASES.items() if sum(counts))


def case_leaves(name):
    counts = fc.CASES[name]
    return fc.random_leaves(sum(counts), seed=len(name) * 104729 + sum(counts))


@pytest.mark.parametrize("name", NON_EMPTY)
def test_gather_equals_the_host_cpu_the_restatement_and_each_tree_s_own_multiproof(gpu, name):
    import vk_merkle_roots_amd as vk
    counts = fc.CASES[name]
    total = sum(counts)
    leaves = case_leaves(name)
    off = fc.offsets_of(counts)
    forest = gpu.build_forest(leaves, counts)
    H, roots = forest.levels, forest.roots()
    assert H == fm.stride_of(total, max(counts))
    rng = np.random.default_rng(len(name) * 31 + 5)
    cache, single = {}, {}
    for set_name, (trees, indices) in fm.entry_sets(counts, rng).items():
        if name == "one_big_among_small" and set_name == "every leaf":
            mine = indices[trees == counts.index(100003)]
            assert mine.min() == 0 and mine.max() == 100002 and mine.shape[0] < 300     # the big tree is sampled
        proof = forest.multiproof(trees, indices)
        assert isinstance(proof, vk.ForestMultiproof) and proof.stride == H
        assert (proof.trees == trees).all() and (proof.indices == indices).all()
        rc, cpu_nodes, cpu_heights, cpu_info = fm.host_make(leaves, off, trees, indices, H)
        assert rc == 0
        assert proof.nodes.shape[0] == int(cpu_info[1]) and [int(x) for x in proof.level_counts] == [int(x) for x in cpu_info[2:]], set_name
        assert (proof.heights == cpu_heights).all(), set_name
        assert (proof.nodes == cpu_nodes).all(), (set_name, np.nonzero((proof.nodes != cpu_nodes).any(axis=1))[0][:10])
        want_nodes, want_heights, want_counts, want_roots = fm.make(leaves, off, trees, indices, H, cache)
        assert (cpu_nodes == want_nodes).all() and (cpu_heights == want_heights).all() and [int(x) for x in cpu_info[2:]] == want_counts
        for t, r in want_roots.items():
            assert (roots[t] == r).all(), t
        proved = fm.leaves_at(leaves, off, trees, indices)
        assert gpu.verify_forest_multiproof(proved, trees, indices, proof.heights, proof.nodes, roots), set_name
        assert fm.host_verify(proved, trees, indices, proof.heights, H, proof.nodes, roots), set_name
        parts = proof.split()
        assert sorted(parts) == sorted(set(int(t) for t in trees))
        assert sum(p.nodes.shape[0] for p in parts.values()) == proof.nodes.shape[0]
        for t in sorted(parts)[:: max(1, len(parts) // 20)][:20]:          # up to 20 trees, spread over the forest
            if t not in single:
                d_slice = gpu.upload(leaves[int(off[t]): int(off[t + 1])])
                single[t] = (gpu.build_tree(d_slice, counts[t]), d_slice)
            tree = single[t][0]
            alone = tree.multiproof(parts[t].indices)
            assert parts[t].height == tree.height == alone.height
            assert (parts[t].indices == alone.indices).all() and (parts[t].nodes == alone.nodes).all(), (set_name, t)
            assert [int(x) for x in parts[t].level_counts] == [int(x) for x in alone.level_counts]
    for tree, d_slice in single.values():
        tree.free()
        d_slice.free()
    forest.free()


def test_ballot_word_and_prefix_block_edges(gpu):
    """k = 1, 63, 64, 65 (a mask word and its successor), 16384, 16385 (a block of 256 words and its successor) and every leaf,
    each a prefix of the sorted every-leaf set of one forest of 186 trees."""
    counts = fc.CASES["sizes_1_to_130"] + fc.CASES["power_of_two_edges"]
    total = sum(counts)
    leaves = fc.random_leaves(total, seed=91)
    off = fc.offsets_of(counts)
    forest = gpu.build_forest(leaves, counts)
    H, roots = forest.levels, forest.roots()
    every_t, every_i = fm.fp.all_queries(counts, sample_above=1 << 30)
    assert every_t.shape[0] == total > 16385 and H == 14      # every prefix length below exists
    for k in (1, 63, 64, 65, 16384, 16385, total):
        trees, indices = every_t[:k], every_i[:k]
        proof = forest.multiproof(trees, indices)
        rc, cpu_nodes, cpu_heights, cpu_info = fm.host_make(leaves, off, trees, indices, H)
        assert rc == 0 and proof.nodes.shape[0] == int(cpu_info[1]), k
        assert [int(x) for x in proof.level_counts] == [int(x) for x in cpu_info[2:]], k
        assert (proof.heights == cpu_heights).all() and (proof.nodes == cpu_nodes).all(), k
        proved = leaves[:k] if k < total else leaves                   # the prefix of the sorted every-leaf set is the first k leaves
        assert gpu.verify_forest_multiproof(proved, trees, indices, proof.heights, proof.nodes, roots), k
    forest.free()


def test_verifier_rejects_each_single_corruption_as_the_host_cpu_and_the_restatement_do(gpu):
    """Every mutation of forest_multiproof_cases.MUTATIONS ran at least once over the tables; a mutation that needs what an entry
    set lacks is skipped there.  The device's verdict is compared with the host CPU verifier's on every set; the restatement
    hashes in Python, so it gives its verdict too on the sets of at most 3000 path levels (every mutation runs on such a set)."""
    ran = set()                                                    # the mutations all three verifiers saw
    for name in NON_EMPTY:
        counts = fc.CASES[name]
        leaves = case_leaves(name)
        off = fc.offsets_of(counts)
        forest = gpu.build_forest(leaves, counts)
        H, roots = forest.levels, forest.roots()
        rng = np.random.default_rng(len(name) * 17 + 3)
        for set_name, (trees, indices) in fm.entry_sets(counts, rng).items():
            heights = np.array([fm.tree_height(counts[int(t)]) for t in trees], dtype=np.uint32)
            model = int(heights.sum()) <= 3000
            proof = forest.multiproof(trees, indices)
            assert (proof.heights == heights).all()
            proved = fm.leaves_at(leaves, off, trees, indices)
            assert not model or fm.verify(proved, trees, indices, heights, H, proof.nodes, roots), (name, set_name)
            for mname, lv, tr, ix, hs, nd, rt in fm.mutations(proved, trees, indices, heights, H, proof.nodes, roots, rng):
                want = mname == fm.STILL_ACCEPTED
                assert not model or fm.verify(lv, tr, ix, hs, H, nd, rt) == want, (name, set_name, mname)
                assert fm.host_verify(lv, tr, ix, hs, H, nd, rt) == want, (name, set_name, mname)
                d_ok = verdict_at_stride(gpu, lv, tr, ix, hs, H, nd, rt)
                assert d_ok == want, (name, set_name, mname)
                if model:
                    ran.add(mname)
        forest.free()
    assert ran == set(fm.MUTATIONS) | {fm.STILL_ACCEPTED}


def verdict_at_stride(gpu, leaves, trees, indices, heights, stride, nodes, roots):
    """vkmr_hip_verify_forest_multiproof_async at the forest's own stride (HipDevice.verify_forest_multiproof picks the tallest
    height it is given, which a mutated height would move): bool.  ok starts as a pattern: the call must write it."""
    k, m = trees.shape[0], nodes.shape[0]
    with gpu.scope() as tmp:
        d_lv, d_tr, d_ix, d_hs, d_nd, d_rt = (tmp.upload(np.ascontiguousarray(a)) for a in (leaves, trees, indices, heights, nodes, roots))
        d_scr = tmp.alloc(gpu.lib.vkmr_hip_forest_multiproof_scratch_bytes(k, stride))
        d_ok = tmp.upload(np.full(1, PATTERN, dtype=np.uint32))
        gpu.verify_forest_multiproof_async(d_lv, d_tr, d_ix, d_hs, k, stride, d_nd if m else None, m, d_rt, roots.shape[0], d_scr, d_ok)
        ok = int(gpu.download(d_ok, 4)[0])
    assert ok in (0, 1)
    return ok == 1


def test_statuses_capacity_exact_buffers_and_canaries(gpu):
    counts = fc.CASES["sizes_1_to_130"] + [4097, 0, 0]
    total, ntrees, max_count = sum(counts), len(counts), 4097
    leaves = fc.random_leaves(total, seed=93)
    off = fc.offsets_of(counts)
    forest = gpu.build_forest(leaves, counts, max_count=max_count)
    H, roots = forest.levels, forest.roots()
    assert H == 13
    rng = np.random.default_rng(94)
    trees, indices = fm.entry_sets(counts, rng)["7 random per tree"]
    k = trees.shape[0]
    rc, cpu_nodes, cpu_heights, cpu_info = fm.host_make(leaves, off, trees, indices, H)
    assert rc == 0
    M = int(cpu_info[1])
    guard = 4096
    scratch_bytes = gpu.lib.vkmr_hip_forest_multiproof_scratch_bytes(k, H)
    assert scratch_bytes % 16 == 0 and scratch_bytes > 0

    def run(trees, indices, capacity):
        """One gather with scratch of exactly the size function, `capacity` node cells, k heights and 2 + H info words, each
        between two canary pages: (nodes [capacity, 8], heights, info) as the call left them; the pages are checked here."""
        sizes = (scratch_bytes, 32 * capacity, 4 * k, 8 * (2 + H))
        bufs = [gpu.upload(np.full((guard + n + guard) // 4, PATTERN, dtype=np.uint32)) for n in sizes]
        d_trees, d_idx = gpu.upload(np.ascontiguousarray(trees, dtype=np.uint32)), gpu.upload(np.ascontiguousarray(indices, dtype=np.uint64))
        d_scr, d_nodes, d_h, d_info = (At(b, guard) for b in bufs)
        forest.multiproof_async(d_trees, d_idx, k, d_scr, d_nodes if capacity else None, capacity, d_h, d_info)
        out = []
        for b, n in zip(bufs, sizes):
            after = gpu.download(b, guard + n + guard)
            assert (after[: guard // 4] == PATTERN).all() and (after[-(guard // 4):] == PATTERN).all(), n
            out.append(after[guard // 4: guard // 4 + n // 4])
        for b in bufs + [d_trees, d_idx]:
            b.free()
        return out[1].reshape(-1, 8), out[2], out[3].view(np.uint64)

    nodes, heights, info = run(trees, indices, M)                  # exactly M cells
    assert int(info[0]) == 0 and int(info[1]) == M and (info[2:] == cpu_info[2:]).all()
    assert (nodes == cpu_nodes).all() and (heights == cpu_heights).all()
    nodes, heights, info = run(trees, indices, M - 1)              # one too few: bit 2, M and the counts valid, no node written
    assert int(info[0]) == 4 and int(info[1]) == M and (info[2:] == cpu_info[2:]).all()
    assert (nodes == PATTERN).all() and (heights == cpu_heights).all()
    nodes, heights, info = run(trees, indices, M)                  # and again with M
    assert int(info[0]) == 0 and (nodes == cpu_nodes).all()

    canary64 = np.uint64(PATTERN * 0x100000001)
    empty = counts.index(0)
    for what, want in (("tree", 1), ("index", 1), ("empty", 1), ("swapped", 2), ("repeated", 2), ("both", 3)):
        t, i = trees.copy(), indices.copy()
        q = int(rng.integers(1, k - 1))
        lasts = np.flatnonzero(t[1:] != t[:-1])                    # the last entry of each tree but the last
        if what == "tree":
            t[-1] = ntrees
        elif what == "index":
            q = int(lasts[int(rng.integers(0, lasts.shape[0]))])
            i[q] = counts[int(t[q])]                               # still in order: the next entry names a later tree
        elif what == "empty":
            t[-1], i[-1] = empty, 0                                # still in order: the empty trees are the last two
            assert counts[empty] == 0 and int(t[-2]) < empty
        elif what == "swapped":
            t[q - 1], t[q], i[q - 1], i[q] = t[q], t[q - 1], i[q], i[q - 1]
        elif what == "repeated":
            t[q], i[q] = t[q - 1], i[q - 1]
        else:
            t[q], i[q] = t[q - 1], i[q - 1]
            t[-1] = 2**32 - 1
        nodes, heights, info = run(t, i, M)
        assert int(info[0]) == want, what
        assert (nodes == PATTERN).all() and (heights == PATTERN).all() and (info[1:] == canary64).all(), what
        rc, _, _, host_info = fm.host_make(leaves, off, t, i, H)
        assert rc == want and int(host_info[0]) == want, what
    # MerkleForest.multiproof names the bits when the device refuses (its own checks bypassed: the counts it holds are widened)
    forest.counts = forest.counts + np.uint64(1)
    with pytest.raises(RuntimeError, match="bit 0"):
        forest.multiproof([0], [1])                                # tree 0 holds one leaf
    forest.free()


def test_multiproof_after_update_on_one_stream_proves_the_updated_forest(gpu):
    """update -> multiproof -> verify -> download on one stream with no synchronisation in between."""
    import vk_merkle_roots_amd as vk
    counts = fc.CASES["sizes_1_to_130"]
    total, ntrees = sum(counts), len(counts)
    leaves = fc.random_leaves(total, seed=95)
    off = fc.offsets_of(counts)
    forest = gpu.build_forest(leaves, counts)
    H = forest.levels
    rng = np.random.default_rng(96)
    trees, indices = fm.entry_sets(counts, rng)["7 random per tree"]
    k = trees.shape[0]
    fresh = fc.random_leaves(k, seed=97)
    updated = leaves.copy()
    updated[(off[trees.astype(np.int64)] + indices).astype(np.int64)] = fresh
    old_roots = forest.roots()
    cap = gpu.lib.vkmr_hip_forest_multiproof_max_nodes(total, ntrees, forest.max_count, k)
    assert cap == fm.max_nodes(total, ntrees, forest.max_count, k)
    with gpu.scope() as tmp:
        d_trees, d_idx, d_fresh = tmp.upload(trees), tmp.upload(indices), tmp.upload(fresh)
        d_scr = tmp.alloc(gpu.lib.vkmr_hip_forest_multiproof_scratch_bytes(k, H))
        d_nodes, d_h, d_info, d_status, d_ok = tmp.alloc(32 * cap), tmp.alloc(4 * k), tmp.alloc(8 * (2 + H)), tmp.alloc(4), tmp.alloc(4)
        d_vscr = tmp.alloc(gpu.lib.vkmr_hip_forest_multiproof_scratch_bytes(k, H))
        s = gpu.new_stream()
        forest.update_async(d_trees, d_idx, d_fresh, k, d_status, stream=s)
        forest.multiproof_async(d_trees, d_idx, k, d_scr, d_nodes, cap, d_h, d_info, stream=s)
        info = np.zeros(2 + H, dtype=np.uint64)
        vk.check(gpu.lib.vkmr_hip_memcpy_d2h_async(gpu.index, s, info.ctypes.data, d_info.ptr, info.nbytes), "d2h")
        gpu.sync(s)                                                # M is an argument of the verifier: the one host read
        m = int(info[1])
        gpu.verify_forest_multiproof_async(d_fresh, d_trees, d_idx, d_h, k, H, d_nodes, m, forest.roots_buf, ntrees, d_vscr, d_ok, stream=s)
        ok = np.zeros(1, dtype=np.uint32)
        vk.check(gpu.lib.vkmr_hip_memcpy_d2h_async(gpu.index, s, ok.ctypes.data, d_ok.ptr, 4), "d2h")
        gpu.sync(s)
        assert int(info[0]) == 0 and int(gpu.download(d_status, 4)[0]) == 0 and ok[0] == 1
        nodes, heights = gpu.download(d_nodes, 32 * m).reshape(m, 8), gpu.download(d_h, 4 * k)
        gpu.lib.vkmr_hip_stream_destroy(gpu.index, s)
    new_roots = forest.roots()
    forest.free()
    assert (new_roots != old_roots).any(axis=1).all()              # every tree was touched
    rc, cpu_nodes, cpu_heights, cpu_info = fm.host_make(updated, off, trees, indices, H)
    assert rc == 0 and (nodes == cpu_nodes).all() and (heights == cpu_heights).all() and (info == cpu_info).all()
    assert fm.host_verify(fresh, trees, indices, heights, H, nodes, new_roots)
    assert not fm.host_verify(fresh, trees, indices, heights, H, nodes, old_roots)
    assert (new_roots == gpu.forest_roots(updated, counts)).all()


def test_rank_prefix_over_more_than_256_level_block_pairs(gpu):
    """2^19 leaves in trees of 1..4095, every second leaf proved (k = 2^18: 4096 ballot words, 16 blocks a level); the forest is
    built with max_count = total, so the stride is 19 and the one-workgroup prefix runs over 304 (level, block) sums."""
    rng = np.random.default_rng(19)
    total = 1 << 19
    counts = []
    while sum(counts) < total:
        counts.append(min(int(rng.integers(1, 4096)), total - sum(counts)))
    leaves = fc.random_leaves(total, seed=98)
    off = fc.offsets_of(counts)
    forest = gpu.build_forest(leaves, counts, max_count=total)
    H, roots = forest.levels, forest.roots()
    assert H == 19
    flat = np.arange(0, total, 2, dtype=np.uint64)
    trees = (np.searchsorted(off, flat, side="right") - 1).astype(np.uint32)
    indices = flat - off[trees.astype(np.int64)]
    k = flat.shape[0]
    assert k == 1 << 18 and ((k + 63) // 64 + 255) // 256 * H > 256
    proof = forest.multiproof(trees, indices)
    forest.free()
    rc, cpu_nodes, cpu_heights, cpu_info = fm.host_make(leaves, off, trees, indices, H)
    assert rc == 0 and proof.nodes.shape[0] == int(cpu_info[1])
    assert [int(x) for x in proof.level_counts] == [int(x) for x in cpu_info[2:]]
    assert (proof.heights == cpu_heights).all() and (proof.nodes == cpu_nodes).all()
    proved = np.ascontiguousarray(leaves[::2])
    assert verdict_at_stride(gpu, proved, trees, indices, proof.heights, H, proof.nodes, roots)
    assert gpu.verify_forest_multiproof(proved, trees, indices, proof.heights, proof.nodes, roots)
    assert fm.host_verify(proved, trees, indices, proof.heights, H, proof.nodes, roots)
    bad = proof.nodes.copy()
    bad[-1, 0] ^= np.uint32(1)                                     # the last node: the top of the last tree
    assert not verdict_at_stride(gpu, proved, trees, indices, proof.heights, H, bad, roots)
