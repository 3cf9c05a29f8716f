"""Leaf updates of a stored tree on the GPU (vkmr_hip_tree_update_async, MerkleTree.update / update_async / update_packed):
every level after an update against hashlib and a fresh build, the device-side index checks, and proofs gathered and verified
on the same stream after an update."""
import numpy as np
import pytest

from merkle_model import At, cpu_levels, node, random_leaves  # noqa: F401

pytestmark = pytest.mark.gpu


def all_levels(tree):
    return [tree.level(l) for l in range(tree.height + 1)]


def assert_levels_equal(tree, want, what):
    for l in range(tree.height + 1):
        got = tree.level(l)
        assert got.shape == want[l].shape and (got == want[l]).all(), (what, l)


def update_sets(count, rng):
    """The first leaf, the last leaf (duplicate-last on odd levels), both children of one pair, a random third, every leaf."""
    sets = {"first": [0], "last": [count - 1]}
    if count >= 2:
        p = int(rng.integers(0, count // 2))
        sets["pair"] = [2 * p, 2 * p + 1]
    sets["third"] = sorted(int(x) for x in rng.choice(count, size=max(1, count // 3), replace=False))
    sets["every"] = list(range(count))
    return sets


@pytest.mark.parametrize("count", [1, 2, 3, 5, 8, 9, 127, 128, 129, 1000, 4097, 65537])
def test_update_equals_hashlib_over_the_updated_leaves(gpu, count):
    from vk_merkle_roots_amd.engine import tree_height
    rng = np.random.default_rng(1000 + count)
    h0 = tree_height(count)
    base = random_leaves(rng, count)
    for height in (h0, h0 + 3):
        for name, idx in update_sets(count, rng).items():
            leaves = base.copy()
            new = random_leaves(rng, len(idx))
            leaves[idx] = new
            d_in = gpu.upload(base)
            tree = gpu.build_tree(d_in, count, height)
            tree.update(idx, new)
            assert_levels_equal(tree, cpu_levels(leaves, height), (count, height, name))
            assert (gpu.download(d_in, 32 * count).reshape(count, 8) == leaves).all()   # the caller's buffer is level 0
            assert (tree.root() == gpu.reduce_digests(leaves, height)).all(), (count, height, name)
            tree.free()
            d_in.free()


def test_successive_rounds_equal_a_fresh_build(gpu):
    count, height = 3001, 14
    rng = np.random.default_rng(9)
    leaves = random_leaves(rng, count)
    d_in = gpu.upload(leaves)
    tree = gpu.build_tree(d_in, count, height)
    for r in range(8):
        k = int(rng.integers(1, 400))
        idx = rng.integers(0, count, size=k)           # repeats allowed: the last value wins
        new = random_leaves(rng, k)
        for i, v in zip(idx, new):
            leaves[i] = v
        tree.update(idx, new)
        d_ref = gpu.upload(leaves)
        fresh = gpu.build_tree(d_ref, count, height)
        for l in range(height + 1):
            assert (tree.level(l) == fresh.level(l)).all(), (r, l)
        fresh.free()
        d_ref.free()
    tree.free()
    d_in.free()


def test_2_22_leaves_2_16_random_updates(gpu):
    count, height = 1 << 22, 22
    rng = np.random.default_rng(22)
    leaves = random_leaves(rng, count)
    d_in = gpu.upload(leaves)
    tree = gpu.build_tree(d_in, count, height)
    idx = rng.choice(count, size=1 << 16, replace=False)
    new = random_leaves(rng, idx.shape[0])
    tree.update(idx, new)
    leaves[idx] = new
    d_ref = gpu.upload(leaves)
    fresh = gpu.build_tree(d_ref, count, height)
    for l in range(height + 1):
        assert (tree.level(l) == fresh.level(l)).all(), l
    d_scr, d_root = gpu.reduce_scratch(count), gpu.alloc(32)
    gpu.reduce_async(d_ref, count, height, d_scr, d_root)
    assert (tree.root() == gpu.download(d_root, 32)).all()
    for b in (d_scr, d_root, d_ref, d_in):
        b.free()
    fresh.free()
    tree.free()


@pytest.mark.parametrize("indices,bits", [([3, 1, 7], 2), ([1, 4, 4, 9], 2), ([0, 5, 1000], 1), ([0, 1000, 2], 3),
                                          ([999, 1000], 1), ([2**64 - 1], 1), ([6], 0), ([0, 999], 0)])
def test_bad_device_indices_change_nothing(gpu, indices, bits):
    count, height = 1000, 10
    rng = np.random.default_rng(len(indices) + bits)
    leaves = random_leaves(rng, count)
    d_in = gpu.upload(leaves)
    tree = gpu.build_tree(d_in, count, height)
    before = all_levels(tree)
    k = len(indices)
    new = random_leaves(rng, k)
    d_idx, d_new = gpu.upload(np.array(indices, dtype=np.uint64)), gpu.upload(new)
    d_status = gpu.upload(np.array([0xDEADBEEF], dtype=np.uint32))     # always written
    tree.update_async(d_idx, d_new, k, d_status)
    assert int(gpu.download(d_status, 4)[0]) == bits
    after = all_levels(tree)
    if bits:
        for l, (a, b) in enumerate(zip(before, after)):
            assert (a == b).all(), l
    else:
        leaves[indices] = new
        assert_levels_equal(tree, cpu_levels(leaves, height), indices)
    for b in (d_idx, d_new, d_status, d_in):
        b.free()
    tree.free()


def test_update_repeated_indices_last_value_wins(gpu):
    count, height = 77, 7
    rng = np.random.default_rng(77)
    leaves = random_leaves(rng, count)
    d_in = gpu.upload(leaves)
    tree = gpu.build_tree(d_in, count, height)
    idx = [5, 76, 5, 0, 76, 5]
    new = random_leaves(rng, len(idx))
    tree.update(idx, new)
    leaves[0], leaves[5], leaves[76] = new[3], new[5], new[4]
    assert_levels_equal(tree, cpu_levels(leaves, height), "repeats")
    tree.free()
    d_in.free()


def test_height_0_writes_only_the_leaf(gpu):
    rng = np.random.default_rng(0)
    d_in = gpu.upload(random_leaves(rng, 1))
    tree = gpu.build_tree(d_in, 1, 0)
    assert tree.tree is None
    new = random_leaves(rng, 1)
    tree.update([0], new)
    assert (tree.root() == new[0]).all()
    tree.free()
    d_in.free()


def test_proofs_on_the_same_stream_see_the_update(gpu):
    count, height = 5000, 13
    rng = np.random.default_rng(5)
    leaves = random_leaves(rng, count)
    d_in = gpu.upload(leaves)
    tree = gpu.build_tree(d_in, count, height)
    idx = np.sort(rng.choice(count, size=300, replace=False)).astype(np.uint64)
    old_proofs = tree.proofs(idx)
    old_leaves = leaves[idx.astype(np.int64)].copy()
    new = random_leaves(rng, idx.shape[0])
    leaves[idx.astype(np.int64)] = new
    want_root = cpu_levels(leaves, height)[height][0]
    k = int(idx.shape[0])
    d_idx, d_new = gpu.upload(idx), gpu.upload(new)
    d_status, d_sib, d_ok = gpu.alloc(4), gpu.alloc(32 * k * height), gpu.alloc(4 * k)
    root_cell = At(tree.tree, gpu.tree_bytes(count, height) - 32)     # the root, read in place by the verifier
    s = gpu.new_stream()
    gpu.sync()
    tree.update_async(d_idx, d_new, k, d_status, stream=s)             # no sync between the three
    tree.proofs_async(d_idx, k, d_sib, stream=s)
    gpu.verify_proofs_async(d_new, d_idx, d_sib, k, height, root_cell, 1, d_ok, stream=s)
    gpu.sync(s)
    assert int(gpu.download(d_status, 4)[0]) == 0
    assert (tree.root() == want_root).all()
    assert (gpu.download(d_ok, 4 * k) == 1).all()
    # the old proofs of the updated leaves fail against the new root
    assert not gpu.verify_proofs(old_leaves, idx, old_proofs, want_root).any()
    for b in (d_idx, d_new, d_status, d_sib, d_ok, d_in):
        b.free()
    tree.free()


def lines(strings):
    return b"".join(s + b"\n" for s in strings)


@pytest.mark.parametrize("count", [1, 6, 1000])
def test_update_packed_equals_a_tree_over_the_edited_strings(gpu, count):
    import vk_merkle_roots_amd as vk
    rng = np.random.default_rng(count)
    strings = [bytes(rng.integers(97, 123, size=int(rng.integers(1, 90)), dtype=np.uint8)) for _ in range(count)]
    tree = vk.merkle_tree_packed(gpu, vk.pack_lines(lines(strings)))
    assert tree.count == count
    idx = [int(x) for x in rng.integers(0, count, size=max(1, count // 4))] + [count - 1, 0]
    repl = [b"edited-%d-%d" % (q, i) for q, i in enumerate(idx)]
    batch = vk.pack_lines(lines(repl))
    assert batch.count == len(idx)
    tree.update_packed(idx, batch)
    edited = list(strings)
    for i, s in zip(idx, repl):            # the last occurrence wins, as in update()
        edited[i] = s
    want = vk.merkle_tree_packed(gpu, vk.pack_lines(lines(edited)))
    for l in range(tree.height + 1):
        assert (tree.level(l) == want.level(l)).all(), l
    tree.free()
    want.free()
