"""Multiproofs on the GPU (vkmr_hip_tree_multiproof_async, vkmr_hip_verify_multiproof_async, MerkleTree.multiproof,
HipDevice.verify_multiproof) against the hashlib restatement in tests/multiproof_cases.py, the single proofs of
vkmr_hip_tree_proofs_async and vkmr_host_cpu_verify_multiproof.  Every comparison is bit-exact."""
import numpy as np
import pytest

import multiproof_cases as mc
from merkle_model import At
from test_gpu_tree_proofs import proof_indices

pytestmark = pytest.mark.gpu


def index_sets(count, rng):
    """One leaf; all leaves; a contiguous run; the edges of the stored-tree test; random k in {2, 50, 1000}."""
    sets = {"one": [int(rng.integers(0, count))], "all": list(range(count))}
    a = int(rng.integers(0, count))
    sets["run"] = list(range(a, min(count, a + max(1, count // 7))))
    sets["edges"] = proof_indices(count, rng)
    for k in (2, 50, 1000):
        sets[f"random{k}"] = sorted(int(x) for x in rng.choice(count, size=min(k, count), replace=False))
    return sets


def gather_raw(gpu, tree, idx, capacity=None, guard=0, pattern=0xA5):
    """(status, M, counts, buffer [guard + capacity + guard, 8]) of one vkmr_hip_tree_multiproof_async over indices `idx`
    as given (no sorting), the node buffer and its guard cells pre-filled with `pattern`; info pre-filled too."""
    idx = np.ascontiguousarray(idx, dtype=np.uint64)
    k = int(idx.shape[0])
    cap = gpu.lib.vkmr_hip_multiproof_max_nodes(tree.count, tree.height, k) if capacity is None else capacity
    cells = guard + cap + guard
    d_idx = gpu.upload(idx)
    d_scr = gpu.alloc(gpu.lib.vkmr_hip_multiproof_scratch_bytes(k, tree.height))
    d_buf = gpu.upload(np.full((max(cells, 1), 32), pattern, dtype=np.uint8))
    d_info = gpu.upload(np.full(2 + tree.height, 0xDEADBEEFDEADBEEF, dtype=np.uint64))
    tree.multiproof_async(d_idx, k, d_scr, At(d_buf, 32 * guard), cap, d_info)
    info = gpu.download(d_info, 8 * (2 + tree.height), dtype=np.uint64)
    buf = gpu.download(d_buf, 32 * max(cells, 1)).reshape(-1, 8)[:cells]
    for b in (d_idx, d_scr, d_buf, d_info):
        b.free()
    return int(info[0]), int(info[1]), [int(x) for x in info[2:]], buf


@pytest.mark.parametrize("count", [2, 3, 9, 129, 1000, 4097, 70001, 300000])
def test_gather_equals_the_restatement_and_both_verifiers_agree(gpu, count):
    rng = np.random.default_rng(700 + count)
    h0 = mc.tree_height(count)
    leaves = mc.random_leaves(rng, count)
    d_in = gpu.upload(leaves)
    for height in (h0, h0 + 3):
        tree = gpu.build_tree(d_in, count, height)
        levels = {}

        def level_of(l):
            if l not in levels:
                levels[l] = tree.level(l)      # the stored-tree tests check these cells against hashlib
            return levels[l]

        root = tree.root()
        for name, idx in index_sets(count, rng).items():
            what = (count, height, name)
            want, counts = mc.make_multiproof(level_of, count, height, idx)
            proof = tree.multiproof(rng.permutation(np.array(idx + idx[:1])))      # sorted and deduplicated by the Python layer
            assert proof.height == height and list(proof.indices) == idx, what
            assert [int(x) for x in proof.level_counts] == counts, what
            assert proof.nodes.shape == want.shape and (proof.nodes == want).all(), what
            assert want.shape[0] <= gpu.lib.vkmr_hip_multiproof_max_nodes(count, height, len(idx)), what
            proved = leaves[idx]
            assert gpu.verify_multiproof(proved, idx, proof.nodes, root, height), what
            assert mc.host_verify(proved, idx, height, proof.nodes, root), what
            for mname, lv, ix, nd in mc.mutations(proved, idx, proof.nodes, height, rng):
                dev_ok = gpu.verify_multiproof(lv, ix, nd, root, height)
                assert not dev_ok, (what, mname)
                assert mc.host_verify(lv, ix, height, nd, root) == dev_ok, (what, mname)
        tree.free()
    d_in.free()


def test_one_leaf_is_the_single_proof(gpu):
    count = 129
    rng = np.random.default_rng(129)
    d_in = gpu.upload(mc.random_leaves(rng, count))
    for height in (8, 10):
        tree = gpu.build_tree(d_in, count, height)
        single = tree.proofs(list(range(count)))
        for i in range(count):
            proof = tree.multiproof([i])
            assert proof.nodes.shape == (height, 8) and (proof.nodes == single[i]).all(), (height, i)
            assert [int(x) for x in proof.level_counts] == [1] * height
        tree.free()
    d_in.free()


@pytest.mark.parametrize("indices,bits", [([0, 5, 1000], 1), ([999, 1000], 1), ([2**64 - 1], 1), ([3, 1, 7], 2), ([1, 4, 4, 9], 2),
                                          ([0, 1000, 2], 3), ([6], 0), ([0, 999], 0)])
def test_refused_indices_write_no_node(gpu, indices, bits):
    count, height, guard = 1000, 10, 4
    rng = np.random.default_rng(len(indices) + bits)
    d_in = gpu.upload(mc.random_leaves(rng, count))
    tree = gpu.build_tree(d_in, count, height)
    status, m, counts, buf = gather_raw(gpu, tree, indices, guard=guard)
    assert status == bits
    pattern = np.full(8, 0xA5A5A5A5, dtype=np.uint32)
    if bits:
        assert (buf == pattern).all()                       # the node buffer and the cells before and behind it
    else:
        want, wc = mc.make_multiproof(tree.level, count, height, indices)
        assert m == want.shape[0] and counts == wc
        assert (buf[guard:guard + m] == want).all()
        assert (buf[:guard] == pattern).all() and (buf[guard + m:] == pattern).all()
    tree.free()
    d_in.free()


def test_a_buffer_one_cell_short_reports_the_size_and_a_second_call_succeeds(gpu):
    count, height, guard = 4097, 13, 3
    rng = np.random.default_rng(4097)
    d_in = gpu.upload(mc.random_leaves(rng, count))
    tree = gpu.build_tree(d_in, count, height)
    idx = sorted(int(x) for x in rng.choice(count, size=200, replace=False))
    want, wc = mc.make_multiproof(tree.level, count, height, idx)
    m_want = want.shape[0]
    status, m, counts, buf = gather_raw(gpu, tree, idx, capacity=m_want - 1, guard=guard)
    assert status == 4 and m == m_want and counts == wc
    assert (buf == np.full(8, 0xA5A5A5A5, dtype=np.uint32)).all()
    status, m, counts, buf = gather_raw(gpu, tree, idx, capacity=m_want, guard=guard)
    assert status == 0 and m == m_want and counts == wc
    assert (buf[guard:guard + m] == want).all()
    assert (buf[:guard] == np.full(8, 0xA5A5A5A5, dtype=np.uint32)).all() and (buf[guard + m:] == np.full(8, 0xA5A5A5A5, dtype=np.uint32)).all()
    tree.free()
    d_in.free()


def test_height_0_and_no_index(gpu):
    rng = np.random.default_rng(0)
    leaf = mc.random_leaves(rng, 1)
    d_in = gpu.upload(leaf)
    tree = gpu.build_tree(d_in, 1, 0)
    proof = tree.multiproof([0])
    assert proof.nodes.shape == (0, 8) and proof.height == 0 and len(proof.level_counts) == 0
    assert mc.host_verify(leaf, [0], 0, proof.nodes, leaf[0])
    tree.free()
    d_in.free()
    assert not gpu.verify_multiproof(np.zeros((0, 8), np.uint32), [], np.zeros((0, 8), np.uint32), leaf[0], 3)


def test_a_multiproof_on_the_same_stream_sees_the_update(gpu):
    count, height = 5000, 13
    rng = np.random.default_rng(50)
    leaves = mc.random_leaves(rng, count)
    d_in = gpu.upload(leaves)
    tree = gpu.build_tree(d_in, count, height)
    old_root = tree.root()
    proved = np.sort(rng.choice(count, size=300, replace=False)).astype(np.uint64)
    # the update touches half of the proved leaves and as many others
    others = np.setdiff1d(rng.choice(count, size=400, replace=False).astype(np.uint64), proved)[:150]
    upd = np.sort(np.concatenate([proved[::2], others])).astype(np.uint64)
    new = mc.random_leaves(rng, upd.shape[0])
    leaves[upd.astype(np.int64)] = new
    k, ku = int(proved.shape[0]), int(upd.shape[0])
    cap = gpu.lib.vkmr_hip_multiproof_max_nodes(count, height, k)
    d_upd, d_new, d_idx = gpu.upload(upd), gpu.upload(new), gpu.upload(proved)
    d_leaves = gpu.upload(leaves[proved.astype(np.int64)])             # the NEW leaves at the proved positions
    d_status, d_info, d_nodes = gpu.alloc(4), gpu.alloc(8 * (2 + height)), gpu.alloc(32 * cap)
    d_scr = gpu.alloc(gpu.lib.vkmr_hip_multiproof_scratch_bytes(k, height))
    s = gpu.new_stream()
    gpu.sync()
    tree.update_async(d_upd, d_new, ku, d_status, stream=s)            # no sync between the two
    tree.multiproof_async(d_idx, k, d_scr, d_nodes, cap, d_info, stream=s)
    gpu.sync(s)
    assert int(gpu.download(d_status, 4)[0]) == 0
    info = gpu.download(d_info, 8 * (2 + height), dtype=np.uint64)
    assert int(info[0]) == 0
    m = int(info[1])
    nodes = gpu.download(d_nodes, 32 * m).reshape(m, 8)
    new_root = tree.root()
    assert (new_root == gpu.reduce_digests(leaves, height)).all() and not (new_root == old_root).all()
    proved_leaves = leaves[proved.astype(np.int64)]
    assert gpu.verify_multiproof(proved_leaves, proved, nodes, new_root, height)
    assert mc.host_verify(proved_leaves, proved, height, nodes, new_root)
    assert not gpu.verify_multiproof(proved_leaves, proved, nodes, old_root, height)
    for b in (d_upd, d_new, d_idx, d_leaves, d_status, d_info, d_nodes, d_scr, d_in):
        b.free()
    tree.free()


def test_full_size_2_26_leaves_2_20_indices(gpu):
    """2^26 random digests, k = 2^20 random sorted unique indices: M and every m_l against numpy on the indices alone, the
    device verifier on the device-resident proof, one overwritten node, 64 sampled nodes against single proofs."""
    import vk_merkle_roots_amd as vk
    log2, k = 26, 1 << 20
    n, height = 1 << log2, log2
    rng = np.random.default_rng(11)
    idx = np.sort(rng.choice(n, size=k, replace=False)).astype(np.uint64)
    leaves = np.empty((k, 8), dtype=np.uint32)                         # the proved leaves, kept while the digests go up
    d_in = gpu.alloc(32 * n)
    chunk = 1 << 22
    for at in range(0, n, chunk):   # random digests, uploaded in pieces
        part = rng.integers(0, 2**32, size=(chunk, 8), dtype=np.uint32)
        vk.check(gpu.lib.vkmr_hip_memcpy_h2d_async(gpu.index, gpu.stream, d_in.at(32 * at), part.ctypes.data, part.nbytes), "h2d")
        gpu.sync()
        lo, hi = np.searchsorted(idx, [at, at + chunk])
        leaves[lo:hi] = part[(idx[lo:hi] - np.uint64(at)).astype(np.int64)]
    tree = gpu.build_tree(d_in, n, height)
    # what the indices alone say: per level the nodes whose sibling is not among them
    want_counts, emitters = [], []
    cur = idx
    for l in range(height):
        lone = cur[~np.isin(cur ^ np.uint64(1), cur)]
        want_counts.append(int(lone.shape[0]))
        emitters.append(lone)
        cur = np.unique(cur >> np.uint64(1))
    m_want = sum(want_counts)
    cap = gpu.lib.vkmr_hip_multiproof_max_nodes(n, height, k)
    assert cap == 7340031 and m_want <= cap
    d_idx = gpu.upload(idx)
    d_scr = gpu.alloc(gpu.lib.vkmr_hip_multiproof_scratch_bytes(k, height))
    d_nodes, d_info = gpu.alloc(32 * cap), gpu.alloc(8 * (2 + height))
    tree.multiproof_async(d_idx, k, d_scr, d_nodes, cap, d_info)
    info = gpu.download(d_info, 8 * (2 + height), dtype=np.uint64)
    print("full size: status", int(info[0]), "M", int(info[1]), "expected", m_want, "bound", cap)
    assert int(info[0]) == 0 and int(info[1]) == m_want
    assert [int(x) for x in info[2:]] == want_counts
    # the device verifier, everything resident
    d_leaves, d_ok = gpu.upload(leaves), gpu.alloc(4)
    root_cell = At(tree.tree, gpu.tree_bytes(n, height) - 32)
    gpu.verify_multiproof_async(d_leaves, d_idx, k, height, d_nodes, m_want, root_cell, d_scr, d_ok)
    assert int(gpu.download(d_ok, 4)[0]) == 1
    # 64 nodes sampled across the levels equal the single proofs' cells for the same (leaf, level)
    starts = np.concatenate([[0], np.cumsum(want_counts)])
    ranks = np.sort(rng.choice(m_want, size=64, replace=False))
    sample_levels = np.searchsorted(starts, ranks, side="right") - 1
    sample_leaves = []
    for r, l in zip(ranks, sample_levels):
        p = int(emitters[l][r - starts[l]])
        sample_leaves.append(int(idx[np.searchsorted(idx, np.uint64(p << int(l)))]))      # a proved leaf below node p
        assert sample_leaves[-1] >> int(l) == p
    single = tree.proofs(sample_leaves)
    for j, (r, l) in enumerate(zip(ranks, sample_levels)):
        got = gpu.download(d_nodes, 32, offset=32 * int(r))
        assert (got == single[j][l]).all(), (int(r), int(l))
    # one node overwritten on the device: rejected
    zero = np.zeros(8, dtype=np.uint32)
    vk.check(gpu.lib.vkmr_hip_memcpy_h2d_async(gpu.index, gpu.stream, d_nodes.at(32 * int(ranks[17])), zero.ctypes.data, 32), "h2d")
    gpu.sync()
    gpu.verify_multiproof_async(d_leaves, d_idx, k, height, d_nodes, m_want, root_cell, d_scr, d_ok)
    assert int(gpu.download(d_ok, 4)[0]) == 0
    for b in (d_idx, d_scr, d_nodes, d_info, d_leaves, d_ok, d_in):
        b.free()
    tree.free()
