"""Stored trees on the GPU: every level (vkmr_hip_reduce_tree_async), proofs gathered from it for any number of leaves
(vkmr_hip_tree_proofs_async) and their batch verification (vkmr_hip_verify_proofs_async), against hashlib, the other
proof entry points, vkmr_host_cpu_fold_proof, the golden roots and the proofs the `vkmr` front end prints."""
import json
import os

import numpy as np
import pytest

from conftest import ROOT
from merkle_model import cpu_levels, host_fold as cpu_fold, node, random_leaves  # noqa: F401

pytestmark = pytest.mark.gpu


def cpu_verify(leaf, index, siblings, height, root):
    """The reference rule of vkmr_hip_verify_proofs_async: the fold of vkmr_host_cpu_fold_proof, and index < 2^height."""
    return int(index) < (1 << height) and bool((cpu_fold(leaf, index, siblings, height) == root).all())


@pytest.mark.parametrize("count", [1, 2, 3, 5, 8, 9, 127, 128, 129, 1000, 4097, 65537])
def test_every_level_of_the_stored_tree(gpu, count):
    from vk_merkle_roots_amd.engine import tree_height
    rng = np.random.default_rng(count)
    leaves = random_leaves(rng, count)
    h0 = tree_height(count)
    want = cpu_levels(leaves, h0 + 3)
    d_in = gpu.upload(leaves)
    for height in (h0, h0 + 3):
        tree = gpu.build_tree(d_in, count, height)
        for l in range(height + 1):
            got = tree.level(l)
            assert got.shape == want[l].shape and (got == want[l]).all(), (count, height, l)
        assert (tree.root() == want[height][0]).all()
        tree.free()
    d_in.free()


def test_root_equals_both_reductions(gpu):
    from vk_merkle_roots_amd.engine import tree_height
    rng = np.random.default_rng(5)
    counts = [int(c) for c in rng.integers(1, 1 << 20, size=10)] + [1 << 20, (1 << 20) - 1, 777]
    for count in counts:
        leaves = random_leaves(rng, count)
        d_in = gpu.upload(leaves)
        for height in (tree_height(count), tree_height(count) + 2):
            tree = gpu.build_tree(d_in, count, height)
            root = tree.root()
            assert (root == gpu.reduce_digests(leaves, height)).all(), (count, height)
            assert (root == gpu.reduce_digests(leaves, height, levels_variant=True)).all(), (count, height)
            tree.free()
        d_in.free()


def proof_indices(count, rng):
    idx = {0, 1, count - 2, count - 1}
    j = 1
    while (1 << j) <= count + 1:
        idx |= {(1 << j) - 1, 1 << j, (1 << j) + 1}
        j += 1
    idx |= {int(x) for x in rng.integers(0, count, size=12)}
    return sorted(i for i in idx if 0 <= i < count)


@pytest.mark.parametrize("count,extra", [(2, 0), (3, 0), (9, 2), (129, 0), (1000, 0), (4097, 0), (4097, 3), (70001, 0), (300000, 1)])
def test_gathered_proofs_equal_the_other_proof_entry_points(gpu, count, extra):
    from vk_merkle_roots_amd.engine import tree_height
    rng = np.random.default_rng(count + extra)
    leaves = random_leaves(rng, count)
    height = tree_height(count) + extra
    d_in = gpu.upload(leaves)
    tree = gpu.build_tree(d_in, count, height)
    idx = proof_indices(count, rng)
    sib = tree.proofs(idx)
    assert sib.shape == (len(idx), height, 8)
    for q, index in enumerate(idx if count < 100000 else idx[:8]):
        want, _ = gpu.proof(d_in, count, height, index)
        assert (sib[q] == want).all(), (count, height, index)
    k16 = idx[:16]
    want16, _ = gpu.reduce_with_proofs(d_in, count, height, k16)
    assert (tree.proofs(k16) == want16).all()
    # out-of-range indices get zero cells; the others beside them are unaffected
    mixed = tree.proofs([count, idx[-1], count + 12345, 2**64 - 1])
    assert not mixed[[0, 2, 3]].any()
    assert (mixed[1] == sib[-1]).all()
    tree.free()
    d_in.free()


def test_every_proof_of_4097_leaves_folds_to_the_root(gpu):
    from vk_merkle_roots_amd.engine import tree_height
    count = 4097
    leaves = random_leaves(np.random.default_rng(4097), count)
    d_in = gpu.upload(leaves)
    tree = gpu.build_tree(d_in, count)
    root = tree.root()
    sib = tree.proofs(np.arange(count))
    for index in range(count):
        assert (cpu_fold(leaves[index], index, sib[index], tree_height(count)) == root).all(), index
    tree.free()
    d_in.free()


def test_verify_matches_the_cpu_rule(gpu):
    rng = np.random.default_rng(21)
    count, height = 3001, 12
    leaves = random_leaves(rng, count)
    d_in = gpu.upload(leaves)
    tree = gpu.build_tree(d_in, count, height)
    root = tree.root()
    idx = np.array([int(x) for x in rng.integers(0, count, size=400)] + [0, count - 1], dtype=np.uint64)
    k = idx.shape[0]
    lv = leaves[idx.astype(np.int64)].copy()
    sib = tree.proofs(idx)
    cases = np.zeros(k, dtype=np.int64)
    for q in range(k):
        cases[q] = q % 6
        if cases[q] == 1:                   # one flipped bit of a random sibling
            sib[q, rng.integers(0, height), rng.integers(0, 8)] ^= np.uint32(1 << int(rng.integers(0, 32)))
        elif cases[q] == 2:                 # a flipped index bit
            idx[q] ^= np.uint64(1 << int(rng.integers(0, height)))
        elif cases[q] == 3:                 # an index >= 2^height, whose low bits still fold to the root
            idx[q] |= np.uint64(1 << int(rng.integers(height, 64)))
        elif cases[q] == 4:                 # a flipped bit of the leaf
            lv[q, rng.integers(0, 8)] ^= np.uint32(1 << int(rng.integers(0, 32)))
    ok = gpu.verify_proofs(lv, idx, sib, root)
    want = np.array([cpu_verify(lv[q], idx[q], sib[q], height, root) for q in range(k)])
    assert (ok == want).all()
    assert ok[cases == 0].all() and ok[cases == 5].all()
    assert not ok[(cases == 1) | (cases == 3) | (cases == 4)].any()
    # a wrong root
    bad_root = root.copy()
    bad_root[3] ^= np.uint32(0x80)
    assert not gpu.verify_proofs(lv, idx, sib, bad_root).any()
    # one root per proof, proofs from several trees of the same height
    roots, lvs, idxs, sibs, trees = [], [], [], [], []
    for n in (3001, 2049, 4096):
        lt = random_leaves(rng, n)
        d_t = gpu.upload(lt)
        tr = gpu.build_tree(d_t, n, height)
        ii = rng.integers(0, n, size=50).astype(np.uint64)
        lvs.append(lt[ii.astype(np.int64)])
        idxs.append(ii)
        sibs.append(tr.proofs(ii))
        roots.append(np.repeat(tr.root()[None], 50, axis=0))
        trees.append((tr, d_t))
    L, I, S, R = (np.concatenate(a) for a in (lvs, idxs, sibs, roots))
    assert gpu.verify_proofs(L, I, S, R).all()
    R2 = np.roll(R, 50, axis=0)              # every proof against another tree's root
    assert not gpu.verify_proofs(L, I, S, R2).any()
    for tr, d_t in trees:
        tr.free()
        d_t.free()
    tree.free()
    d_in.free()


@pytest.fixture(scope="module")
def rndm42_tree(gpu):
    """rndm 42 2^26 127 mapped on the device and its whole tree built (2 GiB of leaves, 2 GiB of tree)."""
    import vk_merkle_roots_amd as vk
    n = 1 << 26
    batch = vk.rndm_packed(42, n, 127)
    d_leaves = gpu.alloc(32 * n)
    step = 1 << 23
    for b0 in range(0, n, step):
        sub = batch.slice(b0, b0 + step)
        d_data, d_meta = gpu.upload(sub.data), gpu.upload(sub.meta)
        gpu.map_async(d_data, sub.words, d_meta, sub.count, d_leaves, out_offset_digests=b0)
        gpu.sync()
        d_data.free()
        d_meta.free()
    del batch
    tree = gpu.build_tree(d_leaves, n)
    yield tree
    tree.free()
    d_leaves.free()


def test_full_size_root_is_the_golden_one(gpu, rndm42_tree):
    from vk_merkle_roots_amd.engine import digest_hex
    big = json.load(open(os.path.join(ROOT, "tests", "golden", "big_roots.json")))
    assert rndm42_tree.count == big["count"]
    assert digest_hex(rndm42_tree.root()) == big["sub_roots"]["42"]["root"]


def test_a_million_proofs_gathered_and_verified_on_one_stream(gpu, rndm42_tree):
    """2^20 random leaves of the 2^26-leaf tree: gather and verify on one non-default stream, no synchronisation between the
    calls; every flag is 1.  Then 1024 tampered proofs: exactly those flags are 0."""
    import vk_merkle_roots_amd as vk
    t = rndm42_tree
    k, height = 1 << 20, t.height
    rng = np.random.default_rng(26)
    idx = rng.integers(0, t.count, size=k, dtype=np.uint64)
    lv = np.ascontiguousarray(t.level(0)[idx.astype(np.int64)])     # the proofs' leaves, picked on the host
    root = t.root()
    s = gpu.new_stream()
    d_idx, d_leaves, d_root = gpu.upload(idx, stream=s), gpu.upload(lv, stream=s), gpu.upload(root, stream=s)
    d_sib = gpu.alloc(32 * k * height)
    d_ok = gpu.alloc(4 * k)
    vk.check(gpu.lib.vkmr_hip_memset_async(gpu.index, s, d_ok.ptr, 0xff, 4 * k), "vkmr_hip_memset_async")
    t.proofs_async(d_idx, k, d_sib, stream=s)
    gpu.verify_proofs_async(d_leaves, d_idx, d_sib, k, height, d_root, 1, d_ok, stream=s)
    ok = gpu.download(d_ok, 4 * k, stream=s)
    assert (ok == 1).all(), int((ok != 1).sum())
    # tamper with 1024 proofs: a sibling bit, the leaf, or the index
    bad = rng.choice(k, size=1024, replace=False)
    sib = gpu.download(d_sib, 32 * k * height, stream=s).reshape(k, height, 8)
    for j, q in enumerate(bad):
        if j % 3 == 0:
            sib[q, rng.integers(0, height), rng.integers(0, 8)] ^= np.uint32(1 << int(rng.integers(0, 32)))
        elif j % 3 == 1:
            lv[q, 0] ^= np.uint32(1)
        else:
            idx[q] ^= np.uint64(1 << int(rng.integers(0, height)))
    d_idx2 = gpu.upload(idx, stream=s)
    d_sib2 = gpu.upload(sib, stream=s)
    d_lv2 = gpu.upload(lv, stream=s)
    gpu.verify_proofs_async(d_lv2, d_idx2, d_sib2, k, height, d_root, 1, d_ok, stream=s)
    ok = gpu.download(d_ok, 4 * k, stream=s)
    want = np.ones(k, dtype=np.uint32)
    want[bad] = 0
    assert (ok == want).all(), (int((ok != want).sum()))
    for b in (d_idx, d_sib, d_leaves, d_root, d_ok, d_idx2, d_sib2, d_lv2):
        b.free()
    gpu.lib.vkmr_hip_stream_destroy(gpu.index, s)


def test_proofs_printed_by_the_front_end_verify_on_the_gpu(native, golden, gpu):
    """`vkmr hip:0` with VKMR_PROOF_INDEX over golden stream G3 in 16 slices of 2^16: the printed leaf and siblings verify
    against the printed root with index = the leaf's index and height = the number of printed levels; the printed sides
    are the index bits."""
    from test_frontend import golden_stream, run_vkmr
    s = golden["streams"]["G3_rndm_42_1048576_127"]
    stream = golden_stream(native, s)
    wanted = [0, 1, 65535, 65536, 131071, 700001, 1048574, 1048575]
    r, out, m = run_vkmr(native, "hip:0", stream, {"VKMR_SLICE_LOG2": "16", "VKMR_PROOF_INDEX": ",".join(map(str, wanted))})
    assert m and m["root"] == s["root"], r.stderr[-300:]
    words = lambda h: np.frombuffer(bytes.fromhex(h), dtype=">u4").astype(np.uint32)
    blocks = []
    for l in (l for l in out if l.startswith("proof: ")):
        if l.startswith("proof: leaf "):
            blocks.append([l])
        else:
            blocks[-1].append(l)
    assert [int(b[0].split()[2]) for b in blocks] == wanted
    leaves, sibs = [], []
    for index, b in zip(wanted, blocks):
        assert len(b) - 1 == 20
        leaves.append(words(b[0].split()[-1]))
        levels = [l.split() for l in b[1:]]
        assert [int(x[2]) for x in levels] == list(range(20))
        assert [x[3] == "sibling-on-left" for x in levels] == [bool((index >> l) & 1) for l in range(20)]
        sibs.append(np.stack([words(x[4]) for x in levels]))
    ok = gpu.verify_proofs(np.stack(leaves), np.array(wanted, dtype=np.uint64), np.stack(sibs), words(s["root"]))
    assert ok.all()
    # the same proofs one position off are refused
    assert not gpu.verify_proofs(np.stack(leaves), np.array(wanted, dtype=np.uint64) ^ np.uint64(1), np.stack(sibs), words(s["root"])).any()


def test_python_tree_of_golden_strings(gpu, golden):
    """merkle_tree_packed on G3 gives the golden root; the proofs of all 2^20 leaves, gathered and verified on the device,
    are all ok."""
    import vk_merkle_roots_amd as vk
    from vk_merkle_roots_amd.engine import digest_hex
    s = golden["streams"]["G3_rndm_42_1048576_127"]
    batch = vk.rndm_packed(42, 1 << 20, 127)
    tree = vk.merkle_tree_packed(gpu, batch)
    assert tree.height == 20
    root = tree.root()
    assert digest_hex(root) == s["root"]
    k = tree.count
    d_idx = gpu.upload(np.arange(k, dtype=np.uint64))
    d_sib = gpu.alloc(32 * k * tree.height)
    d_root = gpu.upload(root)
    d_ok = gpu.alloc(4 * k)
    tree.proofs_async(d_idx, k, d_sib)
    gpu.verify_proofs_async(tree.digests, d_idx, d_sib, k, tree.height, d_root, 1, d_ok)
    assert (gpu.download(d_ok, 4 * k) == 1).all()
    for b in (d_idx, d_sib, d_root, d_ok):
        b.free()
    tree.free()
