"""Partial Merkle trees in BIP37 order (vkmr_hip_forest_merkleblocks_async, vkmr_hip_tree_merkleblock_async,
vkmr_host_cpu_forest_merkleblocks, vkmr_host_cpu_merkleblock_extract, MerkleForest.merkleblocks): the recursive rule restated in
Python over hashlib level lists (walk, model), the receiver's side restated (extract: Bitcoin Core's TraverseAndExtract under the
project's height), the drivers of the CPU twin and of the replay (tests/c/merkleblock_plan_test.cpp) that
tests/test_merkleblock_abi.py (no GPU) and tests/test_gpu_merkleblocks.py share.  A plain module: no fixtures, no GPU.

A tree of c >= 1 leaves: h = max(1, ceil(log2 c)), w(l) = ceil(c / 2^l).  visit(l, p): flag f = (p in A_l); a hash when l == 0 or
not f; else visit(l - 1, 2p) and, if 2p + 1 < w(l - 1), visit(l - 1, 2p + 1).  Flag i is bit i & 7 of byte i >> 3."""
import os
import subprocess

import numpy as np

from consistency_cases import Forest, square, square_counts  # noqa: F401
from merkle_model import ROOT, build_plan_exe, node, tree_height

CANARY32, CANARY64, CANARY8 = 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5, 0xA5
EXTRACT_REFUSALS = {"null pointer": -1, "count == 0": -2, "more hashes than leaves": -3, "fewer flag bits than hashes": -4,
                    "read past the end": -5, "hashes left over": -6, "flag bytes left over": -7, "equal children": -8}


def width(c, l):
    return (c + (1 << l) - 1) >> l


def walk(c, matched):
    """(flags [0/1], [(l, p)] of the hash-carrying nodes in order) of a tree of c leaves: the recursive rule, no hashing."""
    h = tree_height(c)
    A = [set(int(i) for i in matched)]
    for _ in range(h):
        A.append({p >> 1 for p in A[-1]})
    flags, cells = [], []

    def visit(l, p):
        f = p in A[l]
        flags.append(1 if f else 0)
        if l == 0 or not f:
            cells.append((l, p))
            return
        visit(l - 1, 2 * p)
        if 2 * p + 1 < width(c, l - 1):
            visit(l - 1, 2 * p + 1)

    visit(h, 0)
    return flags, cells


def pack(flags):
    out = bytearray((len(flags) + 7) // 8)
    for i, f in enumerate(flags):
        out[i >> 3] |= f << (i & 7)
    return bytes(out)


def by_tree(trees, indices):
    out = {}
    for t, i in zip(trees, indices):
        out.setdefault(int(t), []).append(int(i))
    return {t: sorted(set(out[t])) for t in sorted(out)}


def model(forest, trees, indices):
    """The eight outputs and info of sorted in-range entries over a consistency_cases.Forest:
    (block_trees, block_counts, bit_counts, hash_starts, byte_starts, hashes [N, 8], flags uint8 [bytes], info [4])."""
    groups = by_tree(trees, indices)
    bt, bc, bits, hs, bs, hashes, flags = [], [], [], [0], [0], [], bytearray()
    for t, idx in groups.items():
        c = forest.counts[t]
        f, cells = walk(c, idx)
        levels = forest.levels(t)
        bt.append(t)
        bc.append(c)
        bits.append(len(f))
        hashes += [levels[l][p] for l, p in cells]
        flags += pack(f)
        hs.append(len(hashes))
        bs.append(len(flags))
    return (np.array(bt, np.uint32), np.array(bc, np.uint64), np.array(bits, np.uint64), np.array(hs, np.uint64), np.array(bs, np.uint64),
            np.stack(hashes).astype(np.uint32) if hashes else np.zeros((0, 8), np.uint32), np.frombuffer(bytes(flags), np.uint8).copy(),
            np.array([0, len(bt), len(hashes), len(flags)], np.uint64))


def extract(c, hashes, flag_bytes):
    """The receiver's side restated: (code, root, indices, leaves); code 0 or one of EXTRACT_REFUSALS' values."""
    R = EXTRACT_REFUSALS
    hashes = [np.asarray(x, np.uint32) for x in hashes]
    nbits = 8 * len(flag_bytes)
    if c == 0:
        return R["count == 0"], None, None, None
    if len(hashes) > c:
        return R["more hashes than leaves"], None, None, None
    if nbits < len(hashes):
        return R["fewer flag bits than hashes"], None, None, None
    state = {"bit": 0, "hash": 0, "bad": 0}
    idx, leaves = [], []

    def visit(l, p):
        if state["bad"]:
            return None
        if state["bit"] >= nbits:
            state["bad"] = R["read past the end"]
            return None
        f = (flag_bytes[state["bit"] >> 3] >> (state["bit"] & 7)) & 1
        state["bit"] += 1
        if l == 0 or not f:
            if state["hash"] >= len(hashes):
                state["bad"] = R["read past the end"]
                return None
            x = hashes[state["hash"]]
            state["hash"] += 1
            if l == 0 and f:
                idx.append(p)
                leaves.append(x)
            return x
        left = visit(l - 1, 2 * p)
        right = left
        if 2 * p + 1 < width(c, l - 1):
            right = visit(l - 1, 2 * p + 1)
            if not state["bad"] and (left == right).all():
                state["bad"] = R["equal children"]
        if state["bad"]:
            return None
        return node(left, right)

    root = visit(tree_height(c), 0)
    if state["bad"]:
        return state["bad"], None, None, None
    if state["hash"] != len(hashes):
        return R["hashes left over"], None, None, None
    if (state["bit"] + 7) // 8 != len(flag_bytes):
        return R["flag bytes left over"], None, None, None
    return 0, root, idx, leaves


# ---- the shapes ------------------------------------------------------------------------------------------------------------------
def sorted_entries(pairs):
    pairs = sorted(set((int(t), int(i)) for t, i in pairs))
    return np.array([t for t, _ in pairs], dtype=np.uint32), np.array([i for _, i in pairs], dtype=np.uint64)


def every_leaf(counts):
    return sorted_entries((t, i) for t, c in enumerate(counts) for i in range(c))


def random_entries(counts, rng, share):
    """Each leaf with probability `share`; at least one entry."""
    pairs = [(t, i) for t, c in enumerate(counts) for i in range(c) if rng.random() < share]
    if not pairs:
        pairs = [(next(t for t, c in enumerate(counts) if c), 0)]
    return sorted_entries(pairs)


def single_leaf_batches(counts):
    """Batch j names leaf j of every tree that has one: every single leaf of every tree, each alone in its tree."""
    return [sorted_entries((t, j) for t, c in enumerate(counts) if j < c) for j in range(max(counts))]


# ---- the CPU twin (libvkmr_host.so) ----------------------------------------------------------------------------------------------
def host_merkleblocks(leaves, offsets, trees, indices, hash_capacity=None, flag_capacity=None, slack=5):
    """(return code, the eight outputs as the device call gives them -- whole buffers with their canaries --, info [4]) of
    vkmr_host_cpu_forest_merkleblocks.  The capacities default to a generous bound; `slack` cells of canary lie behind them."""
    import vk_merkle_roots_amd as vk
    leaves = np.ascontiguousarray(leaves, dtype=np.uint32).reshape(-1, 8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    trees, indices = np.ascontiguousarray(trees, dtype=np.uint32), np.ascontiguousarray(indices, dtype=np.uint64)
    k, ntrees = int(trees.shape[0]), int(offsets.shape[0]) - 1
    if hash_capacity is None:
        hash_capacity = k * 66
    if flag_capacity is None:
        flag_capacity = k * 26
    out = fresh_outputs(k, hash_capacity, flag_capacity, slack)
    rc = vk.host_lib().vkmr_host_cpu_forest_merkleblocks(leaves.ctypes.data if leaves.size else None, offsets.ctypes.data, ntrees, trees.ctypes.data,
                                                         indices.ctypes.data, k, *(a.ctypes.data for a in out[:5]), out[5].ctypes.data, hash_capacity,
                                                         out[6].ctypes.data, flag_capacity, out[7].ctypes.data)
    return rc, out


def fresh_outputs(k, hash_capacity, flag_capacity, slack=5):
    """The eight outputs and info, all canary: the per-block arrays with room for k (+ 1) entries, `slack` more behind each."""
    return [np.full(k + slack, CANARY32, np.uint32), np.full(k + slack, CANARY64, np.uint64), np.full(k + slack, CANARY64, np.uint64),
            np.full(k + 1 + slack, CANARY64, np.uint64), np.full(k + 1 + slack, CANARY64, np.uint64),
            np.full((hash_capacity + slack, 8), CANARY32, np.uint32), np.full(flag_capacity + slack, CANARY8, np.uint8), np.full(4 + slack, CANARY64, np.uint64)]


def assert_outputs(out, want, what=""):
    """`out` (whole buffers) holds the model's outputs `want`, and canary behind them."""
    names = ("block_trees", "block_counts", "bit_counts", "hash_starts", "byte_starts", "hashes", "flags", "info")
    fills = (CANARY32, CANARY64, CANARY64, CANARY64, CANARY64, CANARY32, CANARY8, CANARY64)
    for name, got, exp, fill in zip(names, out, want, fills):
        n = exp.shape[0]
        assert (got[:n] == exp).all(), (what, name, np.nonzero((got[:n] != exp).reshape(n, -1).any(axis=1))[0][:8], got[:n][:12], exp[:12])
        assert (got[n:] == fill).all(), (what, name, "written behind its end")


def assert_untouched(out, upto=None):
    """Nothing (or nothing but the arrays in `upto`) was written."""
    fills = (CANARY32, CANARY64, CANARY64, CANARY64, CANARY64, CANARY32, CANARY8, CANARY64)
    for i, (a, fill) in enumerate(zip(out, fills)):
        if upto is None or i in upto:
            assert (a == fill).all(), i


def host_extract(count, hashes, flag_bytes, room=None):
    """(code, root [8], indices uint64 [n], leaves [n, 8]) of vkmr_host_cpu_merkleblock_extract; on a refusal the outputs are
    checked to be untouched and come back as None."""
    import vk_merkle_roots_amd as vk
    hashes = np.ascontiguousarray(hashes, dtype=np.uint32).reshape(-1, 8)
    flag_bytes = np.frombuffer(bytes(flag_bytes), np.uint8).copy()
    n = hashes.shape[0]
    room = max(n, 1) if room is None else room
    root, idx, leaves, nm = np.full(8, CANARY32, np.uint32), np.full(room, CANARY64, np.uint64), np.full((room, 8), CANARY32, np.uint32), np.full(1, CANARY64, np.uint64)
    rc = vk.host_lib().vkmr_host_cpu_merkleblock_extract(int(count), hashes.ctypes.data if n else None, n, flag_bytes.ctypes.data if flag_bytes.size else None,
                                                         int(flag_bytes.shape[0]), root.ctypes.data, idx.ctypes.data, leaves.ctypes.data, nm.ctypes.data)
    if rc != 0:
        assert (root == CANARY32).all() and (idx == CANARY64).all() and (leaves == CANARY32).all() and nm[0] == CANARY64
        return rc, None, None, None
    m = int(nm[0])
    assert (idx[m:] == CANARY64).all() and (leaves[m:] == CANARY32).all()
    return rc, root, idx[:m], leaves[:m]


# ---- the replay ------------------------------------------------------------------------------------------------------------------
def build_merkleblock_plan_exe(directory, sanitize=True):
    """tests/c/merkleblock_plan_test.cpp as a program of its own, by default with AddressSanitizer and UBSan."""
    if not sanitize:
        return build_plan_exe(directory, "merkleblock_plan_test")
    exe = os.path.join(str(directory), "merkleblock_plan_test_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "vk_merkle_roots_amd", "csrc"), os.path.join(ROOT, "tests", "c", "merkleblock_plan_test.cpp"), "-o", exe])
    return exe


def plan_replay(exe, directory, cases, name="merkleblock_cases.txt"):
    """One line per (max_count, counts, [(tree, index), ..] sorted) through tests/c/merkleblock_plan_test.cpp: per case (blocks,
    flags, hashes, flag bytes); the C program has compared every position with its own recursive walk and every total with the
    three bounds on the way."""
    path = os.path.join(str(directory), name)
    with open(path, "w") as f:
        for max_count, counts, entries in cases:
            words = [max_count, len(counts)] + list(counts) + [len(entries)] + [v for e in entries for v in e]
            f.write(" ".join(str(int(x)) for x in words) + "\n")
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    text = r.stdout.decode()
    assert r.returncode == 0 and "FAIL" not in text and f"ok: {len(cases)} cases" in text, text[-2000:]
    return [tuple(int(x) for x in line.split()) for line in text.splitlines()[: len(cases)]]


def expect(counts, entries):
    """(blocks, flags, hashes, flag bytes) of a case from the recursive rule."""
    groups = by_tree([t for t, _ in entries], [i for _, i in entries])
    walks = [walk(counts[t], idx) for t, idx in groups.items()]
    return len(walks), sum(len(f) for f, _ in walks), sum(len(c) for _, c in walks), sum((len(f) + 7) // 8 for f, _ in walks)
