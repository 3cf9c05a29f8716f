"""Multiproofs of a duplicate-last tree restated with hashlib, and the case tables of tests/test_multiproof_abi.py and
tests/test_gpu_multiproof.py: the definition that vkmr_hip_tree_multiproof_async, vkmr_hip_verify_multiproof_async and
vkmr_host_cpu_verify_multiproof are checked against (include/vkmr_hip.h states the same contract in words).  A plain module.

Tree: level l has n_l = ceil(count / 2^l) nodes, node j of level l + 1 = SHA-256d(L[l][2j] || L[l][min(2j + 1, n_l - 1)]),
also above the point where the count has collapsed to one.  A_0 = the proved indices, A_{l+1} = unique(A_l >> 1).  For
l = 0 .. height - 1 and p in A_l ascending: nothing when p ^ 1 is in A_l, else ONE node, L[l][p ^ 1], or L[l][p] where
p ^ 1 >= n_l.  The verifier needs no count: which children are known follows from the indices alone."""
import numpy as np

from merkle_model import cpu_levels, node, random_leaves, tree_height  # noqa: F401  (the tests reach them through this module)

COUNTS = [1, 2, 3, 5, 8, 9, 127, 128, 129, 1000]


def emitted_positions(count, height, indices):
    """([(l, cell)] of the multiproof's nodes in order, the per-level counts).  No hashing."""
    cur = sorted(set(int(i) for i in indices))
    out, counts = [], []
    for l in range(height):
        n = -(-count >> l)
        have = set(cur)
        m = 0
        for p in cur:
            if p ^ 1 in have:
                continue
            out.append((l, p ^ 1 if p ^ 1 < n else p))
            m += 1
        counts.append(m)
        cur = sorted(set(p >> 1 for p in cur))
    return out, counts


def make_multiproof(level_of, count, height, indices):
    """(nodes [M, 8] uint32, counts [height]): level_of(l) returns the [n_l, 8] cells of level l."""
    pos, counts = emitted_positions(count, height, indices)
    cache = {}
    nodes = np.zeros((len(pos), 8), dtype=np.uint32)
    for i, (l, c) in enumerate(pos):
        if l not in cache:
            cache[l] = level_of(l)
        nodes[i] = cache[l][c]
    return nodes, counts


def verify_multiproof(leaves, indices, height, nodes, root):
    """The acceptance rule: indices strictly increasing and < 2^height, exactly len(nodes) nodes consumed, the fold equals root."""
    idx = [int(i) for i in indices]
    if not idx or len(leaves) != len(idx):
        return False
    if any(b <= a for a, b in zip(idx, idx[1:])) or idx[-1] >= (1 << height):
        return False
    cur = {p: np.asarray(v, dtype=np.uint32) for p, v in zip(idx, leaves)}
    used = 0
    for _ in range(height):
        nxt = {}
        for P in sorted(set(p >> 1 for p in cur)):
            kids = []
            for c in (2 * P, 2 * P + 1):
                if c in cur:
                    kids.append(cur[c])
                else:
                    if used >= len(nodes):
                        return False
                    kids.append(np.asarray(nodes[used], dtype=np.uint32))
                    used += 1
            nxt[P] = node(kids[0], kids[1])
        cur = nxt
    return used == len(nodes) and bool((cur[0] == np.asarray(root, dtype=np.uint32)).all())


def max_nodes(count, height, k):
    """The buffer bound: at most one node per pair of a level."""
    return sum(min(k, -(-count >> (l + 1))) for l in range(height))


def small_index_sets(count, rng):
    """k in {1, 2, 7, count} (capped at count), random, sorted, unique."""
    return [sorted(int(x) for x in rng.choice(count, size=min(k, count), replace=False)) for k in (1, 2, 7, count)]


def mutations(leaves, indices, nodes, height, rng):
    """[(name, leaves, indices, nodes)], each of which must be rejected; one that needs what the proof lacks (a node of an
    empty proof, a second index) is left out."""
    leaves, idx = np.array(leaves, dtype=np.uint32).reshape(-1, 8), np.array(indices, dtype=np.uint64)
    nodes = np.array(nodes, dtype=np.uint32).reshape(-1, 8)
    out = []
    if nodes.shape[0]:
        z = nodes.copy()
        z[int(rng.integers(0, nodes.shape[0]))] = 0
        out.append(("node zeroed", leaves, idx, z))
        out.append(("last node dropped", leaves, idx, nodes[:-1].copy()))
    out.append(("node appended", leaves, idx, np.concatenate([nodes, random_leaves(rng, 1)])))
    c = leaves.copy()
    c[int(rng.integers(0, c.shape[0])), 0] ^= np.uint32(1)
    out.append(("leaf changed", c, idx, nodes))
    if idx.shape[0] >= 2:
        s = idx.copy()
        a = int(rng.integers(0, s.shape[0] - 1))
        s[a], s[a + 1] = s[a + 1], s[a]
        out.append(("indices swapped", leaves, s, nodes))
    o = idx.copy()
    o[-1] = np.uint64((1 << height) + int(o[-1]))
    out.append(("index >= 2^height", leaves, o, nodes))
    return out


def host_verify(leaves, indices, height, nodes, root):
    """vkmr_host_cpu_verify_multiproof on host arrays: bool."""
    import vk_merkle_roots_amd as vk
    leaves = np.ascontiguousarray(leaves, dtype=np.uint32).reshape(-1, 8)
    idx = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
    nodes = np.ascontiguousarray(nodes, dtype=np.uint32).reshape(-1, 8)
    root = np.ascontiguousarray(root, dtype=np.uint32).reshape(8)
    r = vk.host_lib().vkmr_host_cpu_verify_multiproof(leaves.ctypes.data, idx.ctypes.data, idx.shape[0], height,
                                                      nodes.ctypes.data if nodes.shape[0] else None, nodes.shape[0], root.ctypes.data)
    assert r in (0, 1)
    return r == 1
