"""The duplicate-last Merkle tree restated with hashlib, once, and the small helpers every tree, multiproof and forest test
shares.  A plain module: no fixtures, no GPU.  tests/test_merkle_model.py anchors it to the host library's CPU backend.

Level l of a tree over `count` leaves has n_l = ceil(count / 2^l) nodes; node j of level l + 1 is
SHA-256d(L[l][2j] || L[l][min(2j + 1, n_l - 1)]), also above the point where the count has collapsed to one.  The proof of
leaf i is, level by level, L[l][p ^ 1] with p = i >> l, or L[l][p] where p ^ 1 >= n_l."""
import hashlib
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def digest_of(b):
    """SHA-256d of the bytes `b` as 8 words: the leaf digest of a string."""
    return np.frombuffer(hashlib.sha256(hashlib.sha256(b).digest()).digest(), dtype=">u4").astype(np.uint32)


def node(l, r):
    """SHA-256d(l || r) of word-valued digests."""
    return digest_of(np.concatenate([l, r]).astype(">u4").tobytes())


def stored_level_base(total, ntrees, l):
    """The cell of a stored forest's level buffers at which level l >= 1 begins: level j has (total >> j) + ntrees cells
    (include/vkmr_hip.h, STORED FOREST)."""
    return sum((int(total) >> j) + int(ntrees) for j in range(1, l))


def stored_node_cell(total, ntrees, offset, t, l, j):
    """The cell of the level buffers that holds node j of level l (1 <= l < h_t) of tree t, a tree whose leaves begin at cell
    `offset` of level 0."""
    return stored_level_base(total, ntrees, l) + (int(offset) >> l) + int(t) + int(j)


def tree_height(count):
    """max(1, ceil(log2 count)): a lone leaf is still hashed with itself once."""
    return max(1, int(count - 1).bit_length())


def cpu_levels(leaves, height=None):
    """Levels 0 .. height of the tree over `leaves` ([count, 8] uint32, count >= 1), the unpaired last node hashed with
    itself (also once it is alone); height None: tree_height(count), and the last level is the root."""
    levels = [np.asarray(leaves, dtype=np.uint32).reshape(-1, 8)]
    for _ in range(tree_height(levels[0].shape[0]) if height is None else height):
        cur = levels[-1]
        n = cur.shape[0]
        levels.append(np.stack([node(cur[2 * p], cur[min(2 * p + 1, n - 1)]) for p in range((n + 1) // 2)]))
    assert height is not None or levels[-1].shape[0] == 1
    return levels


def sibling_index(p, n):
    """The cell a proof takes beside node p of a level of n cells: p ^ 1, or p itself where p ^ 1 is past the end."""
    return p ^ 1 if (p ^ 1) < n else p


def proof_path(levels, index, height):
    """[height, 8]: the sibling of leaf `index`'s path node at every level -- the node itself where it has none."""
    path = np.zeros((height, 8), dtype=np.uint32)
    for l in range(height):
        path[l] = levels[l][sibling_index(int(index) >> l, levels[l].shape[0])]
    return path


def fold(leaf, index, siblings, height):
    """The root a proof claims: bit l of the index set puts the sibling on the left."""
    cur = np.asarray(leaf, dtype=np.uint32)
    for l in range(int(height)):
        cur = node(siblings[l], cur) if (int(index) >> l) & 1 else node(cur, siblings[l])
    return cur


def host_fold(leaf, index, siblings, height):
    """vkmr_host_cpu_fold_proof."""
    import vk_merkle_roots_amd as vk
    leaf = np.ascontiguousarray(leaf, dtype=np.uint32)
    siblings = np.ascontiguousarray(siblings, dtype=np.uint32)
    out = np.zeros(8, dtype=np.uint32)
    vk.host_lib().vkmr_host_cpu_fold_proof(leaf.ctypes.data, int(index), siblings.ctypes.data, int(height), out.ctypes.data)
    return out


def random_leaves(rng, n):
    """[n, 8] uint32 digests: any bits are a valid digest."""
    return rng.integers(0, 2**32, size=(n, 8), dtype=np.uint32)


class At:
    """A device pointer inside another buffer, for the wrappers that read `.ptr`."""

    def __init__(self, buf, offset):
        self.ptr = buf.at(offset)


def random_counts(rng, budget):
    """Tree sizes of one random forest of at most `budget` leaves: a mix of shapes, empty trees included."""
    ntrees = int(rng.integers(1, 33))
    kind = int(rng.integers(0, 4))
    if kind == 0:
        counts = rng.integers(0, 20, size=ntrees)
    elif kind == 1:
        counts = rng.integers(1, 5000, size=ntrees)
    elif kind == 2:
        counts = (1 << rng.integers(0, 15, size=ntrees)) + rng.integers(-1, 2, size=ntrees)
    else:
        counts = rng.integers(1, 200, size=ntrees)
        counts[int(rng.integers(0, ntrees))] = int(rng.integers(1, budget // 2))
    counts = [int(c) for c in counts]
    while sum(counts) > budget:
        counts.pop()
    return counts


def build_plan_exe(directory, name):
    """tests/c/<name>.cpp (a replay of one of the plan headers under csrc/) compiled into `directory`; its path."""
    exe = os.path.join(str(directory), name)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "vk_merkle_roots_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", name + ".cpp"), "-o", exe])
    return exe


def forests_replay(exe, directory, forests, file_name):
    """One line per (first_offset, slack, max_count, counts) written to `file_name` and replayed by a forest plan program:
    the integers of each answer line; the C test has checked bounds and overlaps on the way."""
    path = os.path.join(str(directory), file_name)
    with open(path, "w") as f:
        for first, slack, max_count, counts in forests:
            f.write(" ".join(str(int(x)) for x in [first, slack, max_count] + list(counts)) + "\n")
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = r.stdout.decode()
    assert r.returncode == 0 and "FAIL" not in text and f"ok: {len(forests)} forests" in text, text[-2000:]
    return [tuple(int(x) for x in line.split()) for line in text.splitlines()[: len(forests)]]
