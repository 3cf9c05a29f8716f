"""Case tables for the ragged-edge tests of the bulk reduction (tests/test_gpu_reduce_ragged.py), the schedule of each
case as the real header gives it (csrc/reduce_plan.hpp through tests/c/reduce_plan_test.cpp --steps), and a cheap
expected value for many prefixes of one big array (PrefixRoots).  A plain module: no fixtures, no GPU.

reduce_pass_kernel walks 2^m chunks of 128 nodes per wavefront; S = 128 << m is a walk, 4 S a workgroup.  A count that is
not a multiple of S puts the slice's right edge INSIDE a walk, where the kernel leans on its guards (`first < n_in`,
`2 * j < ck`, `2 * j + 1 >= ck`, stale registers in lanes without a node).  The tables below place that edge at every chunk
of the walk, for every m, in the first and in the second pass, for one slice and for many.
tests/test_reduce_cases.py checks on the CPU that they still reach those regimes after pick_m is retuned."""
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import merkle_model
from merkle_model import ROOT, tree_height  # noqa: F401


# ---- the schedule, asked of the header ------------------------------------------------------------------------------

def build_plan_exe(directory):
    """tests/c/reduce_plan_test.cpp compiled into `directory` (as tests/test_reduce_plan.py does); its path."""
    return merkle_model.build_plan_exe(directory, "reduce_plan_test")


def schedules(exe, triples):
    """For each (n, nslices, height): the launches of reduce_launch as [(kind, levels, n_out), ...], kind 'B', 'C' or 'T'."""
    triples = [tuple(int(x) for x in t) for t in triples]
    out = []
    for at in range(0, len(triples), 2000):      # keep the command line short
        part = triples[at: at + 2000]
        r = subprocess.run([exe, "--steps"] + [str(x) for t in part for x in t], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
        text = r.stdout.decode()
        assert r.returncode == 0 and "invalid" not in text, text[-2000:]
        got = []
        for line in text.splitlines():
            f = line.split()
            if f[0] == "#":
                got.append((tuple(int(x) for x in f[1:]), []))
            else:
                got[-1][1].append((f[0], int(f[1]), int(f[2])))
        assert [g[0] for g in got] == part
        out += [g[1] for g in got]
    return out


def schedule_name(steps):
    """'B3 B1 C C T': a bulk pass is named with its m = levels - 1."""
    return " ".join("B%d" % (levels - 1) if kind == "B" else kind for kind, levels, _ in steps)


# ---- (a) first pass, one slice ----------------------------------------------------------------------------------------

# The one-slice count from which the first pass walks 2^m chunks, as a multiple of the workgroup's span (the regime begins
# with the 4096th wavefront's first node, S - 1 nodes earlier: base - 1 is already in it, base - S is not).
FIRST_PASS_BASE = {1: 1 << 20, 2: 1 << 21, 3: 1 << 22}


def edge_offsets(m):
    """Where the edge falls, counted from a multiple of the workgroup's span 4 S: just behind it, around every chunk
    boundary of the walk and the middle of every chunk (a lane holds a PAIR: 63, 64, 65 nodes are 31.5, 32, 32.5 lanes --
    the `lane < 32` split of a merge step), and around one, two and four walks."""
    S = 128 << m
    r = {1, 2, 3}
    r |= {128 * c + d for c in range((1 << m) + 1) for d in (-1, 0, 1, 2, 63, 64, 65)}
    r |= {S - 1, S + 1, 2 * S - 1, 2 * S + 1, 4 * S - 1, 4 * S + 1}
    return sorted(r)


def first_pass_counts(m):
    base, S = FIRST_PASS_BASE[m], 128 << m
    counts = [base + r for r in edge_offsets(m)]       # base - 1 (c = 0, d = -1): the last wavefront of 4096 lacks one node
    if m < 3:
        # the top of the regime: the last walk of m that still leaves fewer than 4096 wavefronts for m + 1 ends at
        # 2 base - 2 S; and 2 base - 1, which already walks 2^(m+1) chunks, its edge one node short of a whole walk
        counts += [2 * base - 2 * S - 1, 2 * base - 1]
    return counts


def first_pass_cases(m):
    """(count, height): the natural height for every count, and on every fifth count also natural + 1 and + 5, which run
    the tail's "lone node hashed with itself" trips."""
    cases = []
    for i, n in enumerate(first_pass_counts(m)):
        h = tree_height(n)
        cases.append((n, h))
        if i % 5 == 0:
            cases += [(n, h + 1), (n, h + 5)]
    return cases


# ---- (b) second pass, one slice -----------------------------------------------------------------------------------------

def second_pass_counts(m2):
    """Counts whose first pass (m = 3: 16 leaves per output node) leaves FIRST_PASS_BASE[m2] + r nodes, r from
    edge_offsets(m2): both ends of the 16-leaf group that maps to that last node.  B3 B1 for m2 = 1 (2^24..2^25),
    B3 B2 for m2 = 2 (2^25..)."""
    S = 128 << m2
    counts = []
    for r in (1, 129, S - 1, S + 1, 2 * S + 1, 4 * S - 1):
        assert r in edge_offsets(m2)
        n1 = FIRST_PASS_BASE[m2] + r
        counts += [16 * (n1 - 1) + 1, 16 * n1]
    return counts


BIG_COUNT = max(second_pass_counts(2)) + 1024      # leaves of the one array every one-slice case is a prefix of


# ---- (c) many slices, short last slice --------------------------------------------------------------------------------

SLICE_GEOMETRIES = [      # (capacity, nslices): the schedule is the full slice's; the last slice rides along
    (1024, 4096),         # B3 T
    (1024, 4095),         # B2 T
    (512, 8192),          # B2 T
    (256, 32768),         # B1 T
    (4096, 1024),         # B3 B0 T
    (1 << 15, 128),       # B3 B0 C T
    (256, 5),             # C T
]


def slice_lasts(cap, nslices):
    lasts = {1, 2, 127, 128, 129, cap // 2 - 1, cap // 2 + 1, cap - 1, cap}
    if (cap, nslices) == (1 << 15, 128):
        lasts.add(cap - 1000)      # grid.y > 1 and a last slice long enough for its own B3 B0 ... edge
    return sorted(x for x in lasts if 1 <= x <= cap)


# ---- (d) chunked runs: more than 32768 slices go in chunks of 32768, each with its own schedule ---------------------------

SLICES_PER_CHUNK = 32768
CHUNKED_RUNS = [(256, SLICES_PER_CHUNK + 5, 77), (256, 2 * SLICES_PER_CHUNK + 1, 256)]      # (capacity, nslices, last)


def chunks_of(nslices):
    """The nslices of each reduce_launch vkmr_hip_reduce_slices_async makes."""
    return [min(SLICES_PER_CHUNK, nslices - first) for first in range(0, nslices, SLICES_PER_CHUNK)]


# ---- (e), (f): counts of (a) that also get proofs written in the pass / the one-level-per-launch variant -----------------

def proof_counts(m):
    """Edge in the first chunk of the walk (every later chunk empty) and in the middle of its last chunk."""
    base = FIRST_PASS_BASE[m]
    return [base + 3, base + 128 * ((1 << m) - 1) + 65]


def levels_variant_counts(m):
    base, S = FIRST_PASS_BASE[m], 128 << m
    return [base + 1, base + S + 1, base + 128 * ((1 << m) - 1) + 63]


# ---- expected roots of many prefixes of one array ---------------------------------------------------------------------

class PrefixRoots:
    """Roots of prefixes leaves[:n] of one big array without hashing the prefix again for every n.

    Level-B node q of the tree over the first n leaves is reduce_height(leaves[q << B : min(n, (q + 1) << B)], B): it does
    not depend on n while its block is complete.  So the level-B nodes of the complete blocks are computed once (for
    each B of `block_log2`, ascending, each level from the one below), and the root of a prefix at height H >= B is
    reduce_height(cached[: n >> B] + [the partial block's node], H - B).  Every hash is made by the oracle's C code
    (conftest.Oracle.reduce_height, spread over threads: ctypes releases the GIL); this class only slices and stacks."""

    def __init__(self, oracle, leaves, block_log2=(10, 16), threads=None):
        self.oracle = oracle
        self.levels = [(0, np.ascontiguousarray(leaves, dtype=np.uint32).reshape(-1, 8))]
        threads = threads or min(16, os.cpu_count() or 1)
        for B in block_log2:
            b, below = self.levels[-1]
            assert B > b
            width = 1 << (B - b)
            nblocks = below.shape[0] // width
            nodes = np.zeros((nblocks, 8), dtype=np.uint32)

            def run(lo, hi, below=below, width=width, nodes=nodes, up=B - b):
                for q in range(lo, hi):
                    nodes[q] = oracle.reduce_height(below[q * width: (q + 1) * width], up)

            step = max(1, -(-nblocks // (threads * 8)))
            with ThreadPoolExecutor(threads) as pool:
                for f in [pool.submit(run, lo, min(nblocks, lo + step)) for lo in range(0, nblocks, step)]:
                    f.result()
            self.levels.append((B, nodes))

    def _nodes(self, lo, n, i):
        """Level-B_i nodes of the tree over leaves[:n] that cover leaves[lo:n]; lo is a multiple of every block size."""
        B, cached = self.levels[i]
        if i == 0:
            return cached[lo:n]
        full = n >> B
        out = [cached[lo >> B: full]]
        if n > full << B:
            b = self.levels[i - 1][0]
            out.append(self.oracle.reduce_height(self._nodes(full << B, n, i - 1), B - b)[None, :])
        return np.concatenate(out)

    def root(self, n, height):
        """oracle.reduce_height(leaves[:n], height)."""
        assert 1 <= n <= self.levels[0][1].shape[0] and -(-n >> height) == 1
        i = max(k for k, (B, _) in enumerate(self.levels) if B <= height)
        return self.oracle.reduce_height(self._nodes(0, n, i), height - self.levels[i][0])
