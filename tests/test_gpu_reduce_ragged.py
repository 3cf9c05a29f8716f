"""The bulk reduction's ragged edges at every walk length, against the oracle.

reduce_pass_kernel has one code path per (m, position of a slice's right edge inside the wavefront's walk of 2^m chunks).
The cases of tests/reduce_cases.py put the edge in every chunk of the walk for m = 1, 2, 3, in the first and in the second
bulk pass, for one slice and for many slices with a short last one, for runs of more than 32768 slices whose chunks get
different schedules, with proofs written in the pass, and for the one-level-per-launch variant at the same counts.  Every
expected value comes from oracle/ (PrefixRoots: the oracle's C code on cached blocks) or hashlib; every failure names
(count, height, schedule).  One big random array is uploaded once and its prefixes are reduced: every load stays inside
the allocation whatever a kernel does at the edge, and the scratch (sized by the ABI's own size functions) is guarded."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import reduce_cases as rc
from merkle_model import sibling_index
from test_gpu_parity import _guarded_scratch
from test_gpu_tree_proofs import cpu_fold, cpu_levels

pytestmark = pytest.mark.gpu

THREADS = min(16, os.cpu_count() or 1)


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    return rc.build_plan_exe(tmp_path_factory.mktemp("reduce_plan"))


class Big:
    pass


@pytest.fixture(scope="module")
def big(gpu, oracle):
    """rc.BIG_COUNT random leaves (about 1.1 GB) on the host and on the device, and the oracle's nodes of their blocks."""
    b = Big()
    b.leaves = np.random.default_rng(70).integers(0, 2**32, size=(rc.BIG_COUNT, 8), dtype=np.uint32)
    b.roots = rc.PrefixRoots(oracle, b.leaves, threads=THREADS)
    b.d_in = gpu.upload(b.leaves)
    yield b
    b.d_in.free()
    del b.leaves, b.roots


def named(plan_exe, n, nslices, height):
    return rc.schedule_name(rc.schedules(plan_exe, [(n, nslices, height)])[0])


def reduce_prefix(gpu, big, n, height, levels_variant=False):
    """Root of the first n leaves of the big array, and whether the guard behind a scratch of exactly the ABI's size held."""
    size = gpu.lib.vkmr_hip_reduce_levels_scratch_bytes if levels_variant else gpu.lib.vkmr_hip_reduce_scratch_bytes
    d_scratch, intact = _guarded_scratch(gpu, size(n))
    d_root = gpu.alloc(32)
    gpu.reduce_async(big.d_in, n, height, d_scratch, d_root, levels_variant=levels_variant)
    got = gpu.download(d_root, 32)
    ok = intact()
    d_scratch.free()
    d_root.free()
    return got, ok


def check_prefixes(gpu, big, plan_exe, cases, levels_variant=False):
    wrong = []
    for n, height in cases:
        got, intact = reduce_prefix(gpu, big, n, height, levels_variant)
        if not intact or not (got == big.roots.root(n, height)).all():
            wrong.append((n, height, named(plan_exe, n, 1, height), "root differs from the oracle" if intact else "wrote behind its scratch"))
    assert not wrong, "%d of %d (count, height, schedule): %s" % (len(wrong), len(cases), wrong[:12])


# ---- (a) first pass, one slice ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", [1, 2, 3])
def test_first_pass_edge_in_every_chunk_of_the_walk(gpu, big, plan_exe, m):
    check_prefixes(gpu, big, plan_exe, rc.first_pass_cases(m))


# ---- (b) second pass, one slice -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("m2", [1, 2])
def test_second_pass_ragged_input(gpu, big, plan_exe, m2):
    """B3 B1 (2^24..2^25 leaves) and B3 B2 (2^25..): the first pass leaves 2^20 + r or 2^21 + r nodes."""
    check_prefixes(gpu, big, plan_exe, [(n, rc.tree_height(n)) for n in rc.second_pass_counts(m2)])


# ---- (c), (d) many slices -----------------------------------------------------------------------------------------------

def slice_roots(oracle, leaves, cap, nslices, height):
    """oracle.reduce_height of every full slice, the calls spread over threads (ctypes releases the GIL)."""
    want = np.zeros((nslices, 8), dtype=np.uint32)

    def run(lo, hi):
        for k in range(lo, hi):
            want[k] = oracle.reduce_height(leaves[k * cap: (k + 1) * cap], height)

    step = max(1, -(-nslices // (THREADS * 4)))
    with ThreadPoolExecutor(THREADS) as pool:
        for f in [pool.submit(run, lo, min(nslices, lo + step)) for lo in range(0, nslices, step)]:
            f.result()
    return want


def check_slices(gpu, oracle, plan_exe, cap, nslices, lasts, seed):
    height = rc.tree_height(cap)
    leaves = np.random.default_rng(seed).integers(0, 2**32, size=(nslices * cap, 8), dtype=np.uint32)
    want = slice_roots(oracle, leaves, cap, nslices, height)
    d_in = gpu.upload(leaves)      # the whole run: a shorter last slice still has real nodes behind its edge
    d_roots = gpu.alloc(32 * nslices)
    name = " | ".join(named(plan_exe, cap, ns, height) for ns in rc.chunks_of(nslices))
    for last in lasts:
        want[nslices - 1] = oracle.reduce_height(leaves[(nslices - 1) * cap: (nslices - 1) * cap + last], height)
        d_scratch, intact = _guarded_scratch(gpu, gpu.lib.vkmr_hip_reduce_slices_scratch_bytes(cap, nslices))
        gpu.reduce_slices_async(d_in, nslices, cap, last, height, d_scratch, d_roots)
        got = gpu.download(d_roots, 32 * nslices).reshape(-1, 8)
        assert intact(), "wrote behind its scratch: capacity %d x %d slices, last %d, height %d, schedule %s" % (cap, nslices, last, height, name)
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, "%d slice roots differ from the oracle (first: slice %d): capacity %d x %d slices, last %d, height %d, schedule %s" % (
            bad.size, bad[0], cap, nslices, last, height, name)
        d_scratch.free()
    d_in.free()
    d_roots.free()


@pytest.mark.parametrize("cap,nslices", rc.SLICE_GEOMETRIES)
def test_many_slices_short_last_slice(gpu, oracle, plan_exe, cap, nslices):
    check_slices(gpu, oracle, plan_exe, cap, nslices, rc.slice_lasts(cap, nslices), seed=71)


@pytest.mark.parametrize("cap,nslices,last", rc.CHUNKED_RUNS)
def test_chunked_runs_with_a_schedule_per_chunk(gpu, oracle, plan_exe, cap, nslices, last):
    """More than 32768 slices: the full chunks run B1 T, the remainder C T, into the same scratch."""
    check_slices(gpu, oracle, plan_exe, cap, nslices, [last], seed=72)


# ---- (e) proofs written in the pass ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", [2, 3])
def test_proofs_written_in_the_pass_at_ragged_edges(gpu, big, plan_exe, m):
    S = 128 << m
    rng = np.random.default_rng(73)
    for n in rc.proof_counts(m):
        height = rc.tree_height(n)
        what = (n, height, named(plan_exe, n, 1, height))
        walk = (n - 1) // S * S                   # first leaf of the last wavefront's walk; its last leaf is n - 1
        idx = [n - 1, n - 2, walk, (n // S - 1) * S, 0]
        idx += [int(x) for x in rng.integers(walk, n, size=3)] + [int(x) for x in rng.integers(0, n, size=16)]
        idx = list(dict.fromkeys(idx))[:16]
        assert len(idx) == 16
        sib, root = gpu.reduce_with_proofs(big.d_in, n, height, idx)
        want_root = big.roots.root(n, height)
        assert (root == want_root).all(), what
        for q, index in enumerate(idx):
            assert (cpu_fold(big.leaves[index], index, sib[q], height) == want_root).all(), what + (index,)
        # the levels inside the walk, where the duplicate-last rule acts: hashlib over the last workgroup's leaves
        w0 = (n - 1) // (4 * S) * (4 * S)
        levels = cpu_levels(big.leaves[w0:n], m + 1)
        edge = [(q, index) for q, index in enumerate(idx) if index >= w0]
        assert len(edge) >= 3      # n - 1, n - 2 and the walk's first leaf at the least
        for q, index in edge:
            for l in range(m + 1):
                s = sibling_index(index >> l, -(-n >> l))
                assert (sib[q][l] == levels[l][s - (w0 >> l)]).all(), what + (index, l)


# ---- (f) one level per launch, at the same counts ---------------------------------------------------------------------------

@pytest.mark.parametrize("m", [1, 2, 3])
def test_levels_variant_equals_the_oracle_at_the_same_counts(gpu, big, plan_exe, m):
    check_prefixes(gpu, big, plan_exe, [(n, rc.tree_height(n)) for n in rc.levels_variant_counts(m)], levels_variant=True)
