"""The case tables of tests/reduce_cases.py reach the regimes of the bulk reduction they are meant to reach -- asked of the
real schedule (csrc/reduce_plan.hpp, through tests/c/reduce_plan_test.cpp --steps), so that a retuned pick_m fails here
and not by a kernel bug slipping through -- and PrefixRoots equals the oracle called directly.  No GPU."""
import numpy as np
import pytest

import reduce_cases as rc


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    return rc.build_plan_exe(tmp_path_factory.mktemp("reduce_plan"))


def ragged(n, m):
    return n % (128 << m) != 0


def test_steps_mode_prints_the_schedule_of_the_header(plan_exe):
    """The --steps mode against schedules read off reduce_plan.hpp by hand (thresholds as committed: a bulk pass from 2048
    wavefronts of 128 nodes, a longer walk while 4096 wavefronts remain, collapse by 7 levels, tail from 128 nodes)."""
    got = rc.schedules(plan_exe, [(1, 1, 1), (128, 1, 9), (129, 1, 8), (1 << 18, 1, 18), (1 << 20, 1, 20), (256, 5, 8)])
    assert got[0] == [("T", 1, 1)]
    assert got[1] == [("T", 9, 1)]
    assert got[2] == [("C", 7, 2), ("T", 1, 1)]
    assert got[3] == [("B", 1, 1 << 17), ("C", 7, 1024), ("C", 7, 8), ("T", 3, 1)]
    assert got[4] == [("B", 2, 1 << 18), ("B", 1, 1 << 17), ("C", 7, 1024), ("C", 7, 8), ("T", 3, 1)]
    assert got[5] == [("C", 7, 2), ("T", 1, 1)]
    assert rc.schedule_name(got[4]) == "B1 B0 C C T"


def test_tables_reach_every_regime(plan_exe):
    # one slice, first pass: B1, B2, B3, each with the edge inside a walk; the base is where its regime begins
    for m in (1, 2, 3):
        base = rc.FIRST_PASS_BASE[m]
        cases = rc.first_pass_cases(m)
        steps = rc.schedules(plan_exe, [(n, 1, h) for n, h in cases])
        hit = [n for (n, h), st in zip(cases, steps) if st[0][:2] == ("B", m + 1) and ragged(n, m)]
        assert len(hit) >= 20, (m, len(hit))
        for (n, h), st in zip(cases, steps):
            if base - 1 <= n <= 2 * base - 2 * (128 << m):
                assert st[0][:2] == ("B", m + 1), (n, h, rc.schedule_name(st))
            assert sum(levels for _, levels, _ in st) == h, (n, h)
        below, at = rc.schedules(plan_exe, [(base - (128 << m), 1, rc.tree_height(base - 1)), (base, 1, rc.tree_height(base))])
        assert below[0][:2] == ("B", m) and at[0][:2] == ("B", m + 1) and base % (4 * (128 << m)) == 0, (m, base)
        # the edge is placed in every chunk of the walk, and one, two and four walks on
        S = 128 << m
        for c in range(1 << m):
            assert any(128 * c < (n - base) % S < 128 * (c + 1) for n in hit), (m, c)
        assert {(n - base) // S for n in hit} >= {0, 1, 2, 4}, m
        if m < 3:      # the top of the regime, and the first count past it
            top, past = rc.schedules(plan_exe, [(2 * base - 2 * S - 1, 1, rc.tree_height(2 * base - 1)), (2 * base - 1, 1, rc.tree_height(2 * base - 1))])
            assert top[0][:2] == ("B", m + 1) and past[0][:2] == ("B", m + 2), m
            assert {2 * base - 2 * S - 1, 2 * base - 1} <= {n for n, _ in cases}, m
        # ... and so do the counts that also get proofs in the pass and the one-level-per-launch variant
        assert set(rc.proof_counts(m)) <= set(hit) and set(rc.levels_variant_counts(m)) <= set(hit), m

    # one slice, second pass: B3 B1 and B3 B2 with a ragged input to the second pass
    for m2 in (1, 2):
        counts = rc.second_pass_counts(m2)
        assert len(counts) >= 12 and max(counts) <= rc.BIG_COUNT
        steps = rc.schedules(plan_exe, [(n, 1, rc.tree_height(n)) for n in counts])
        for n, st in zip(counts, steps):
            assert st[0][:2] == ("B", 4) and st[1][:2] == ("B", m2 + 1), (n, rc.schedule_name(st))
            assert ragged(st[0][2], m2), (n, st[0][2])
            assert st[0][2] - rc.FIRST_PASS_BASE[m2] in rc.edge_offsets(m2), n
        assert {n % 16 for n in counts} == {0, 1}, m2      # both ends of the 16-leaf group behind the last node

    # many slices: B1, B2, B3 first passes, each with lasts shorter than the capacity; one case with a second bulk pass
    # and a collapse (grid.y > 1 throughout), one with no bulk pass at all
    names = {}
    for (cap, nslices), st in zip(rc.SLICE_GEOMETRIES, rc.schedules(plan_exe, [(cap, ns, rc.tree_height(cap)) for cap, ns in rc.SLICE_GEOMETRIES])):
        assert nslices <= rc.SLICES_PER_CHUNK
        assert any(last < cap for last in rc.slice_lasts(cap, nslices))
        names[(cap, nslices)] = rc.schedule_name(st)
    first = {name.split()[0] for name in names.values()}
    assert {"B1", "B2", "B3", "C"} <= first, names
    assert names[(1 << 15, 128)].startswith("B3 B0 C"), names
    assert (1 << 15) - 1000 in rc.slice_lasts(1 << 15, 128)

    # a chunked run whose full chunk and remainder chunk get different kinds of steps
    different = 0
    for cap, nslices, last in rc.CHUNKED_RUNS:
        assert nslices > rc.SLICES_PER_CHUNK and 1 <= last <= cap
        chunks = rc.chunks_of(nslices)
        assert sum(chunks) == nslices and len(chunks) >= 2
        st = rc.schedules(plan_exe, [(cap, ns, rc.tree_height(cap)) for ns in chunks])
        kinds = [[kind for kind, _, _ in s] for s in st]
        different += kinds[0] != kinds[-1]
        assert st[0][0][0] == "B" and st[0][0][1] >= 2, (cap, nslices, rc.schedule_name(st[0]))      # the full chunk walks: m >= 1
    assert different == len(rc.CHUNKED_RUNS)
    assert any(last < cap for cap, _, last in rc.CHUNKED_RUNS)


def test_prefix_roots_equal_the_oracle_called_directly(oracle):
    """The composed value against oracle.reduce_height(leaves[:n], H): n below one block, at k blocks and one to either
    side, across the boundaries of both block sizes, at natural and taller heights (and heights below a block size, where
    the helper has nothing cached to use)."""
    rng = np.random.default_rng(31)
    total = (1 << 13) + 700
    leaves = rng.integers(0, 2**32, size=(total, 8), dtype=np.uint32)
    for blocks in ((4,), (4, 9), (6, 8, 11)):
        pre = rc.PrefixRoots(oracle, leaves, block_log2=blocks, threads=4)
        ns = {1, 2, 3, 5, 15, 16, 17, 31, 33, 63, 64, 65, 100, total - 1, total}
        for B in blocks:
            for k in (1, 2, 3, 5, 8, (total >> B) - 1, total >> B):
                ns |= {(k << B) - 1, k << B, (k << B) + 1, (k << B) + (1 << B) // 2}
        ns |= {int(x) for x in rng.integers(1, total + 1, size=40)}
        checked = 0
        for n in sorted(x for x in ns if 1 <= x <= total):
            h0 = rc.tree_height(n)
            for h in (h0, h0 + 1, h0 + 4, 14, 20):
                if h < h0:
                    continue
                assert (pre.root(n, h) == oracle.reduce_height(leaves[:n], h)).all(), (blocks, n, h)
                checked += 1
        assert checked > 200
    # the default block sizes, across the 2^16 boundary
    leaves = rng.integers(0, 2**32, size=((1 << 17) + 2000, 8), dtype=np.uint32)
    pre = rc.PrefixRoots(oracle, leaves)
    for n in (1, 1023, 1024, 1025, 65535, 65536, 65537, 66560, 66561, 131071, 131072, 131073, (1 << 17) + 1024, (1 << 17) + 1999):
        for h in (rc.tree_height(n), 18, 23):
            if h >= rc.tree_height(n):
                assert (pre.root(n, h) == oracle.reduce_height(leaves[:n], h)).all(), (n, h)
