"""The integer rules behind the C ABI without a GPU: every recorded result of the twelve size functions
(tests/golden/abi_sizes.json, written by tests/golden/make_abi_sizes.py before the rules moved into the plan headers), and the
rules themselves replayed from the headers by tests/c/abi_plan_test.cpp -- the multiproof scratch layout, the chunks and the
scratch of a run of slices, the stored tree's levels, the map kernel's mode and tile."""
import json
import os
import subprocess

import pytest

import merkle_model

SIZES = os.path.join(merkle_model.ROOT, "tests", "golden", "abi_sizes.json")
BIG_ROOTS = os.path.join(merkle_model.ROOT, "tests", "golden", "big_roots.json")
SIZE_FUNCTIONS = ["vkmr_hip_sizes_scratch_bytes", "vkmr_hip_reduce_scratch_bytes", "vkmr_hip_reduce_slices_scratch_bytes",
                  "vkmr_hip_reduce_levels_scratch_bytes", "vkmr_hip_tree_bytes", "vkmr_hip_multiproof_max_nodes", "vkmr_hip_multiproof_scratch_bytes",
                  "vkmr_hip_forest_scratch_bytes", "vkmr_hip_forest_tree_bytes", "vkmr_hip_forest_multiproof_max_nodes",
                  "vkmr_hip_forest_multiproof_scratch_bytes", "vkmr_hip_find_scratch_bytes"]


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    return merkle_model.build_plan_exe(tmp_path_factory.mktemp("abi_plan"), "abi_plan_test")


def replay(plan_exe, *args):
    r = subprocess.run([plan_exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = r.stdout.decode()
    assert r.returncode == 0 and "FAIL" not in text and f"ok: {args[0]}" in text, text[-2000:]
    return text.splitlines()


@pytest.mark.parametrize("name", SIZE_FUNCTIONS)
def test_the_library_returns_every_recorded_size(native, name):
    from vk_merkle_roots_amd import _abi
    with open(SIZES) as f:
        rows = json.load(f)[name]
    assert len(rows) >= 10
    fn = getattr(_abi.lib(), name)
    wrong = [(row[:-1], row[-1], got) for row in rows for got in [fn(*row[:-1])] if got != row[-1]]
    assert not wrong, (len(wrong), wrong[:5])


def test_the_recording_covers_the_edges_it_is_meant_to():
    """A self-check of the fixture: the counts, heights, k and slice runs at which a rule can turn."""
    with open(SIZES) as f:
        rec = json.load(f)
    assert sum(len(rec[n]) for n in SIZE_FUNCTIONS) >= 3000
    counts = {r[0] for r in rec["vkmr_hip_reduce_scratch_bytes"]}
    assert {0, 1, 2, 127, 128, 129, 2**19 - 1, 2**19 + 1, 2**58, 2**63} <= counts
    assert {0, 1, 63, 64} <= {r[1] for r in rec["vkmr_hip_tree_bytes"]}
    assert {63, 64, 65, 16383, 16384, 16385} <= {r[0] for r in rec["vkmr_hip_multiproof_scratch_bytes"]}
    assert {32767, 32768, 32769, 65536, 65537, 98305} <= {r[1] for r in rec["vkmr_hip_reduce_slices_scratch_bytes"]}


def test_multiproof_layout_parts_in_order_and_the_library_reports_its_bytes(native, plan_exe):
    from vk_merkle_roots_amd import _abi
    rows = [tuple(int(x) for x in line.split()) for line in replay(plan_exe, "layout") if line[:1].isdigit()]
    assert len(rows) == 7 * 5
    for k, height, nbytes in rows:
        assert _abi.lib().vkmr_hip_multiproof_scratch_bytes(k, height) == nbytes, (k, height)


def test_every_chunk_of_a_run_of_slices_fits_the_reported_scratch(plan_exe):
    replay(plan_exe, "slices")


def test_stored_tree_levels_are_the_sums_of_the_levels_below(plan_exe):
    replay(plan_exe, "levels")


def test_map_plan_ladder_tiles_and_the_bench_shape(plan_exe):
    """The mode flips at 32 and 128 words on average and at the count whose per-lane tile reaches 1024; the bench workload,
    `rndm 42 2^26 127`, is staged.  Its packed words are not recorded: a string of b bytes packs into ceil(b / 4) words, so
    they lie between bytes / 4 and (bytes + 3 * items) / 4, and the plan is asked at both ends."""
    with open(BIG_ROOTS) as f:
        stream = json.load(f)["sub_roots"]["42"]
    items, nbytes = stream["items"], stream["bytes"]
    assert items == 1 << 26
    for words, avg in (((nbytes + 3) // 4, 16), ((nbytes + 3 * items) // 4, 17)):
        mode, tile, got_avg = [l for l in replay(plan_exe, "map", words, items) if l.startswith("bench ")][0].split()[1:]
        assert mode == "STAGED" and int(got_avg) == avg and int(tile) % 64 == 0 and 256 <= int(tile) <= 1024, (words, mode, tile, got_avg)
