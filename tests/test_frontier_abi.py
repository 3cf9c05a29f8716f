"""Frontiers without a GPU: the C ABI's declarations and argument checks (vkmr_hip_frontier_extend_async and its neighbours), the
rules of csrc/frontier_plan.hpp replayed on the CPU with frontier_level_kernel's own tests (tests/c/frontier_plan_test.cpp), the
CPU twins (vkmr_host_cpu_frontier_extend, _frontier_roots, _forest_frontier) against the hashlib model of tests/frontier_cases.py,
and the host-side checks of vk.Frontier.  No compute call on a device here."""
import ctypes as C

import numpy as np
import pytest

import frontier_cases as fr
from abi_support import Refusals, assert_bound, assert_exported, assert_key_resolves, assert_no_spills, isa_record
from merkle_model import random_leaves
from no_device import NoDevice

ENTRY_POINTS = {"vkmr_hip_forest_frontier_async": 12, "vkmr_hip_frontier_roots_async": 7, "vkmr_hip_verify_frontier_async": 8,
                "vkmr_hip_frontier_extend_scratch_bytes": 2, "vkmr_hip_frontier_extend_async": 15}
HOST_ENTRY_POINTS = ("vkmr_host_cpu_frontier_roots", "vkmr_host_cpu_frontier_extend", "vkmr_host_cpu_forest_frontier")
HASHING = ("frontier_level_kernel", "frontier_roots_kernel")
KERNELS = ("frontier_check_kernel", "frontier_commit_kernel", "frontier_gather_kernel") + HASHING
EXTEND = "vkmr_hip_frontier_extend_async"


def test_header_declares_them_and_the_stub_binds_every_argument():
    for name, nparams in ENTRY_POINTS.items():
        assert_bound(name, nparams=nparams, restype=C.c_size_t if name.endswith("_bytes") else C.c_int)


def test_libraries_export_them(native):
    assert_exported(native.HIP_LIB, ENTRY_POINTS)
    assert_exported(native.HOST_LIB, HOST_ENTRY_POINTS)


def test_bad_arguments_are_refused_before_any_hip_call(native):
    from vk_merkle_roots_amd import _abi
    lib = _abi.lib()
    d = C.c_void_p(0x1000)                 # never dereferenced: every call below returns before launching anything
    # counts, peaks, stride, T, leaves, total_new, offsets, max_new, scratch, new_counts, new_peaks, roots, status
    extend = Refusals(lib.vkmr_hip_frontier_extend_async, EXTEND, good=[d, d, 8, 3, d, 6, d, 4, d, d, d, d, d])
    extend.null(0, 1, 4, 6, 8, 9, 10, 11, 12)
    extend.changed({2: 0}, {2: 65}, {5: (1 << 58) + 1}, {8: C.c_void_p(0x1008)})
    extend.ok((None, None, 0, 0, None, 0, None, 0, None, None, None, None, None))       # no tree
    # the root walk and the verifier: counts, peaks, stride, T, roots (, ok)
    roots = Refusals(lib.vkmr_hip_frontier_roots_async, "vkmr_hip_frontier_roots_async", good=[d, d, 8, 3, d])
    verify = Refusals(lib.vkmr_hip_verify_frontier_async, "vkmr_hip_verify_frontier_async", good=[d, d, 8, 3, d, d])
    roots.null(0, 1, 4)
    verify.null(0, 1, 4, 5)
    roots.changed({2: 0}, {2: 65})
    verify.changed({2: 0}, {2: 65})
    roots.ok((None, None, 0, 0, None))
    verify.ok((None, None, 0, 0, None, None))
    # the gather: digests, forest, total, offsets, ntrees, max_count, roots, stride, counts_out, peaks_out
    gather = Refusals(lib.vkmr_hip_forest_frontier_async, "vkmr_hip_forest_frontier_async", good=[d, d, 100, d, 8, 50, d, 6, d, d])
    gather.null(0, 1, 3, 6, 8, 9)
    gather.changed({7: 0}, {7: 65}, {7: 5}, {5: 0}, {2: (1 << 58) + 1})           # stride 5: a tree of 50 leaves has six bits
    gather.ok((None, None, 0, None, 0, 0, None, 0, None, None))


def test_the_scratch_budget(native):
    from vk_merkle_roots_amd import _abi
    lib = _abi.lib()
    for total_new, T in ((0, 1), (1, 1), (6, 3), (33000, 1681), (1 << 26, 1), (1 << 16, 1 << 15)):
        assert lib.vkmr_hip_frontier_extend_scratch_bytes(total_new, T) == 32 * (2 * ((total_new >> 1) + 2 * T) + 64 * T)
    assert lib.vkmr_hip_frontier_extend_scratch_bytes(5, 0) == 0 and lib.vkmr_hip_frontier_extend_scratch_bytes((1 << 58) + 1, 1) == 0


# ---- the replay of the launches ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    return fr.build_frontier_plan_exe(tmp_path_factory.mktemp("frontier_plan"))


def check_replay(native, plan_exe, directory, batches):
    from vk_merkle_roots_amd import _abi
    lib = _abi.lib()
    got = fr.plan_replay(plan_exe, directory, batches)
    for (stride, pairs), (launches, touched, hashes, lanes) in zip(batches, got):
        total_new, T = sum(n for _, n in pairs), len(pairs)
        assert launches == min(stride, 58)
        assert 32 * touched <= lib.vkmr_hip_frontier_extend_scratch_bytes(total_new, T), pairs     # what the library reports covers the last cell
        assert hashes <= sum((n >> l) + 2 for _, n in pairs for l in range(1, launches + 1))
        assert lanes <= sum(sum((n >> l) + 2 for _, n in pairs) + 63 for l in range(1, launches + 1))


def test_every_pair_up_to_130_replayed(native, plan_exe, tmp_path):
    batches = [((c + n).bit_length() or 1, [(c, n)]) for c in range(131) for n in range(131)]                 # each alone, the tightest stride
    for n in range(131):                                                                                      # and side by side: T = 32, 32, 32, 32, 3
        batches += [(9 + n % 3, [(c, n) for c in range(lo, min(lo + 32, 131))]) for lo in range(0, 131, 32)]
    check_replay(native, plan_exe, tmp_path, batches)


def test_a_thousand_random_batches_replayed(native, plan_exe, tmp_path):
    rng = np.random.default_rng(20263)
    batches = []
    while len(batches) < 1000:
        T = int(rng.integers(1, 33))
        top_c, top_n = ((5000, 3000), (300, 300), (20, 5))[len(batches) % 3]
        pairs = [(int(rng.integers(0, top_c)) * int(rng.integers(0, 4) > 0), int(rng.integers(0, top_n)) * int(rng.integers(0, 4) > 0)) for _ in range(T)]
        if len(batches) % 5 == 0:
            pairs = [(1 << int(rng.integers(0, 12)), n) for _, n in pairs]                                    # powers of two: the peak that is the root
        batches.append((int(rng.integers(max((c + n).bit_length() for c, n in pairs) or 1, 65)), pairs))
    check_replay(native, plan_exe, tmp_path, batches)


# ---- the CPU twins against the model -------------------------------------------------------------------------------------------------
def check_twin(batch):
    status, counts, peaks, roots = fr.host_extend(batch.counts, batch.peaks, batch.leaves, batch.offsets)
    assert status == 0
    assert (counts == batch.want_counts).all() and (peaks == batch.want_peaks).all() and (roots == batch.want_roots).all()
    in_place = fr.host_extend(batch.counts, batch.peaks, batch.leaves, batch.offsets, in_place=True)
    assert in_place[0] == 0 and all((a == b).all() for a, b in zip(in_place[1:], (counts, peaks, roots)))
    rc, again = fr.host_roots(counts, peaks)
    assert rc == 0 and (again == roots).all()


def test_every_pair_up_to_40_in_one_batched_call(native):
    batch = fr.square()
    assert batch.T == 1681 and 32000 < batch.leaves.shape[0] < 34000
    check_twin(batch)


def test_counts_around_the_wavefront_edges(native):
    check_twin(fr.edges())


def test_a_tree_of_two_to_the_forty_leaves_whose_peaks_are_random_digests(native):
    batch = fr.big()
    assert int(batch.counts[0]) == (1 << 40) + (1 << 33) + 7 and batch.new_counts[0] == 70
    check_twin(batch)
    rc, roots = fr.host_roots(batch.counts, batch.peaks)            # and the old root from the old frontier by the first rule
    assert rc == 0 and (roots[0] == fr.model_root(int(batch.counts[0]), batch.peaks[0])).all()


def test_the_frontier_of_a_forest_from_its_leaves(native):
    rng = np.random.default_rng(321)
    counts = [0, 1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 127, 128, 129, 0, 1000]
    leaves = random_leaves(rng, sum(counts))
    rc, got_counts, got_peaks = fr.host_forest_frontier(leaves, counts)
    assert rc == 0 and got_counts.tolist() == counts
    at = 0
    for q, c in enumerate(counts):
        assert (got_peaks[q] == fr.brute_frontier(leaves[at: at + c])[0]).all(), c
        at += c
    assert fr.host_forest_frontier(leaves, counts, stride=9)[0] == 1                     # 1 000 leaves: ten bits
    assert (fr.host_forest_frontier(leaves, counts, stride=9)[2] == fr.CANARY).all()


@pytest.mark.parametrize("what,status,counts,offsets,max_new,stride", fr.REFUSALS, ids=[r[0] for r in fr.REFUSALS])
def test_a_refused_extend_writes_nothing(native, what, status, counts, offsets, max_new, stride):
    old_counts, old_peaks, leaves = fr.refusal_frontier(counts, stride)
    got = fr.host_extend(old_counts, old_peaks, leaves, offsets, max_new=max_new, total_new=6)
    assert got[0] == status, what
    assert (got[1] == 0xA5A5A5A5A5A5A5A5).all() and (got[2] == fr.CANARY).all() and (got[3] == fr.CANARY).all()
    # and the same batch with the fault taken out goes through
    fine = fr.host_extend([3, 4, 5], fr.refusal_frontier([3, 4, 5], 8)[1], leaves, [0, 1, 4, 6], max_new=4, total_new=6)
    assert fine[0] == 0 and fine[1].tolist() == [4, 7, 7]


def test_a_count_the_frontier_cannot_hold_gives_the_zero_root(native):
    counts, peaks, _ = fr.refusal_frontier([5, 300, (1 << 58) + 1], 8)
    rc, roots = fr.host_roots(counts, peaks)
    assert rc == 1 and roots[0].any() and not roots[1:].any()


# ---- the Python layer ------------------------------------------------------------------------------------------------------------------
def test_frontier_refuses_on_the_host(native):
    import vk_merkle_roots_amd as vk
    f = vk.Frontier.empty(3, stride=4)
    assert f.T == 3 and f.stride == 4 and f.counts.tolist() == [0, 0, 0] and not f.peaks.any() and f.peaks.shape == (3, 4, 8)
    assert f.same_as(vk.Frontier.empty(3, 4)) and not f.same_as(vk.Frontier.empty(3, 5))
    for digests, counts in ((np.zeros((4, 8), np.uint32), [1, 1, 1]),          # do not add up
                            (np.zeros((4, 8), np.uint32), [2, 2]),             # not one per tree
                            (np.zeros((16, 8), np.uint32), [16, 0, 0])):       # sixteen leaves: five bits
        with pytest.raises(ValueError):
            f.extend(NoDevice(), digests, counts)
    with pytest.raises(ValueError):
        f.extend_packed(NoDevice(), vk.pack_lines(b"a\nb\n"), [1, 1, 1])
    with pytest.raises(ValueError):
        vk.Frontier.empty(2, 65)
    with pytest.raises(ValueError):
        vk.Frontier([1, 2], np.zeros((3, 4, 8), np.uint32))
    assert vk.Frontier.empty(0).roots(NoDevice()).shape == (0, 8)


def test_the_status_text_names_every_bit(native):
    import vk_merkle_roots_amd as vk
    assert vk.frontier_status_text(0) == "ok"
    for bit in range(4):
        assert f"bit {bit}:" in vk.frontier_status_text(1 << bit) and "unknown" not in vk.frontier_status_text(1 << bit)
    assert "unknown bits" in vk.frontier_status_text(16)


def test_the_wrappers_on_raw_buffers_are_not_named_async(native):
    import vk_merkle_roots_amd as vk
    for name in ("frontier_extend_enqueue", "frontier_roots_enqueue", "verify_frontier_enqueue", "forest_frontier_enqueue"):
        assert callable(getattr(vk.HipDevice, name))
    assert not any("frontier" in n and n.endswith("_async") for n in dir(vk.HipDevice))
    assert callable(vk.MerkleForest.frontier)


def test_the_kernel_keys_resolve_to_themselves_and_the_build_lists_them(native):
    from vk_merkle_roots_amd import isa_prio_pass
    keys = isa_prio_pass.EXPECTED_HASH_BLOCKS
    for mine in HASHING:
        assert keys[mine] == 1
        assert_key_resolves(mine)
    for name in KERNELS:
        assert name in HASHING or not any(k in name for k in keys), name      # no hash expected in the others
    rec = isa_record(native)
    if rec is not None:                    # written by a build that ran the issue pass (tests/test_isa_prio_pass.py covers its absence)
        assert rec["audit"]["block_count_errors"] == [] and rec["audit"]["unclassified"] == []
        mine = {k: v for k, v in rec["audit"]["blocks"].items() if "frontier" in k}
        assert sorted(mine.values()) == [1, 1] and all(any(h in k for h in HASHING) for k in mine)
    assert_no_spills(native, KERNELS, max_vgprs=64)        # 512 registers a lane, 8 wavefronts per SIMD
