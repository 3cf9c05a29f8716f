"""The audit of a stored forest or tree without a GPU: the C ABI's declarations, its size function and argument checks, the
scratch layout replayed by tests/c/audit_plan_test.cpp, the CPU counterparts (vkmr_host_cpu_forest_audit, vkmr_host_cpu_tree_audit)
against the rule restated with hashlib in tests/audit_cases.py, and the theorem the rule stands on: no bad node <=> the stored
cells are those of a rebuild."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import audit_cases as ac
import forest_cases
import merkle_model
from abi_support import Refusals, assert_bound, assert_exported, assert_key_resolves, isa_record
from no_device import NoDeviceAt as NoDevice

NEW = {"vkmr_hip_audit_scratch_bytes": 3, "vkmr_hip_forest_audit_async": 16, "vkmr_hip_tree_audit_async": 11}
HOST_NEW = {"vkmr_host_cpu_forest_audit": 13, "vkmr_host_cpu_tree_audit": 8}
TABLE_FORESTS = sorted(forest_cases.CASES.items())
FULL_SCAN_LEAVES = 3000                    # above this the hashlib model looks only at the nodes a write can change


def test_libraries_export_the_symbols_and_the_stub_binds_them(native):
    from vk_merkle_roots_amd import _abi
    assert_exported(native.HIP_LIB, NEW)
    assert_exported(native.HOST_LIB, HOST_NEW)
    for name, nargs in NEW.items():
        assert_bound(name, nparams=nargs)
    for name, nargs in HOST_NEW.items():
        assert_bound(name, nparams=nargs, table=_abi.HOST_SIGNATURES, header="vkmr_host.h")
    _abi.host_lib()


# ---- the model itself: what the rule implies --------------------------------------------------------------------------------

def test_the_rule_counts_what_the_issue_says_it_counts():
    """A self-check of the fixture (no product code).  One flipped inner cell: the cell and its parent.  A flipped root, a
    flipped leaf: one.  An inner node replaced with every ancestor rehashed: one.  A padding cell: none."""
    f = ac.Forest([5, 0, 9, 1], seed=1, first=3, slack=2)
    assert f.levels == 4 and f.audit(99).n_bad == 0 and f.audit().checked == (3 + 2 + 1) + 1 + (5 + 3 + 2 + 1) + 1
    base = [a.copy() for a in f.arrays()]

    def fresh():
        for a, b in zip(f.arrays(), base):
            a[:] = b

    ac.flip(f, f.cell(2, 2, 1))
    r = f.audit(9)
    assert list(zip(r.levels, r.trees, r.nodes)) == [(2, 2, 1), (3, 2, 0)] and list(r.masks) == [0, 0, 0b110, 0] and r.flagged == 1
    fresh()
    ac.flip(f, f.cell(2, 4, 0))                # tree 2's root
    assert [tuple(x) for x in zip(f.audit(9).levels, f.audit(9).trees)] == [(4, 2)]
    fresh()
    ac.flip(f, f.cell(0, 0, 4))                # the last leaf of an odd tree: hashed with itself in its level-1 parent
    r = f.audit(9)
    assert list(zip(r.levels, r.trees, r.nodes)) == [(1, 0, 2)]
    fresh()
    ac.flip(f, f.cell(2, 1, 3))
    f.rehash_above(2, 1, 3)                    # the forgery made consistent: only the forged node disagrees with its children
    r = f.audit(9)
    assert list(zip(r.levels, r.trees, r.nodes)) == [(1, 2, 3)] and not np.array_equal(f.roots[2], base[2][2])
    fresh()
    f.roots[1, 5] = 7                          # the empty tree's root
    r = f.audit(9)
    assert list(zip(r.levels, r.trees, r.nodes)) == [(1, 1, 0)] and list(r.masks) == [0, 1, 0, 0]
    fresh()
    pads = np.flatnonzero((f.forest == ac.PADDING).all(axis=1))
    assert pads.size > 0
    f.forest[pads] ^= np.uint32(1)             # every cell that is no node, and the leaves outside the trees
    f.leaves[:3] ^= np.uint32(1)
    f.leaves[-2:] ^= np.uint32(1)
    assert f.audit(9).n_bad == 0
    # the cut list: the first `capacity`, bit 2, the true count
    fresh()
    for l, t, j in ((1, 0, 0), (1, 0, 1), (1, 2, 4)):
        ac.flip(f, f.cell(t, l, j))
    full, cut = f.audit(9), f.audit(2)
    assert full.n_bad == cut.n_bad == 5 and full.status == 0 and cut.status == 4 and list(cut.nodes) == list(full.nodes[:2])
    t = ac.Tree(5, 6, seed=2)                  # lone-node levels 4, 5, 6 above ceil(log2 5) = 3
    assert t.node_count() == 3 + 2 + 1 + 3 and t.audit(9).n_bad == 0
    ac.flip(t, t.cell(4, 0))
    r = t.audit(9)
    assert list(zip(r.levels, r.nodes)) == [(4, 0), (5, 0)] and int(r.masks[0]) == 0b11000 and r.flagged == 0b11000


# ---- the CPU counterparts against the model -----------------------------------------------------------------------------------

def check_host_forest(f, report_capacities, what):
    for capacity in report_capacities:
        want = f.audit(capacity)
        rc, info, masks, trees, levels, nodes = ac.host_forest_audit(f, capacity)
        assert rc == 0, what
        ac.assert_matches(want, info, masks, trees, levels, nodes, (what, capacity))


def forest_rounds(f, what):
    """A clean audit, then every corruption of the shape by itself, each at capacity n, n - 1 and 0."""
    base = [a.copy() for a in f.arrays()]
    check_host_forest(f, [0, 4], what)
    assert f.audit().n_bad == 0
    for name, ids, write, n in ac.forest_corruptions(f):
        write()
        got = f.audit(n + 1)
        assert got.n_bad == n, (what, name, got.n_bad)
        check_host_forest(f, sorted({n, max(n - 1, 0), 0}), (what, name))
        for a, b in zip(f.arrays(), base):
            a[:] = b


@pytest.mark.parametrize("name,counts,first,slack", ac.FORESTS[:-1], ids=[c[0] for c in ac.FORESTS[:-1]])
def test_the_cpu_forest_audit_equals_the_rule_on_the_shared_shapes(native, name, counts, first, slack):
    forest_rounds(ac.Forest(counts, seed=len(counts), first=first, slack=slack), name)


@pytest.mark.parametrize("name,counts", TABLE_FORESTS, ids=[c[0] for c in TABLE_FORESTS])
def test_the_cpu_forest_audit_equals_the_rule_on_the_forest_tables(native, name, counts):
    """Every table of tests/forest_cases.py.  The CPU counterpart always scans the whole forest; for the large tables the model,
    which built the structure itself with hashlib, looks only at the flipped cells' own nodes and their parents -- a node's
    verdict depends on its cell and its two children alone."""
    f = ac.Forest(counts, seed=7)
    full = f.total <= FULL_SCAN_LEAVES
    rng = np.random.default_rng(len(counts))
    ids = list(f.node_ids())
    flipped = []

    def check(capacities):
        for capacity in capacities:
            want = f.audit(capacity, only=None if full else ac.touched(flipped))
            rc, info, masks, trees, levels, nodes = ac.host_forest_audit(f, capacity)
            assert rc == 0
            ac.assert_matches(want, info, masks, trees, levels, nodes, (name, capacity))
        return want.n_bad

    assert check([0, 3]) == 0
    for l, t, j in [ids[int(i)] for i in rng.choice(len(ids), size=min(5, len(ids)), replace=False)]:
        ac.flip(f, f.cell(t, l, j))
        flipped.append((l, t, j))
    n = f.audit(only=None if full else ac.touched(flipped)).n_bad
    assert n >= 1
    check(sorted({n, max(n - 1, 0), 0}))


def test_the_cpu_forest_audit_equals_the_rule_on_random_forests(native):
    rng = np.random.default_rng(20)
    for k in range(25):
        counts = []
        while not counts:
            counts = merkle_model.random_counts(rng, 700)
        first, slack = (int(x) for x in rng.integers(0, 5, size=2))
        f = ac.Forest(counts, seed=k, first=first, slack=slack, max_count=max(max(counts), 1) + int(rng.integers(0, 2)) * 900)
        ids = list(f.node_ids())
        for _ in range(int(rng.integers(0, 6))):
            l, t, j = ids[int(rng.integers(0, len(ids)))]
            l -= int(rng.integers(0, 2))       # the node's own cell, or a child's (a leaf for l == 1)
            if f.counts[t]:
                ac.flip(f, f.cell(t, l, min(j, ac.level_count(f.counts[t], l) - 1)), word=int(rng.integers(0, 8)), bit=1 << int(rng.integers(0, 32)))
        n = f.audit().n_bad
        check_host_forest(f, sorted({n, max(n - 1, 0), 0, n + 3}), ("random", k, counts))


@pytest.mark.parametrize("count,height", ac.TREES + [(1000, 12)])
def test_the_cpu_tree_audit_equals_the_rule(native, count, height):
    tr = ac.Tree(count, height, seed=count)
    base = tr.leaves.copy(), tr.tree.copy()

    def check(capacities, what):
        for capacity in capacities:
            rc, info, levels, nodes = ac.host_tree_audit(tr, capacity)
            assert rc == 0
            ac.assert_matches(tr.audit(capacity), info, None, None, levels, nodes, (count, height, what, capacity))

    check([0, 4], "clean")
    assert tr.audit().n_bad == 0 and tr.audit().checked == tr.node_count()
    for name, ids, write, n in ac.tree_corruptions(tr):
        write()
        assert tr.audit().n_bad == n, (count, height, name)
        check(sorted({n, max(n - 1, 0), 0}), name)
        tr.leaves[:], tr.tree[:] = base


def test_the_cpu_counterparts_report_bad_offsets_and_refuse_missing_arguments(native):
    f = ac.Forest([5, 0, 9], seed=3)
    for offsets, max_count, bits in (([0, 5, 4, 13], None, 1), ([0, 5, 5, 15], 20, 1), ([0, 5, 5, 14], 8, 2), ([0, 14, 5, 14], 9, 3)):
        rc, info, masks, trees, levels, nodes = ac.host_forest_audit(f, 4, max_count=max_count, offsets=offsets)
        assert rc == 0 and list(info) == [bits, 0, 0, 0] and not masks.any() and (nodes == ac.FILL64).all(), (offsets, list(info))
    import vk_merkle_roots_amd as vk
    host = vk.host_lib()
    d = f.leaves.ctypes.data
    good = [d, d, d, 14, f.offsets.ctypes.data, 3, 9, d, d, d, d, 4, d]
    for i in (0, 1, 2, 4, 7, 8, 9, 10, 12):
        args = good[:i] + [None] + good[i + 1:]
        assert host.vkmr_host_cpu_forest_audit(*args) == -1, i
    assert host.vkmr_host_cpu_forest_audit(*(good[:6] + [0] + good[7:])) == -1                  # no max_count
    assert host.vkmr_host_cpu_forest_audit(None, None, None, 0, None, 0, 0, None, None, None, None, 0, None) == 0     # no tree: nothing to do
    tgood = [d, d, 5, 3, d, d, 4, d]
    for i in (0, 1, 4, 5, 7):
        args = tgood[:i] + [None] + tgood[i + 1:]
        assert host.vkmr_host_cpu_tree_audit(*args) == -1, i
    assert host.vkmr_host_cpu_tree_audit(d, d, 5, 2, d, d, 4, d) == -1 and host.vkmr_host_cpu_tree_audit(d, d, 5, 64, d, d, 4, d) == -1
    assert host.vkmr_host_cpu_tree_audit(None, None, 0, 3, None, None, 4, None) == 0


# ---- the theorem --------------------------------------------------------------------------------------------------------------

def test_an_audit_is_clean_exactly_when_the_stored_cells_are_those_of_a_rebuild(native):
    """The property the audit stands on, on the CPU rule: after any writes -- to leaves, inner cells, roots, with or without the
    ancestors rehashed -- the audit reports no bad node <=> every node cell equals what a rebuild from the current leaves
    writes.  A consistent forgery is caught at the forged node; a rewritten leaf with its whole path rehashed is clean."""
    rng = np.random.default_rng(2459)
    outcomes = {True: 0, False: 0}
    for k in range(40):
        counts = []
        while not counts:
            counts = merkle_model.random_counts(rng, 300)
        f = ac.Forest(counts, seed=100 + k, first=int(rng.integers(0, 3)))
        ids = list(f.node_ids())
        for _ in range(int(rng.integers(1, 4))):
            l, t, j = ids[int(rng.integers(0, len(ids)))]
            if not f.counts[t]:
                continue
            kind = int(rng.integers(0, 4))
            if kind == 0:                      # a leaf rewritten and its path rehashed: a legitimate update
                i = int(rng.integers(0, f.counts[t]))
                ac.flip(f, f.cell(t, 0, i))
                f.rehash_above(t, 0, i)
            elif kind == 1:                    # a consistent forgery
                ac.flip(f, f.cell(t, l, j))
                f.rehash_above(t, l, j)
            elif kind == 2:                    # a flipped cell, nothing rehashed
                ac.flip(f, f.cell(t, l, j))
            else:                              # flipped and flipped back
                ac.flip(f, f.cell(t, l, j))
                ac.flip(f, f.cell(t, l, j))
        rebuilt = ac.Forest(counts, seed=100 + k, first=f.offsets[0])
        rebuilt.leaves[:] = f.leaves
        rebuilt.build()
        same = all(np.array_equal(f.get(t, l, j), rebuilt.get(t, l, j)) for l, t, j in ids)
        rc, info, *_ = ac.host_forest_audit(f, 0)
        assert rc == 0 and (int(info[1]) == 0) == same == (f.audit().n_bad == 0), (k, counts, list(info))
        outcomes[same] += 1
    assert outcomes[True] >= 5 and outcomes[False] >= 5, outcomes


# ---- the C ABI without a device -------------------------------------------------------------------------------------------------

def py_words_bound(total, ntrees):
    return sum(((total >> l) + ntrees + 63) // 64 for l in range(1, 64))


def py_scratch_bytes(total, ntrees, capacity):
    if capacity == 0 or ntrees == 0:
        return 0
    up16 = lambda n: (n + 15) & ~15      # noqa: E731
    w = py_words_bound(total, ntrees)
    return 2 * up16(8 * w) + up16(8 * ((w + 255) // 256)) + 32


def test_the_size_function_is_the_layout_monotone_and_zero_without_a_list(native):
    from vk_merkle_roots_amd import _abi
    fn = _abi.lib().vkmr_hip_audit_scratch_bytes
    shapes = [(0, 1), (1, 1), (64, 1), (65, 3), (4096, 1), (600001, 1), (1 << 26, 1 << 15), (1 << 26, 1), (1 << 40, 1 << 20)]
    for total, ntrees in shapes:
        assert fn(total, ntrees, 0) == 0
        for capacity in (1, 7, 2**32 - 1):
            got = fn(total, ntrees, capacity)
            assert got == py_scratch_bytes(total, ntrees, capacity) and got % 16 == 0 and got > 0
            assert fn(total + 1, ntrees, capacity) >= got and fn(total, ntrees + 1, capacity) >= got and got >= fn(total, ntrees, capacity - 1)
    assert fn(1 << 26, 1 << 15, 1) < (1 << 26) * 32 // 8       # a small fraction of the leaves: a bit per cell, twice, and ranking words
    assert fn(100, 0, 5) == 0


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_the_scratch_layout_replayed(tmp_path, sanitize):
    if sanitize:                               # the same stand-alone program with the sanitizers' runtime linked in
        exe = os.path.join(str(tmp_path), "audit_plan_test_san")
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I", os.path.join(merkle_model.ROOT, "vk_merkle_roots_amd", "csrc"),
                               os.path.join(merkle_model.ROOT, "tests", "c", "audit_plan_test.cpp"), "-o", exe])
    else:
        exe = merkle_model.build_plan_exe(tmp_path, "audit_plan_test")
    rng = np.random.default_rng(5)
    lines, want = [], []
    for name, counts, first, slack in ac.FORESTS:
        total, ntrees = first + sum(counts) + slack, len(counts)
        for capacity in (0, 1, 1000):
            lines.append(f"F {total} {ntrees} {max(max(counts), 1)} {capacity}")
            want.append((total, ntrees, capacity))
    for _ in range(300):
        total, ntrees, capacity = int(rng.integers(0, 1 << int(rng.integers(1, 40)))), int(rng.integers(1, 1 << int(rng.integers(1, 20)))), int(rng.integers(0, 3))
        lines.append(f"F {total} {ntrees} {int(rng.integers(1, total + 2))} {capacity}")
        want.append((total, ntrees, capacity))
    for count, height in ac.TREES + [ac.BIG_TREE, (1, 63), (3, 63), (1 << 58, 58)]:
        for capacity in (0, 5):
            lines.append(f"T {count} {merkle_model.tree_height(count) if height is None else height} {capacity}")
            want.append((count, 1, capacity))
    path = os.path.join(str(tmp_path), "shapes.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    text = r.stdout.decode()
    assert r.returncode == 0 and "FAIL" not in text and f"ok: {len(lines)} shapes" in text, text[-2000:]
    for row, (total, ntrees, capacity) in zip(text.splitlines(), want):
        nbytes, used, bound, launches = (int(x) for x in row.split())
        assert nbytes == py_scratch_bytes(total, ntrees, capacity), (row, total, ntrees, capacity)
        assert used <= bound and (bound == py_words_bound(total, ntrees) if capacity else bound == 0)


def test_the_forest_call_refuses_bad_arguments_before_any_hip_call(native):
    from vk_merkle_roots_amd import _abi
    lib = _abi.lib()
    d = C.c_void_p(0x1000)                     # never dereferenced: every call below returns before launching anything
    # digests, forest, roots, total, offsets, ntrees, max_count, scratch, masks, bad_trees, bad_levels, bad_nodes, capacity, info
    audit = Refusals(lib.vkmr_hip_forest_audit_async, "vkmr_hip_forest_audit_async", good=[d, d, d, 100, d, 4, 50, d, d, d, d, d, 8, d])
    audit.null(0, 1, 2, 4, 7, 8, 9, 10, 11, 13)
    audit.changed({6: 0}, {3: (1 << 58) + 1}, {7: C.c_void_p(0x1008)})        # no max_count, too many leaves, scratch off the 16-byte grid
    # a level of more than 2^32 - 1 cells cannot be listed; the refusal names the way out
    audit.changed({3: 1 << 34})
    assert b"capacity must be 0" in lib.vkmr_hip_last_error()
    # capacity 0: the lists and the scratch may be missing -- the masks and the counters may not
    audit.changed(*({7: None, 9: None, 10: None, 11: None, 12: 0, i: None} for i in (8, 13)))
    # no tree: nothing to do, whatever the rest
    audit.ok((None, None, None, 1 << 60, None, 0, 0, None, None, None, None, None, 7, None))


def test_the_tree_call_refuses_bad_arguments_before_any_hip_call(native):
    from vk_merkle_roots_amd import _abi
    lib = _abi.lib()
    d = C.c_void_p(0x1000)
    # digests, tree, count, height, scratch, bad_levels, bad_nodes, capacity, info
    audit = Refusals(lib.vkmr_hip_tree_audit_async, "vkmr_hip_tree_audit_async", good=[d, d, 100, 7, d, d, d, 8, d])
    audit.null(0, 1, 4, 5, 6, 8)
    audit.changed(*({2: count, 3: height} for count, height in ((100, 6), (100, 64), (1 << 59, 59))))
    audit.changed({4: C.c_void_p(0x1004)})
    audit.changed({2: 1 << 34, 3: 34})
    assert b"capacity must be 0" in lib.vkmr_hip_last_error()
    # capacity 0: the digests, the tree and the counters are still needed
    audit.changed(*({4: None, 5: None, 6: None, 7: 0, i: None} for i in (0, 1, 8)))
    audit.ok((None, None, 0, 99, None, None, None, 7, None))                              # no leaf: nothing to do


def test_the_python_layer_checks_the_capacity_before_any_device_call():
    import vk_merkle_roots_amd as vk
    f = vk.MerkleForest(NoDevice(0), None, 14, [5, 0, 9], None, 9, None, None)
    t = vk.MerkleTree(NoDevice(0), None, 14, 4, None)
    for s in (f, t):
        for capacity in (-1, 2**32):
            with pytest.raises(ValueError):
                s.audit(capacity=capacity)
    empty = vk.MerkleForest(NoDevice(0), None, 0, [], None, 1, None, None).audit()
    assert empty.clean and empty.n_bad == 0 and empty.checked == 0 and empty.masks.shape == (0,) and empty.nodes.shape == (0,)
    assert callable(vk.HipDevice.audit_scratch_bytes)
    assert callable(vk.MerkleForest.audit_async) and callable(vk.MerkleTree.audit_async) and vk.MerkleForest.audit is vk.MerkleTree.audit


class _Buf:
    def __init__(self, ptr):
        self.ptr = ptr


class _Recorder:
    """Stands for the ctypes library: every function returns 0 and notes (C name, arguments)."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, list(args)))
            return 0
        return fn


def test_audit_async_hands_the_abi_its_arguments_in_the_headers_order():
    """What MerkleForest.audit_async and MerkleTree.audit_async pass to the C ABI, over a recording library and without a GPU:
    the structure's own buffers and sizes, then the caller's buffers, each in its place; a None buffer goes as NULL, and
    `stream` replaces the device's own."""
    import vk_merkle_roots_amd as vk
    from vk_merkle_roots_amd import _abi, engine
    dev = object.__new__(engine.HipDevice)
    dev.lib, dev.index, dev.stream = _Recorder(), 3, 0x5000
    leaves, off, forest, roots, tree = (_Buf(0x100000 * i) for i in range(1, 6))
    scr, masks, trees, levels, nodes, info = (_Buf(0x1000000 * i) for i in range(1, 7))
    f = vk.MerkleForest(dev, leaves, 14, [5, 0, 9], off, 9, forest, roots)
    f.audit_async(scr, masks, trees, levels, nodes, 7, info)
    f.audit_async(None, masks, None, None, None, 0, info, stream=0x6000)
    t = vk.MerkleTree(dev, leaves, 14, 5, tree)
    t.audit_async(scr, levels, nodes, 7, info)
    t.audit_async(None, None, None, 0, info, stream=0x6000)
    assert dev.lib.calls == [
        ("vkmr_hip_forest_audit_async", [3, 0x5000, leaves.ptr, forest.ptr, roots.ptr, 14, off.ptr, 3, 9, scr.ptr, masks.ptr, trees.ptr, levels.ptr,
                                         nodes.ptr, 7, info.ptr]),
        ("vkmr_hip_forest_audit_async", [3, 0x6000, leaves.ptr, forest.ptr, roots.ptr, 14, off.ptr, 3, 9, None, masks.ptr, None, None, None, 0, info.ptr]),
        ("vkmr_hip_tree_audit_async", [3, 0x5000, leaves.ptr, tree.ptr, 14, 5, scr.ptr, levels.ptr, nodes.ptr, 7, info.ptr]),
        ("vkmr_hip_tree_audit_async", [3, 0x6000, leaves.ptr, tree.ptr, 14, 5, None, None, None, 0, info.ptr])]
    for name, args in dev.lib.calls:
        assert len(args) == len(_abi.SIGNATURES[name][1])


# ---- the build ------------------------------------------------------------------------------------------------------------------

def test_the_level_kernels_hold_one_hash_block_each_and_the_build_lists_them(native):
    from vk_merkle_roots_amd import isa_prio_pass
    keys = isa_prio_pass.EXPECTED_HASH_BLOCKS
    for mine in ("forest_audit_level_kernel", "tree_audit_level_kernel"):
        assert keys[mine] == 1
        assert_key_resolves(mine)
    rec = isa_record(native)
    if rec is None:                        # as tests/test_isa_prio_pass.py: only a build without the llvm tools leaves no record
        pytest.skip("the library in the tree was built without the issue pass (llvm tools absent)")
    assert rec["audit"]["block_count_errors"] == [] and rec["audit"]["unclassified"] == []
    blocks = {k: v for k, v in rec["audit"]["blocks"].items() if "_audit_" in k}
    assert sorted(blocks.values()) == [1, 1] and all("audit_level_kernel" in k for k in blocks)       # the emit kernels hold none
