"""Stored tree, proofs from it, batch verification: the C ABI's declarations, the tree layout and the argument checks.
No compute calls here: every case returns before the library touches HIP, so this runs without a GPU."""
import ctypes as C

from abi_support import Refusals, declared_symbols

ENTRY_POINTS = ("vkmr_hip_tree_bytes", "vkmr_hip_reduce_tree_async", "vkmr_hip_tree_proofs_async", "vkmr_hip_verify_proofs_async")


def test_header_declares_the_tree_entry_points():
    declared = declared_symbols()
    for name in ENTRY_POINTS:
        assert name in declared, name


def layout_cells(count, height):
    """Levels 1..height back to back, level l holding ceil(count / 2^l) cells."""
    return sum(-(-count >> l) for l in range(1, height + 1))


def test_tree_bytes_is_the_layout(native):
    from vk_merkle_roots_amd import _abi
    lib = _abi.lib()
    for count in list(range(1, 301)) + [1 << 26, (1 << 32) + 1]:
        for height in range(0, 64):
            assert lib.vkmr_hip_tree_bytes(count, height) == 32 * layout_cells(count, height), (count, height)
    assert lib.vkmr_hip_tree_bytes(0, 3) == 0
    assert lib.vkmr_hip_tree_bytes(5, 64) == 0


def test_tree_layout_of_the_python_object(native):
    """MerkleTree's level offsets restate the same layout (no device needed to compute them)."""
    import vk_merkle_roots_amd as vk
    for count, height in [(1, 1), (5, 3), (5, 6), (1000, 10), (4097, 16)]:
        t = vk.MerkleTree(None, None, count, height, None)
        assert [t.level_size(l) for l in range(height + 1)][-1] == 1
        for l in range(1, height + 1):
            assert t.level_offset(l) == layout_cells(count, l - 1)
        assert t.level_offset(height) + 1 == layout_cells(count, height)


def test_bad_arguments_are_refused_before_any_hip_call(native):
    from vk_merkle_roots_amd import _abi
    lib = _abi.lib()
    bad = _abi.ERR_INVALID
    d = C.c_void_p(0x1000)           # never dereferenced: every call below returns before launching anything
    # build: null pointers, a height that does not reduce count to one node, count 0, height > 63
    assert lib.vkmr_hip_reduce_tree_async(0, None, None, 8, 3, d) == bad
    assert lib.vkmr_hip_reduce_tree_async(0, None, d, 8, 3, None) == bad
    assert lib.vkmr_hip_reduce_tree_async(0, None, d, 9, 3, d) == bad
    assert lib.vkmr_hip_reduce_tree_async(0, None, d, 0, 1, d) == bad
    assert lib.vkmr_hip_reduce_tree_async(0, None, d, 8, 64, d) == bad
    # gather: a null pointer where k > 0, a bad height; k == 0 is a no-op whatever the rest
    for args in ((None, d, 8, 3, d, 4, d), (d, None, 8, 3, d, 4, d), (d, d, 8, 3, None, 4, d), (d, d, 8, 3, d, 4, None),
                 (d, d, 8, 2, d, 4, d), (d, d, 8, 64, d, 4, d), (d, d, 0, 3, d, 4, d)):
        assert lib.vkmr_hip_tree_proofs_async(0, None, *args) == bad, args
    assert lib.vkmr_hip_tree_proofs_async(0, None, d, d, 8, 3, d, 0, d) == _abi.OK
    assert lib.vkmr_hip_tree_proofs_async(0, None, None, None, 8, 3, None, 0, None) == _abi.OK
    # verify: null pointers, height 0 or above 63, nroots not in {1, k}
    verify = Refusals(lib.vkmr_hip_verify_proofs_async, "vkmr_hip_verify_proofs_async", good=(d, d, d, 4, 3, d, 1, d))
    verify.null(0, 1, 2, 5, 7)
    verify.changed({4: 0}, {4: 64}, {4: 100})                  # the height
    verify.changed({6: 0}, {6: 2}, {6: 3}, {6: 5})             # nroots
    verify.ok((None, None, None, 0, 3, None, 1, None))
