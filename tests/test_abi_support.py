"""tests/abi_support.py fails when it should: nineteen ABI files lean on it, so a helper that cannot fail would weaken them all
at once.  Synthetic header text, Python callables and listing text only: no library, no GPU."""
import ctypes as C

import pytest

import abi_support as A

HEADER = """
#define VKMR_API __attribute__((visibility("default")))
typedef int vkmr_status;
typedef struct vkmr_stream_s* vkmr_stream;   /* a handle: a pointer by another name */
typedef struct vkmr_digest { uint32_t data[8]; } vkmr_digest;
/* VKMR_API vkmr_status vkmr_hip_in_a_comment(int dev); */
VKMR_API vkmr_status vkmr_hip_thing_async(int dev, vkmr_stream s, const vkmr_digest* digests_dev, /* leaves, (count) of them, */
                                          uint64_t count,   // how many (a comma, and a parenthesis)
                                          uint32_t height, vkmr_digest* const* out);
VKMR_API size_t vkmr_hip_thing_bytes(uint64_t n, unsigned height);
VKMR_API const char* vkmr_hip_text(void);
VKMR_API void vkmr_hip_hex(const vkmr_digest* d, char* out);
"""
TABLE = {"vkmr_hip_thing_async": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(C.c_void_p)]),
         "vkmr_hip_thing_bytes": (C.c_size_t, [C.c_uint64, C.c_uint]),
         "vkmr_hip_text": (C.c_char_p, []),
         "vkmr_hip_hex": (None, [C.c_void_p, C.c_char_p])}
THING = "vkmr_hip_thing_async"


def bound(header=HEADER, table=TABLE, name=THING, **literals):
    A.assert_bound(name, table=table, header=header, **literals)


def test_the_header_is_read_as_written():
    d = A.declarations(HEADER)
    assert sorted(d) == sorted(TABLE) == A.declared_symbols(HEADER)                 # the one in a comment is none
    assert d[THING].restype == "vkmr_status" and d[THING].handles == {"vkmr_stream"}
    assert d[THING].params == (("int", "dev"), ("vkmr_stream", "s"), ("const vkmr_digest*", "digests_dev"), ("uint64_t", "count"),
                               ("uint32_t", "height"), ("vkmr_digest* const*", "out"))    # the comments' comma and parentheses split nothing
    assert d["vkmr_hip_text"].params == () and d["vkmr_hip_text"].restype == "const char*"
    assert A.ctypes_of(d[THING]) == (C.c_int, [C.c_int, A.POINTER, A.POINTER, C.c_uint64, C.c_uint32, A.POINTER])
    assert A.ctypes_of(d["vkmr_hip_thing_bytes"]) == (C.c_size_t, [C.c_uint64, C.c_uint])
    assert A.ctypes_of(d["vkmr_hip_hex"]) == (None, [A.POINTER, A.POINTER])
    for name in TABLE:
        bound(name=name)
    bound(nparams=6, scalars=[C.c_int, C.c_uint64, C.c_uint32], restype=C.c_int)


def test_the_repositorys_handles_are_read_from_its_header():
    d = A.declarations()
    assert d["vkmr_hip_last_error"].handles == {"vkmr_stream", "vkmr_event", "vkmr_comm"}
    assert A.declarations("vkmr_hip_experiments.h")["vkmr_hip_split_text_async"].handles == d["vkmr_hip_last_error"].handles


@pytest.mark.parametrize("what,old,new", [
    ("a parameter is dropped", "uint32_t height, ", ""),
    ("uint32_t has become uint64_t", "uint32_t height", "uint64_t height"),
    ("a pointer has become a scalar", "const vkmr_digest* digests_dev", "uint64_t digests_dev"),
    ("a scalar has become a pointer", "uint64_t count,", "const uint64_t* count,"),
    ("a handle has become a scalar", "vkmr_stream s", "int s"),
    ("the return type differs", "VKMR_API vkmr_status vkmr_hip_thing_async", "VKMR_API size_t vkmr_hip_thing_async"),
    ("the return type has become a pointer", "VKMR_API vkmr_status vkmr_hip_thing_async", "VKMR_API const char* vkmr_hip_thing_async"),
    ("the name is not declared", "vkmr_hip_thing_async", "vkmr_hip_other_async"),
])
def test_a_header_that_differs_from_the_stub_is_caught(what, old, new):
    assert HEADER.count(old) == 1
    with pytest.raises(AssertionError):
        bound(header=HEADER.replace(old, new))


HOST_HEADER = """
#include "vkmr_hip.h"
/* VKMR_API int vkmr_host_in_a_comment(int n); */
VKMR_API int64_t vkmr_host_thing(const uint8_t* buf, uint64_t len, uint32_t maxlen, int which, const vkmr_digest* roots, char* root_hex,
                                 double* seconds);
VKMR_API void* vkmr_host_thing_open(uint32_t seed);
VKMR_API void vkmr_host_thing_rand(uint32_t seed, int32_t* out, uint64_t n);
"""
HOST_TABLE = {"vkmr_host_thing": (C.c_int64, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_void_p, C.c_char_p, C.POINTER(C.c_double)]),
              "vkmr_host_thing_open": (C.c_void_p, [C.c_uint32]),
              "vkmr_host_thing_rand": (None, [C.c_uint32, C.c_void_p, C.c_uint64])}
HOST_THING = "vkmr_host_thing"


def test_a_host_header_is_read_as_written():
    d = A.declarations(HOST_HEADER)
    assert sorted(d) == sorted(HOST_TABLE) == A.declared_symbols(HOST_HEADER)
    assert A.ctypes_of(d[HOST_THING]) == (C.c_int64, [A.POINTER, C.c_uint64, C.c_uint32, C.c_int, A.POINTER, A.POINTER, A.POINTER])
    assert A.ctypes_of(d["vkmr_host_thing_open"]) == (A.POINTER, [C.c_uint32])
    assert A.ctypes_of(d["vkmr_host_thing_rand"]) == (None, [C.c_uint32, A.POINTER, C.c_uint64])       # an int32_t* is a pointer
    for name in HOST_TABLE:
        bound(header=HOST_HEADER, table=HOST_TABLE, name=name)
    bound(header=HOST_HEADER, table=HOST_TABLE, name=HOST_THING, nparams=7, scalars=[C.c_uint64, C.c_uint32, C.c_int], restype=C.c_int64)


@pytest.mark.parametrize("what,old,new", [
    ("a parameter is dropped", "uint32_t maxlen, ", ""),
    ("uint32_t has become uint64_t", "uint32_t maxlen", "uint64_t maxlen"),
    ("uint64_t has become uint32_t", "uint64_t len", "uint32_t len"),
    ("a pointer has become a scalar", "const uint8_t* buf", "uint64_t buf"),
    ("a scalar has become a pointer", "int which", "int* which"),
    ("the return type differs", "VKMR_API int64_t vkmr_host_thing(", "VKMR_API int vkmr_host_thing("),
    ("the return type has become a pointer", "VKMR_API int64_t vkmr_host_thing(", "VKMR_API void* vkmr_host_thing("),
    ("the name is not declared", "vkmr_host_thing(", "vkmr_host_other("),
])
def test_a_host_header_that_differs_from_the_stub_is_caught(what, old, new):
    assert HOST_HEADER.count(old) == 1
    with pytest.raises(AssertionError):
        bound(header=HOST_HEADER.replace(old, new), table=HOST_TABLE, name=HOST_THING)


def test_a_host_stub_that_differs_from_the_header_is_caught():
    res, args = HOST_TABLE[HOST_THING]
    for entry in ((res, args[:-1]), (C.c_int, args), (res, args[:1] + [C.c_uint32] + args[2:]), (res, args[:2] + [C.c_uint64] + args[3:]),
                  (res, [C.c_uint64] + args[1:])):
        with pytest.raises(AssertionError):
            bound(header=HOST_HEADER, table={HOST_THING: entry}, name=HOST_THING)


def test_a_stub_that_differs_from_the_header_is_caught():
    res, args = TABLE[THING]
    for entry in ((res, args[:-1]), (res, args + [C.c_void_p]), (C.c_size_t, args), (None, args), (res, [C.c_uint32] + args[1:]),
                  (res, args[:1] + [C.c_uint64] + args[2:]), (res, args[:3] + [C.c_void_p] + args[4:])):
        with pytest.raises(AssertionError):
            bound(table={THING: entry})
    with pytest.raises(AssertionError):
        bound(table={})


def test_the_literals_pin_the_header():
    for literals in ({"nparams": 5}, {"nparams": 7}, {"scalars": [C.c_int, C.c_uint64]}, {"scalars": [C.c_int, C.c_uint32, C.c_uint64]},
                     {"restype": C.c_size_t}):
        with pytest.raises(AssertionError):
            bound(**literals)


def test_an_unknown_type_is_an_error_and_not_a_pointer():
    header = HEADER.replace("uint32_t height", "vkmr_levels height")
    with pytest.raises(ValueError, match="vkmr_levels"):
        bound(header=header)
    with pytest.raises(ValueError, match="vkmr_event"):                             # a handle the header itself does not declare
        bound(header=HEADER.replace("vkmr_stream s", "vkmr_event s"))


# ---- Refusals over a Python callable ----------------------------------------------------------------------------------------
class Entry:
    """Stands where an entry point would: refuses a NULL among the first two arguments and a height outside 1..63, does
    nothing for k == 0, and leaves what refuse() would in the last error."""

    def __init__(self, says="vkmr_hip_thing_async: bad argument", accepts_null_at=None, refuses_no_op=False):
        self.says, self.accepts_null_at, self.refuses_no_op, self.error, self.calls = says.encode(), accepts_null_at, refuses_no_op, b"", []

    def __call__(self, dev, stream, a, b, height, k):
        self.calls.append((a, b, height, k))
        bad = any(x is None and i != self.accepts_null_at for i, x in enumerate((a, b))) or not 1 <= height <= 63
        if (k == 0 and not self.refuses_no_op) or not bad and k:
            return 0
        self.error = self.says
        return -1

    def last_error(self):
        return self.error


def refusals(entry):
    return A.Refusals(entry, THING, good=["a", "b", 5, 9], last_error=entry.last_error, ok=0, invalid=-1)     # nothing of the product is loaded


def test_refusals_send_what_they_are_told_and_pass_on_an_entry_point_that_refuses():
    entry = Entry()
    r = refusals(entry)
    r.null(0, 1)
    r.changed({2: 0}, {2: 64}, {0: None, 2: 7})
    r.ok((None, None, 0, 0), ["a", "b", 5, 0])
    assert entry.calls == [(None, "b", 5, 9), ("a", None, 5, 9), ("a", "b", 0, 9), ("a", "b", 64, 9), (None, "b", 7, 9), (None, None, 0, 0), ("a", "b", 5, 0)]
    assert r.good == ["a", "b", 5, 9]


def test_ok_where_a_refusal_is_due_is_caught():
    with pytest.raises(AssertionError, match="returned 0"):
        refusals(Entry(accepts_null_at=1)).null(0, 1)
    with pytest.raises(AssertionError, match="returned 0"):
        refusals(Entry()).changed({2: 64}, {2: 63})


def test_a_refusal_that_names_another_function_is_caught():
    entry = Entry(says="vkmr_hip_thing_bytes: bad argument")
    with pytest.raises(AssertionError, match="last error"):
        refusals(entry).null(0)
    with pytest.raises(AssertionError, match="last error"):
        refusals(entry).changed({2: 0})
    refusals(entry).null(0, 1, names_itself=False)                                 # the way out is explicit, call by call


def test_a_refused_no_op_is_caught():
    with pytest.raises(AssertionError, match="returned -1"):
        refusals(Entry(refuses_no_op=True)).ok((None, None, 0, 0))


# ---- the code object's metadata ----------------------------------------------------------------------------------------------
def entry_of(symbol, vgprs=40, scratch=0, sgpr_spills=0, vgpr_spills=0):
    return (f"  - .args:\n      - .offset:         0\n        .size:           8\n    .group_segment_fixed_size: 0\n    .max_flat_workgroup_size: 256\n"
            f"    .name:           {symbol}\n    .private_segment_fixed_size: {scratch}\n    .sgpr_count:     30\n    .sgpr_spill_count: {sgpr_spills}\n"
            f"    .symbol:         {symbol}.kd\n    .vgpr_count:     {vgprs}\n    .vgpr_spill_count: {vgpr_spills}\n    .wavefront_size: 64\n")


def listing(*entries):
    return "amdhsa.kernels:\n" + "".join(entries) + "amdhsa.target:   amdgcn-amd-amdhsa--gfx950\n"


PLAIN, TEMPLATE = "_Z10foo_kernelPK4Nodej", "_Z10foo_kernelILb1EEvPK4Nodej"


def test_a_clean_kernel_passes_in_its_own_form_only():
    assert A.assert_no_spills(listing(entry_of(PLAIN)), ["foo_kernel"], max_vgprs=64) is True
    assert A.assert_no_spills(listing(entry_of(TEMPLATE)), ["foo_kernel"], max_vgprs=64, prefix=True) is True
    assert A.kernel_metadata(listing(entry_of(PLAIN, vgprs=17)), "foo_kernel")["vgpr_count"] == "17"
    with pytest.raises(AssertionError, match="not in the listing"):                 # the plain form does not take a template's instantiation
        A.assert_no_spills(listing(entry_of(TEMPLATE)), ["foo_kernel"])


@pytest.mark.parametrize("fault,match", [({"vgpr_spills": 3}, "vgpr_spill_count is 3"), ({"sgpr_spills": 1}, "sgpr_spill_count is 1"),
                                         ({"scratch": 16}, "private_segment_fixed_size is 16"), ({"vgprs": 65}, "65 VGPRs")])
@pytest.mark.parametrize("symbol,prefix", [(PLAIN, False), (TEMPLATE, True)])
def test_spills_scratch_and_registers_are_caught(fault, match, symbol, prefix):
    text = listing(entry_of("_Z10bar_kernelPK4Nodej"), entry_of(symbol, **fault))
    with pytest.raises(AssertionError, match=match):
        A.assert_no_spills(text, ["bar_kernel", "foo_kernel"] if not prefix else ["foo_kernel"], max_vgprs=64, prefix=prefix)
    if "vgprs" in fault:
        assert A.assert_no_spills(text, ["foo_kernel"], prefix=prefix) is True      # no bound asked, none applied


def test_an_absent_kernel_is_an_error_and_an_absent_listing_is_said():
    with pytest.raises(AssertionError, match="foo_kernel is not in the listing"):
        A.assert_no_spills(listing(entry_of("_Z10bar_kernelPK4Nodej")), ["bar_kernel", "foo_kernel"])

    class NoListing:
        HIP_LIB = "/nowhere/libnone.so"
    assert A.code_object(NoListing) is None and A.assert_no_spills(NoListing, ["foo_kernel"]) is False
    assert A.isa_record(NoListing) is None


@pytest.mark.parametrize("prefix", [False, True])
def test_of_two_kernels_where_one_name_begins_or_ends_the_other_each_finds_its_own(prefix):
    tail = "ILb1EEvPKj" if prefix else "PKj"
    long_first = listing(entry_of("_Z18foo_kernel_flagged" + tail, vgprs=18), entry_of("_Z14big_foo_kernel" + tail, vgprs=14),
                         entry_of("_Z10foo_kernel" + tail, vgprs=10))
    for name, vgprs in (("foo_kernel", "10"), ("foo_kernel_flagged", "18"), ("big_foo_kernel", "14")):
        assert A.kernel_metadata(long_first, name, prefix)["vgpr_count"] == vgprs


# ---- the issue pass's keys ---------------------------------------------------------------------------------------------------
def test_a_key_resolves_to_itself_or_is_caught():
    keys = {"ELi64ELi5ELb1": 3, "reduce_pass_kernel": 1, "map_kernel": 2, "forest_level_kernel": 1}
    for k in list(keys)[1:]:
        A.assert_key_resolves(k, keys)
    with pytest.raises(AssertionError, match="no key"):
        A.assert_key_resolves("tree_level_kernel", keys)
    with pytest.raises(AssertionError, match="resolves to the key level_kernel"):   # a key in front that is a substring of mine: first match wins
        A.assert_key_resolves("forest_level_kernel", {"level_kernel": 1, **keys})
    with pytest.raises(AssertionError, match="shadow each other"):                  # and behind mine: I would take its kernels
        A.assert_key_resolves("level_kernel", {**keys, "level_kernel": 1})
    with pytest.raises(AssertionError, match="shadow each other"):
        A.assert_key_resolves("forest_level_kernel", {**keys, "forest_level_kernel_flagged": 1})
