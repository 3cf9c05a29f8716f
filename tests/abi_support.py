"""What every tests/test_*_abi.py needs of the C ABI, once: the header read into declarations, a stub entry checked against its
declaration, the refusal loops, the code object's metadata and the issue pass's key rule.  A plain module (no fixtures, not a
conftest), imported the way the *_cases.py modules are.  Every function takes its text or its library as an argument and has
the repository's own as the default; tests/test_abi_support.py feeds each one input that must fail.

A new operation's ABI file starts from a table of arguments:

    from abi_support import Refusals, assert_bound, assert_exported, assert_key_resolves, assert_no_spills, isa_record

    assert_bound("vkmr_hip_thing_async", nparams=9, scalars=[C.c_int, C.c_uint64, C.c_uint32])   # the literals pin the header
    assert_bound("vkmr_host_cpu_thing", nparams=7, table=_abi.HOST_SIGNATURES, header="vkmr_host.h")   # the CPU twin, against its own
    assert_exported(native.HIP_LIB, ["vkmr_hip_thing_async"])
    r = Refusals(lib.vkmr_hip_thing_async, "vkmr_hip_thing_async", good=[d, d, 100, d, 8, d, d])
    r.null(0, 1, 3, 5, 6)                          # each pointer set to NULL alone
    r.changed({2: 0}, {4: 64}, {5: C.c_void_p(0x1008)})   # a bad value, a misaligned pointer
    r.ok([None, None, 0, None, 0, None, None])     # the calls that have nothing to do
    assert_key_resolves("thing_level_kernel")
    assert_no_spills(native, ("thing_level_kernel", "thing_gather_kernel"))
"""
import ctypes as C
import functools
import json
import os
import re
from typing import NamedTuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
POINTER = "a pointer"          # what ctypes_of says of a parameter the stub may bind as c_void_p, c_char_p or a POINTER(...) type
SCALARS = {"int": C.c_int, "vkmr_status": C.c_int, "unsigned": C.c_uint, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "size_t": C.c_size_t,
           "int32_t": C.c_int32, "int64_t": C.c_int64}     # vkmr_host.h's; its uint8_t, char, double and void stand behind a `*` only


class Declaration(NamedTuple):
    restype: str               # C type text, "void" included
    params: tuple              # of (C type text, parameter name), in order
    handles: frozenset         # the `typedef struct x* name;` names in scope: pointers by another name


def _source(header):
    """The text, without its comments, of a header of include/ given by its file name, or of header text given as it is
    (anything with a line break in it)."""
    text = header if "\n" in header else open(os.path.join(INCLUDE, header)).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def _handles(text):
    found = set(re.findall(r"\btypedef\s+struct\s+\w+\s*\*\s*(\w+)\s*;", text))
    for included in re.findall(r'^\s*#\s*include\s+"([^"]+)"', text, flags=re.M):       # the experiments header takes its handles from vkmr_hip.h
        if os.path.exists(os.path.join(INCLUDE, included)):
            found |= _handles(_source(included))
    return found


@functools.lru_cache(maxsize=None)
def declarations(header="vkmr_hip.h"):
    """{name: Declaration} of every `VKMR_API <type> vkmr_hip_<name>(<parameters>);` or `... vkmr_host_<name>(...)` of the header
    itself; what it includes declares its own."""
    text = _source(header)
    handles = frozenset(_handles(text))
    text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)                                   # `#define VKMR_API ...` declares nothing
    found = {}
    for restype, name, params in re.findall(r"\bVKMR_API\s+([^;()]+?)\b(vkmr_(?:hip|host)_\w+)\s*\(([^()]*)\)\s*;", text):
        assert name not in found, name
        params = " ".join(params.split())
        pairs = []
        for p in ([] if params in ("void", "") else params.split(",")):
            m = re.fullmatch(r"\s*(.*?[\s\*])(\w+)\s*", p)
            assert m, (name, p)                                                         # a parameter without a name, or an array: not this header's style
            pairs.append((re.sub(r"\s*\*", "*", " ".join(m.group(1).split())), m.group(2)))
        found[name] = Declaration(re.sub(r"\s*\*", "*", " ".join(restype.split())), tuple(pairs), handles)
    return found


def declared_symbols(header="vkmr_hip.h"):
    return sorted(declarations(header))


def _ctype(text, handles):
    if "*" in text or text in handles:
        return POINTER
    bare = " ".join(w for w in text.split() if w != "const")
    if bare not in SCALARS:
        raise ValueError(f"abi_support knows no ctypes type for {text!r}")              # an unknown type is an error, not a pointer
    return SCALARS[bare]


def ctypes_of(declaration):
    """(restype, [argtypes]) the stub must hold for a Declaration: a ctypes type for a scalar, POINTER for a pointer or a
    handle, None for a void return."""
    res = None if declaration.restype == "void" else _ctype(declaration.restype, declaration.handles)
    return res, [_ctype(t, declaration.handles) for t, _ in declaration.params]


def is_pointer(ctype):
    return ctype in (C.c_void_p, C.c_char_p) or (isinstance(ctype, type) and issubclass(ctype, C._Pointer))


def _same(stub, want):
    return is_pointer(stub) if want is POINTER else stub is want


def assert_bound(name, nparams=None, scalars=None, restype=None, table=None, header="vkmr_hip.h"):
    """The header declares `name` and the stub's entry binds it argument by argument: the same arity, every scalar the
    header's own type, every pointer a pointer, the same return type.  nparams, scalars (the stub's non-pointer argtypes, in
    order) and restype are the caller's literals: given, they pin the header as well."""
    if table is None:
        from vk_merkle_roots_amd import _abi
        table = _abi.SIGNATURES
    declared = declarations(header)
    assert name in declared, f"{name} is not declared"
    assert name in table, f"{name} has no stub entry"
    want_res, want = ctypes_of(declared[name])
    res, args = table[name]
    assert len(args) == len(want), f"{name}: the stub binds {len(args)} arguments, the header declares {len(want)}"
    for i, (a, w, (ctext, pname)) in enumerate(zip(args, want, declared[name].params)):
        assert _same(a, w), f"{name}: argument {i} ({ctext} {pname}) is bound as {a}"
    assert _same(res, want_res), f"{name}: returns {declared[name].restype}, bound as {res}"
    if nparams is not None:
        assert len(want) == nparams, f"{name}: {len(want)} parameters declared, {nparams} expected"
    if scalars is not None:
        assert [a for a in args if not is_pointer(a)] == list(scalars), f"{name}: the scalars are {[a for a in args if not is_pointer(a)]}"
    if restype is not None:
        assert res is restype, f"{name}: bound to return {res}"


def assert_exported(path, names):
    lib = C.CDLL(path)
    for name in names:
        assert hasattr(lib, name), f"{os.path.basename(path)} does not export {name}"


class Refusals:
    """The argument checks of one entry point: `good` is an argument list that would pass them (after `lead`, the device and
    the stream), and every call below differs from it in what is said.  Nothing is launched: a refused call returns before
    its first HIP call, and after each one the last error names the function (names_itself=False where one does not)."""

    def __init__(self, fn, name, good, lead=(0, None), last_error=None, ok=None, invalid=None):
        self.fn, self.name, self.good, self.lead = fn, name, list(good), tuple(lead)
        if last_error is None or ok is None or invalid is None:        # the library's own, where the caller brings none
            from vk_merkle_roots_amd import _abi
            last_error = last_error or _abi.lib().vkmr_hip_last_error
            ok, invalid = (_abi.OK if ok is None else ok), (_abi.ERR_INVALID if invalid is None else invalid)
        self.last_error, self.OK, self.ERR_INVALID = last_error, ok, invalid

    def changed(self, *dicts, names_itself=True):
        """Each {index: value, ...} applied to the good list alone is refused."""
        for changes in dicts:
            args = list(self.good)
            for i, value in changes.items():
                args[i] = value
            status = self.fn(*self.lead, *args)
            assert status == self.ERR_INVALID, f"{self.name} with {changes} returned {status}"
            if names_itself:
                text = self.last_error() or b""
                assert self.name.encode() in text, f"{self.name} with {changes} left {text!r} as the last error"

    def null(self, *indices, names_itself=True):
        """Each of these arguments set to NULL alone is refused."""
        self.changed(*({i: None} for i in indices), names_itself=names_itself)

    def ok(self, *argument_lists):
        """The calls that have nothing to do, whole argument lists: each returns OK."""
        for args in argument_lists:
            status = self.fn(*self.lead, *args)
            assert status == self.OK, f"{self.name}{tuple(args)} returned {status}"


def isa_record(native):
    """The record the build writes beside the library when it ran the issue pass, parsed; None where it did not."""
    path = os.path.splitext(native.HIP_LIB)[0] + ".isa.json"
    return json.load(open(path)) if os.path.exists(path) else None


def listing_path(native, name="device.s"):
    """Where the build leaves the library's device assembly (device_prio.s: the same after the issue pass)."""
    return os.path.join(ROOT, "build", "obj", os.path.basename(native.HIP_LIB), name)


def code_object(native):
    """The device assembly the build left behind (the code object's own metadata is at its end), or None: a library may
    come built without it.  Listing text given as it is comes back as it is."""
    if isinstance(native, str):
        return native
    path = listing_path(native)
    return open(path).read() if os.path.exists(path) else None


def kernel_metadata(listing, kernel, prefix=False):
    """The fields of a kernel's `.name:` entry.  Two forms of name, different on purpose, both with the mangled length so that
    neither can pick a neighbour whose name merely ends or begins alike:
      prefix=False  _Z<len><kernel>P...   a plain function whose first parameter is a pointer; a template's instantiation of
                                          the same name is not taken for it
      prefix=True   _Z<len><kernel>...    whatever follows the name.  The apply, forest-update and forest-multiproof tests have
                                          always asked this much and no more of their level kernels: today those are plain
                                          functions that the first form finds too, and the check holds on if one becomes a
                                          template's instantiation or takes a first parameter that is no pointer
    """
    m = re.search(r"\.name:\s+_Z" + str(len(kernel)) + re.escape(kernel) + (r"\w*" if prefix else r"P\w*") + r"\n((?:    \..*\n)+)", listing)
    assert m, f"{kernel} is not in the listing"
    return dict(re.findall(r"\.(\w+):\s+(\S+)", m.group(1)))


def assert_no_spills(native, kernels, max_vgprs=None, prefix=False):
    """No kernel of `kernels` has scratch or spills (and none more than max_vgprs registers).  True when checked, False when
    there is no listing to check."""
    listing = code_object(native)
    if listing is None:
        return False
    for kernel in kernels:
        fields = kernel_metadata(listing, kernel, prefix)
        for field in ("private_segment_fixed_size", "sgpr_spill_count", "vgpr_spill_count"):
            assert fields[field] == "0", f"{kernel}: {field} is {fields[field]}"
        if max_vgprs is not None:
            assert int(fields["vgpr_count"]) <= max_vgprs, f"{kernel}: {fields['vgpr_count']} VGPRs, {max_vgprs} allowed"
    return True


def assert_key_resolves(kernel, keys=None):
    """isa_prio_pass.EXPECTED_HASH_BLOCKS is matched by substring, first match wins: the kernel's mangled name must resolve to
    its own key, and the key must shadow nobody's nor be shadowed."""
    if keys is None:
        from vk_merkle_roots_amd import isa_prio_pass
        keys = isa_prio_pass.EXPECTED_HASH_BLOCKS
    assert kernel in keys, f"{kernel} has no key"
    first = next(k for k in keys if k in f"_Z{len(kernel)}{kernel}PK")
    assert first == kernel, f"{kernel} resolves to the key {first}"
    for other in keys:
        assert other == kernel or (other not in kernel and kernel not in other), f"{kernel} and {other} shadow each other"
