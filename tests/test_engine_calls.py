"""What HipDevice's wrappers hand to the C ABI, without a GPU.  The `*_async` ones: every call recorded in
tests/golden/engine_calls.json (written by tests/golden/make_engine_calls.py from the wrappers as they were before they shared
one call path) replayed with the same helper over a recording library, and compared argument for argument.  The `*_enqueue`
ones, which are not in that record: the same helper, held against include/vkmr_hip.h."""
import importlib.util
import inspect
import json
import os

import pytest

from conftest import ROOT

GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")

_spec = importlib.util.spec_from_file_location("make_engine_calls", os.path.join(GOLDEN_DIR, "make_engine_calls.py"))
calls = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(calls)

with open(os.path.join(GOLDEN_DIR, "engine_calls.json")) as f:
    RECORDED = {k: v for k, v in json.load(f).items() if not k.startswith("_")}


def test_every_enqueue_wrapper_passes_every_argument_in_the_headers_order():
    """The raw wrappers that came after the recorded list was closed, every `*_enqueue` method of HipDevice, over the recording
    library and the synthesised cases (default, another stream, every buffer as None, every option off its default): one call,
    of vkmr_hip_<name>_async, with (device, stream) and then the wrapper's own parameters in declaration order; as many of them
    as the header declares behind `dev, s`, and a `_buf` exactly where the header's is a pointer or a handle."""
    from abi_support import POINTER, ctypes_of, declarations
    from vk_merkle_roots_amd import _abi, engine
    covered = set()
    for method in calls.methods("_enqueue"):
        c_name = "vkmr_hip_" + method[: -len("_enqueue")] + "_async"
        declared = declarations()[c_name]
        assert [t for t, _ in declared.params[:2]] == ["int", "vkmr_stream"], c_name
        own = [p for p in inspect.signature(getattr(engine.HipDevice, method)).parameters if p not in ("self", "stream")]
        kinds = ctypes_of(declared)[1][2:]
        assert len(own) == len(kinds), (method, own, declared.params)
        assert [p.endswith("_buf") for p in own] == [k is POINTER for k in kinds], (method, own, declared.params)
        cases = calls.cases(method)
        assert {"default", "stream"} <= set(cases) and {f"{p}=None" for p in own if p.endswith("_buf")} <= set(cases), method
        for case, kwargs in cases.items():
            kw = dict(kwargs)
            stream = kw.pop("stream", calls.DEVICE_STREAM)
            assert list(kw) == own, (method, case)
            want = [calls.DEVICE_INDEX, stream] + [getattr(v, "ptr", v) for v in kw.values()]      # the parameters in declaration order
            assert calls.record(method, kwargs) == [c_name, want], (method, case)
            assert len(want) == len(_abi.SIGNATURES[c_name][1]), (method, case)
        covered.add(method)
    assert covered == {n for n in dir(engine.HipDevice) if n.endswith("_enqueue")} and len(covered) >= 27     # a new wrapper cannot stay outside
    assert {"forest_audit_enqueue", "tree_audit_enqueue"} <= covered


def test_every_wrapper_is_recorded():
    assert calls.methods() == sorted(RECORDED)
    for method, cases in RECORDED.items():
        assert {"default", "stream"} <= set(cases), method
        assert set(cases) <= set(calls.cases(method)), method


@pytest.mark.parametrize("method", sorted(RECORDED))
def test_the_wrapper_passes_the_recorded_arguments(method):
    from vk_merkle_roots_amd import _abi
    synthesised = calls.cases(method)
    for case, (c_name, args) in RECORDED[method].items():
        got = calls.record(method, synthesised[case])
        assert got is not None, (method, case)
        assert got == [c_name, args], (method, case)
        assert c_name in _abi.SIGNATURES, (method, case)
        assert len(got[1]) == len(_abi.SIGNATURES[c_name][1]), (method, case)
