"""What HipDevice's `*_async` wrappers hand to the C ABI, without a GPU: every call recorded in tests/golden/engine_calls.json
(written by tests/golden/make_engine_calls.py from the wrappers as they were before they shared one call path) replayed with
the same helper over a recording library, and compared argument for argument."""
import importlib.util
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
