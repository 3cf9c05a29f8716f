#!/usr/bin/env python3
"""Generates tests/golden/engine_calls.json: what every `*_async` wrapper of engine.HipDevice hands to the C ABI
(include/vkmr_hip.h) -- the C function's name and its argument list -- for arguments synthesised from the wrapper's own
signature.  tests/test_engine_calls.py replays the recorded cases and asserts that the wrappers still pass the same
arguments, so a change to how they forward (one shared call path, say) cannot move an argument with it.

No library is loaded and no GPU is needed: the device is made without __init__ and its `lib` is a recorder.  Run it on the
engine.py whose calls are to be pinned, BEFORE the change that must keep them:

    python tests/golden/make_engine_calls.py
"""
import inspect
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "engine_calls.json")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DEVICE_INDEX, DEVICE_STREAM, OTHER_STREAM = 3, 0x5000, 0x6000


class Buf:
    """Stands for a DeviceBuffer: a pointer, and at() for a byte offset into it."""

    def __init__(self, ptr):
        self.ptr = ptr

    def at(self, byte_offset):
        return self.ptr + int(byte_offset)


class Recorder:
    """Stands for the ctypes library: every function returns 0 and notes (C name, arguments)."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, list(args)))
            return 0
        return fn


def device():
    from vk_merkle_roots_amd import engine
    dev = object.__new__(engine.HipDevice)
    dev.lib, dev.index, dev.stream = Recorder(), DEVICE_INDEX, DEVICE_STREAM
    return dev


def methods(suffix="_async"):
    """The public `*_async` methods of HipDevice, by name (or those of another suffix: the record holds only these)."""
    from vk_merkle_roots_amd import engine
    return sorted(n for n, f in vars(engine.HipDevice).items() if n.endswith(suffix) and not n.startswith("_") and inspect.isfunction(f))


def cases(method):
    """{case: keyword arguments} for one wrapper: a distinct buffer for each *_buf parameter, a distinct small integer for each
    other positional one; `default`, `stream`, each option at a value that is not its default, each buffer as None."""
    from vk_merkle_roots_amd import engine
    params = [p for p in inspect.signature(getattr(engine.HipDevice, method)).parameters.values() if p.name not in ("self", "stream")]
    base, options = {}, {}
    for i, p in enumerate(params):
        if p.name.endswith("_buf"):
            base[p.name] = Buf(0x100000 * (i + 1))
        elif p.default is inspect.Parameter.empty:
            base[p.name] = 11 + i
        else:
            options[p.name] = True if isinstance(p.default, bool) else p.default + 7
    out = {"default": dict(base), "stream": dict(base, stream=OTHER_STREAM)}
    for name, value in options.items():
        out[f"{name}={value}"] = dict(base, **{name: value})
    for name in base:
        if name.endswith("_buf"):
            out[f"{name}=None"] = dict(base, **{name: None})
    return out


def record(method, kwargs):
    """[C name, arguments] of the one ABI call the wrapper makes, or None when it refuses a None buffer by itself."""
    dev = device()
    try:
        getattr(dev, method)(**kwargs)
    except AttributeError:
        return None
    (call,) = dev.lib.calls
    return [call[0], call[1]]


def main():
    rec = {"_about": "wrapper -> {case: [C name, arguments]} of engine.HipDevice's *_async wrappers over a recording library "
                     f"(device {DEVICE_INDEX}, stream {DEVICE_STREAM}), recorded before the wrappers shared one call path; "
                     "regenerate with tests/golden/make_engine_calls.py"}
    total = 0
    for m in methods():
        got = {c: record(m, kw) for c, kw in cases(m).items()}
        rec[m] = {c: r for c, r in got.items() if r is not None}
        total += len(rec[m])
    with open(OUT, "w") as f:   # one line per wrapper: a moved argument shows as one changed line
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in rec.items()) + "\n}\n")
    print("wrote", OUT, len(rec) - 1, "wrappers,", total, "calls")


if __name__ == "__main__":
    main()
