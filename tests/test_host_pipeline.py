"""The host logic of the GPU backend on a CPU-only machine: the UNMODIFIED stream processor, pools, mappings,
reductions and the several-device combine (csrc/host/*.cpp) built with AddressSanitizer + UBSan and linked
against a test double of the C ABI (tests/c/fake_vkmr_hip.cpp: host memory, asynchronous-looking events, hashing
by the product's own "CPU" functions, optional HBM cap and injected device failures).  What the GPU suite cannot
provoke on demand -- real allocation failures, failing events, failing dispatches -- is checked here: the root is
the golden one, or there is no root, never a wrong one.  The double is test infrastructure, not a fallback: the
product never loads it."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

HOST = os.path.join(ROOT, "vk_merkle_roots_amd", "csrc", "host")
CSRC = os.path.join(ROOT, "vk_merkle_roots_amd", "csrc")
OUT = os.path.join(ROOT, "tests", "_build", "fake")
LINE = re.compile(r"^(?P<name>.+?): computed root \(of (?P<items>\d+) item\(s\), (?P<bytes>\d+) byte\(s\)\) => (?P<root>[0-9a-f]*) in [0-9.e+-]+$")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]


def _newer(target, sources):
    return os.path.exists(target) and all(os.path.getmtime(s) <= os.path.getmtime(target) for s in sources)


def _build_fake_vkmr(native, defines=(), suffix=""):
    os.makedirs(OUT, exist_ok=True)
    inc = ["-I", os.path.join(ROOT, "include"), "-I", HOST, "-I", CSRC]
    lib = os.path.join(OUT, "libvkmr_hip.so")
    lib_src = [os.path.join(ROOT, "tests", "c", "fake_vkmr_hip.cpp"), os.path.join(HOST, "cpu_sha256d.cpp")]
    hdrs = [os.path.join(ROOT, "include", "vkmr_hip.h"), os.path.join(CSRC, "reduce_plan.hpp")]
    if not _newer(lib, lib_src + hdrs):
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-shared", "-fPIC"] + SAN + inc + lib_src + ["-o", lib])
    exe = os.path.join(OUT, "vkmr_asan" + suffix)
    files = ["vkmr_main.cpp", "cpu_sha256d.cpp", "hip_sha256d.cpp", "inputs.cpp", "batches.cpp", "slices.cpp", "mappings.cpp", "reductions.cpp",
             "stream_pack.cpp"]
    srcs = [os.path.join(HOST, f) for f in files]
    deps = srcs + [os.path.join(HOST, f) for f in os.listdir(HOST) if f.endswith(".hpp")] + hdrs + [lib]
    if not _newer(exe, deps):
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-pthread"] + SAN + list(defines) + inc + srcs + ["-o", exe, "-L", OUT, "-lvkmr_hip", "-Wl,-rpath," + OUT])
    env = {k: v for k, v in os.environ.items() if not k.startswith("VKMR_") and k != "LD_PRELOAD"}
    env.update(LD_LIBRARY_PATH=OUT, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    return exe, env


@pytest.fixture(scope="session")
def fake_vkmr(native):
    """(path of the sanitized vkmr linked against the fake ABI, base environment)."""
    return _build_fake_vkmr(native)


@pytest.fixture(scope="session")
def fake_vkmr_experiments(native):
    """The same front end built with -DVKMR_EXPERIMENTS: the host side of the paths that are measured but not shipped
    (the device-split mode, include/vkmr_hip_experiments.h)."""
    return _build_fake_vkmr(native, ["-DVKMR_EXPERIMENTS"], "_exp")


def run(fake_vkmr, backend, stream, **knobs):
    exe, env = fake_vkmr
    env = dict(env, **{k: str(v) for k, v in knobs.items()})
    r = subprocess.run([exe, backend], input=stream, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
    assert b"AddressSanitizer" not in r.stderr and b"runtime error" not in r.stderr and b"LeakSanitizer" not in r.stderr, r.stderr[-3000:].decode()
    out = r.stdout.decode().splitlines()
    res = [m for m in (LINE.match(l) for l in out) if m]
    return r, out, (res[-1].groupdict() if res else None)


def stream_of(native, s):
    tool = os.path.join(os.path.dirname(native.HIP_LIB), "bin", "rndm")
    if "stream_hex" in s:
        return bytes.fromhex(s["stream_hex"])
    return subprocess.run([tool] + s["generator"].split()[1:], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout


SHAPES = [
    {},
    {"VKMR_SLICE_LOG2": 10, "VKMR_BATCH_BYTES": 65536, "VKMR_MAX_INFLIGHT": 2},
    {"VKMR_SLICE_LOG2": 12, "VKMR_BATCH_BYTES": 20000, "VKMR_MAX_INFLIGHT": 1, "VKMR_FAKE_EVENT_POLLS": 7},
    {"VKMR_SLICE_LOG2": 6, "VKMR_BATCH_BYTES": 8192, "VKMR_SLICE_BUDGET": 1, "VKMR_FAKE_EVENT_POLLS": 0},
    {"VKMR_SLICE_LOG2": 16, "VKMR_BATCH_MB": 1, "VKMR_VERBOSE": 1, "VKMR_PACK_THREADS": 5},
]


@pytest.mark.parametrize("shape", SHAPES)
def test_golden_streams_through_the_host_pipeline(fake_vkmr, native, golden, shape):
    for name in ("G2_rndm_1712489279_1024_127", "G6_rndm_7_1000_300", "G4_rndm_42_4096_4096", "L2_empty_lines", "L3_no_trailing_newline", "L7_three"):
        s = golden["streams"][name]
        r, out, m = run(fake_vkmr, "hip:0", stream_of(native, s), **shape)
        assert r.returncode == 0, r.stderr[-500:]
        assert m and (m["name"], int(m["items"]), int(m["bytes"]), m["root"]) == ("hip:0", s["items"], s["bytes"], s["root"]), (name, shape)


@pytest.mark.parametrize("ndev,shape", [(2, {"VKMR_SLICE_LOG2": 7}), (3, {"VKMR_SLICE_LOG2": 5, "VKMR_BATCH_BYTES": 8192}),
                                        (8, {"VKMR_SLICE_LOG2": 7}), (5, {"VKMR_SLICE_LOG2": 9}), (4, {"VKMR_SLICE_LOG2": 3, "VKMR_SLICE_BUDGET": 1})])
def test_hip_all_over_several_devices(fake_vkmr, native, golden, ndev, shape):
    """Slices dealt round-robin, one root array per device, ONE gather, slice order, combine on the first device --
    including fewer slices than devices and more than 4096 / ndev slices per device is not needed to see the order."""
    for name in ("G2_rndm_1712489279_1024_127", "G6_rndm_7_1000_300", "L7_three"):
        s = golden["streams"][name]
        r, out, m = run(fake_vkmr, "hip:all", stream_of(native, s), VKMR_FAKE_DEVICES=ndev, **shape)
        assert r.returncode == 0 and out[0] == "Initializing for: hip:all", r.stderr[-500:]
        assert m and (int(m["items"]), m["root"]) == (s["items"], s["root"]), (name, ndev, shape)


def test_device_can_be_chosen_by_its_marketing_name(fake_vkmr, native, golden):
    """The reference takes a Vulkan deviceName on the command line (Vkmr.cpp:69-96); a HIP marketing name works too."""
    s = golden["streams"]["L7_three"]
    r, out, m = run(fake_vkmr, "fake device 1", stream_of(native, s), VKMR_FAKE_DEVICES=3)
    assert r.returncode == 0 and out[0] == "Initializing for: fake device 1" and m and m["root"] == s["root"]
    r, out, m = run(fake_vkmr, "hip:7", b"a\n", VKMR_FAKE_DEVICES=3)
    assert r.returncode == 1 and b"No device selected; aborting." in r.stderr
    r, out, m = run(fake_vkmr, "hip:all", b"a\n", VKMR_FAKE_DEVICES=1)      # one device: no "hip:all"
    assert r.returncode == 1


def test_root_array_grows_past_its_first_capacity(fake_vkmr, native, oracle):
    """More than 4096 slices on one device: the per-device root array is re-allocated and the roots copied over."""
    tool = os.path.join(os.path.dirname(native.HIP_LIB), "bin", "rndm")
    stream = subprocess.run([tool, "5", "20000", "20"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout
    want, cnt, nb = oracle.root_of_stream(stream)
    r, out, m = run(fake_vkmr, "hip:0", stream, VKMR_SLICE_LOG2=2)          # 5000 slices of 4
    assert m and (m["root"], int(m["items"])) == (want, cnt), r.stderr[-300:]
    r, out, m = run(fake_vkmr, "hip:all", stream, VKMR_SLICE_LOG2=1, VKMR_FAKE_DEVICES=2)   # 10000 slices over 2 devices
    assert m and m["root"] == want


def test_real_allocation_failures_wait_instead_of_halting(fake_vkmr, native, golden):
    """HBM that holds two slices plus the batches: device_alloc returns VKMR_ERR_OOM, the stream processor blocks on the
    oldest reduction / mapping and re-uses what comes back (reference README.md:113; it halts, SHA-256vk.cpp:396-399)."""
    s = golden["streams"]["G6_rndm_7_1000_300"]
    stream = stream_of(native, s)
    # slices of 2^5 cells = 1 KiB; batches of 16 KiB data + 4 KiB meta per landing zone; scratch and root arrays are small
    # the root array (4096 x 32 B) and one scratch set are reserved when the backend starts: 131 KiB
    for hbm, budget in ((400000, 64), (260000, 64), (160000, 8)):
        r, out, m = run(fake_vkmr, "hip:0", stream, VKMR_SLICE_LOG2=5, VKMR_BATCH_BYTES=16384, VKMR_BATCH_MAX_MB=0, VKMR_MAX_INFLIGHT=4,
                        VKMR_SLICE_BUDGET=budget, VKMR_FAKE_HBM_BYTES=hbm)
        assert r.returncode == 0, r.stderr[-500:]
        assert m and (int(m["items"]), m["root"]) == (s["items"], s["root"]), (hbm, r.stderr[-300:])


def test_no_room_for_the_reduction_reserve_is_reported_at_start(fake_vkmr):
    r, out, m = run(fake_vkmr, "hip:0", b"a\nb\n", VKMR_SLICE_LOG2=5, VKMR_FAKE_HBM_BYTES=100000)
    assert r.returncode == 0 and m is None
    assert b"Failed to prepare reductions" in r.stderr


def test_allocation_failure_with_nothing_in_flight_is_reported(fake_vkmr):
    """No room for even the first batch: Add() refuses, nothing is printed, exit code 0 (reference Vkmr.cpp:44-52)."""
    r, out, m = run(fake_vkmr, "hip:0", b"a\nb\n", VKMR_SLICE_LOG2=20, VKMR_FAKE_HBM_BYTES=30 << 20)   # the default 64 MiB batch does not fit 30 MiB
    assert r.returncode == 0 and m is None
    assert b"Failed to allocate a batch" in r.stderr


def test_a_slice_size_that_does_not_fit_is_clamped_with_a_message(fake_vkmr, native, golden):
    """the slice capacity is derived from the devices (reference Slices<T>::SliceSize, Slices.h:421-454:
    the largest power of two within the device limits); a VKMR_SLICE_LOG2 beyond what free memory holds is clamped and
    said so, instead of being discovered by a failed allocation."""
    s = golden["streams"]["G6_rndm_7_1000_300"]
    r, out, m = run(fake_vkmr, "hip:0", stream_of(native, s), VKMR_SLICE_LOG2=30, VKMR_BATCH_BYTES=65536, VKMR_BATCH_MAX_MB=0, VKMR_FAKE_HBM_BYTES=8 << 20,
                    VKMR_VERBOSE=1)
    assert r.returncode == 0 and m and m["root"] == s["root"], r.stderr[-400:]
    assert b"VKMR_SLICE_LOG2=30 does not fit the device memory" in r.stderr
    line = [l for l in out if l.startswith("Slices of 2^")]
    assert line and 1 <= int(line[0].split("2^")[1].split()[0]) < 30 and "clamped" in line[0]
    # and without the knob: the reference's 2^23, or less when memory is short
    r, out, m = run(fake_vkmr, "hip:0", stream_of(native, s), VKMR_VERBOSE=1)
    assert m and m["root"] == s["root"] and any(l.startswith("Slices of 2^23 digests (the reference's 256 MiB slice") for l in out)
    r, out, m = run(fake_vkmr, "hip:0", stream_of(native, s), VKMR_VERBOSE=1, VKMR_BATCH_BYTES=65536, VKMR_BATCH_MAX_MB=0, VKMR_FAKE_HBM_BYTES=8 << 20)
    line = [l for l in out if l.startswith("Slices of 2^")]
    assert m and m["root"] == s["root"] and line and int(line[0].split("2^")[1].split()[0]) < 23 and b"does not fit" not in r.stderr


def test_hip_all_deals_one_slice_per_device_when_the_input_size_is_known(fake_vkmr, native, oracle, tmp_path):
    """`vkmr hip:all < file` on an 8-GPU node: no knob, the slice capacity becomes ceil(expected leaves / 8) rounded up to a
    power of two -- BASELINE's north star shape, one slice per GPU (2^29 leaves -> 2^26 per GPU; here 2^17 -> 2^14)."""
    tool = os.path.join(os.path.dirname(native.HIP_LIB), "bin", "rndm")
    f = tmp_path / "in.txt"
    with open(f, "wb") as fh:
        subprocess.run([tool, "11", str(1 << 17), "127"], stdout=fh, stderr=subprocess.DEVNULL, check=True)
    want, cnt, nb = oracle.root_of_stream(f.read_bytes())
    exe, env = fake_vkmr
    env = dict(env, VKMR_FAKE_DEVICES="8", VKMR_VERBOSE="1", VKMR_BATCH_MB="1")
    with open(f, "rb") as fh:
        r = subprocess.run([exe, "hip:all"], stdin=fh, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
    assert b"AddressSanitizer" not in r.stderr and b"runtime error" not in r.stderr, r.stderr[-2000:].decode()
    out = r.stdout.decode().splitlines()
    res = [m for m in (LINE.match(l) for l in out) if m]
    assert res and res[-1].group("root") == want and int(res[-1].group("items")) == cnt
    line = [l for l in out if l.startswith("Slices of 2^")]
    assert line and line[0].startswith("Slices of 2^14 digests (one slice per device for about"), line
    filled = [l for l in out if l.startswith("Slice #") and "has been filled" in l]
    alloc = [l for l in out if l.startswith("Allocations:")]
    assert alloc and " for 8 slice(s)" in alloc[0], (alloc, len(filled))
    # through a pipe the size is unknown: the reference's slice size is used
    r = subprocess.run([exe, "hip:all"], input=f.read_bytes(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
    out = r.stdout.decode().splitlines()
    assert any(l.startswith("Slices of 2^23 digests") for l in out) and [m for m in (LINE.match(l) for l in out) if m][-1].group("root") == want


@pytest.mark.parametrize("knobs", [
    {},
    {"VKMR_PACK_THREADS": 5, "VKMR_INPUT_SPAN_MB": 2, "VKMR_BATCH_MB": 3, "VKMR_SLICE_LOG2": 15},     # most spans hold more strings than the slice has room for
    {"VKMR_PACK_THREADS": 7, "VKMR_INPUT_SPAN_MB": 3, "VKMR_SLICE_LOG2": 18, "VKMR_MAX_INFLIGHT": 1},
    {"VKMR_PACK_THREADS": 1, "VKMR_INPUT_SPAN_MB": 5, "VKMR_BATCH_MB": 4},                            # the span does not fit the batch's text area
])
def test_text_split_on_the_device(fake_vkmr_experiments, native, golden, oracle, knobs, tmp_path):
    """EXPERIMENTS BUILD (the mode measured no gain and is not in the product: the product front end ignores the knob, see the
    last lines).  VKMR_DEVICE_SPLIT=1: spans of 1 MiB and more are copied into pinned memory as they are (their lines counted on the
    way), split into strings by vkmr_hip_split_text_async, and mapped; spans that do not qualify take the host packer.  The
    golden 2^20-string stream from a file and through a pipe, and a stream with runs of empty lines, CRs and no final
    newline, for thread counts that do not divide the spans, spans larger than the batch, and slices smaller than a span:
    always the reference's root, items and bytes -- and the device path was taken (the fake ABI counts its calls)."""
    s = golden["streams"]["G3_rndm_42_1048576_127"]
    stream = stream_of(native, s)
    odd = b"\n\n" + stream[:3 << 20].replace(b"a", b"\r\n\n", 40).replace(b"b", b"\n", 5000)[:-1]
    want_odd = oracle.root_of_stream(odd)
    path = tmp_path / "g3.txt"
    path.write_bytes(stream)
    for body, want, via_file in ((stream, (s["root"], s["items"], s["bytes"]), True), (stream, (s["root"], s["items"], s["bytes"]), False), (odd, want_odd, False)):
        exe, env = fake_vkmr_experiments
        env = dict(env, VKMR_DEVICE_SPLIT="1", VKMR_FAKE_COUNT_FORMS="1", **{k: str(v) for k, v in knobs.items()})
        if via_file:
            with open(path, "rb") as f:
                r = subprocess.run([exe, "hip:0"], stdin=f, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
        else:
            r = subprocess.run([exe, "hip:0"], input=body, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
        assert b"Sanitizer" not in r.stderr and b"runtime error" not in r.stderr, r.stderr[-2000:].decode()
        m = [x for x in (LINE.match(l) for l in r.stdout.decode().splitlines()) if x][-1].groupdict()
        assert (m["root"], int(m["items"]), int(m["bytes"])) == tuple(want), (knobs, via_file)
        split = [l for l in r.stderr.decode().splitlines() if l.startswith("fake: texts split on the device")]
        assert split and int(re.findall(r"(\d+)", split[-1])[0]) > 0, r.stderr[-300:]


def test_the_product_front_end_has_no_device_split_mode(fake_vkmr, native, golden):
    """an opt-in mode that measured no gain is not a product feature.  The product build of the front end does
    not read VKMR_DEVICE_SPLIT: same root, and the device-side splitter is never called."""
    s = golden["streams"]["G3_rndm_42_1048576_127"]
    r, out, m = run(fake_vkmr, "hip:0", stream_of(native, s), VKMR_DEVICE_SPLIT=1, VKMR_FAKE_COUNT_FORMS=1)
    assert m["root"] == s["root"]
    split = [l for l in r.stderr.decode().splitlines() if l.startswith("fake: texts split on the device")]
    assert not split or int(re.findall(r"(\d+)", split[-1])[0]) == 0


def test_batches_cross_as_sizes_or_as_entries(fake_vkmr, native, oracle):
    """A batch whose strings are all shorter than 65 536 bytes is described to the device by 16-bit sizes
    (vkmr_hip_metadata_from_sizes_async writes the entries there); one string of 65 535 bytes or more and the batch goes
    with its 8-byte entries, as the reference sends them.  Both give the oracle's root, at the boundary sizes, with the
    long string first, last, alone in its batch, and with VKMR_SEND_METADATA=1 forcing the entries throughout; the fake
    ABI counts which form each batch took."""
    tool = os.path.join(os.path.dirname(native.HIP_LIB), "bin", "rndm")
    short = subprocess.run([tool, "9", "3000", "200"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout
    cases = {"short only": short,
             "65534 bytes": b"a" * 65534 + b"\n" + short,
             "65535 bytes": short + b"b" * 65535 + b"\n",
             "65536 bytes in the middle": short + b"c" * 65536 + b"\n" + short,
             "70000 bytes alone": b"d" * 70000 + b"\n"}
    for name, stream in cases.items():
        want, cnt, nb = oracle.root_of_stream(stream)
        for knobs in ({}, {"VKMR_SEND_METADATA": 1}, {"VKMR_BATCH_BYTES": 262144, "VKMR_BATCH_MAX_MB": 0, "VKMR_SLICE_LOG2": 9}):
            r, out, m = run(fake_vkmr, "hip:0", stream, VKMR_FAKE_COUNT_FORMS=1, **knobs)
            assert m and (int(m["items"]), m["root"]) == (cnt, want), (name, knobs, r.stderr[-300:])
            forms = [l for l in r.stderr.decode().splitlines() if l.startswith("fake: batches described by")]
            assert forms, r.stderr[-300:]
            by_sizes, by_entries = (int(x) for x in re.findall(r"(\d+)", forms[-1])[:2])
            if knobs.get("VKMR_SEND_METADATA"):
                assert by_sizes == 0 and by_entries > 0, (name, knobs, forms)
            elif name in ("short only", "65534 bytes"):
                assert by_entries == 0 and by_sizes > 0, (name, knobs, forms)
            else:
                assert by_entries > 0, (name, knobs, forms)


@pytest.mark.parametrize("which", range(1, 40, 3))
def test_a_failing_event_never_yields_a_wrong_root(fake_vkmr, native, golden, which):
    """a mapping or reduction whose event reports a device error must not contribute a zero-filled or
    missing root.  Whatever event fails, the printed root is the golden one (the failure hit nothing that mattered,
    e.g. a timing event) or empty -- never anything else."""
    s = golden["streams"]["G6_rndm_7_1000_300"]
    r, out, m = run(fake_vkmr, "hip:0", stream_of(native, s), VKMR_SLICE_LOG2=6, VKMR_BATCH_BYTES=16384, VKMR_FAKE_FAIL_EVENT=which,
                    VKMR_FAKE_EVENT_POLLS=1)
    assert r.returncode == 0
    assert m is None or m["root"] in ("", s["root"]), (which, m)
    if m is not None and m["root"] == "":
        assert b"failed" in r.stderr or b"Reduced" in r.stderr


@pytest.mark.parametrize("which", [1, 2, 7, 16])
def test_a_failing_reduce_dispatch_yields_no_root(fake_vkmr, native, golden, which):
    """The last slice's Reduce failing used to leave the roots of slices 1..n-1 to be combined and printed."""
    s = golden["streams"]["G6_rndm_7_1000_300"]        # 1000 strings, slices of 64: 16 reductions
    r, out, m = run(fake_vkmr, "hip:0", stream_of(native, s), VKMR_SLICE_LOG2=6, VKMR_FAKE_FAIL_REDUCE=which)
    assert r.returncode == 0
    assert m is None or m["root"] == "", (which, m)
    assert b"Failed to dispatch a reduction" in r.stderr


def test_hip_all_combine_failure_is_loud(fake_vkmr, native, golden):
    s = golden["streams"]["G2_rndm_1712489279_1024_127"]
    # 16 slices over 4 devices; the 17th reduce call is the combine on device 0
    r, out, m = run(fake_vkmr, "hip:all", stream_of(native, s), VKMR_SLICE_LOG2=6, VKMR_FAKE_DEVICES=4, VKMR_FAKE_FAIL_REDUCE=17)
    assert m is None or m["root"] == ""
    assert b"Failed to combine the slice roots" in r.stderr


COUNTED = {"VKMR_SLICE_LOG2": 8, "VKMR_BATCH_BYTES": 16384, "VKMR_MAX_INFLIGHT": 2, "VKMR_FAKE_COUNT_CALLS": 1}
BACKENDS = [("hip:0", {}), ("hip:all", {"VKMR_FAKE_DEVICES": 3})]
_counted_streams = {}


def counted_calls(fake_vkmr, native, backend, strings, **knobs):
    """`rndm 7 <strings> 60` through the front end on the double; the counters of its "fake: calls" line, and the result line."""
    if strings not in _counted_streams:
        _counted_streams[strings] = stream_of(native, {"generator": "rndm 7 %d 60" % strings})
    r, out, m = run(fake_vkmr, backend, _counted_streams[strings], **dict(COUNTED, **knobs))
    lines = [l for l in r.stderr.decode().splitlines() if l.startswith("fake: calls ")]
    assert r.returncode == 0 and len(lines) == 1, r.stderr[-500:]
    return {k: int(v) for k, v in (f.split("=") for f in lines[0].split()[2:])}, m


@pytest.mark.parametrize("backend,devices", BACKENDS)
@pytest.mark.parametrize("injected,has_root", [
    ({}, True), ({"VKMR_FAKE_FAIL_EVENT": 1}, False), ({"VKMR_FAKE_FAIL_EVENT": 2}, False), ({"VKMR_FAKE_FAIL_EVENT": 5}, False),
    ({"VKMR_FAKE_FAIL_REDUCE": 1}, False), ({"VKMR_FAKE_HBM_BYTES": 400000}, True), ({"VKMR_FAKE_HBM_BYTES": 260000}, True),
    ({"VKMR_FAKE_HBM_BYTES": 160000}, False), ({"VKMR_PROOF_INDEX": 777}, True)])
def test_every_hip_resource_is_released_exactly_once(fake_vkmr, native, backend, devices, injected, has_root):
    """Every device buffer, pinned buffer, event and stream of the front end has one owner (csrc/host/hip_handles.hpp): when
    the process ends, as many were freed as were allocated -- on a clean run, with a failing event, a failing dispatch,
    device memory that runs out on the way (the first two sizes) or at the start (the third), and with a proof asked for.
    (LeakSanitizer sees the double's malloc behind a leak; a double free of a pooled event or stream only shows here.)"""
    calls, m = counted_calls(fake_vkmr, native, backend, 20000, **dict(devices, **injected))
    for made, released in (("device_alloc", "device_free"), ("host_alloc", "host_free"), ("event_create", "event_destroy"), ("stream_create", "stream_destroy")):
        assert calls[made] == calls[released] and calls[made] > 0, (made, calls)
    assert bool(m and m["root"]) == has_root, (m, calls)


@pytest.mark.parametrize("backend,devices", BACKENDS)
def test_a_longer_stream_allocates_nothing_more(fake_vkmr, native, backend, devices):
    """The pools hold: twice the strings -- twice the batches, mappings and reductions -- and not one more device buffer,
    pinned buffer or event (hipMalloc / hipFree synchronise the device, pinning a batch is 10-15 ms).  Events complete at
    once and one thread packs, so that the counts do not depend on timing; all three were equal at both lengths before
    the handles too (profiles/host_handles_calls.txt)."""
    knobs = dict(devices, VKMR_FAKE_EVENT_POLLS=0, VKMR_PACK_THREADS=1)
    short, m1 = counted_calls(fake_vkmr, native, backend, 20000, **knobs)
    long_, m2 = counted_calls(fake_vkmr, native, backend, 40000, **knobs)
    assert m1 and m2 and m1["root"] and m2["root"] and int(m2["items"]) == 2 * int(m1["items"]) == 40000
    assert long_["map_async"] > short["map_async"] and long_["reduce_async"] > short["reduce_async"], (short, long_)
    for made in ("device_alloc", "host_alloc", "event_create"):
        assert long_[made] == short[made], (made, short, long_)


def test_parallel_packer_in_the_pipeline_under_tsan(native, golden, tmp_path):
    """The fork-join packer feeding the stream processor (mapped file, spans cut at line ends, parts packed at their
    prefix offsets into the pinned batch) under ThreadSanitizer, end to end through the fake ABI."""
    os.makedirs(OUT, exist_ok=True)
    inc = ["-I", os.path.join(ROOT, "include"), "-I", HOST, "-I", CSRC]
    tsan = ["-fsanitize=thread", "-g", "-O1"]
    lib = os.path.join(OUT, "tsan", "libvkmr_hip.so")
    os.makedirs(os.path.dirname(lib), exist_ok=True)
    lib_src = [os.path.join(ROOT, "tests", "c", "fake_vkmr_hip.cpp"), os.path.join(HOST, "cpu_sha256d.cpp")]
    files = ["vkmr_main.cpp", "cpu_sha256d.cpp", "hip_sha256d.cpp", "inputs.cpp", "batches.cpp", "slices.cpp", "mappings.cpp", "reductions.cpp",
             "stream_pack.cpp"]
    srcs = [os.path.join(HOST, f) for f in files]
    exe = os.path.join(OUT, "tsan", "vkmr_tsan")
    deps = srcs + lib_src + [os.path.join(HOST, f) for f in os.listdir(HOST) if f.endswith(".hpp")] + [os.path.join(ROOT, "include", "vkmr_hip.h")]
    if not _newer(exe, deps):
        subprocess.check_call(["g++", "-std=c++17", "-shared", "-fPIC"] + tsan + inc + lib_src + ["-o", lib])
        subprocess.check_call(["g++", "-std=c++17", "-pthread"] + tsan + inc + srcs + ["-o", exe, "-L", os.path.dirname(lib), "-lvkmr_hip",
                               "-Wl,-rpath," + os.path.dirname(lib)])
    s = golden["streams"]["G3_rndm_42_1048576_127"]
    path = tmp_path / "g3.txt"
    path.write_bytes(stream_of(native, s))
    env = {k: v for k, v in os.environ.items() if not k.startswith("VKMR_") and k != "LD_PRELOAD"}
    env.update(LD_LIBRARY_PATH=os.path.dirname(lib), VKMR_PACK_THREADS="6", VKMR_BATCH_MB="8", VKMR_SLICE_LOG2="17", VKMR_INPUT_SPAN_MB="4",
               TSAN_OPTIONS="halt_on_error=0")
    with open(path, "rb") as f:
        r = subprocess.run([exe, "hip:0"], stdin=f, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=900)
    assert b"ThreadSanitizer" not in r.stderr, r.stderr[-3000:].decode()
    m = [x for x in (LINE.match(l) for l in r.stdout.decode().splitlines()) if x][-1].groupdict()
    assert (int(m["items"]), int(m["bytes"]), m["root"]) == (s["items"], s["bytes"], s["root"])
    # the device-split path: the fork-join copy-and-count into the pinned text area
    with open(path, "rb") as f:
        r = subprocess.run([exe, "hip:0"], stdin=f, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(env, VKMR_DEVICE_SPLIT="1"), timeout=900)
    assert b"ThreadSanitizer" not in r.stderr, r.stderr[-3000:].decode()
    m = [x for x in (LINE.match(l) for l in r.stdout.decode().splitlines()) if x][-1].groupdict()
    assert (int(m["items"]), int(m["bytes"]), m["root"]) == (s["items"], s["bytes"], s["root"])
    # the same stream through a pipe: blocks of whole lines come from Input's reading thread (three buffers in turn, the
    # unfinished last line of one block carried into the next) while this thread and the pool pack the block before
    r = subprocess.run([exe, "hip:0"], input=path.read_bytes(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=900)
    assert b"ThreadSanitizer" not in r.stderr, r.stderr[-3000:].decode()
    m = [x for x in (LINE.match(l) for l in r.stdout.decode().splitlines()) if x][-1].groupdict()
    assert (int(m["items"]), int(m["bytes"]), m["root"]) == (s["items"], s["bytes"], s["root"])


def fold_proof(lines):
    """Folds "proof: ..." lines (leaf digest, then one sibling per level with its side) into a root, with hashlib."""
    import hashlib
    d = lambda b: hashlib.sha256(hashlib.sha256(b).digest()).digest()
    cur = bytes.fromhex(lines[0].split()[-1])
    for l in lines[1:]:
        _, _, level, side, hexsib = l.split()
        sib = bytes.fromhex(hexsib)
        cur = d(sib + cur) if side == "sibling-on-left" else d(cur + sib)
    return cur.hex()


@pytest.mark.parametrize("ndev,shape", [(1, {}), (1, {"VKMR_SLICE_LOG2": 6}), (1, {"VKMR_SLICE_LOG2": 4, "VKMR_SLICE_BUDGET": 1}), (3, {"VKMR_SLICE_LOG2": 5}),
                                        (8, {"VKMR_SLICE_LOG2": 3})])
def test_merkle_proof_of_a_leaf_folds_to_the_printed_root(fake_vkmr, native, golden, oracle, ndev, shape):
    """VKMR_PROOF_INDEX (the reference's to-do, README.md:118-120): the leaf's digest and one sibling per level -- inside
    the leaf's slice, then over the slice roots -- fold to the root the same run prints, for first, last, middle and
    ragged-edge leaves, one or several devices."""
    s = golden["streams"]["G6_rndm_7_1000_300"]
    stream = stream_of(native, s)
    lines_in = [l for l in stream.split(b"\n") if l]
    for index in (0, 512, 640, 999):
        r, out, m = run(fake_vkmr, "hip:all" if ndev > 1 else "hip:0", stream, VKMR_FAKE_DEVICES=ndev, VKMR_PROOF_INDEX=index, **shape)
        assert m and m["root"] == s["root"], (index, shape)
        proof = [l for l in out if l.startswith("proof: ")]
        assert proof[0].split()[:3] == ["proof:", "leaf", str(index)], proof[:2]
        assert proof[0].split()[-1] == oracle.hex(oracle.leaf(lines_in[index])), index
        assert fold_proof(proof) == s["root"], (index, ndev, shape)
    r, out, m = run(fake_vkmr, "hip:0", stream, VKMR_PROOF_INDEX=1000, **shape)      # one past the last leaf
    assert m["root"] == s["root"] and any("is not in the stream" in l for l in out)


def test_several_merkle_proofs_in_one_run(fake_vkmr, native, golden):
    """VKMR_PROOF_INDEX=a,b,c: the proofs are written by the reductions that hold the leaves (and by the combine above them);
    each block of lines folds to the root; a leaf beyond the stream is reported, not invented."""
    s = golden["streams"]["G2_rndm_1712489279_1024_127"]
    stream = stream_of(native, s)
    for shape in ({}, {"VKMR_SLICE_LOG2": 6}, {"VKMR_SLICE_LOG2": 5, "VKMR_FAKE_DEVICES": 3}):
        backend = "hip:all" if "VKMR_FAKE_DEVICES" in shape else "hip:0"
        r, out, m = run(fake_vkmr, backend, stream, VKMR_PROOF_INDEX="0,63,64,1023,517,5000,64", **shape)
        assert m["root"] == s["root"]
        proof = [l for l in out if l.startswith("proof: ")]
        blocks, cur = [], []
        for l in proof:
            if l.startswith("proof: leaf "):
                if cur:
                    blocks.append(cur)
                cur = [l]
            else:
                cur.append(l)
        blocks.append(cur)
        assert [b[0].split()[2] for b in blocks] == ["0", "63", "64", "1023", "517", "5000", "64"]
        for b in blocks:
            if b[0].split()[2] == "5000":
                assert "is not in the stream" in b[0] and len(b) == 1
            else:
                assert fold_proof(b) == s["root"], (shape, b[0])


def test_merkle_proof_of_a_lone_leaf(fake_vkmr):
    r, out, m = run(fake_vkmr, "hip:0", b"solo\n", VKMR_PROOF_INDEX=0)
    proof = [l for l in out if l.startswith("proof: ")]
    assert len(proof) == 2 and fold_proof(proof) == m["root"]      # a lone leaf is hashed with itself: one level


def test_packed_pipeline_entry_point_through_the_stream_processor(native, oracle, tmp_path):
    """vkmr_host_pipeline_packed (libvkmr_pipeline.so: bench.py's PCIe-inclusive measurement, bindings): pre-packed strings
    staged into the stream processor's own pinned batches, then Mappings / Reductions / combine as `vkmr hip:<n>` runs
    them.  Here built against the fake ABI (no sanitizer: it is loaded into a Python child) on 1 and 3 devices, several
    batch and slice shapes, against the oracle."""
    out = os.path.join(ROOT, "tests", "_build", "fake_plain")
    os.makedirs(out, exist_ok=True)
    inc = ["-I", os.path.join(ROOT, "include"), "-I", HOST, "-I", CSRC]
    fake = os.path.join(out, "libvkmr_hip.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-shared", "-fPIC"] + inc +
                          [os.path.join(ROOT, "tests", "c", "fake_vkmr_hip.cpp"), os.path.join(HOST, "cpu_sha256d.cpp"), "-o", fake])
    files = ["packed_pipeline.cpp", "cpu_sha256d.cpp", "hip_sha256d.cpp", "batches.cpp", "slices.cpp", "mappings.cpp", "reductions.cpp", "stream_pack.cpp"]
    lib = os.path.join(out, "libvkmr_pipeline.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-pthread", "-shared", "-fPIC"] + inc + [os.path.join(HOST, f) for f in files] +
                          ["-o", lib, "-L", out, "-lvkmr_hip", "-Wl,-rpath," + out])
    code = r'''
import ctypes as C, sys, json, numpy as np
sys.path.insert(0, %r)
import vk_merkle_roots_amd as vk
L = C.CDLL(%r)
L.vkmr_host_pipeline_packed.restype = C.c_int
L.vkmr_host_pipeline_packed.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_char_p, C.POINTER(C.c_double)]
res = []
for seed, n, maxlen, per_batch, slice_log2, dev in ((3, 5000, 127, 700, 10, 0), (4, 5000, 127, 5000, 0, 0), (5, 9000, 300, 1000, 11, -1), (6, 100, 40, 7, 3, -1), (7, 1, 9, 1, 0, 0)):
    b = vk.rndm_packed(seed, n, maxlen)
    hexbuf = C.create_string_buffer(65); secs = C.c_double()
    rc = L.vkmr_host_pipeline_packed(dev, b.data.ctypes.data, b.words, b.meta.ctypes.data, b.count, per_batch, slice_log2, hexbuf, C.byref(secs))
    res.append((seed, n, maxlen, rc, hexbuf.value.decode()))
L.vkmr_host_pipeline_text.restype = C.c_int
L.vkmr_host_pipeline_text.argtypes = [C.c_int, C.c_char_p, C.c_uint64, C.c_uint64, C.c_char_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
text = []
import subprocess
for seed, n, maxlen, span, dev in ((11, 40000, 127, 0, 0), (12, 40000, 127, 1 << 20, -1), (13, 300, 3000, 4096, 0), (14, 3, 5, 0, 0)):
    t = subprocess.run([%r, str(seed), str(n), str(maxlen)], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout
    for variant, body in (("as written", t), ("no final newline, empty lines, a CR", b"\n\n" + t[:-1].replace(b"\n", b"\r\n\n", 1))):
        hexbuf = C.create_string_buffer(65); items = C.c_uint64(); nbytes = C.c_uint64(); secs = C.c_double()
        rc = L.vkmr_host_pipeline_text(dev, body, len(body), span, hexbuf, C.byref(items), C.byref(nbytes), C.byref(secs))
        text.append((seed, n, maxlen, variant, rc, hexbuf.value.decode(), items.value, nbytes.value))
hexbuf = C.create_string_buffer(65); items = C.c_uint64(7); nbytes = C.c_uint64(7)
rc = L.vkmr_host_pipeline_text(0, b"\n\n\n", 3, 0, hexbuf, C.byref(items), C.byref(nbytes), None)
text.append((0, 0, 0, "only empty lines", rc, hexbuf.value.decode(), items.value, nbytes.value))
print(json.dumps([res, text]))
''' % (ROOT, lib, os.path.join(os.path.dirname(native.HIP_LIB), "bin", "rndm"))
    env = {k: v for k, v in os.environ.items() if not k.startswith("VKMR_") and k != "LD_PRELOAD"}
    env.update(VKMR_FAKE_DEVICES="3", VKMR_BATCH_MAX_MB="0")
    r = subprocess.run([os.sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:].decode()
    import json
    import vk_merkle_roots_amd as vk
    from vk_merkle_roots_amd.engine import digest_hex
    packed, text = json.loads(r.stdout.decode().splitlines()[-1])
    for seed, n, maxlen, rc, root in packed:
        b = vk.rndm_packed(seed, n, maxlen)
        want = digest_hex(oracle.root(oracle.leaves_packed(b.data, b.meta)))
        assert rc == 0 and root == want, (seed, n, maxlen, rc, root, want)
    # vkmr_host_pipeline_text: the reference's run() as one call on text in memory -- same line rules as stdin
    tool = os.path.join(os.path.dirname(native.HIP_LIB), "bin", "rndm")
    for seed, n, maxlen, variant, rc, root, items, nbytes in text:
        if variant == "only empty lines":
            assert (rc, root, items, nbytes) == (0, "", 0, 0)
            continue
        t = subprocess.run([tool, str(seed), str(n), str(maxlen)], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout
        body = t if variant == "as written" else b"\n\n" + t[:-1].replace(b"\n", b"\r\n\n", 1)
        want, cnt, nb = oracle.root_of_stream(body)
        assert (rc, root, items, nbytes) == (0, want, cnt, nb), (seed, n, maxlen, variant, rc, root, want)


def test_packed_pipeline_that_runs_out_of_slices_gives_up_cleanly(native, oracle, tmp_path):
    """vkmr_host_pipeline_packed stages every batch before it maps the first.  When staging fails half way
    (no device memory for the next slice) the instance still holds staged batches, each with a raw pointer into its
    pool: they must be released before the pools, not by the vector's destructor after them.  And with slice_log2 = 0
    the slice budget must follow the size the instance picks from the device's memory, not the 2^23 the caller guessed.
    The stream processor + entry point under ASan/UBSan against the fake ABI with an HBM cap."""
    import numpy as np
    import vk_merkle_roots_amd as vk
    from vk_merkle_roots_amd.engine import digest_hex
    out = os.path.join(ROOT, "tests", "_build", "fake")
    os.makedirs(out, exist_ok=True)
    inc = ["-I", os.path.join(ROOT, "include"), "-I", HOST, "-I", CSRC]
    lib = os.path.join(out, "libvkmr_hip.so")
    lib_src = [os.path.join(ROOT, "tests", "c", "fake_vkmr_hip.cpp"), os.path.join(HOST, "cpu_sha256d.cpp")]
    if not os.path.exists(lib):
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-shared", "-fPIC"] + SAN + inc + lib_src + ["-o", lib])
    files = ["packed_pipeline.cpp", "cpu_sha256d.cpp", "hip_sha256d.cpp", "batches.cpp", "slices.cpp", "mappings.cpp", "reductions.cpp", "stream_pack.cpp"]
    exe = os.path.join(out, "packed_pipeline_client_asan")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-pthread"] + SAN + inc + [os.path.join(ROOT, "tests", "c", "packed_pipeline_client.cpp")] +
                          [os.path.join(HOST, f) for f in files] + ["-o", exe, "-L", out, "-lvkmr_hip", "-Wl,-rpath," + out])
    b = vk.rndm_packed(21, 60000, 127)
    want = digest_hex(oracle.root(oracle.leaves_packed(b.data, b.meta)))
    dpath, mpath = str(tmp_path / "data.u32"), str(tmp_path / "meta.u32")
    np.ascontiguousarray(b.data).tofile(dpath)
    np.ascontiguousarray(b.meta).tofile(mpath)
    base = {k: v for k, v in os.environ.items() if not k.startswith("VKMR_") and k != "LD_PRELOAD"}
    base.update(LD_LIBRARY_PATH=out, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", VKMR_BATCH_MAX_MB="0")

    def client(per_batch, slice_log2, **knobs):
        r = subprocess.run([exe, dpath, mpath, str(per_batch), str(slice_log2)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           env=dict(base, **{k: str(v) for k, v in knobs.items()}), timeout=300)
        assert b"AddressSanitizer" not in r.stderr and b"runtime error" not in r.stderr and b"LeakSanitizer" not in r.stderr, r.stderr[-3000:].decode()
        assert r.returncode == 0, r.stderr[-2000:].decode()
        line = r.stdout.decode().strip().splitlines()[-1]
        return line, r.stderr.decode()

    # plenty of memory: the golden root, with a given slice size and with the instance's own choice
    assert client(4000, 12)[0] == "rc=0 root=" + want
    assert client(4000, 0)[0] == "rc=0 root=" + want
    # 2.2 MB of "HBM": slices of 2^10 x 32 B; the batches' landing zones take most of it, the 59 slices the strings fill do not fit --
    # staging stops with batches staged, the call fails, nothing is used after it was freed
    line, err = client(4000, 10, VKMR_FAKE_HBM_BYTES=2200000)
    assert line == "rc=-1 root=" and "Failed to allocate" in err, (line, err[-500:])
    # 10 MB and no slice size given: the instance clamps the slice to what fits (2^12 digests: 15 slices) and sizes the budget
    # for THAT size -- the root is the golden one (before: a budget for 2^23-digest slices, "slice budget used up and nothing
    # in flight")
    line, err = client(4000, 0, VKMR_FAKE_HBM_BYTES=10000000)
    assert line == "rc=0 root=" + want, (line, err[-800:])
