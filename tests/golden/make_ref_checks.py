#!/usr/bin/env python3
"""Regenerates tests/golden/ref_checks.json from the REFERENCE ITSELF.

Like make_golden.py, it runs only where the reference sources are present (oracle/Makefile `ref`
compiles its CPU-serial path into oracle/_ref/) and records what that build returns, so that
tests/test_oracle.py can hold the oracle against the reference where oracle/_ref/ cannot be built:
  leaves  -- vkmr::cpu_sha256d of the messages of conftest.ref_check_inputs()
  trees   -- CpuSha256D::Root over its string lists
  driver  -- the root line vkmr_cpu_ref prints for the L2_empty_lines stream, up to its timing
The inputs are regenerated from their seed and pinned by their sha256.

    python tests/golden/make_ref_checks.py
"""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.path.join(ROOT, "oracle", "_ref")
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402

from conftest import ref_check_inputs, strings_sha256  # noqa: E402


def main():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "all", "ref"], stdout=subprocess.DEVNULL)
    lib = C.CDLL(os.path.join(REF, "libvkmr_ref.so"))
    msgs, trees = ref_check_inputs()
    rec = {"_about": "outputs of the reference CPU-serial path (g++ -O2 build of src/vkmr/{SHA-256plus,Debug,Inputs,StopWatch}.cpp) for "
                     "the inputs of tests/conftest.py::ref_check_inputs; regenerate with tests/golden/make_ref_checks.py"}
    leaves = []
    for msg in msgs:
        out = C.create_string_buffer(32)
        lib.ref_sha256d(msg, C.c_size_t(len(msg)), out)
        leaves.append({"len": len(msg), "input_sha256": hashlib.sha256(msg).hexdigest(), "sha256d": out.raw.hex()})
    rec["leaves"] = leaves
    roots = []
    for strs in trees:
        blob = b"".join(strs)
        offs = np.zeros(len(strs) + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(s) for s in strs])
        hexbuf = C.create_string_buffer(65)
        lib.ref_root(blob, C.c_void_p(offs.ctypes.data), C.c_size_t(len(strs)), hexbuf)
        roots.append({"count": len(strs), "input_sha256": strings_sha256(strs), "root": hexbuf.value.decode()})
    rec["trees"] = roots
    vectors = json.load(open(os.path.join(HERE, "vectors.json")))
    stream = bytes.fromhex(vectors["streams"]["L2_empty_lines"]["stream_hex"])
    out = subprocess.run([os.path.join(REF, "vkmr_cpu_ref")], input=stream, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout.decode()
    line = [ln for ln in out.splitlines() if "computed root" in ln][0]
    rec["driver"] = {"L2_empty_lines": line.rsplit(" in ", 1)[0] + " in "}
    with open(os.path.join(HERE, "ref_checks.json"), "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    print("wrote", os.path.join(HERE, "ref_checks.json"))


if __name__ == "__main__":
    main()
