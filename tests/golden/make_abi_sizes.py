#!/usr/bin/env python3
"""Generates tests/golden/abi_sizes.json: what the twelve size functions of the C ABI (include/vkmr_hip.h) return for a few
thousand argument tuples at the edges of their rules.  tests/test_abi_plans.py asserts that the library still returns every
recorded value, so a change that moves a sizing rule (into a plan header, say) cannot move a size with it.

The size functions make no HIP call, so the library loads and answers without a GPU.  Run it against the library whose sizes
are to be pinned, BEFORE the change that must keep them:

    python tests/golden/make_abi_sizes.py [--lib vk_merkle_roots_amd/libvkmr_hip.so]
"""
import argparse
import ctypes as C
import itertools
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "abi_sizes.json")

U32, U64 = C.c_uint32, C.c_uint64
FUNCTIONS = {
    "vkmr_hip_sizes_scratch_bytes": [U32],
    "vkmr_hip_reduce_scratch_bytes": [U64],
    "vkmr_hip_reduce_slices_scratch_bytes": [U64, U32],
    "vkmr_hip_reduce_levels_scratch_bytes": [U64],
    "vkmr_hip_tree_bytes": [U64, U32],
    "vkmr_hip_multiproof_max_nodes": [U64, U32, U32],
    "vkmr_hip_multiproof_scratch_bytes": [U32, U32],
    "vkmr_hip_forest_scratch_bytes": [U64, U32],
    "vkmr_hip_forest_tree_bytes": [U64, U32, U64],
    "vkmr_hip_forest_multiproof_max_nodes": [U64, U32, U64, U32],
    "vkmr_hip_forest_multiproof_scratch_bytes": [U32, U32],
    "vkmr_hip_find_scratch_bytes": [U32],
}

M32 = 2**32 - 1


def around(exponents):
    return sorted({v for e in exponents for v in (2**e - 1, 2**e, 2**e + 1)})


# counts: the small ones, 2^k +- 1 through every regime of the reduction schedule, and the ends of the range
COUNTS = sorted(set([0, 1, 2, 3, 127, 128, 129] + around([8, 11, 12, 15, 16, 18, 19, 20, 26, 31, 32, 33, 40, 58]) + [2**63 - 1, 2**63]))
COUNTS_FEW = [0, 1, 2, 127, 128, 129, 2**12 + 1, 2**19 - 1, 2**19, 2**26, 2**32 + 1, 2**58, 2**63]
COUNTS32 = [c for c in COUNTS if c <= M32] + [M32]
HEIGHTS = [0, 1, 2, 26, 58, 63, 64]
KS = [0, 1, 2, 63, 64, 65, 16383, 16384, 16385, M32]
SLICES = [0, 1, 2, 3, 64, 1000, 4095, 4096, 32767, 32768, 32769, 65536, 65537, 98305, M32]
NTREES = [0, 1, 2, 33, 65536, M32]
MAX_COUNTS = [0, 1, 2, 129, 2**20, 2**58, 2**63]


def heights_of(count):
    """0, 1, 63, 64 and the height that takes `count` to one node, with its neighbours."""
    h = max(0, int(count - 1).bit_length()) if count else 0
    return sorted({0, 1, 63, 64, h, max(h - 1, 0), min(h + 1, 64)})


def tuples():
    t = {}
    t["vkmr_hip_sizes_scratch_bytes"] = [(c,) for c in COUNTS32 + [4095, 4096, 4097, 8192, 8193]]
    t["vkmr_hip_reduce_scratch_bytes"] = [(c,) for c in COUNTS]
    t["vkmr_hip_reduce_slices_scratch_bytes"] = list(itertools.product(COUNTS, SLICES))
    t["vkmr_hip_reduce_levels_scratch_bytes"] = [(c,) for c in COUNTS]
    t["vkmr_hip_tree_bytes"] = [(c, h) for c in COUNTS for h in heights_of(c)]
    t["vkmr_hip_multiproof_max_nodes"] = [(c, h, k) for c in COUNTS_FEW for h in heights_of(c) for k in KS]
    t["vkmr_hip_multiproof_scratch_bytes"] = list(itertools.product(KS, HEIGHTS))
    t["vkmr_hip_forest_scratch_bytes"] = list(itertools.product(COUNTS, NTREES))
    t["vkmr_hip_forest_tree_bytes"] = list(itertools.product(COUNTS_FEW, NTREES, MAX_COUNTS))
    t["vkmr_hip_forest_multiproof_max_nodes"] = list(itertools.product(COUNTS_FEW, [0, 1, 33, M32], [0, 1, 129, 2**58, 2**63], [0, 1, 64, 16385, M32]))
    t["vkmr_hip_forest_multiproof_scratch_bytes"] = list(itertools.product(KS, HEIGHTS))
    t["vkmr_hip_find_scratch_bytes"] = [(k,) for k in KS + [31, 32, 33, 2**20, 2**31 - 1, 2**31, 2**31 + 1]]
    return t


def load(path):
    lib = C.CDLL(path)
    for name, argtypes in FUNCTIONS.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = C.c_size_t, argtypes
    return lib


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--lib", default=os.path.join(ROOT, "vk_merkle_roots_amd", "libvkmr_hip.so"))
    a = p.parse_args()
    lib = load(a.lib)
    rec = {"_about": "name -> [arguments..., result] of the C ABI's size functions, recorded from the library before the sizing rules moved "
                     "into the plan headers; regenerate with tests/golden/make_abi_sizes.py"}
    total = 0
    for name, args in tuples().items():
        rec[name] = [list(t) + [int(getattr(lib, name)(*t))] for t in args]
        total += len(args)
    with open(OUT, "w") as f:   # one line per function: a moved size shows as one changed line
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in rec.items()) + "\n}\n")
    print("wrote", OUT, total, "tuples")


if __name__ == "__main__":
    main()
