"""MI355X-native Merkle-root engine (SHA-256d map + pairwise reduce) -- Python harness.

The product is the C ABI in include/vkmr_hip.h (HIP kernels for gfx950) and the C++
front end under csrc/host.  This package only holds what tests and bench.py need to
drive that ABI from Python: the ctypes stub (`_abi`), a small RAII-style wrapper over
device buffers (`engine`) and the build recipes (`build`).  Nothing here computes a
hash on the CPU; without the built HIP extension every entry point raises.
"""
from . import build  # noqa: F401
from ._abi import Digest, Metadata, VkmrError, check, host_lib, lib  # noqa: F401
from .engine import (NO_TREE, NOT_FOUND, AbsenceProofs, AuditReport, ConsistencyProof, DiffOverflow, ForestMultiproof, Frontier, HipDevice, MerkleForest, MerkleTree, Multiproof, PackedBatch, PartialMerkleTree, PartialMerkleTrees, RangeProofs, RndmStream, consistency_status_text, forest_append_status_text, forest_copy_status_text, frontier_status_text, leafsort_status_text, merge_status_text, merkle_forest_packed, merkleblocks_status_text, merkle_root_packed,  # noqa: F401
                     merkle_root_packed_batched, merkle_roots_packed_forest, merkle_roots_packed_forest_mutated, merkle_tree_packed, pack_lines, range_status_text, rndm_packed, sort_digests, sorted_forest_packed, tree_height, UpdateWitness)
