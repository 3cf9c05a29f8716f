// map_plan.hpp -- which fetch mode and tile vkmr_hip_map_async gives a batch (csrc/map_kernel.hpp has the modes).  Host-only
// arithmetic, no HIP types: shared by the C ABI (vkmr_hip.hip), the experiments build (map_experiments.hpp) and the CPU-side
// replay in tests/c/abi_plan_test.cpp.
//
// The mode is chosen from the batch alone:
//   average packed string < 128 B   LDS-staged tiles (HBM traffic == algorithmic bytes)
//   128 B .. 512 B                  per-lane 16-byte loads, one 64-byte block per trip, 8 wavefronts per SIMD (256-lane workgroups when the launch is short)
//   512 B and more                  per-lane loads, TWO blocks (128 bytes) per trip: a 128-byte line is asked for by at most two trips instead
//                                   of three -- 8.6 instead of 11.3 GB at the L2-fabric boundary for 4.3 GB of rndm * 4096, the same
//                                   2.29 ms (87 VGPRs, 5 wavefronts per SIMD); at 150 B on average it is 3 % slower, hence the threshold
//                                   (profiles/r04_long_strings_two_blocks.txt)
// Round 2 also shipped a third mode for strings of 1 KiB and more -- whole 128-byte lines through a per-lane LDS window,
// 1.06x instead of 1.46x the algorithmic reads for 1-2 % of time.  Its 272 bytes of LDS per lane allow two wavefronts
// per SIMD, and since the issue pass (isa_prio_pass.py) the instruction pairing that decides the speed needs
// occupancy: 2.56 ms against 2.26 ms for the per-lane loads on rndm * 4096 (profiles/r03_long_strings_modes.txt).
// It stays in the experiments build (VKMR_MAP_VARIANT=5).
#pragma once
#include <stdint.h>

namespace vkmr_map {

// Strings per LDS-staged tile: what is expected to fit the staging area, three standard deviations of a tile's
// size below it (string lengths spread like rndm's, uniform in [1, max]: sigma / mean of T strings is about
// 0.6 / sqrt(T)); a tile that overflows anyway falls back to per-lane loads inside the kernel.  The more strings a
// tile sorts the better: fewer of its groups straddle a block-count boundary, and 1024 strings are exactly two
// groups of 64 for each of the 8 wavefronts (profiles/r02_map_tile_fill.txt).  69 KiB of staging is what still
// lets two workgroups share a CU's LDS.  `fit_pct` (experiments build only) replaces the 3-sigma rule.
inline uint32_t staged_tile(uint64_t data_words, uint32_t count, uint32_t max_tile, uint32_t stage_words, int fit_pct = 0)
{
    uint32_t tile = max_tile;
    if (data_words > 0) {
        const double r = (double)stage_words * (double)count / (double)data_words;   // strings that fill the area on average
        const double want = fit_pct ? r * fit_pct / 100.0 : r * (1.0 - 1.8 / __builtin_sqrt(r > 4.0 ? r : 4.0));
        const uint64_t fit = want > 0.0 ? (uint64_t)want : 0;
        if (fit >= max_tile / 4 && fit < tile) tile = (uint32_t)(fit & ~63ull);
    }
    // a launch too short to give every CU its two workgroups: smaller tiles, so that it still spreads over the chip
    const uint32_t spread = (uint32_t)((count / 512u) & ~63u);
    if (spread < tile) tile = spread < max_tile / 4 ? max_tile / 4 : spread;
    return tile;
}

// Tiles of the per-lane modes: up to 2048 strings, smaller when the batch is short so that it still spreads over
// the chip (>= ~1024 workgroups when it can).
inline uint32_t direct_tile(uint32_t count)
{
    const uint32_t tile = (count / 1024u) & ~63u;
    return tile < 256u ? 256u : (tile > 2048u ? 2048u : tile);
}

inline uint32_t tiles_of(uint32_t count, uint32_t tile) { return (uint32_t)(((uint64_t)count + tile - 1) / tile); }   // count + tile can pass 2^32

// Words of the average packed string, rounded up; count >= 1.
inline uint64_t avg_words(uint64_t data_words, uint32_t count) { return (data_words + count - 1) / count; }

// The shipped modes: the staged one (tiles of up to 1024 strings in 17664 words of LDS), and the per-lane ones by loads per
// trip (DIRECT one block, LONG two) and workgroup size (256 lanes when the launch is short: a tile below 1024 strings).
enum Mode { STAGED, DIRECT512, DIRECT256, LONG512, LONG256 };
struct Plan { Mode mode; uint32_t tile; };

inline Plan plan(uint64_t data_words, uint32_t count)
{
    const uint64_t avg = avg_words(data_words, count);
    const uint32_t tile = direct_tile(count);
    // strings of 128 B and more on average (a short launch: smaller workgroups spread it over the chip)
    if (avg >= 128) return Plan{tile >= 1024u ? LONG512 : LONG256, tile};
    if (avg >= 32) return Plan{tile >= 1024u ? DIRECT512 : DIRECT256, tile};
    // short strings (a cache line holds several): the per-lane mode is 1-2 % faster but re-reads lines that
    // fell out of L2 (1.6x traffic, profiles/r01_map_fetch_modes.txt)
    return Plan{STAGED, staged_tile(data_words, count, 1024, 17664)};
}

}  // namespace vkmr_map
