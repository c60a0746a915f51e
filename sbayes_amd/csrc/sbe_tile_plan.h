// sbe_tile_plan.h -- the numbers of the units that count co-occurrences as 32 x 32 tiles of a 0/1 matrix product on the
// matrix pipe (sbe_assoc.hip, sbe_pairppc.hip, sbe_consensus.hip, sbe_partdist.hip, sbe_simerr.hip, sbe_objpair.hip; DESIGN.md section 13 has the arguments): the geometry of
// a tile and of a round of the contraction, where a lane's accumulator registers lie in the tile, the enumeration of the
// tile pairs I <= J, the launch budget and the rounding to whole rounds and tiles.  Plain C++17, no HIP and nothing of a
// unit's handle; the kernels take the same functions through SBE_TILE_HD (sbe_unit_tiles.hip.h includes this file).
// tests/c/tile_plan.cpp drives it without a GPU (tests/test_tile_plan_cpu.py).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

#ifdef __HIPCC__
#define SBE_TILE_HD __host__ __device__
#else
#define SBE_TILE_HD
#endif

namespace sbe_tile {

// ---- geometry ---------------------------------------------------------------------------------------------------------------
constexpr int kTile = 32;                            // rows and columns of a tile (of v_mfma_f32_32x32x64_f8f6f4's result)
constexpr int kStep = 64;                            // contraction elements per MFMA
constexpr int kRound = 4;                            // steps per round: a round's loads are issued together
constexpr int kRoundElems = kRound * kStep;          // the contraction axis is padded to whole rounds
constexpr int kRoundBytes = kRoundElems / 2;         // of one packed FP4 row (a nibble per element)
constexpr int kAccRegs = 16;                         // f32 accumulator registers of a lane: 32 x 32 entries over 64 lanes

// The tile row of accumulator register `reg` of a lane in half `half` = lane >> 5 (its column is lane & 31): the result
// lies in blocks of four consecutive rows, the blocks dealt alternately to the two lane halves -- rows 0..3 to half 0,
// 4..7 to half 1, 8..11 to half 0 again -- so a lane's registers 4 b .. 4 b + 3 are the rows of its half's b-th block.
// (Index: int, or int64_t where the row goes into 64-bit addresses, which the compiler then forms without widening each.)
template <class Index>
SBE_TILE_HD constexpr Index acc_row(int reg, Index half) { return (reg & 3) + 8 * (reg >> 2) + 4 * half; }

// ---- the tile pairs I <= J, enumerated t = J (J + 1) / 2 + I --------------------------------------------------------------
struct TilePair {
    int64_t I, J;
};

// t >= 0 back to its pair: the root of J (J + 1) / 2 = t as a first guess, which the rounding of the double may leave one off
// in either direction
SBE_TILE_HD inline TilePair tile_pair(int64_t t) {
    int64_t J = (int64_t)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while (J * (J + 1) / 2 > t) --J;
    while ((J + 1) * (J + 2) / 2 <= t) ++J;
    return {t - J * (J + 1) / 2, J};
}

// ---- the launch budget ------------------------------------------------------------------------------------------------------
// contraction steps per launch: a launch of one full wave per SIMD then stays in the milliseconds however long the
// contraction axis (a tile at 2^24 elements takes 2^18 steps: 16 tiles per launch), and at most 2^16 tiles
constexpr int64_t kStepsPerLaunch = (int64_t)1 << 22;
constexpr int64_t kMaxLaunchTiles = (int64_t)1 << 16;

// tiles per launch for tiles of `steps` >= 1 contraction steps each; `override_tiles` > 0 (a unit's set_launch_tiles) wins
inline int64_t tiles_per_launch(int64_t steps, int64_t override_tiles = 0) {
    return override_tiles > 0 ? override_tiles : std::max<int64_t>(1, std::min(kMaxLaunchTiles, kStepsPerLaunch / steps));
}

// ---- whole rounds and whole tiles -------------------------------------------------------------------------------------------
constexpr int64_t rounds_of(int64_t elems) { return (elems + kRoundElems - 1) / kRoundElems; }
constexpr int64_t whole_rounds(int64_t elems) { return rounds_of(elems) * kRoundElems; }
constexpr int64_t tiles_of(int64_t rows) { return (rows + kTile - 1) / kTile; }
constexpr int64_t whole_tiles(int64_t rows) { return tiles_of(rows) * kTile; }

}  // namespace sbe_tile
