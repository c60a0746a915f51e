#pragma once
// sbe_unit_tiles.hip.h -- what the units on the matrix pipe share beyond sbe_unit.hip.h (sbe_consensus.hip, sbe_partdist.hip, sbe_simerr.hip, sbe_objpair.hip,
// and through sbe_assoc_pair.hip.h sbe_assoc.hip and sbe_pairppc.hip; no other file): the FP4 contraction step of a 32 x 32 tile of a 0/1 matrix product,
// the walk over a lane's part of the finished tile, and the launches of a range of tiles within the budget.  The numbers
// are sbe_tile_plan.h's; DESIGN.md section 13 says why the operands are FP4 and why their placement is free.  Everything
// lives in an unnamed namespace, as in the sibling headers.
#include "sbe_unit.hip.h"
#include "sbe_tile_plan.h"

namespace {

using namespace sbe_tile;

typedef int v8i __attribute__((ext_vector_type(8)));        // an MFMA operand: FP4 fills the first four dwords (32 nibbles)
typedef float v16f __attribute__((ext_vector_type(16)));    // a lane's accumulator registers

// the packed operands of one lane for one round: q[u] holds its 32 elements of step u, a nibble each.  A round's loads are
// issued together, so their latency is paid once per round
struct LaneRound {
    uint4 q[kRound];
};

// p: the lane's 16 bytes of the round's first step (its row of the image, its half of the step)
__device__ inline LaneRound load_round(const uint8_t* p) {
    LaneRound c;
#pragma unroll
    for (int u = 0; u < kRound; ++u) c.q[u] = *reinterpret_cast<const uint4*>(p + u * (kStep / 2));
    return c;
}

__device__ inline v8i fp4_operand(const uint4 q) {
    v8i v = {};
    v[0] = (int)q.x;
    v[1] = (int)q.y;
    v[2] = (int)q.z;
    v[3] = (int)q.w;
    return v;
}

// acc += A B over one step of 64 elements, v_mfma_f32_32x32x64_f8f6f4: the two format selectors (cbsz for a, blgp for b) say
// what the operand registers hold, 4 = FP4 (e2m1: 0x0 is 0, 0x2 is 1).  The four arguments behind them are the block scales
// and their selectors; all zero, the compiler emits the instruction without scaling
constexpr int kMfmaFp4 = 4;
__device__ inline v16f mfma_fp4(const v8i a, const v8i b, const v16f acc) {
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, acc, kMfmaFp4, kMfmaFp4, 0, 0, 0, 0);
}

// fn(row, column, value) for the 16 entries of the tile that a lane holds in acc: the lane of half `half` = lane >> 5 whose
// column is `col` = lane & 31 (acc_row of sbe_tile_plan.h)
template <class Index, class Fn>
__device__ inline void for_acc_entries(const v16f& acc, Index half, int col, Fn fn) {
#pragma unroll
    for (int reg = 0; reg < kAccRegs; ++reg) fn(acc_row(reg, half), col, acc[reg]);
}

// What a unit's handle derives from beside sbe_unit_handle: the tiles per launch a caller has asked for
struct unit_tile_launches {
    int64_t launch_tiles = 0;                    // 0: the default (tiles_per_launch of sbe_tile_plan.h)
};

// the whole body of sbe_<unit>_set_launch_tiles
template <class H>
int unit_set_launch_tiles(H* h, int64_t tile_pairs, const char* null_text) {
    CHECK_HANDLE(h, null_text);
    if (tile_pairs < 0 || tile_pairs > kMaxLaunchTiles)
        return fail(h, SBE_ERR_ARG, "tile_pairs=%lld out of range [0, %lld]", (long long)tile_pairs, (long long)kMaxLaunchTiles);
    h->launch_tiles = tile_pairs;
    return SBE_OK;
}

// fn(t0, t_end) for consecutive ranges of [0, total) of at most per_launch >= 1 each (one launch each, a workgroup per
// entry); returns the first non-zero code
template <class Fn>
int unit_for_tile_launches(int64_t total, int64_t per_launch, Fn fn) {
    for (int64_t t0 = 0; t0 < total; t0 += per_launch)
        if (const int rc = fn(t0, std::min(total, t0 + per_launch))) return rc;
    return SBE_OK;
}

}  // namespace
