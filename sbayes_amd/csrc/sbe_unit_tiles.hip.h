#pragma once
// sbe_unit_tiles.hip.h -- what the units on the matrix pipe share beyond sbe_unit.hip.h (sbe_consensus.hip, sbe_partdist.hip, sbe_simerr.hip, sbe_objpair.hip,
// and through sbe_assoc_pair.hip.h sbe_assoc.hip and sbe_pairppc.hip; no other file): the FP4 contraction step of a 32 x 32 tile of a 0/1 matrix product,
// the walk over a lane's part of the finished tile, the launches of a range of tiles within the budget, and the host part of
// the segmented operand image that sbe_consensus.hip and sbe_simerr.hip keep (unit_segment_image).  The numbers
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

// ... with a kernel that computes one tile pair I <= J of an N x N result per wave (Args has t0 and t_end: the pairs of a
// launch), between the handle's two events; steps: the contraction steps of a pair
template <class H, class Args>
int unit_launch_tile_pairs(H* h, int64_t steps, Args& args, void (*kernel)(const Args)) {
    const int64_t tiles = tiles_of(h->N), tile_pairs = tiles * (tiles + 1) / 2;
    return unit_timed(h, [&] {
        return unit_for_tile_launches(tile_pairs, tiles_per_launch(steps, h->launch_tiles), [&](int64_t t0, int64_t t_end) {
            args.t0 = t0;
            args.t_end = t_end;
            kernel<<<(unsigned)(t_end - t0), 64, 0, h->stream>>>(args);
            HIPCHK(h, hipGetLastError());
            return SBE_OK;
        });
    });
}

// What the handles of sbe_consensus.hip and sbe_simerr.hip derive from beside the bit store: the operand image of the runs,
// [whole tiles of objects][n_runs segments][seg_bytes] and zero wherever no element was appended, the version of the store
// and the versions of the two results (slots, sides) that the unit computes from it.  `word` names a result in the messages,
// `producer` the entry point that computes one.
struct unit_segment_image {
    int64_t seg_bytes = 0, stride = 0;  // of a run's segment, of one object's image
    uint64_t version = 0;               // of the store: every reset and every appended piece makes a new one
    uint64_t result_version[2] = {};    // of the store when the result was computed (0: empty)
    uint8_t* d_img = nullptr;           // [whole_tiles(N)][n_runs][seg_bytes]
    size_t img_bytes = 0;

    // The middle of <prefix>_reset, behind the shape checks: the store loses its shape and the results their versions, the
    // image and -- ensure_rest() -- the unit's other buffers are allocated, the image is zeroed.  set_shape follows
    template <class H, class Rest>
    int reset_image(H* h, int n_runs, int64_t n_objects, int64_t seg, Rest ensure_rest) {
        const size_t img = (size_t)(whole_tiles(n_objects) * n_runs * seg);
        h->runs.rows.clear();                                 // (a failed allocation leaves an unshaped store)
        result_version[0] = result_version[1] = 0;
        ++version;
        HIPCHK(h, hipSetDevice(h->device));
        int rc = unit_ensure(h, d_img, img_bytes, img);
        if (!rc) rc = ensure_rest();
        if (rc) return rc;
        // the image is zero wherever no element was appended: the padding of every segment and the objects behind N
        HIPCHK(h, hipMemsetAsync(d_img, 0, img, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        seg_bytes = seg;
        stride = n_runs * seg;
        return SBE_OK;
    }
    // The code <prefix>_append_rows returns.  After a failure a piece may be in the image already while the run's row count
    // is not: the next append would OR new elements onto it.  The store is unshaped instead (<prefix>_reset comes next), as
    // after a failed allocation
    template <class H>
    static int append_done(H* h, int rc) {
        if (rc) h->runs.rows.clear();
        return rc;
    }
    template <class H>
    static int check_result_index(H* h, const char* word, int i) {
        return i == 0 || i == 1 ? SBE_OK : fail(h, SBE_ERR_ARG, "%s=%d is neither 0 nor 1", word, i);
    }
    // a result a later call reads: computed, and on the store as it is now
    template <class H>
    int check_result_current(H* h, const char* word, const char* producer, int i) const {
        if (result_version[i] == 0) return fail(h, SBE_ERR_STATE, "%s %d is empty (%s comes first)", word, i, producer);
        if (result_version[i] != version)
            return fail(h, SBE_ERR_STATE, "%s %d was computed before the store last changed (%s again)", word, i, producer);
        return SBE_OK;
    }
};

}  // namespace
