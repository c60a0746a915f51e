#pragma once
// sbe_unit_device.hip.h -- what the device code of the side units shares (sbe_unit.hip.h has the host side): the fixed-tree
// reductions, the 32 x 32 transpose that fills a row store, the pack kernel that fills a bit store and the launch limits.
// Device code only and nothing of the engine: a unit that includes this header compiles no kernels but its own and the
// fill kernels it launches.  Everything lives in an unnamed namespace: every unit compiles its own copy.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace {

// workgroups per launch along x: an AQL dispatch holds its grid in work-items as a uint32, so every launch of a unit stays
// under 2^32 work-items (blocks of up to 256 threads) and longer ranges are launched in chunks, each with its offset
// (unit_for_grid_chunks of sbe_unit.hip.h)
constexpr int64_t kMaxGridBlocks = ((int64_t)1 << 24) - 1;
constexpr size_t kLdsBudget = (size_t)160 << 10;     // LDS per CU on MI355X

constexpr int pow2_at_least(int v) { return v <= 1 ? 1 : 2 * pow2_at_least((v + 1) / 2); }

// ---- reductions (fixed tree: lanes by xor exchanges, then the waves in index order) ---------------------------------
// NOT the engine's wave_sum / block_sum (sbe_device_common.hip.h: __shfl_down, then a pairwise sum of the four waves,
// valid in thread 0 only).  The two families add in different orders, so their float results differ in the last bits:
// they are not interchangeable, and every unit's oracle fixes the order below.
struct unit_sum { template <class T> __device__ T operator()(T a, T b) const { return a + b; } };
struct unit_or { __device__ int operator()(int a, int b) const { return a | b; } };
struct unit_min {
    __device__ double operator()(double a, double b) const { return fmin(a, b); }
    __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return min(a, b); }
};
struct unit_max {
    __device__ double operator()(double a, double b) const { return fmax(a, b); }
    __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return max(a, b); }
    __device__ long long operator()(long long a, long long b) const { return a > b ? a : b; }
};

// every lane ends with the wave's result
template <class T, class Op>
__device__ inline T unit_wave_reduce(T v, Op op) {
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
    return v;
}

// every thread of a block of kWaves waves ends with red[0] op red[1] op ...; red: [kWaves] in LDS
template <int kWaves, class T, class Op>
__device__ inline T unit_block_reduce(T v, T* red, Op op) {
    v = unit_wave_reduce(v, op);
    __syncthreads();                                   // (red may still be read by the previous reduction)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    T t = red[0];
    for (int w = 1; w < kWaves; ++w) t = op(t, red[w]);
    return t;
}

// ---- a row store's fill: host rows [n][C] (staging) -> store columns [C][cap] at row offset r0, 32 x 32 tiles through LDS;
// blockIdx.x + ct0: column tile, blockIdx.y: row tile
template <class T>
__global__ __launch_bounds__(256) void k_unit_transpose(const T* rows, int64_t n, int64_t C, T* store, int64_t cap, int64_t r0, int64_t ct0) {
    __shared__ T tile[32][33];
    const int64_t c0 = (ct0 + blockIdx.x) * 32, n0 = (int64_t)blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;     // 32 x 8
    for (int r = ty; r < 32; r += 8) {
        const int64_t row = n0 + r, col = c0 + tx;
        if (row < n && col < C) tile[r][tx] = rows[row * C + col];
    }
    __syncthreads();
    for (int c = ty; c < 32; c += 8) {
        const int64_t col = c0 + c, row = n0 + tx;
        if (row < n && col < C) store[col * cap + r0 + row] = tile[tx][c];
    }
}

// ---- a bit store's fill: host bytes [n][K][N] (staging) -> bit words [n][K][W]; a wave takes 64 objects of one (row, cluster);
// blockIdx.x + line0: the line, blockIdx.y: kBlock objects.  (A template, as the transpose is: only a unit that launches it
// compiles it.)
template <int kBlock>
__global__ __launch_bounds__(kBlock) void k_unit_pack_bits(const uint8_t* rows, int64_t n_lines, int N, int W, uint32_t* out, int64_t line0) {
    const int64_t line = line0 + blockIdx.x;                   // row * K + cluster, within this piece
    const int n = blockIdx.y * kBlock + threadIdx.x;
    const bool bit = line < n_lines && n < N && rows[line * N + n] != 0;
    const unsigned long long both = __ballot(bit);
    const int w = n >> 5;
    if ((threadIdx.x & 63) == 0 && line < n_lines) {
        if (w < W) out[line * W + w] = (uint32_t)both;
        if (w + 1 < W) out[line * W + w + 1] = (uint32_t)(both >> 32);
    }
}

}  // namespace
