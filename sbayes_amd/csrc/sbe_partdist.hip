// sbe_partdist.hip -- pairwise distances between cluster samples on the device (include/sbe_partdist.h): the store of R runs
// of cluster samples in two forms (the bit rows are sbe_unit.hip.h's bit store), the pack kernel of the operand image, the
// tile kernel on the matrix pipe with its per-pair epilogue, the row-sum kernel of the sums and the table kernel on the
// vector pipe.  The contract is tests/_partdist_oracle.py; DESIGN.md section 23 has the layout, the kernels and the limits.
//
// With Z the 0/1 matrix of all cluster rows, [T K_pad][N], the contingency tables of all sample pairs are the K_pad x K_pad
// blocks of Z Z^T.  k_partdist_tiles computes its 32 x 32 tiles with the FP4 contraction of sbe_unit_tiles.hip.h over the
// objects (counts <= N are exact in the f32 accumulator), a wave a strip of up to four tiles that share their rows of the
// row side.
//   image: [run][row K_pad + k][N_pad / 2 bytes]; object i is nibble i & 7 of dword i >> 3 of its row; a run holds
//   cap K_pad rows rounded up to whole tiles; the rows k >= K, the rows behind a run's last and the objects >= N are zero.
//   A lane owns one row of a tile (lane & 31) and one half of a step (lane >> 5): 32 objects, one 16-byte load, and both
//   operands come from this one image.
// A tile is 32 / K_pad x 32 / K_pad whole sample pairs; the epilogue takes the strip's pairs from LDS, one pair per lane and turn.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "sbe_unit_tiles.hip.h"
#include "../../include/sbe_partdist.h"

namespace {

constexpr int kMaxK = SBE_PARTDIST_MAX_CLUSTERS;
constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
// tiles of the column side a wave holds (a strip): it loads its rows of the row side once for all of them, and the launch
// has a quarter of the workgroups.  The plain form, one tile per wave, re-read 32 KiB of operands for sixteen MFMAs and was
// bound by that and by the dispatch of its single-wave workgroups
constexpr int kStrip = 4;
// entries of the dense block a chunk of the sums holds in scratch: 128 MiB of int32 and 256 MiB of float64
constexpr int64_t kSumChunkEntries = (int64_t)1 << 25;
static_assert(kRoundElems == SBE_PARTDIST_ROUND, "the header states the round length");
static_assert(kMaxK == 8, "the epilogue's loops are unrolled to 8 areas");

// ---- pack: host bytes [n][K][N] (staging) -> image rows of one run ----------------------------------------------------
// A thread owns one dword of one line (row, cluster): 8 objects.  blockIdx.x + line0: the line within the piece,
// blockIdx.y: kBlock dwords.  img: the image row of the piece's first sample.
__global__ __launch_bounds__(kBlock) void k_partdist_pack(const uint8_t* rows, int K, int K_pad, int N, int64_t row_dwords, uint32_t* img, int64_t line0) {
    const int64_t line = line0 + blockIdx.x;
    const int64_t d = (int64_t)blockIdx.y * kBlock + threadIdx.x;
    if (d >= row_dwords) return;
    const uint8_t* src = rows + line * N;
    uint32_t bits = 0;
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const int64_t i = 8 * d + b;
        if (i < N && src[i]) bits |= 2u << (4 * b);
    }
    img[((line / K) * K_pad + line % K) * row_dwords + d] = bits;
}

// ---- sizes: one wave per line of the bit rows ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_partdist_sizes(const uint32_t* bits, int64_t n_lines, int W, int32_t* sizes, int64_t line0) {
    const int64_t line = line0 + (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (line >= n_lines) return;                                 // (uniform for the wave)
    const int lane = threadIdx.x & 63;
    int sum = 0;
    for (int w = lane; w < W; w += 64) sum += __popc(bits[line * W + w]);
    sum = unit_wave_reduce(sum, unit_sum());
    if (lane == 0) sizes[line] = sum;
}

// ---- the tile kernel ------------------------------------------------------------------------------------------------
struct TileArgs {
    const uint8_t* img_a;     // the row run's image
    const uint8_t* img_b;     // the column run's
    int64_t row_bytes;        // N_pad / 2
    int rounds;               // N_pad / 256
    const int32_t* size_a;    // [cap][K] of the row run
    const int32_t* size_b;
    const double* L;          // [N + 1]
    int K, K_pad, shift;      // K_pad = 1 << shift
    int N;
    int order;                // of the two runs: -1 the row run is the earlier, +1 the later, 0 the same run
    int64_t row_first, row_end, col_first, col_end;   // samples of the block
    int64_t ti0, tj0, TJ;     // first tile of each side, tiles along the columns
    int64_t SJ;               // strips along the columns: ceil(TJ / kStrip)
    int64_t t0, t_end;        // strips [t0, t_end) of the enumeration t = ti SJ + sj
    int32_t* binder;          // [n_rows][n_cols] each, or null
    double* vi;
    int32_t* sumsq;
};

__global__ __launch_bounds__(64) void k_partdist_tiles(const TileArgs g) {
    __shared__ uint16_t tile[kStrip][kTile][kTile + 2];          // (a count is at most N <= 16384)
    const int64_t t = g.t0 + blockIdx.x;
    if (t >= g.t_end) return;
    const int64_t I = g.ti0 + t / g.SJ, j0 = (t % g.SJ) * kStrip;
    const int n_tiles = (int)(g.TJ - j0 < kStrip ? g.TJ - j0 : kStrip);     // of the strip; uniform for the wave
    const int lane = threadIdx.x, half = lane >> 5;
    // (a run's image has whole tiles of rows: the rows behind its last are zero.  A strip that ends behind the block's last
    // tile repeats that tile: its surplus accumulators are not read)
    const uint8_t* a = g.img_a + (I * kTile + (lane & 31)) * g.row_bytes + (kStep / 4) * half;
    const uint8_t* b[kStrip];
#pragma unroll
    for (int m = 0; m < kStrip; ++m)
        b[m] = g.img_b + ((g.tj0 + j0 + (m < n_tiles ? m : n_tiles - 1)) * kTile + (lane & 31)) * g.row_bytes + (kStep / 4) * half;
    v16f acc[kStrip] = {};
    for (int r = 0; r < g.rounds; ++r, a += kRoundBytes) {
        const LaneRound ca = load_round(a);
#pragma unroll
        for (int m = 0; m < kStrip; ++m) {
            const LaneRound cb = load_round(b[m]);
            b[m] += kRoundBytes;
#pragma unroll
            for (int u = 0; u < kRound; ++u) acc[m] = mfma_fp4(fp4_operand(ca.q[u]), fp4_operand(cb.q[u]), acc[m]);
        }
    }
    // the tile's rows are rows of tile I, its columns rows of the strip's tile m
#pragma unroll
    for (int m = 0; m < kStrip; ++m) for_acc_entries(acc[m], half, lane & 31, [&](int row, int col, float v) { tile[m][row][col] = (uint16_t)(int)v; });
    __syncthreads();
    // ---- the epilogue: one sample pair per lane and turn; x is the earlier sample of the pair, y the later --------------
    const int K = g.K, N = g.N;
    const int P = kTile >> g.shift;                           // samples per tile edge
    const int64_t ld = g.col_end - g.col_first;
    const double* L = g.L;
    auto lx = [&](int e) { return L[e < 0 ? 0 : e > N ? N : e]; };      // (disjoint areas keep every entry in [0, N])
    for (int idx = lane; idx < n_tiles * P * P; idx += 64) {    // (pair idx of the strip: tile m, row sample p, column sample q)
        const int m = idx >> (2 * (5 - g.shift)), p = (idx >> (5 - g.shift)) & (P - 1), q = idx & (P - 1);
        const int64_t srow = I * P + p, scol = (g.tj0 + j0 + m) * P + q;
        if (srow < g.row_first || srow >= g.row_end || scol < g.col_first || scol >= g.col_end) continue;
        const bool swap = g.order > 0 || (g.order == 0 && srow > scol);
        const int32_t* px = swap ? g.size_b + scol * K : g.size_a + srow * K;
        const int32_t* py = swap ? g.size_a + srow * K : g.size_b + scol * K;
        const uint16_t* base = &tile[m][p << g.shift][q << g.shift];
        const int sx = swap ? 1 : kTile + 2, sy = swap ? kTile + 2 : 1;      // n(k, l) = base[k sx + l sy]
        int ax[kMaxK], by[kMaxK], cs[kMaxK];
        int sum_a = 0, sum_b = 0, squares = 0;
#pragma unroll
        for (int k = 0; k < kMaxK; ++k) {
            ax[k] = k < K ? px[k] : 0;
            by[k] = k < K ? py[k] : 0;
            cs[k] = 0;
            sum_a += ax[k];
            sum_b += by[k];
            squares += ax[k] * ax[k] + by[k] * by[k];
        }
        int sum_n = 0, sum_n2 = 0;
#pragma unroll
        for (int k = 0; k < kMaxK; ++k) {
            if (k >= K) continue;
#pragma unroll
            for (int l = 0; l < kMaxK; ++l) {
                if (l >= K) continue;
                const int c = (int)base[k * sx + l * sy];
                cs[l] += c;
                sum_n += c;
                sum_n2 += c * c;
            }
        }
        const int64_t at = (srow - g.row_first) * ld + (scol - g.col_first);
        if (g.binder) g.binder[at] = squares - 2 * sum_n2;
        if (!g.vi && !g.sumsq) continue;
        // the extended table in the contract's order: k major, l minor, from block 0 on
        double hx = 0.0, hy = 0.0, j = 0.0;
        hx += lx(N - sum_a);
        hy += lx(N - sum_b);
#pragma unroll
        for (int k = 0; k < kMaxK; ++k) {
            if (k >= K) continue;
            hx += lx(ax[k]);
            hy += lx(by[k]);
        }
        int e = N - sum_a - sum_b + sum_n;
        int ss = e * e;
        j += lx(e);
#pragma unroll
        for (int l = 0; l < kMaxK; ++l) {
            if (l >= K) continue;
            e = by[l] - cs[l];
            ss += e * e;
            j += lx(e);
        }
#pragma unroll
        for (int k = 0; k < kMaxK; ++k) {
            if (k >= K) continue;
            int rs = 0;
#pragma unroll
            for (int l = 0; l < kMaxK; ++l)
                if (l < K) rs += (int)base[k * sx + l * sy];
            e = ax[k] - rs;
            ss += e * e;
            j += lx(e);
#pragma unroll
            for (int l = 0; l < kMaxK; ++l) {
                if (l >= K) continue;
                const int c = (int)base[k * sx + l * sy];
                ss += c * c;
                j += lx(c);
            }
        }
        if (g.sumsq) g.sumsq[at] = ss;
        if (g.vi) g.vi[at] = fmax(0.0, ((hx + hy) - 2.0 * j) / (double)N);
    }
}

// ---- the row sums of a dense block [n_rows][S]: one wave per row, the contract's tree -------------------------------------
// lane j adds the columns j, j + 64, .. onto 0, then xor exchanges at distances 32 .. 1 (unit_wave_reduce)
__global__ __launch_bounds__(kBlock) void k_partdist_rowsum(const int32_t* binder, const double* vi, int64_t n_rows, int64_t S, long long* bsum, double* vsum,
                                                           int64_t ldo, int64_t row0) {
    const int64_t row = row0 + (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (row >= n_rows) return;                                   // (uniform for the wave)
    const int lane = threadIdx.x & 63;
    long long b = 0;
    double v = 0.0;
    for (int64_t t = lane; t < S; t += 64) {
        b += binder[row * S + t];
        v += vi[row * S + t];
    }
    b = unit_wave_reduce(b, unit_sum());
    v = unit_wave_reduce(v, unit_sum());
    if (lane == 0) {
        bsum[row * ldo] = b;
        vsum[row * ldo] = v;
    }
}

// ---- the raw tables of listed pairs from the bit rows: one wave per pair -------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_partdist_tables(const uint32_t* bits, const int64_t* pairs, int64_t n_pairs, int K, int W, int64_t cap, int32_t* out,
                                                           int64_t pair0) {
    const int64_t pair = pair0 + (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (pair >= n_pairs) return;                                 // (uniform for the wave)
    const int lane = threadIdx.x & 63;
    const int64_t* p = pairs + 4 * pair;
    const uint32_t* x = bits + (p[0] * cap + p[1]) * K * W;
    const uint32_t* y = bits + (p[2] * cap + p[3]) * K * W;
    for (int k = 0; k < K; ++k)
        for (int l = 0; l < K; ++l) {
            int sum = 0;
            for (int w = lane; w < W; w += 64) sum += __popc(x[k * W + w] & y[l * W + w]);
            sum = unit_wave_reduce(sum, unit_sum());
            if (lane == 0) out[(pair * K + k) * K + l] = sum;
        }
}

template <class T>
struct Buffer {
    T* d = nullptr;
    size_t bytes = 0;
};

}  // namespace

struct sbe_partdist : sbe_unit_handle, unit_bit_store, unit_tile_launches {   // (ev: around the kernels of the last block, sums or tables)
    int K_pad = 0, shift = 0;
    int64_t N_pad = 0, run_rows = 0;    // image rows of one run: cap K_pad rounded up to whole tiles
    Buffer<uint8_t> img;                // [n_runs][run_rows][N_pad / 2]
    Buffer<int32_t> sizes;              // [n_runs][cap][K]
    Buffer<double> xlogx;               // [N + 1]
    Buffer<int32_t> binder, sumsq;      // a dense block each (the results of block, the scratch of sums)
    Buffer<double> vi;
    Buffer<long long> bsum;             // [T_sel][R_sel]
    Buffer<double> vsum;
    Buffer<int64_t> pairs;              // [n_pairs][4]
    Buffer<int32_t> tables;             // [n_pairs][K][K]
    std::vector<void*> buffers() const {
        return {img.d, sizes.d, xlogx.d, binder.d, sumsq.d, vi.d, bsum.d, vsum.d, pairs.d, tables.d, d_bits, d_stage};
    }
    const uint8_t* image_of(int run) const { return img.d + (int64_t)run * run_rows * (N_pad / 2); }
    const int32_t* sizes_of(int run) const { return sizes.d + (int64_t)run * runs.cap * K; }
};

namespace {

constexpr char kNullHandle[] = "null handle";
constexpr char kLane[] = "run", kReset[] = "sbe_partdist_reset";

constexpr unit_store_limits kLimits{SBE_PARTDIST_MAX_RUNS, kMaxK, SBE_PARTDIST_MAX_OBJECTS, SBE_PARTDIST_MAX_ROWS, SBE_PARTDIST_MAX_IMAGE_BYTES,
                                    "(2 N^2 fits an int32)"};

int64_t run_image_rows(int K, int64_t cap) { return whole_tiles(cap * pow2_at_least(K)); }

int64_t image_only_bytes(int n_runs, int K, int64_t N, int64_t cap) { return n_runs * run_image_rows(K, cap) * (whole_rounds(N) / 2); }

int64_t store_bytes(int n_runs, int K, int64_t N, int64_t cap) {
    const int64_t W = (N + 31) / 32;
    return image_only_bytes(n_runs, K, N, cap) + (int64_t)n_runs * cap * K * W * (int64_t)sizeof(uint32_t);
}

template <class T>
int ensure(sbe_partdist* h, Buffer<T>& b, size_t count) { return unit_ensure(h, b.d, b.bytes, std::max<size_t>(count, 1) * sizeof(T)); }

// the samples [first, first + n) of a stored run, named `side` in the messages
int check_range(sbe_partdist* h, const char* side, int run, int64_t first, int64_t n) {
    if (run < 0 || run >= h->runs.count()) return fail(h, SBE_ERR_ARG, "%s_run %d out of range [0,%d)", side, run, h->runs.count());
    const int64_t have = h->runs.rows[(size_t)run];
    if (first < 0 || n < 1 || first > have || n > have - first)
        return fail(h, SBE_ERR_ARG, "%ss [%lld, %lld + %lld) are not within the %lld rows of run %d (at least one row)", side, (long long)first,
                    (long long)first, (long long)n, (long long)have, run);
    return SBE_OK;
}

// The launches of one dense block on the handle's stream: the outputs are device pointers [nr][nc] or null.  The ranges
// have passed check_range.
int launch_block(sbe_partdist* h, int ra, int64_t r0, int64_t nr, int rb, int64_t c0, int64_t nc, int32_t* binder, double* vi, int32_t* sumsq) {
    TileArgs g{};
    g.img_a = h->image_of(ra);
    g.img_b = h->image_of(rb);
    g.row_bytes = h->N_pad / 2;
    g.rounds = (int)(h->N_pad / kRoundElems);
    g.size_a = h->sizes_of(ra);
    g.size_b = h->sizes_of(rb);
    g.L = h->xlogx.d;
    g.K = h->K;
    g.K_pad = h->K_pad;
    g.shift = h->shift;
    g.N = (int)h->N;
    g.order = ra < rb ? -1 : ra > rb ? 1 : 0;
    g.row_first = r0;
    g.row_end = r0 + nr;
    g.col_first = c0;
    g.col_end = c0 + nc;
    const int64_t P = kTile / h->K_pad;
    g.ti0 = r0 / P;
    g.tj0 = c0 / P;
    const int64_t TI = (r0 + nr - 1) / P - g.ti0 + 1;
    g.TJ = (c0 + nc - 1) / P - g.tj0 + 1;
    g.binder = binder;
    g.vi = vi;
    g.sumsq = sumsq;
    g.SJ = (g.TJ + kStrip - 1) / kStrip;
    const int64_t strips = TI * g.SJ, steps = (int64_t)g.rounds * kRound;
    // (tiles per launch, in whole strips)
    const int64_t per_launch = std::max<int64_t>(1, tiles_per_launch(steps, h->launch_tiles) / kStrip);
    return unit_for_tile_launches(strips, per_launch, [&](int64_t t0, int64_t t_end) {               // one wave per strip
        g.t0 = t0;
        g.t_end = t_end;
        k_partdist_tiles<<<(unsigned)(t_end - t0), 64, 0, h->stream>>>(g);
        HIPCHK(h, hipGetLastError());
        return SBE_OK;
    });
}

// the host scan of an appended call: 0 / 1 bytes and disjoint areas per sample
int scan_rows(sbe_partdist* h, const uint8_t* rows, int64_t n_rows) {
    const int K = h->K;
    const int64_t N = h->N;
    std::vector<uint8_t> held((size_t)N);
    for (int64_t s = 0; s < n_rows; ++s) {
        if (const int rc = h->check_binary(h, rows, s, 1)) return rc;
        const uint8_t* sample = rows + s * K * N;
        std::fill(held.begin(), held.end(), (uint8_t)0);
        for (int k = 0; k < K; ++k)
            for (int64_t i = 0; i < N; ++i) held[(size_t)i] = (uint8_t)(held[(size_t)i] + sample[k * N + i]);
        uint8_t most = 0;
        for (int64_t i = 0; i < N; ++i) most = std::max(most, held[(size_t)i]);
        if (most > 1) {
            int64_t i = 0;
            while (held[(size_t)i] <= 1) ++i;
            return fail(h, SBE_ERR_DATA, "rows[%lld]: object %lld is in %d areas of the sample (the areas of a sample must be disjoint)", (long long)s,
                        (long long)i, (int)held[(size_t)i]);
        }
    }
    return SBE_OK;
}

}  // namespace

extern "C" {

int sbe_partdist_abi_version(void) { return SBE_PARTDIST_ABI_VERSION; }

const char* sbe_partdist_last_error(const sbe_partdist* h) { return unit_last_error(h); }

int64_t sbe_partdist_image_bytes(int n_runs, int n_clusters, int64_t n_objects, int64_t capacity_rows) {
    return unit_bit_store::shape_ok(kLimits, n_runs, n_clusters, n_objects, capacity_rows) ? store_bytes(n_runs, n_clusters, n_objects, capacity_rows) : 0;
}

int sbe_partdist_create(sbe_partdist** out, int device) { return unit_create_on_device(out, device, "sbe_partdist_create"); }

int sbe_partdist_destroy(sbe_partdist* h) { return unit_destroy(h, kNullHandle); }

int sbe_partdist_last_kernel_ms(const sbe_partdist* h, float* ms_out) { return unit_last_kernel_ms(h, ms_out, kNullHandle); }

int sbe_partdist_set_launch_tiles(sbe_partdist* h, int64_t tile_pairs) { return unit_set_launch_tiles(h, tile_pairs, kNullHandle); }

int sbe_partdist_reset(sbe_partdist* h, int n_runs, int n_clusters, int64_t n_objects, int64_t capacity_rows, const double* xlogx) {
    CHECK_HANDLE(h, kNullHandle);
    if (const int rc = h->check_shape(h, kLimits, n_runs, n_clusters, n_objects, capacity_rows)) return rc;
    if (!xlogx) return fail(h, SBE_ERR_ARG, "null pointer argument: xlogx");
    if (const int rc = h->check_device_bytes(h, kLimits, n_runs, n_clusters, n_objects, capacity_rows, store_bytes(n_runs, n_clusters, n_objects, capacity_rows)))
        return rc;
    const size_t image = (size_t)image_only_bytes(n_runs, n_clusters, n_objects, capacity_rows);
    h->runs.rows.clear();                                 // (a failed allocation leaves an unshaped store)
    HIPCHK(h, hipSetDevice(h->device));
    int rc = ensure(h, h->img, image);
    if (!rc) rc = h->alloc_bits(h, n_runs, n_clusters, n_objects, capacity_rows);
    if (!rc) rc = ensure(h, h->sizes, (size_t)n_runs * (size_t)capacity_rows * (size_t)n_clusters);
    if (!rc) rc = ensure(h, h->xlogx, (size_t)n_objects + 1);
    if (rc) return rc;
    // the image is zero wherever nothing was appended: the rows k >= K, the rows behind a run's last, the objects behind N
    HIPCHK(h, hipMemsetAsync(h->img.d, 0, image, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->xlogx.d, xlogx, ((size_t)n_objects + 1) * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->K_pad = pow2_at_least(n_clusters);
    h->shift = h->K_pad == 1 ? 0 : h->K_pad == 2 ? 1 : h->K_pad == 4 ? 2 : 3;
    h->N_pad = whole_rounds(n_objects);
    h->run_rows = run_image_rows(n_clusters, capacity_rows);
    h->set_shape(n_runs, n_clusters, n_objects, capacity_rows);
    return SBE_OK;
}

int sbe_partdist_rows(const sbe_partdist* h, int run, int64_t* n_rows_out) {
    CHECK_HANDLE(h, kNullHandle);
    return h->runs.get(h, kLane, run, n_rows_out);
}

int sbe_partdist_append_rows(sbe_partdist* h, int run, const uint8_t* rows, int64_t n_rows) {
    CHECK_HANDLE(h, kNullHandle);
    int rc = h->runs.check_append(h, kLane, kReset, run, rows, n_rows);
    if (rc || n_rows == 0) return rc;
    if ((rc = scan_rows(h, rows, n_rows))) return rc;     // (before the first piece: a refused call leaves the store as it was)
    HIPCHK(h, hipSetDevice(h->device));
    const int64_t have = h->runs.rows[(size_t)run], row_dwords = h->N_pad / 8;
    uint32_t* image = reinterpret_cast<uint32_t*>(h->img.d) + (int64_t)run * h->run_rows * row_dwords;
    rc = h->append_pieces(h, run, rows, n_rows, [&](int64_t k, int64_t row) {
        return unit_for_grid_chunks(k * h->K, [&](int64_t l0, int64_t n) {
            k_partdist_pack<<<dim3((unsigned)n, (unsigned)div_up(row_dwords, kBlock)), kBlock, 0, h->stream>>>(
                (const uint8_t*)h->d_stage, h->K, h->K_pad, (int)h->N, row_dwords, image + row * h->K_pad * row_dwords, l0);
            HIPCHK(h, hipGetLastError());
            return SBE_OK;
        });
    });
    if (!rc) {                                            // the sizes of the new rows, from their bit rows
        const int64_t lines = n_rows * h->K;
        rc = unit_for_grid_chunks(div_up(lines, kWaves), [&](int64_t b0, int64_t n) {
            k_partdist_sizes<<<(unsigned)n, kBlock, 0, h->stream>>>(h->at(run, have), lines, (int)h->W, h->sizes.d + ((int64_t)run * h->runs.cap + have) * h->K,
                                                                  b0 * kWaves);
            HIPCHK(h, hipGetLastError());
            return SBE_OK;
        });
        if (!rc) {
            const hipError_t err = hipStreamSynchronize(h->stream);
            if (err != hipSuccess) rc = fail(h, SBE_ERR_HIP, "hipStreamSynchronize failed: %s", hipGetErrorString(err));
        }
    }
    // a piece may be in the image already while the run's row count is not: the store is unshaped instead
    // (sbe_partdist_reset comes next), as after a failed allocation
    if (rc) h->runs.rows.clear();
    return rc;
}

int sbe_partdist_sizes(sbe_partdist* h, int run, int32_t* sizes_out) {
    CHECK_HANDLE(h, kNullHandle);
    if (const int rc = h->runs.check_shaped(h, kReset)) return rc;
    if (run < 0 || run >= h->runs.count()) return fail(h, SBE_ERR_ARG, "run %d out of range [0,%d)", run, h->runs.count());
    if (!sizes_out) return fail(h, SBE_ERR_ARG, "null pointer argument: sizes_out");
    const int64_t rows = h->runs.rows[(size_t)run];
    if (rows == 0) return SBE_OK;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpyAsync(sizes_out, h->sizes_of(run), (size_t)rows * (size_t)h->K * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return SBE_OK;
}

int sbe_partdist_block(sbe_partdist* h, int row_run, int64_t row_first, int64_t n_rows, int col_run, int64_t col_first, int64_t n_cols,
                       int32_t* binder_out, double* vi_out, int32_t* sumsq_out) {
    CHECK_HANDLE(h, kNullHandle);
    if (const int rc = h->runs.check_shaped(h, kReset)) return rc;
    if (const int rc = check_range(h, "row", row_run, row_first, n_rows)) return rc;
    if (const int rc = check_range(h, "col", col_run, col_first, n_cols)) return rc;
    if (n_rows * n_cols > SBE_PARTDIST_MAX_BLOCK)
        return fail(h, SBE_ERR_ARG, "a block of %lld x %lld = %lld entries, the limit is %d (2^28)", (long long)n_rows, (long long)n_cols,
                    (long long)(n_rows * n_cols), SBE_PARTDIST_MAX_BLOCK);
    if (!binder_out && !vi_out && !sumsq_out) return fail(h, SBE_ERR_ARG, "null pointer argument: binder_out, vi_out and sumsq_out (at least one is needed)");
    const size_t entries = (size_t)(n_rows * n_cols);
    HIPCHK(h, hipSetDevice(h->device));
    int rc = SBE_OK;
    if (binder_out) rc = ensure(h, h->binder, entries);
    if (!rc && vi_out) rc = ensure(h, h->vi, entries);
    if (!rc && sumsq_out) rc = ensure(h, h->sumsq, entries);
    if (rc) return rc;
    rc = unit_timed(h, [&] {
        return launch_block(h, row_run, row_first, n_rows, col_run, col_first, n_cols, binder_out ? h->binder.d : nullptr, vi_out ? h->vi.d : nullptr,
                            sumsq_out ? h->sumsq.d : nullptr);
    });
    if (!rc && binder_out) rc = unit_copy_back(h, (const int32_t*)h->binder.d, entries, {binder_out});
    if (!rc && vi_out) rc = unit_copy_back(h, (const double*)h->vi.d, entries, {vi_out});
    if (!rc && sumsq_out) rc = unit_copy_back(h, (const int32_t*)h->sumsq.d, entries, {sumsq_out});
    if (!rc) rc = unit_sync_timed(h);
    return rc;
}

int sbe_partdist_sums(sbe_partdist* h, const uint8_t* run_mask, int64_t* binder_sum_out, double* vi_sum_out) {
    CHECK_HANDLE(h, kNullHandle);
    if (const int rc = h->runs.check_shaped(h, kReset)) return rc;
    if (!run_mask) return fail(h, SBE_ERR_ARG, "null pointer argument: run_mask");
    if (!binder_sum_out && !vi_sum_out) return fail(h, SBE_ERR_ARG, "null pointer argument: binder_sum_out and vi_sum_out (at least one is needed)");
    std::vector<int> sel;
    int64_t T = 0;
    for (int r = 0; r < h->runs.count(); ++r)
        if (run_mask[r]) {
            sel.push_back(r);
            T += h->runs.rows[(size_t)r];
        }
    if (T == 0) return fail(h, SBE_ERR_STATE, "the selected runs hold no rows");
    if (T > SBE_PARTDIST_MAX_SUM_ROWS)
        return fail(h, SBE_ERR_ARG, "the selection holds %lld rows, the limit for the sums is %d (2^16)", (long long)T, SBE_PARTDIST_MAX_SUM_ROWS);
    const int64_t R = (int64_t)sel.size();
    const size_t cells = (size_t)(T * R);
    int64_t longest = 0;
    for (int r : sel) longest = std::max(longest, h->runs.rows[(size_t)r]);
    // rows of a chunk: its dense block against the longest run stays within kSumChunkEntries (at least one row: 2^16 entries)
    const int64_t chunk_rows = std::max<int64_t>(1, kSumChunkEntries / longest);
    const size_t scratch = (size_t)(std::min(chunk_rows, longest) * longest);
    HIPCHK(h, hipSetDevice(h->device));
    int rc = ensure(h, h->binder, scratch);
    if (!rc) rc = ensure(h, h->vi, scratch);
    if (!rc) rc = ensure(h, h->bsum, cells);
    if (!rc) rc = ensure(h, h->vsum, cells);
    if (rc) return rc;
    rc = unit_timed(h, [&] {
        // (an empty run of the selection has a column of zeros)
        HIPCHK(h, hipMemsetAsync(h->bsum.d, 0, cells * sizeof(long long), h->stream));
        HIPCHK(h, hipMemsetAsync(h->vsum.d, 0, cells * sizeof(double), h->stream));
        int64_t out0 = 0;
        for (int ra : sel) {
            const int64_t rows_a = h->runs.rows[(size_t)ra];
            for (int64_t col = 0; col < R; ++col) {
                const int rb = sel[(size_t)col];
                const int64_t rows_b = h->runs.rows[(size_t)rb];
                if (rows_b == 0) continue;
                for (int64_t r0 = 0; r0 < rows_a; r0 += chunk_rows) {
                    const int64_t c = std::min(chunk_rows, rows_a - r0);
                    if (const int lrc = launch_block(h, ra, r0, c, rb, 0, rows_b, h->binder.d, h->vi.d, nullptr)) return lrc;
                    const int64_t at = (out0 + r0) * R + col;
                    const int brc = unit_for_grid_chunks(div_up(c, kWaves), [&](int64_t b0, int64_t n) {
                        k_partdist_rowsum<<<(unsigned)n, kBlock, 0, h->stream>>>(h->binder.d, h->vi.d, c, rows_b, h->bsum.d + at, h->vsum.d + at, R, b0 * kWaves);
                        HIPCHK(h, hipGetLastError());
                        return SBE_OK;
                    });
                    if (brc) return brc;
                }
            }
            out0 += rows_a;
        }
        return (int)SBE_OK;
    });
    if (!rc && binder_sum_out) rc = unit_copy_back(h, (const int64_t*)h->bsum.d, cells, {binder_sum_out});
    if (!rc && vi_sum_out) rc = unit_copy_back(h, (const double*)h->vsum.d, cells, {vi_sum_out});
    if (!rc) rc = unit_sync_timed(h);
    return rc;
}

int sbe_partdist_tables(sbe_partdist* h, const int64_t* pairs, int64_t n_pairs, int32_t* tables_out) {
    CHECK_HANDLE(h, kNullHandle);
    if (const int rc = h->runs.check_shaped(h, kReset)) return rc;
    if (n_pairs < 1 || n_pairs > SBE_PARTDIST_MAX_PAIRS)
        return fail(h, SBE_ERR_ARG, "n_pairs=%lld out of range [1, %d]", (long long)n_pairs, SBE_PARTDIST_MAX_PAIRS);
    if (!pairs || !tables_out) return fail(h, SBE_ERR_ARG, "null pointer argument: %s", !pairs ? "pairs" : "tables_out");
    for (int64_t p = 0; p < n_pairs; ++p)
        for (int side = 0; side < 2; ++side) {
            const int64_t run = pairs[4 * p + 2 * side], row = pairs[4 * p + 2 * side + 1];
            if (run < 0 || run >= h->runs.count() || row < 0 || row >= h->runs.rows[(size_t)run])
                return fail(h, SBE_ERR_ARG, "pairs[%lld]: (run %lld, row %lld) is not a stored sample", (long long)p, (long long)run, (long long)row);
        }
    const size_t cells = (size_t)n_pairs * (size_t)h->K * (size_t)h->K;
    HIPCHK(h, hipSetDevice(h->device));
    int rc = ensure(h, h->pairs, (size_t)n_pairs * 4);
    if (!rc) rc = ensure(h, h->tables, cells);
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(h->pairs.d, pairs, (size_t)n_pairs * 4 * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
    rc = unit_timed(h, [&] {
        return unit_for_grid_chunks(div_up(n_pairs, kWaves), [&](int64_t b0, int64_t n) {
            k_partdist_tables<<<(unsigned)n, kBlock, 0, h->stream>>>(h->d_bits, h->pairs.d, n_pairs, h->K, (int)h->W, h->runs.cap, h->tables.d, b0 * kWaves);
            HIPCHK(h, hipGetLastError());
            return SBE_OK;
        });
    });
    if (!rc) rc = unit_copy_back(h, (const int32_t*)h->tables.d, cells, {tables_out});
    if (!rc) rc = unit_sync_timed(h);
    return rc;
}

}  // extern "C"
