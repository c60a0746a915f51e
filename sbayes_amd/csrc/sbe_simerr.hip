// sbe_simerr.hip -- the Monte-Carlo error of the posterior similarity matrix by batch means, and two selections of runs
// compared in units of it (include/sbe_simerr.h): the store of R runs of cluster samples as an operand image whose batches
// start on step boundaries, its pack kernel, the moments kernel on the matrix pipe and the comparison of two sides.  The
// contract is tests/_simerr_oracle.py; DESIGN.md section 30 has the layout, the structure of the kernels and the limits.
//
// With Z_q the 0/1 matrix of the cluster rows of batch q, [b K][N], the batch's counts are Z_q^T Z_q: the contraction of
// sbe_consensus.hip (the FP4 step of sbe_unit_tiles.hip.h), closed at every batch boundary.  k_simerr_moments computes one
// 32 x 32 tile per wave, for the tile pairs I <= J, and keeps the tile's sum of the batch counts (int32) and of their squares
// (int64) in registers over all batches of the side.
//   image: [N_pad objects][n_runs segments][seg_bytes]; a segment is ceil(cap / b) batches of batch_steps = ceil(b K / 64)
//   steps of 32 bytes; element t K + k of batch q (t the sample within the batch) is nibble p & 7 of dword p >> 3 of the
//   segment, p = 64 batch_steps q + t K + k; a batch is zero behind its b K elements, the image is zero wherever no element
//   was appended.  A lane owns one object (lane & 31) and one half of a step (lane >> 5), as in the consensus unit.
// k_simerr_compare takes one matrix row per workgroup.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "sbe_unit_tiles.hip.h"
#include "../../include/sbe_simerr.h"

namespace {

constexpr int kMaxRuns = SBE_SIMERR_MAX_RUNS;
constexpr int kMaxThresholds = SBE_SIMERR_MAX_THRESHOLDS;
constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kStepBytes = kStep / 2;                 // of one packed FP4 row
static_assert(kStep == SBE_SIMERR_STEP, "the header states the step length");

// ---- pack: host bytes [n][K][N] (staging) -> the operand image of one run's segment ----------------------------------
// A thread owns one (object, dword) of the segment.  A dword lies within one batch (a batch is whole steps); its positions
// behind the batch's bk = b K elements are padding and stay zero.  e0, n_elems: the run's elements s K + k that this piece
// holds.  A piece may start and end inside a batch and inside a dword; that dword then already holds the elements of the
// piece before (or zeros), which are kept.  blockIdx.x: four dwords from d_first on, blockIdx.y: 64 objects.
__global__ __launch_bounds__(kBlock) void k_simerr_pack(const uint8_t* rows, int64_t e0, int64_t n_elems, int N, int64_t bk, int64_t batch_elems,
                                                       uint8_t* seg, int64_t stride, int64_t d_first) {
    const int n = blockIdx.y * 64 + (threadIdx.x & 63);
    const int64_t d = d_first + (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    const int64_t q = 8 * d / batch_elems, o = 8 * d - q * batch_elems;      // the batch and the dword's place in it
    if (n >= N || o >= bk) return;
    const int64_t first = q * bk + o, valid = bk - o < 8 ? bk - o : 8;        // the run's element at the dword's nibble 0
    const int64_t lo = first > e0 ? first : e0, hi = first + valid < e0 + n_elems ? first + valid : e0 + n_elems;
    if (lo >= hi) return;
    uint32_t bits = 0;
    for (int64_t e = lo; e < hi; ++e)
        if (rows[(e - e0) * N + n]) bits |= 2u << (4 * (int)(e - first));
    uint32_t* out = reinterpret_cast<uint32_t*>(seg + (int64_t)n * stride) + d;
    if (hi - lo == valid) *out = bits;
    else *out |= bits;
}

// ---- the moments kernel -----------------------------------------------------------------------------------------------
struct MomentArgs {
    const uint8_t* img;       // [N_pad][stride]
    int64_t stride;           // bytes of one object's image
    int32_t* s1;              // [N][N]
    long long* s2;            // [N][N]
    int N;
    int n_seg;                // selected runs that hold a complete batch
    int batch_steps;          // steps of one batch
    int64_t t0, t_end;        // tile pairs [t0, t_end) of the enumeration t = J (J + 1) / 2 + I, I <= J
    int64_t seg_off[kMaxRuns];      // byte offset of the segment within an object's image
    int32_t seg_batches[kMaxRuns];  // complete batches of the run
};

// a lane's 16 entries of the tile: the open batch's counts and the two sums over the closed batches, all in registers
struct MomentSums {
    v16f acc = {};
    int32_t s1[kAccRegs] = {};
    long long s2[kAccRegs] = {};
    // the batch is closed: its counts (exact integers up to 2^24) go into the two sums and the accumulator is cleared;
    // returns the steps of the next batch
    __device__ inline int close_batch(int batch_steps) {
#pragma unroll
        for (int reg = 0; reg < kAccRegs; ++reg) {
            const int32_t c = (int32_t)acc[reg];
            s1[reg] += c;
            s2[reg] += (long long)c * c;
            acc[reg] = 0.0f;
        }
        return batch_steps;
    }
};

__global__ __launch_bounds__(64) void k_simerr_moments(const MomentArgs g) {
    const int64_t t = g.t0 + blockIdx.x;
    if (t >= g.t_end) return;
    const TilePair pair = tile_pair(t);
    const int64_t I = pair.I, J = pair.J;
    const int lane = threadIdx.x, half = lane >> 5;
    // (the image has whole tiles of objects: the rows behind N are zero)
    const uint8_t* pa = g.img + (I * kTile + (lane & 31)) * g.stride + (kStep / 4) * half;
    const uint8_t* pb = g.img + (J * kTile + (lane & 31)) * g.stride + (kStep / 4) * half;
    MomentSums sums;
    int left = g.batch_steps;                                  // steps until the open batch closes
    for (int q = 0; q < g.n_seg; ++q) {
        // the complete batches of a run are consecutive steps of its segment: the loads go in rounds of kRound steps whatever
        // the batch length, a batch closes after its last step's MFMA wherever in the round that is (uniform for the wave).
        // The steps behind the last whole round go one by one: a round there would read behind the complete batches
        const uint8_t* a = pa + g.seg_off[q];
        const uint8_t* b = pb + g.seg_off[q];
        const int steps = g.seg_batches[q] * g.batch_steps;    // (T K <= 2^24: below 2^25)
        for (int r = 0; r < steps / kRound; ++r, a += kRoundBytes, b += kRoundBytes) {
            const LaneRound ca = load_round(a), cb = load_round(b);
#pragma unroll
            for (int u = 0; u < kRound; ++u) {
                sums.acc = mfma_fp4(fp4_operand(ca.q[u]), fp4_operand(cb.q[u]), sums.acc);
                if (--left == 0) left = sums.close_batch(g.batch_steps);
            }
        }
        for (int u = 0; u < steps % kRound; ++u, a += kStepBytes, b += kStepBytes) {
            sums.acc = mfma_fp4(fp4_operand(*reinterpret_cast<const uint4*>(a)), fp4_operand(*reinterpret_cast<const uint4*>(b)), sums.acc);
            if (--left == 0) left = sums.close_batch(g.batch_steps);
        }
    }
    const int32_t (&s1)[kAccRegs] = sums.s1;
    const long long (&s2)[kAccRegs] = sums.s2;
    // the tile's rows are objects of tile I, its columns objects of tile J
    const int64_t j = J * kTile + (lane & 31);
    if (j >= g.N) return;
    int32_t* const out1 = g.s1;
    long long* const out2 = g.s2;
    const int64_t N = g.N;
#pragma unroll
    for (int reg = 0; reg < kAccRegs; ++reg) {
        const int64_t i = I * kTile + acc_row(reg, (int64_t)half);
        if (i >= N) continue;
        out1[i * N + j] = s1[reg];
        out2[i * N + j] = s2[reg];
        if (I != J) {                                          // (a diagonal tile holds both triangles itself)
            out1[j * N + i] = s1[reg];
            out2[j * N + i] = s2[reg];
        }
    }
}

// ---- the comparison: one workgroup per row ------------------------------------------------------------------------------
struct CompareArgs {
    const int32_t *s1a, *s1b;     // [N][N]
    const long long *s2a, *s2b;
    long long nba, nbb;           // batches of the two sides, each >= 2
    int N, n_thr;
    double thr[kMaxThresholds];
    double* z2;                   // [N][N] or null
    double* row_max;              // [N]
    int32_t* row_arg;             // [N]
    int32_t* row_count;           // [N][n_thr]
};

// the float64 steps of the header, in its order (the file is compiled without contraction; none of the steps could contract)
__device__ inline double z_squared(long long s1a, long long s2a, long long nba, long long s1b, long long s2b, long long nbb) {
    const long long va = nba * s2a - s1a * s1a, vb = nbb * s2b - s1b * s1b, D = s1a * nbb - s1b * nba;
    const double d = (double)D, num = d * d;
    const double qa = ((double)va * (double)(nbb * nbb)) / (double)(nba - 1);
    const double qb = ((double)vb * (double)(nba * nba)) / (double)(nbb - 1);
    const double den = qa + qb;
    return den > 0.0 ? num / den : (D == 0 ? 0.0 : (double)INFINITY);
}

__global__ __launch_bounds__(kBlock) void k_simerr_compare(const CompareArgs g) {
    __shared__ double red_max[kWaves];
    __shared__ uint32_t red_arg[kWaves];
    __shared__ int red_count[kWaves];
    const int64_t row = (int64_t)blockIdx.x * g.N;
    double mx = -1.0;                                          // (z2 >= 0: a thread without a column loses to every other)
    uint32_t arg = 0xffffffffu;
    int count[kMaxThresholds] = {};
    for (int j = threadIdx.x; j < g.N; j += kBlock) {
        const double z = z_squared(g.s1a[row + j], g.s2a[row + j], g.nba, g.s1b[row + j], g.s2b[row + j], g.nbb);
        if (g.z2) g.z2[row + j] = z;
        if (z > mx) {                                          // (ascending j: a thread keeps its first maximum)
            mx = z;
            arg = (uint32_t)j;
        }
#pragma unroll
        for (int m = 0; m < kMaxThresholds; ++m) count[m] += m < g.n_thr && z > g.thr[m];
    }
    const double best = unit_block_reduce<kWaves>(mx, red_max, unit_max());
    const uint32_t at = unit_block_reduce<kWaves>(mx == best ? arg : 0xffffffffu, red_arg, unit_min());
#pragma unroll
    for (int m = 0; m < kMaxThresholds; ++m) {
        if (m >= g.n_thr) break;                               // (uniform for the block)
        const int total = unit_block_reduce<kWaves>(count[m], red_count, unit_sum());
        if (threadIdx.x == 0) g.row_count[(int64_t)blockIdx.x * g.n_thr + m] = total;
    }
    if (threadIdx.x == 0) {
        g.row_max[blockIdx.x] = best;
        g.row_arg[blockIdx.x] = (int32_t)at;
    }
}

struct Side {
    int32_t* d_s1 = nullptr;            // [N][N]
    size_t s1_bytes = 0;
    long long* d_s2 = nullptr;          // [N][N]
    size_t s2_bytes = 0;
    int64_t n_batches = 0;
};

}  // namespace

// (the bit store's lanes, shape, staging buffer and host checks; its bit rows are not kept: d_bits stays null.  ev: around
// the kernels of the last moments or compare; the image's two results are the sides)
struct sbe_simerr : sbe_unit_handle, unit_bit_store, unit_tile_launches, unit_segment_image {
    int64_t batch_rows = 0, batch_steps = 0;
    Side side[2];
    double* d_z2 = nullptr;             // [N][N], once a compare has asked for it
    size_t z2_bytes = 0;
    double* d_row_max = nullptr;        // [N]
    size_t row_max_bytes = 0;
    int32_t* d_row_int = nullptr;       // [N] row_arg, then [N][kMaxThresholds] row_count
    size_t row_int_bytes = 0;
    std::vector<void*> buffers() const {
        return {side[0].d_s1, side[0].d_s2, side[1].d_s1, side[1].d_s2, d_img, d_bits, d_stage, d_z2, d_row_max, d_row_int};
    }
};

namespace {

constexpr char kNullHandle[] = "null handle";
constexpr char kLane[] = "run", kReset[] = "sbe_simerr_reset", kSide[] = "side", kMoments[] = "sbe_simerr_moments";

constexpr unit_store_limits kLimits{kMaxRuns, SBE_SIMERR_MAX_CLUSTERS, SBE_SIMERR_MAX_OBJECTS, SBE_SIMERR_MAX_ROWS, SBE_SIMERR_MAX_IMAGE_BYTES,
                                    "(a side holds 12 N^2 bytes: at most 768 MiB)"};

int64_t steps_of_batch(int K, int64_t b) { return (b * K + kStep - 1) / kStep; }

int64_t segment_bytes(int K, int64_t cap, int64_t b) { return (cap + b - 1) / b * steps_of_batch(K, b) * kStepBytes; }

int64_t store_bytes(int n_runs, int K, int64_t N, int64_t cap, int64_t b) { return whole_tiles(N) * n_runs * segment_bytes(K, cap, b); }

bool batch_ok(int64_t cap, int64_t b) { return b >= 1 && b <= cap; }

}  // namespace

extern "C" {

int sbe_simerr_abi_version(void) { return SBE_SIMERR_ABI_VERSION; }

const char* sbe_simerr_last_error(const sbe_simerr* h) { return unit_last_error(h); }

int64_t sbe_simerr_image_bytes(int n_runs, int n_clusters, int64_t n_objects, int64_t capacity_rows, int64_t batch_rows) {
    return unit_bit_store::shape_ok(kLimits, n_runs, n_clusters, n_objects, capacity_rows) && batch_ok(capacity_rows, batch_rows)
               ? store_bytes(n_runs, n_clusters, n_objects, capacity_rows, batch_rows)
               : 0;
}

int sbe_simerr_create(sbe_simerr** out, int device) { return unit_create_on_device(out, device, "sbe_simerr_create"); }

int sbe_simerr_destroy(sbe_simerr* h) { return unit_destroy(h, kNullHandle); }

int sbe_simerr_last_kernel_ms(const sbe_simerr* h, float* ms_out) { return unit_last_kernel_ms(h, ms_out, kNullHandle); }

int sbe_simerr_set_launch_tiles(sbe_simerr* h, int64_t tile_pairs) { return unit_set_launch_tiles(h, tile_pairs, kNullHandle); }

int sbe_simerr_reset(sbe_simerr* h, int n_runs, int n_clusters, int64_t n_objects, int64_t capacity_rows, int64_t batch_rows) {
    CHECK_HANDLE(h, kNullHandle);
    if (const int rc = h->check_shape(h, kLimits, n_runs, n_clusters, n_objects, capacity_rows)) return rc;
    if (!batch_ok(capacity_rows, batch_rows))
        return fail(h, SBE_ERR_ARG, "batch_rows=%lld out of range [1, %lld] (the capacity of a run)", (long long)batch_rows, (long long)capacity_rows);
    const int64_t img = store_bytes(n_runs, n_clusters, n_objects, capacity_rows, batch_rows);
    if (const int rc = h->check_device_bytes(h, kLimits, n_runs, n_clusters, n_objects, capacity_rows, img)) return rc;
    // (the image is zero in the padding of every batch too)
    const auto ensure_rows = [&] {
        const int rc = unit_ensure(h, h->d_row_max, h->row_max_bytes, (size_t)n_objects * sizeof(double));
        return rc ? rc : unit_ensure(h, h->d_row_int, h->row_int_bytes, (size_t)n_objects * (1 + kMaxThresholds) * sizeof(int32_t));
    };
    if (const int rc = h->reset_image(h, n_runs, n_objects, segment_bytes(n_clusters, capacity_rows, batch_rows), ensure_rows)) return rc;
    h->batch_rows = batch_rows;
    h->batch_steps = steps_of_batch(n_clusters, batch_rows);
    h->set_shape(n_runs, n_clusters, n_objects, capacity_rows);
    return SBE_OK;
}

int sbe_simerr_rows(const sbe_simerr* h, int run, int64_t* n_rows_out) {
    CHECK_HANDLE(h, kNullHandle);
    return h->runs.get(h, kLane, run, n_rows_out);
}

int sbe_simerr_append_rows(sbe_simerr* h, int run, const uint8_t* rows, int64_t n_rows) {
    CHECK_HANDLE(h, kNullHandle);
    int rc = h->runs.check_append(h, kLane, kReset, run, rows, n_rows);
    if (rc || n_rows == 0) return rc;
    if ((rc = h->check_binary(h, rows, 0, n_rows))) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    uint8_t* seg = h->d_img + (int64_t)run * h->seg_bytes;
    const int64_t have = h->runs.rows[(size_t)run], bk = h->batch_rows * h->K, batch_elems = h->batch_steps * kStep;
    auto place = [&](int64_t e) { return e / bk * batch_elems + e % bk; };      // of a run's element in its segment
    rc = unit_append_pieces(h, h->d_stage, h->stage_bytes, rows, n_rows, (int64_t)h->K * h->N, h->runs.cap, [&](int64_t k, int64_t r) {
        ++h->version;                                     // (the store changes from the first piece on)
        const int64_t e0 = (have + r) * h->K, n_elems = k * h->K;
        const int64_t d_first = place(e0) / 8, blocks = div_up(place(e0 + n_elems - 1) / 8 - d_first + 1, kWaves);
        return unit_for_grid_chunks(blocks, [&](int64_t b0, int64_t n) {
            k_simerr_pack<<<dim3((unsigned)n, (unsigned)div_up(h->N, 64)), kBlock, 0, h->stream>>>((const uint8_t*)h->d_stage, e0, n_elems, (int)h->N, bk,
                                                                                                 batch_elems, seg, h->stride, d_first + b0 * kWaves);
            HIPCHK(h, hipGetLastError());
            return SBE_OK;
        });
    });
    if (!rc) h->runs.rows[(size_t)run] = have + n_rows;
    return h->append_done(h, rc);
}

int sbe_simerr_moments(sbe_simerr* h, const uint8_t* run_mask, int side, int32_t* s1_out, int64_t* s2_out, int64_t* n_batches_out) {
    CHECK_HANDLE(h, kNullHandle);
    if (const int rc = h->runs.check_shaped(h, kReset)) return rc;
    if (!run_mask) return fail(h, SBE_ERR_ARG, "null pointer argument: run_mask");
    if (const int rc = h->check_result_index(h, kSide, side)) return rc;
    MomentArgs args{};
    int64_t nB = 0, rows_selected = 0;
    for (int r = 0; r < h->runs.count(); ++r) {
        if (!run_mask[r]) continue;
        const int64_t rows = h->runs.rows[(size_t)r], batches = rows / h->batch_rows;
        rows_selected += rows;
        if (batches == 0) continue;
        nB += batches;
        args.seg_off[args.n_seg] = (int64_t)r * h->seg_bytes;
        args.seg_batches[args.n_seg] = (int32_t)batches;
        ++args.n_seg;
    }
    if (nB < 2)
        return fail(h, SBE_ERR_STATE, "the selected runs hold %lld complete batches of %lld rows (%lld rows in all); a side takes at least 2 batches",
                    (long long)nB, (long long)h->batch_rows, (long long)rows_selected);
    const int64_t T = nB * h->batch_rows;
    if (T * h->K > SBE_SIMERR_MAX_ELEMENTS)
        return fail(h, SBE_ERR_ARG, "the side holds %lld rows x %d clusters = %lld elements, the limit is %d (2^24: the counts are exact in the f32 accumulator up to there)",
                    (long long)T, h->K, (long long)(T * h->K), SBE_SIMERR_MAX_ELEMENTS);
    Side& s = h->side[side];
    const size_t nn = (size_t)h->N * (size_t)h->N;
    HIPCHK(h, hipSetDevice(h->device));
    h->result_version[side] = 0;                          // (until the new moments are in place)
    int rc = unit_ensure(h, s.d_s1, s.s1_bytes, nn * sizeof(int32_t));
    if (!rc) rc = unit_ensure(h, s.d_s2, s.s2_bytes, nn * sizeof(long long));
    if (rc) return rc;
    args.img = h->d_img;
    args.stride = h->stride;
    args.s1 = s.d_s1;
    args.s2 = s.d_s2;
    args.N = (int)h->N;
    args.batch_steps = (int)h->batch_steps;
    rc = unit_launch_tile_pairs(h, nB * h->batch_steps, args, k_simerr_moments);
    if (!rc && s1_out) rc = unit_copy_back(h, (const int32_t*)s.d_s1, nn, {s1_out});
    if (!rc && s2_out) rc = unit_copy_back(h, (const int64_t*)s.d_s2, nn, {s2_out});
    if (!rc) rc = unit_sync_timed(h);
    if (rc) return rc;
    if (n_batches_out) *n_batches_out = nB;
    s.n_batches = nB;
    h->result_version[side] = h->version;
    return SBE_OK;
}

int sbe_simerr_compare(sbe_simerr* h, const double* thresholds, int n_thresholds, double* z2_out, double* row_max, int32_t* row_arg,
                       int32_t* row_count) {
    CHECK_HANDLE(h, kNullHandle);
    if (const int rc = h->runs.check_shaped(h, kReset)) return rc;
    if (n_thresholds < 0 || n_thresholds > kMaxThresholds)
        return fail(h, SBE_ERR_ARG, "n_thresholds=%d out of range [0, %d]", n_thresholds, kMaxThresholds);
    if (!row_max || !row_arg) return fail(h, SBE_ERR_ARG, "null pointer argument: %s", !row_max ? "row_max" : "row_arg");
    if (n_thresholds > 0 && (!thresholds || !row_count))
        return fail(h, SBE_ERR_ARG, "null pointer argument: %s", !thresholds ? "thresholds" : "row_count");
    CompareArgs args{};
    for (int m = 0; m < n_thresholds; ++m) {
        if (std::isnan(thresholds[m])) return fail(h, SBE_ERR_ARG, "thresholds[%d] is not a number", m);
        args.thr[m] = thresholds[m];
    }
    for (int side = 0; side < 2; ++side)
        if (const int rc = h->check_result_current(h, kSide, kMoments, side)) return rc;
    const size_t N = (size_t)h->N, nn = N * N;
    HIPCHK(h, hipSetDevice(h->device));
    if (z2_out)
        if (const int rc = unit_ensure(h, h->d_z2, h->z2_bytes, nn * sizeof(double))) return rc;
    args.s1a = h->side[0].d_s1;
    args.s2a = h->side[0].d_s2;
    args.nba = h->side[0].n_batches;
    args.s1b = h->side[1].d_s1;
    args.s2b = h->side[1].d_s2;
    args.nbb = h->side[1].n_batches;
    args.N = (int)h->N;
    args.n_thr = n_thresholds;
    args.z2 = z2_out ? h->d_z2 : nullptr;
    args.row_max = h->d_row_max;
    args.row_arg = h->d_row_int;
    args.row_count = h->d_row_int + N;
    int rc = unit_timed(h, [&] {
        k_simerr_compare<<<(unsigned)N, kBlock, 0, h->stream>>>(args);
        HIPCHK(h, hipGetLastError());
        return SBE_OK;
    });
    if (!rc && z2_out) rc = unit_copy_back(h, (const double*)h->d_z2, nn, {z2_out});
    if (!rc) rc = unit_copy_back(h, (const double*)h->d_row_max, N, {row_max});
    if (!rc) rc = unit_copy_back(h, (const int32_t*)h->d_row_int, N, {row_arg});
    if (!rc && n_thresholds) rc = unit_copy_back(h, (const int32_t*)(h->d_row_int + N), N * (size_t)n_thresholds, {row_count});
    if (!rc) rc = unit_sync_timed(h);
    return rc;
}

}  // extern "C"
