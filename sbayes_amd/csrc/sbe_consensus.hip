// sbe_consensus.hip -- posterior similarity of objects and the consensus clustering on the device (include/sbe_consensus.h):
// the store of R runs of cluster samples in two forms (the bit rows are sbe_unit.hip.h's bit store), the pack kernel of the
// operand image, the similarity kernel on the matrix pipe, the score kernel and the comparison of two matrices.  The
// contract is tests/_consensus_oracle.py; DESIGN.md section 19 has the layout, the structure of the kernels and the limits.
//
// With Z the 0/1 matrix of all cluster rows of the selected runs, [T K][N], the similarity counts are Z^T Z.
// k_consensus_similarity computes one 32 x 32 tile of it per wave, for the tile pairs I <= J, with the FP4 contraction of
// sbe_unit_tiles.hip.h (the counts are exact in the f32 accumulator while T K <= 2^24).  The pack kernel has written the
// operands, so the loop is loads and MFMAs only.
//   image: [N_pad objects][n_runs segments][seg_bytes]; element e = s K + k of a run is nibble e & 7 of dword e >> 3 of
//   the run's segment; a segment is zero behind the run's last element and padded to whole rounds of 256 elements.
//   A lane owns one object (lane & 31) and one half of a step (lane >> 5): 32 elements, one 16-byte load, and both
//   operands come from this one image.
// k_consensus_scores takes one (sample, cluster) row per workgroup from the bit rows, k_consensus_compare one matrix row.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "sbe_unit_tiles.hip.h"
#include "../../include/sbe_consensus.h"

namespace {

constexpr int kMaxRuns = SBE_CONSENSUS_MAX_RUNS;
constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
// the score kernel's launches are bounded as the similarity kernel's are: a row gathers at most N^2 entries, (N / 64)^2 units of 64 x 64, and
// a launch holds at most 2^26 units (1024 rows at N = 16384, every row at N <= 512)
constexpr int64_t kScoreUnitsPerLaunch = (int64_t)1 << 26;
static_assert(kRoundElems == SBE_CONSENSUS_ROUND, "the header states the round length");

// ---- pack: host bytes [n][K][N] (staging) -> the operand image of one run's segment ----------------------------------
// A thread owns one (object, dword): the elements [8 d, 8 d + 8) of the segment that this piece holds.  A piece may start
// and end inside a dword; that dword then already holds the elements of the piece before (or zeros), which are kept.
// blockIdx.x: four dwords from d_first on, blockIdx.y: 64 objects.
__global__ __launch_bounds__(kBlock) void k_consensus_pack(const uint8_t* rows, int64_t e0, int64_t n_elems, int N, uint8_t* seg, int64_t stride,
                                                          int64_t d_first) {
    const int n = blockIdx.y * 64 + (threadIdx.x & 63);
    const int64_t d = d_first + (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    const int64_t lo = 8 * d > e0 ? 8 * d : e0, hi = 8 * d + 8 < e0 + n_elems ? 8 * d + 8 : e0 + n_elems;
    if (n >= N || lo >= hi) return;
    uint32_t bits = 0;
    for (int64_t e = lo; e < hi; ++e)
        if (rows[(e - e0) * N + n]) bits |= 2u << (4 * (int)(e & 7));
    uint32_t* out = reinterpret_cast<uint32_t*>(seg + (int64_t)n * stride) + d;
    if (hi - lo == 8) *out = bits;
    else *out |= bits;
}

// ---- the similarity kernel ------------------------------------------------------------------------------------------
struct SimArgs {
    const uint8_t* img;       // [N_pad][stride]
    int64_t stride;           // bytes of one object's image
    int32_t* counts;          // [N][N]
    int N;
    int n_seg;                // selected runs that hold rows
    int64_t t0, t_end;        // tile pairs [t0, t_end) of the enumeration t = J (J + 1) / 2 + I, I <= J
    int64_t seg_off[kMaxRuns];   // byte offset of the segment within an object's image
    int32_t seg_rounds[kMaxRuns];
};

__global__ __launch_bounds__(64) void k_consensus_similarity(const SimArgs g) {
    const int64_t t = g.t0 + blockIdx.x;
    if (t >= g.t_end) return;
    const TilePair pair = tile_pair(t);
    const int64_t I = pair.I, J = pair.J;
    const int lane = threadIdx.x, half = lane >> 5;
    // (the image has whole tiles of objects: the rows behind N are zero)
    const uint8_t* pa = g.img + (I * kTile + (lane & 31)) * g.stride + (kStep / 4) * half;
    const uint8_t* pb = g.img + (J * kTile + (lane & 31)) * g.stride + (kStep / 4) * half;
    v16f acc = {};
    for (int q = 0; q < g.n_seg; ++q) {
        const uint8_t* a = pa + g.seg_off[q];
        const uint8_t* b = pb + g.seg_off[q];
        for (int r = 0; r < g.seg_rounds[q]; ++r, a += kRoundBytes, b += kRoundBytes) {
            const LaneRound ca = load_round(a), cb = load_round(b);
#pragma unroll
            for (int u = 0; u < kRound; ++u) acc = mfma_fp4(fp4_operand(ca.q[u]), fp4_operand(cb.q[u]), acc);
        }
    }
    // the tile's rows are objects of tile I, its columns objects of tile J
    const int64_t j = J * kTile + (lane & 31);
    if (j >= g.N) return;
    // (copies for the loop's body, and a 64-bit row: the compiler then forms j N and loads counts once, not per row)
    int32_t* const counts = g.counts;
    const int64_t N = g.N;
    for_acc_entries(acc, (int64_t)half, lane & 31, [=](int64_t row, int, float v) {
        const int64_t i = I * kTile + row;
        if (i >= N) return;
        const int32_t c = (int32_t)v;
        counts[i * N + j] = c;
        if (I != J) counts[j * N + i] = c;                   // (a diagonal tile holds both triangles itself)
    });
}

// ---- the score kernel: one workgroup per (sample, cluster) row ---------------------------------------------------------
// score of the row = sum_{i,j in row} (T - 2 C[i][j]) = T m^2 - 2 sum_{i,j in row} C[i][j], m the row's size.  The member
// list goes to LDS (its order does not matter: the sums are integers); the waves take members i, the lanes members j.
__global__ __launch_bounds__(kBlock) void k_consensus_scores(const uint32_t* bits, int64_t line0, int K, int N, int W, const int32_t* counts,
                                                            long long T, unsigned long long* score) {
    extern __shared__ uint16_t members[];                      // [32 W]
    __shared__ long long red[kWaves];
    __shared__ int n_members;
    const int64_t line = line0 + blockIdx.x;                   // sample * K + cluster, within the run
    const uint32_t* row = bits + line * W;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) n_members = 0;
    __syncthreads();
    for (int w = tid; w < W; w += kBlock) {
        uint32_t word = row[w];
        if (!word) continue;
        int at = atomicAdd(&n_members, __popc(word));
        while (word) {
            members[at++] = (uint16_t)(32 * w + __ffs(word) - 1);
            word &= word - 1;
        }
    }
    __syncthreads();
    const int m = n_members;
    if (m == 0) return;                                        // (an empty cluster adds 0; uniform for the block)
    long long sum = 0;
    for (int a = wave; a < m; a += kWaves) {
        const int32_t* crow = counts + (int64_t)members[a] * N;
        for (int b = lane; b < m; b += 64) sum += crow[members[b]];
    }
    sum = unit_block_reduce<kWaves>(sum, red, unit_sum());
    if (tid == 0) atomicAdd(&score[line / K], (unsigned long long)(T * m * m - 2 * sum));
}

// ---- the comparison: one workgroup per row ------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_consensus_compare(const int32_t* ca, long long Ta, const int32_t* cb, long long Tb, int N,
                                                             long long* row_max, long long* row_sum) {
    __shared__ long long red[kWaves];
    const int i = blockIdx.x;
    long long mx = 0, sum = 0;
    for (int j = threadIdx.x; j < N; j += kBlock) {
        const long long v = ca[(int64_t)i * N + j] * Tb - cb[(int64_t)i * N + j] * Ta;
        const long long d = v < 0 ? -v : v;
        mx = d > mx ? d : mx;
        sum += d;
    }
    mx = unit_block_reduce<kWaves>(mx, red, unit_max());
    sum = unit_block_reduce<kWaves>(sum, red, unit_sum());
    if (threadIdx.x == 0) {
        row_max[i] = mx;
        row_sum[i] = sum;
    }
}

struct Slot {
    int32_t* d_counts = nullptr;        // [N][N]
    size_t bytes = 0;
    int64_t T = 0;
};

}  // namespace

// (ev: around the kernels of the last similarity, scores or compare; the image's two results are the slots)
struct sbe_consensus : sbe_unit_handle, unit_bit_store, unit_tile_launches, unit_segment_image {
    Slot slot[2];
    unsigned long long* d_score = nullptr;   // [cap]
    size_t score_bytes = 0;
    long long* d_cmp = nullptr;         // [2][N]
    size_t cmp_bytes = 0;
    std::vector<void*> buffers() const { return {slot[0].d_counts, slot[1].d_counts, d_img, d_bits, d_stage, d_score, d_cmp}; }
};

namespace {

constexpr char kNullHandle[] = "null handle";
constexpr char kLane[] = "run", kReset[] = "sbe_consensus_reset", kSlot[] = "slot", kSimilarity[] = "sbe_consensus_similarity";

constexpr unit_store_limits kLimits{kMaxRuns, SBE_CONSENSUS_MAX_CLUSTERS, SBE_CONSENSUS_MAX_OBJECTS, SBE_CONSENSUS_MAX_ROWS,
                                    SBE_CONSENSUS_MAX_IMAGE_BYTES, "(an int32 matrix [N][N] of at most 1 GiB)"};

int64_t segment_bytes(int K, int64_t cap) { return rounds_of(cap * K) * kRoundBytes; }

int64_t store_bytes(int n_runs, int K, int64_t N, int64_t cap) {
    const int64_t W = (N + 31) / 32;
    return 32 * W * n_runs * segment_bytes(K, cap) + (int64_t)n_runs * cap * K * W * (int64_t)sizeof(uint32_t);
}

}  // namespace

extern "C" {

int sbe_consensus_abi_version(void) { return SBE_CONSENSUS_ABI_VERSION; }

const char* sbe_consensus_last_error(const sbe_consensus* h) { return unit_last_error(h); }

int64_t sbe_consensus_image_bytes(int n_runs, int n_clusters, int64_t n_objects, int64_t capacity_rows) {
    return unit_bit_store::shape_ok(kLimits, n_runs, n_clusters, n_objects, capacity_rows) ? store_bytes(n_runs, n_clusters, n_objects, capacity_rows) : 0;
}

int sbe_consensus_create(sbe_consensus** out, int device) { return unit_create_on_device(out, device, "sbe_consensus_create"); }

int sbe_consensus_destroy(sbe_consensus* h) { return unit_destroy(h, kNullHandle); }

int sbe_consensus_last_kernel_ms(const sbe_consensus* h, float* ms_out) { return unit_last_kernel_ms(h, ms_out, kNullHandle); }

int sbe_consensus_set_launch_tiles(sbe_consensus* h, int64_t tile_pairs) { return unit_set_launch_tiles(h, tile_pairs, kNullHandle); }

int sbe_consensus_reset(sbe_consensus* h, int n_runs, int n_clusters, int64_t n_objects, int64_t capacity_rows) {
    CHECK_HANDLE(h, kNullHandle);
    if (const int rc = h->check_shape(h, kLimits, n_runs, n_clusters, n_objects, capacity_rows)) return rc;
    if (const int rc = h->check_device_bytes(h, kLimits, n_runs, n_clusters, n_objects, capacity_rows, store_bytes(n_runs, n_clusters, n_objects, capacity_rows)))
        return rc;
    const auto ensure_rest = [&] {
        int rc = h->alloc_bits(h, n_runs, n_clusters, n_objects, capacity_rows);
        if (!rc) rc = unit_ensure(h, h->d_score, h->score_bytes, (size_t)capacity_rows * sizeof(unsigned long long));
        if (!rc) rc = unit_ensure(h, h->d_cmp, h->cmp_bytes, (size_t)2 * (size_t)n_objects * sizeof(long long));
        return rc;
    };
    if (const int rc = h->reset_image(h, n_runs, n_objects, segment_bytes(n_clusters, capacity_rows), ensure_rest)) return rc;
    h->set_shape(n_runs, n_clusters, n_objects, capacity_rows);
    return SBE_OK;
}

int sbe_consensus_rows(const sbe_consensus* h, int run, int64_t* n_rows_out) {
    CHECK_HANDLE(h, kNullHandle);
    return h->runs.get(h, kLane, run, n_rows_out);
}

int sbe_consensus_append_rows(sbe_consensus* h, int run, const uint8_t* rows, int64_t n_rows) {
    CHECK_HANDLE(h, kNullHandle);
    int rc = h->runs.check_append(h, kLane, kReset, run, rows, n_rows);
    if (rc || n_rows == 0) return rc;
    if ((rc = h->check_binary(h, rows, 0, n_rows))) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    uint8_t* seg = h->d_img + (int64_t)run * h->seg_bytes;
    rc = h->append_pieces(h, run, rows, n_rows, [&](int64_t k, int64_t row) {
        ++h->version;                                     // (the store changes from the first piece on)
        const int64_t e0 = row * h->K, n_elems = k * h->K;
        const int64_t d_first = e0 / 8, dwords = (e0 + n_elems - 1) / 8 - d_first + 1;
        k_consensus_pack<<<dim3((unsigned)div_up(dwords, kWaves), (unsigned)div_up(h->N, 64)), kBlock, 0, h->stream>>>(
            (const uint8_t*)h->d_stage, e0, n_elems, (int)h->N, seg, h->stride, d_first);
        HIPCHK(h, hipGetLastError());
        return SBE_OK;
    });
    return h->append_done(h, rc);
}

int sbe_consensus_similarity(sbe_consensus* h, const uint8_t* run_mask, int slot, int32_t* counts_out) {
    CHECK_HANDLE(h, kNullHandle);
    if (const int rc = h->runs.check_shaped(h, kReset)) return rc;
    if (!run_mask) return fail(h, SBE_ERR_ARG, "null pointer argument: run_mask");
    if (const int rc = h->check_result_index(h, kSlot, slot)) return rc;
    SimArgs args{};
    int64_t T = 0, steps = 0;
    for (int r = 0; r < h->runs.count(); ++r) {
        const int64_t rows = h->runs.rows[(size_t)r];
        if (!run_mask[r] || rows == 0) continue;
        T += rows;
        args.seg_off[args.n_seg] = (int64_t)r * h->seg_bytes;
        args.seg_rounds[args.n_seg] = (int32_t)rounds_of(rows * h->K);
        steps += (int64_t)args.seg_rounds[args.n_seg] * kRound;
        ++args.n_seg;
    }
    if (T == 0) return fail(h, SBE_ERR_STATE, "the selected runs hold no rows");
    if (T * h->K > SBE_CONSENSUS_MAX_ELEMENTS)
        return fail(h, SBE_ERR_ARG, "the selection holds %lld rows x %d clusters = %lld elements, the limit is %d (2^24: the counts are exact in the f32 accumulator up to there)",
                    (long long)T, h->K, (long long)(T * h->K), SBE_CONSENSUS_MAX_ELEMENTS);
    Slot& s = h->slot[slot];
    const size_t nn = (size_t)h->N * (size_t)h->N;
    HIPCHK(h, hipSetDevice(h->device));
    h->result_version[slot] = 0;                          // (until the new matrix is in place)
    int rc = unit_ensure(h, s.d_counts, s.bytes, nn * sizeof(int32_t));
    if (rc) return rc;
    args.img = h->d_img;
    args.stride = h->stride;
    args.counts = s.d_counts;
    args.N = (int)h->N;
    rc = unit_launch_tile_pairs(h, steps, args, k_consensus_similarity);
    if (!rc && counts_out) rc = unit_copy_back(h, (const int32_t*)s.d_counts, nn, {counts_out});
    if (!rc) rc = unit_sync_timed(h);
    if (rc) return rc;
    s.T = T;
    h->result_version[slot] = h->version;
    return SBE_OK;
}

int sbe_consensus_scores(sbe_consensus* h, int slot, int run, int64_t* score_out) {
    CHECK_HANDLE(h, kNullHandle);
    if (const int rc = h->runs.check_shaped(h, kReset)) return rc;
    if (const int rc = h->check_result_index(h, kSlot, slot)) return rc;
    if (run < 0 || run >= h->runs.count()) return fail(h, SBE_ERR_ARG, "run %d out of range [0,%d)", run, h->runs.count());
    if (!score_out) return fail(h, SBE_ERR_ARG, "null pointer argument: score_out");
    if (const int rc = h->check_result_current(h, kSlot, kSimilarity, slot)) return rc;
    const int64_t rows = h->runs.rows[(size_t)run];
    HIPCHK(h, hipSetDevice(h->device));
    const Slot& s = h->slot[slot];
    const uint32_t* bits = h->d_bits + (int64_t)run * h->runs.cap * h->K * h->W;
    int rc = unit_timed(h, [&] {
        if (rows == 0) return (int)SBE_OK;
        HIPCHK(h, hipMemsetAsync(h->d_score, 0, (size_t)rows * sizeof(unsigned long long), h->stream));
        const int64_t side = (h->N + 63) / 64, lines = rows * h->K;
        const int64_t per_launch = std::max<int64_t>(1, std::min(kMaxGridBlocks, kScoreUnitsPerLaunch / (side * side)));
        for (int64_t l0 = 0; l0 < lines; l0 += per_launch) {
            k_consensus_scores<<<(unsigned)std::min(per_launch, lines - l0), kBlock, (size_t)(32 * h->W) * sizeof(uint16_t), h->stream>>>(
                bits, l0, h->K, (int)h->N, (int)h->W, s.d_counts, (long long)s.T, h->d_score);
            HIPCHK(h, hipGetLastError());
        }
        return (int)SBE_OK;
    });
    if (!rc && rows) rc = unit_copy_back(h, (const int64_t*)h->d_score, (size_t)rows, {score_out});
    if (!rc) rc = unit_sync_timed(h);
    return rc;
}

int sbe_consensus_compare(sbe_consensus* h, int64_t* row_max, int64_t* row_sum) {
    CHECK_HANDLE(h, kNullHandle);
    if (const int rc = h->runs.check_shaped(h, kReset)) return rc;
    if (!row_max || !row_sum) return fail(h, SBE_ERR_ARG, "null pointer argument: %s", !row_max ? "row_max" : "row_sum");
    for (int slot = 0; slot < 2; ++slot)
        if (const int rc = h->check_result_current(h, kSlot, kSimilarity, slot)) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    int rc = unit_timed(h, [&] {
        k_consensus_compare<<<(unsigned)h->N, kBlock, 0, h->stream>>>(h->slot[0].d_counts, (long long)h->slot[0].T, h->slot[1].d_counts,
                                                                    (long long)h->slot[1].T, (int)h->N, h->d_cmp, h->d_cmp + h->N);
        HIPCHK(h, hipGetLastError());
        return SBE_OK;
    });
    if (!rc) rc = unit_copy_back(h, (const int64_t*)h->d_cmp, (size_t)h->N, {row_max, row_sum});
    if (!rc) rc = unit_sync_timed(h);
    return rc;
}

}  // extern "C"
