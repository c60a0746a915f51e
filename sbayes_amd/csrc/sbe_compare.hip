// sbe_compare.hip -- models compared by their pointwise ELPD values on the device (include/sbe_compare.h): the store of M
// models, totals and differences with their standard errors, stacking weights by the EM fixed point and pseudo-BMA+ weights
// by the Bayesian bootstrap.  The contract is tests/_compare_oracle.py; DESIGN.md section 20 has the layout, the structure of
// the kernels, the chunk sizes and the measured figures.
//
// The store is model-major, x[k][N_pad] float64 with N_pad whole chunks of kChunk and zeros behind N, so a wave that reads
// consecutive observations of one model is coalesced.  Every sum is a fixed tree: a thread adds at most kRun terms in
// sequence (16 in the totals and stacking kernels, kBootChunk = 1024 in the bootstrap), lanes combine by xor exchanges, waves
// in index order (sbe_unit_device.hip.h), chunks in a second kernel in index order.  There is no floating-point atomic, and
// no size depends on the card: results are bit-identical from call to call and from card to card.
//   totals / differences: two passes (sum, then squares about the mean), each k_compare_moments over (chunk, model) and
//     k_compare_moments_total over the chunk partials.
//   stacking: one update is k_compare_stack_pass (per chunk: d_i = sum_k w_k p_ik for 16 observations per thread in
//     registers, then per model the chunk's sum of p_ik / d_i) and k_compare_stack_update (one workgroup: g, the gap, the
//     new weights; the weights never leave the device).  Plain back-to-back launches; the host reads the gap every kCheckEvery.
//   bootstrap: k_compare_boot gives a lane one replicate and a chunk of kBootChunk observations: Philox, one log and M + 1
//     multiply-adds per draw into private registers, x[k][i] a wave-uniform load.  The partials [chunk][M + 1][replicate] are
//     added per replicate by k_compare_boot_reduce; k_compare_boot_rows forms z and the softmax, k_compare_boot_cols the
//     mean weights and the standard deviations.  Replicates go in batches so that the partials stay under kBootPartBytes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "sbe_philox.hip.h"
#include "sbe_unit.hip.h"
#include "../../include/sbe_compare.h"

namespace {

constexpr int kMaxM = SBE_COMPARE_MAX_MODELS;
constexpr int kBlock = SBE_COMPARE_BLOCK;
constexpr int kWaves = kBlock / 64;
constexpr int kChunk = SBE_COMPARE_CHUNK;            // observations per workgroup of the totals and stacking kernels
constexpr int kPerThread = kChunk / kBlock;          // terms a thread adds in sequence there
constexpr int kRun = SBE_COMPARE_RUN;
constexpr int kBootChunk = SBE_COMPARE_BOOT_CHUNK;   // observations per lane of the bootstrap kernel
constexpr int kCheckEvery = SBE_COMPARE_CHECK_EVERY;
constexpr int64_t kBootPartBytes = (int64_t)512 << 20;   // the bootstrap's chunk partials of one batch of replicates
constexpr int64_t kMaxChunks = SBE_COMPARE_MAX_POINTS / kChunk;
static_assert(kChunk % kBlock == 0 && kPerThread <= kRun && kBootChunk <= kRun, "no accumulator adds more than kRun terms in sequence");
static_assert(kMaxChunks <= 64 * kRun && kMaxM <= kBlock, "the chunk partials of one model are added by one wave, 64 per lane at most");
static_assert((int64_t)(SBE_COMPARE_MAX_POINTS / kBootChunk) * (kMaxM + 1) * 8 * 64 <= kBootPartBytes, "a batch of one wave of replicates always fits");

// ---- the store's check: the index of the first value of a model that is not finite --------------------------------------
__global__ __launch_bounds__(kBlock) void k_compare_check(const double* __restrict__ x, int64_t N, unsigned long long* first_bad) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < N && !isfinite(x[i])) atomicMin(first_bad, (unsigned long long)i);
}

// ---- totals and differences ------------------------------------------------------------------------------------------------
// v_i = x[k][i] (ref < 0) or x[ref][i] - x[k][i]; the chunk's sum of (v_i - center[k]) or of its square.
// blockIdx.x: chunk, blockIdx.y: model k.
struct MomentArgs {
    const double* x;          // [M][N_pad]
    int64_t N_pad, N;
    int ref;                  // -1: totals
    int square;
    const double* center;     // [M], or null: 0
    double* part;             // [M][n_chunks]
    int n_chunks;
};

__global__ __launch_bounds__(kBlock) void k_compare_moments(const MomentArgs g) {
    __shared__ double red[kWaves];
    const int k = blockIdx.y;
    const double* a = g.x + (int64_t)k * g.N_pad;
    const double* b = g.ref >= 0 ? g.x + (int64_t)g.ref * g.N_pad : nullptr;
    const double c = g.center ? g.center[k] : 0.0;
    const int64_t base = (int64_t)blockIdx.x * kChunk + threadIdx.x;
    double acc = 0.0;
#pragma unroll
    for (int u = 0; u < kPerThread; ++u) {
        const int64_t i = base + (int64_t)u * kBlock;
        if (i < g.N) {
            const double v = b ? b[i] - a[i] : a[i];
            const double t = v - c;
            acc += g.square ? t * t : t;
        }
    }
    acc = unit_block_reduce<kWaves>(acc, red, unit_sum());
    if (threadIdx.x == 0) g.part[(int64_t)k * g.n_chunks + blockIdx.x] = acc;
}

// one wave per model adds the chunk partials: lane l those of the chunks l, l + 64, ...; then sum / mean, or the root
__global__ __launch_bounds__(64) void k_compare_moments_total(const double* __restrict__ part, int n_chunks, int64_t N, int square, double* sum_out,
                                                             double* mean_out, double* root_out) {
    const int k = blockIdx.x;
    double s = 0.0;
    for (int c = threadIdx.x; c < n_chunks; c += 64) s += part[(int64_t)k * n_chunks + c];
    s = unit_wave_reduce(s, unit_sum());
    if (threadIdx.x != 0) return;
    if (square) root_out[k] = sqrt(s);                    // sqrt(N var) = sqrt(sum of squares about the mean)
    else {
        sum_out[k] = s;
        mean_out[k] = s / (double)N;
    }
}

// ---- stacking ----------------------------------------------------------------------------------------------------------------
// p[k][i] = exp(x[k][i] - max_j x[j][i]); zeros behind N
__global__ __launch_bounds__(kBlock) void k_compare_p(const double* __restrict__ x, int64_t N_pad, int64_t N, int M, double* __restrict__ p) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= N_pad) return;
    if (i >= N) {
        for (int k = 0; k < M; ++k) p[(int64_t)k * N_pad + i] = 0.0;
        return;
    }
    double mx = x[i];
    for (int k = 1; k < M; ++k) mx = fmax(mx, x[(int64_t)k * N_pad + i]);
    for (int k = 0; k < M; ++k) p[(int64_t)k * N_pad + i] = exp(x[(int64_t)k * N_pad + i] - mx);
}

__global__ void k_compare_stack_init(double* w, int M) {
    if ((int)threadIdx.x < M) w[threadIdx.x] = 1.0 / (double)M;
}

// part[k][chunk] = sum over the chunk's observations of p[k][i] / d_i, d_i = sum_j w_j p[j][i].  A thread keeps the
// reciprocals of its 16 observations in registers (the loops over u are unrolled: no indexed register array).
__global__ __launch_bounds__(kBlock) void k_compare_stack_pass(const double* __restrict__ p, int64_t N_pad, int64_t N, int M,
                                                             const double* __restrict__ w, double* __restrict__ part, int n_chunks) {
    __shared__ double red[kMaxM][kWaves];
    const int64_t base = (int64_t)blockIdx.x * kChunk + threadIdx.x;      // (N_pad holds whole chunks: every load below is inside the image)
    double r[kPerThread];
#pragma unroll
    for (int u = 0; u < kPerThread; ++u) r[u] = 0.0;
    for (int k = 0; k < M; ++k) {
        const double wk = w[k];
        const double* pk = p + (int64_t)k * N_pad + base;
#pragma unroll
        for (int u = 0; u < kPerThread; ++u) r[u] += wk * pk[u * kBlock];
    }
#pragma unroll
    for (int u = 0; u < kPerThread; ++u) r[u] = base + (int64_t)u * kBlock < N ? 1.0 / r[u] : 0.0;
    for (int k = 0; k < M; ++k) {
        const double* pk = p + (int64_t)k * N_pad + base;
        double s = 0.0;
#pragma unroll
        for (int u = 0; u < kPerThread; ++u) s += pk[u * kBlock] * r[u];
        s = unit_wave_reduce(s, unit_sum());
        if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = s;
    }
    __syncthreads();
    if ((int)threadIdx.x < M) {
        double t = red[threadIdx.x][0];
        for (int v = 1; v < kWaves; ++v) t += red[threadIdx.x][v];
        part[(int64_t)threadIdx.x * n_chunks + blockIdx.x] = t;
    }
}

// one workgroup: g_k = (sum of the chunk partials) / N by the waves in turn, then gap = max g - 1 and the new weights
__global__ __launch_bounds__(kBlock) void k_compare_stack_update(const double* __restrict__ part, int n_chunks, int M, int64_t N,
                                                               const double* __restrict__ w_in, double* __restrict__ w_out, double* gap_out) {
    __shared__ double g[kMaxM];
    const int lane = threadIdx.x & 63;
    for (int k = threadIdx.x >> 6; k < M; k += kWaves) {
        double s = 0.0;
        for (int c = lane; c < n_chunks; c += 64) s += part[(int64_t)k * n_chunks + c];
        s = unit_wave_reduce(s, unit_sum());
        if (lane == 0) g[k] = s / (double)N;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double mx = g[0], total = 0.0;
    for (int k = 0; k < M; ++k) {
        mx = fmax(mx, g[k]);
        total += w_in[k] * g[k];
    }
    for (int k = 0; k < M; ++k) w_out[k] = w_in[k] * g[k] / total;      // (total = 1 but for rounding: the weights do not drift off the simplex)
    *gap_out = mx - 1.0;
}

// ---- the Bayesian bootstrap ----------------------------------------------------------------------------------------------
// A lane owns replicate b0 + 64 blockIdx.x + lane and walks chunk blockIdx.y: e = -log(1 - u), E += e, A_k += e x[k][i].
// part: [chunk][M + 1][reps] (A_0 .. A_{M-1}, E), reps the batch's replicates in whole waves.  MT >= M accumulators; those
// behind M repeat the last model and are not written.
template <int MT>
__global__ __launch_bounds__(64) void k_compare_boot(const double* __restrict__ x, int64_t N_pad, int64_t N, int M, uint64_t seed, int64_t b0,
                                                    double* __restrict__ part, int64_t reps) {
    const int64_t rb = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const uint64_t b = (uint64_t)(b0 + rb);
    const int64_t i0 = (int64_t)blockIdx.y * kBootChunk, i1 = i0 + kBootChunk < N ? i0 + kBootChunk : N;
    const double* xk[MT];
#pragma unroll
    for (int k = 0; k < MT; ++k) xk[k] = x + (int64_t)(k < M ? k : M - 1) * N_pad;
    double acc[MT], E = 0.0;
#pragma unroll
    for (int k = 0; k < MT; ++k) acc[k] = 0.0;
    for (int64_t i = i0; i < i1; ++i) {
        const double u = sbe::philox_uniform(seed, b, (uint64_t)i);
        const double e = -log(1.0 - u);
        E += e;
#pragma unroll
        for (int k = 0; k < MT; ++k) acc[k] += e * xk[k][i];
    }
    double* out = part + (int64_t)blockIdx.y * (M + 1) * reps + rb;
#pragma unroll
    for (int k = 0; k < MT; ++k)
        if (k < M) out[(int64_t)k * reps] = acc[k];
    out[(int64_t)M * reps] = E;
}

// sums[b][j] = the chunk partials of (replicate, j) added in index order, in runs of kRun; a thread per (j, replicate)
__global__ __launch_bounds__(kBlock) void k_compare_boot_reduce(const double* __restrict__ part, int n_chunks, int M, int64_t reps, int64_t b0, int64_t B,
                                                              double* __restrict__ sums) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t rb = t % reps, j = t / reps;
    if (j > M || b0 + rb >= B) return;
    double total = 0.0;
    for (int c0 = 0; c0 < n_chunks; c0 += kRun) {
        const int c1 = c0 + kRun < n_chunks ? c0 + kRun : n_chunks;
        double s = 0.0;
        for (int c = c0; c < c1; ++c) s += part[((int64_t)c * (M + 1) + j) * reps + rb];
        total += s;
    }
    sums[(b0 + rb) * (M + 1) + j] = total;
}

// a thread per replicate: z[b][k] = N A_k / E and w_b = softmax(z[b])
__global__ __launch_bounds__(kBlock) void k_compare_boot_rows(const double* __restrict__ sums, int64_t B, int M, int64_t N, double* __restrict__ z,
                                                            double* __restrict__ wb) {
    const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (b >= B) return;
    const double* s = sums + b * (M + 1);
    const double E = s[M];
    double mx = -INFINITY;
    for (int k = 0; k < M; ++k) {
        const double zk = (double)N * s[k] / E;
        z[b * M + k] = zk;
        mx = fmax(mx, zk);
    }
    double total = 0.0;
    for (int k = 0; k < M; ++k) {
        const double t = exp(z[b * M + k] - mx);
        wb[b * M + k] = t;
        total += t;
    }
    for (int k = 0; k < M; ++k) wb[b * M + k] /= total;
}

// a workgroup per model: out[k] = mean_b w_b[k], out[M + k] = the standard deviation of z[.][k] (two passes); a thread adds
// at most MAX_REPLICATES / kBlock = 256 terms
__global__ __launch_bounds__(kBlock) void k_compare_boot_cols(const double* __restrict__ z, const double* __restrict__ wb, int64_t B, int M, double* out) {
    __shared__ double red[kWaves];
    const int k = blockIdx.x;
    double sw = 0.0, sz = 0.0;
    for (int64_t b = threadIdx.x; b < B; b += kBlock) {
        sw += wb[b * M + k];
        sz += z[b * M + k];
    }
    sw = unit_block_reduce<kWaves>(sw, red, unit_sum());
    sz = unit_block_reduce<kWaves>(sz, red, unit_sum());
    const double mean = sz / (double)B;
    double s2 = 0.0;
    for (int64_t b = threadIdx.x; b < B; b += kBlock) {
        const double t = z[b * M + k] - mean;
        s2 += t * t;
    }
    s2 = unit_block_reduce<kWaves>(s2, red, unit_sum());
    if (threadIdx.x == 0) {
        out[k] = sw / (double)B;
        out[M + k] = sqrt(s2 / (double)B);
    }
}
static_assert(SBE_COMPARE_MAX_REPLICATES / kBlock <= kRun, "a thread of k_compare_boot_cols adds at most kRun terms");

}  // namespace

struct sbe_compare : sbe_unit_handle {         // (sbe_unit.hip.h; ev: around the kernels of the last compute call)
    int M = 0;                          // (0: no shape yet)
    int64_t N = 0, N_pad = 0;
    int n_chunks = 0;                   // of kChunk observations
    std::vector<char> is_set;           // [M]
    uint64_t generation = 0;            // of the store: every reset and every set_model makes a new one
    uint64_t p_generation = 0;          // of the store when d_p was built (0: never)
    int64_t boot_batch = 0;             // replicates per batch of the bootstrap; 0: the default
    double* d_x = nullptr;              // [M][N_pad]
    size_t x_bytes = 0;
    double* d_p = nullptr;              // [M][N_pad]
    size_t p_bytes = 0;
    double* d_part = nullptr;           // [M][n_chunks]
    size_t part_bytes = 0;
    double* d_small = nullptr;          // kSmall doubles: results [3][M], weights [2][kMaxM], gap
    unsigned long long* d_flag = nullptr;
    double* d_bpart = nullptr;          // [boot chunks][M + 1][reps]
    size_t bpart_bytes = 0;
    double* d_bsums = nullptr;          // [B][M + 1]
    size_t bsums_bytes = 0;
    double* d_z = nullptr;              // [2][B][M]: z, w_b
    size_t z_bytes = 0;
    std::vector<void*> buffers() const { return {d_x, d_p, d_part, d_small, d_flag, d_bpart, d_bsums, d_z}; }
};

namespace {

constexpr char kNullHandle[] = "null handle";
constexpr int kResAt = 0, kWeightsAt = 3 * kMaxM, kGapAt = 5 * kMaxM, kSmall = 5 * kMaxM + 1;

int64_t padded(int64_t N) { return (N + kChunk - 1) / kChunk * kChunk; }

int check_ready(sbe_compare* h) {
    if (h->M == 0) return fail(h, SBE_ERR_STATE, "the store has no shape yet (sbe_compare_reset)");
    for (int k = 0; k < h->M; ++k)
        if (!h->is_set[(size_t)k]) return fail(h, SBE_ERR_STATE, "model %d has not been set since the last reset (sbe_compare_set_model)", k);
    return SBE_OK;
}

// elpd / se of the models (ref < 0) or of the differences against model ref, into d_small[kResAt ..): sums [M], roots [M]
int launch_moments(sbe_compare* h, int ref) {
    double* res = h->d_small + kResAt;
    MomentArgs args{h->d_x, h->N_pad, h->N, ref, 0, nullptr, h->d_part, h->n_chunks};
    const dim3 grid((unsigned)h->n_chunks, (unsigned)h->M);
    for (int square = 0; square < 2; ++square) {
        args.square = square;
        args.center = square ? res + 2 * h->M : nullptr;
        k_compare_moments<<<grid, kBlock, 0, h->stream>>>(args);
        HIPCHK(h, hipGetLastError());
        k_compare_moments_total<<<(unsigned)h->M, 64, 0, h->stream>>>(h->d_part, h->n_chunks, h->N, square, res, res + 2 * h->M, res + h->M);
        HIPCHK(h, hipGetLastError());
    }
    return SBE_OK;
}

int moments_call(sbe_compare* h, int ref, double* sum_out, double* root_out) {
    HIPCHK(h, hipSetDevice(h->device));
    int rc = unit_timed(h, [&] { return launch_moments(h, ref); });
    if (!rc) rc = unit_copy_back(h, (const double*)(h->d_small + kResAt), (size_t)h->M, {sum_out, root_out});
    if (!rc) rc = unit_sync_timed(h);
    return rc;
}

template <int MT>
void launch_boot(sbe_compare* h, uint64_t seed, int64_t b0, int64_t reps, int boot_chunks) {
    k_compare_boot<MT><<<dim3((unsigned)(reps / 64), (unsigned)boot_chunks), 64, 0, h->stream>>>(h->d_x, h->N_pad, h->N, h->M, seed, b0, h->d_bpart, reps);
}

}  // namespace

extern "C" {

int sbe_compare_abi_version(void) { return SBE_COMPARE_ABI_VERSION; }

const char* sbe_compare_last_error(const sbe_compare* h) { return unit_last_error(h); }

int sbe_compare_create(sbe_compare** out, int device) { return unit_create_on_device(out, device, "sbe_compare_create"); }

int sbe_compare_destroy(sbe_compare* h) { return unit_destroy(h, kNullHandle); }

int sbe_compare_last_kernel_ms(const sbe_compare* h, float* ms_out) { return unit_last_kernel_ms(h, ms_out, kNullHandle); }

int sbe_compare_set_bootstrap_batch(sbe_compare* h, int64_t replicates) {
    CHECK_HANDLE(h, kNullHandle);
    if (replicates < 0 || replicates > SBE_COMPARE_MAX_REPLICATES || replicates % 64)
        return fail(h, SBE_ERR_ARG, "replicates=%lld is not a multiple of 64 in [0, %d]", (long long)replicates, SBE_COMPARE_MAX_REPLICATES);
    h->boot_batch = replicates;
    return SBE_OK;
}

int sbe_compare_reset(sbe_compare* h, int n_models, int64_t n_points) {
    CHECK_HANDLE(h, kNullHandle);
    if (n_models < 1 || n_models > kMaxM) return fail(h, SBE_ERR_ARG, "n_models=%d out of range [1, %d]", n_models, kMaxM);
    if (n_points < 1 || n_points > SBE_COMPARE_MAX_POINTS)
        return fail(h, SBE_ERR_ARG, "n_points=%lld out of range [1, %d]", (long long)n_points, SBE_COMPARE_MAX_POINTS);
    const int64_t N_pad = padded(n_points), image = (int64_t)n_models * N_pad * (int64_t)sizeof(double);
    if (2 * image > SBE_COMPARE_MAX_IMAGE_BYTES)
        return fail(h, SBE_ERR_ARG, "a store of %d models x %lld points takes %lld bytes on the device, the limit is %lld", n_models, (long long)n_points,
                    (long long)(2 * image), (long long)SBE_COMPARE_MAX_IMAGE_BYTES);
    h->M = 0;                                             // (a failed allocation leaves an unshaped store)
    ++h->generation;
    HIPCHK(h, hipSetDevice(h->device));
    const int n_chunks = (int)(N_pad / kChunk);
    int rc = unit_ensure(h, h->d_x, h->x_bytes, (size_t)image);
    if (!rc) rc = unit_ensure(h, h->d_part, h->part_bytes, (size_t)n_models * (size_t)n_chunks * sizeof(double));
    if (!rc) rc = unit_ensure(h, h->d_small, (size_t)kSmall * sizeof(double));
    if (!rc) rc = unit_ensure(h, h->d_flag, sizeof(unsigned long long));
    if (rc) return rc;
    HIPCHK(h, hipMemsetAsync(h->d_x, 0, (size_t)image, h->stream));      // (the padding behind N stays zero)
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->N = n_points;
    h->N_pad = N_pad;
    h->n_chunks = n_chunks;
    h->is_set.assign((size_t)n_models, 0);
    h->M = n_models;
    return SBE_OK;
}

int sbe_compare_set_model(sbe_compare* h, int k, const double* x) {
    CHECK_HANDLE(h, kNullHandle);
    if (h->M == 0) return fail(h, SBE_ERR_STATE, "the store has no shape yet (sbe_compare_reset)");
    if (k < 0 || k >= h->M) return fail(h, SBE_ERR_ARG, "model %d out of range [0,%d)", k, h->M);
    if (!x) return fail(h, SBE_ERR_ARG, "null pointer argument: x");
    HIPCHK(h, hipSetDevice(h->device));
    h->is_set[(size_t)k] = 0;
    ++h->generation;
    double* dst = h->d_x + (int64_t)k * h->N_pad;
    unsigned long long first_bad = ~0ull;
    HIPCHK(h, hipMemsetAsync(h->d_flag, 0xff, sizeof first_bad, h->stream));
    HIPCHK(h, hipMemcpyAsync(dst, x, (size_t)h->N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    k_compare_check<<<(unsigned)div_up(h->N, kBlock), kBlock, 0, h->stream>>>(dst, h->N, h->d_flag);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(&first_bad, h->d_flag, sizeof first_bad, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (first_bad != ~0ull)
        return fail(h, SBE_ERR_DATA, "model %d: x[%llu]=%g is not finite", k, first_bad, x[first_bad]);
    h->is_set[(size_t)k] = 1;
    return SBE_OK;
}

int sbe_compare_totals(sbe_compare* h, double* elpd, double* se) {
    CHECK_HANDLE(h, kNullHandle);
    if (!elpd || !se) return fail(h, SBE_ERR_ARG, "null pointer argument: %s", !elpd ? "elpd" : "se");
    if (const int rc = check_ready(h)) return rc;
    return moments_call(h, -1, elpd, se);
}

int sbe_compare_differences(sbe_compare* h, int ref, double* elpd_diff, double* dse) {
    CHECK_HANDLE(h, kNullHandle);
    if (!elpd_diff || !dse) return fail(h, SBE_ERR_ARG, "null pointer argument: %s", !elpd_diff ? "elpd_diff" : "dse");
    if (const int rc = check_ready(h)) return rc;
    if (ref < 0 || ref >= h->M) return fail(h, SBE_ERR_ARG, "ref=%d out of range [0,%d)", ref, h->M);
    return moments_call(h, ref, elpd_diff, dse);
}

int sbe_compare_stacking(sbe_compare* h, double tol, int64_t max_iter, double* weights, double* gap_out, int64_t* updates_out) {
    CHECK_HANDLE(h, kNullHandle);
    if (!(tol > 0.0) || !std::isfinite(tol)) return fail(h, SBE_ERR_ARG, "tol=%g must be positive and finite", tol);
    if (max_iter < 1 || max_iter > INT32_MAX) return fail(h, SBE_ERR_ARG, "max_iter=%lld out of range [1, %d]", (long long)max_iter, INT32_MAX);
    if (!weights || !gap_out || !updates_out)
        return fail(h, SBE_ERR_ARG, "null pointer argument: %s", !weights ? "weights" : !gap_out ? "gap_out" : "updates_out");
    if (const int rc = check_ready(h)) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    const size_t image = (size_t)h->M * (size_t)h->N_pad * sizeof(double);
    if (h->p_generation != h->generation) h->p_generation = 0;
    if (const int rc = unit_ensure(h, h->d_p, h->p_bytes, image)) return rc;
    double* w = h->d_small + kWeightsAt;                  // [2][kMaxM]: evaluation e reads w[e & 1] and writes the other
    double* gap = h->d_small + kGapAt;
    double host[2 * kMaxM + 1];
    int64_t e = 0;
    int rc = unit_timed(h, [&] {
        if (h->p_generation == 0) {                       // once per generation of the store
            k_compare_p<<<(unsigned)(h->N_pad / kBlock), kBlock, 0, h->stream>>>(h->d_x, h->N_pad, h->N, h->M, h->d_p);
            HIPCHK(h, hipGetLastError());
        }
        k_compare_stack_init<<<1, 64, 0, h->stream>>>(w, h->M);
        HIPCHK(h, hipGetLastError());
        for (;; ++e) {
            k_compare_stack_pass<<<(unsigned)h->n_chunks, kBlock, 0, h->stream>>>(h->d_p, h->N_pad, h->N, h->M, w + (e & 1) * kMaxM, h->d_part, h->n_chunks);
            HIPCHK(h, hipGetLastError());
            k_compare_stack_update<<<1, kBlock, 0, h->stream>>>(h->d_part, h->n_chunks, h->M, h->N, w + (e & 1) * kMaxM, w + ((e + 1) & 1) * kMaxM, gap);
            HIPCHK(h, hipGetLastError());
            if ((e + 1) % kCheckEvery != 0 && e != max_iter) continue;
            HIPCHK(h, hipMemcpyAsync(host, w, sizeof host, hipMemcpyDeviceToHost, h->stream));
            HIPCHK(h, hipStreamSynchronize(h->stream));
            if (host[2 * kMaxM] <= tol || e == max_iter) return (int)SBE_OK;
        }
    });
    if (!rc) rc = unit_sync_timed(h);
    if (rc) return rc;
    h->p_generation = h->generation;
    std::copy(host + (e & 1) * kMaxM, host + (e & 1) * kMaxM + h->M, weights);
    *gap_out = host[2 * kMaxM];
    *updates_out = e;
    return SBE_OK;
}

int sbe_compare_bootstrap(sbe_compare* h, uint64_t seed, int64_t replicates, double* weights, double* se, double* z_out) {
    CHECK_HANDLE(h, kNullHandle);
    if (replicates < 1 || replicates > SBE_COMPARE_MAX_REPLICATES)
        return fail(h, SBE_ERR_ARG, "replicates=%lld out of range [1, %d]", (long long)replicates, SBE_COMPARE_MAX_REPLICATES);
    if (!weights || !se) return fail(h, SBE_ERR_ARG, "null pointer argument: %s", !weights ? "weights" : "se");
    if (const int rc = check_ready(h)) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    const int M = h->M, boot_chunks = div_up(h->N, kBootChunk);
    const int64_t B = replicates, B_waves = (B + 63) / 64 * 64, per_rep = (int64_t)boot_chunks * (M + 1) * (int64_t)sizeof(double);
    const int64_t fit = std::max<int64_t>(64, kBootPartBytes / per_rep / 64 * 64);
    const int64_t batch = std::min(B_waves, h->boot_batch > 0 ? std::min(h->boot_batch, fit) : fit);
    int rc = unit_ensure(h, h->d_bpart, h->bpart_bytes, (size_t)(batch * per_rep));
    if (!rc) rc = unit_ensure(h, h->d_bsums, h->bsums_bytes, (size_t)B * (size_t)(M + 1) * sizeof(double));
    if (!rc) rc = unit_ensure(h, h->d_z, h->z_bytes, (size_t)2 * (size_t)B * (size_t)M * sizeof(double));
    if (rc) return rc;
    double* z = h->d_z;
    double* wb = h->d_z + B * M;
    double* res = h->d_small + kResAt;
    rc = unit_timed(h, [&] {
        for (int64_t b0 = 0; b0 < B; b0 += batch) {
            const int64_t reps = std::min(batch, B_waves - b0);      // whole waves; the lanes behind B draw replicates nobody reads
            if (M <= 8) launch_boot<8>(h, seed, b0, reps, boot_chunks);
            else launch_boot<kMaxM>(h, seed, b0, reps, boot_chunks);
            HIPCHK(h, hipGetLastError());
            k_compare_boot_reduce<<<(unsigned)div_up(reps * (M + 1), kBlock), kBlock, 0, h->stream>>>(h->d_bpart, boot_chunks, M, reps, b0, B, h->d_bsums);
            HIPCHK(h, hipGetLastError());
        }
        k_compare_boot_rows<<<(unsigned)div_up(B, kBlock), kBlock, 0, h->stream>>>(h->d_bsums, B, M, h->N, z, wb);
        HIPCHK(h, hipGetLastError());
        k_compare_boot_cols<<<(unsigned)M, kBlock, 0, h->stream>>>(z, wb, B, M, res);
        HIPCHK(h, hipGetLastError());
        return (int)SBE_OK;
    });
    if (!rc) rc = unit_copy_back(h, (const double*)res, (size_t)M, {weights, se});
    if (!rc && z_out) rc = unit_copy_back(h, (const double*)z, (size_t)B * (size_t)M, {z_out});
    if (!rc) rc = unit_sync_timed(h);
    return rc;
}

}  // extern "C"
