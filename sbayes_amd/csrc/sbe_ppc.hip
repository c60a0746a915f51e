// sbe_ppc.hip -- the posterior predictive check on the device (include/sbe_ppc.h): per logged sample a replicated data set
// drawn from the mixture row of every cell that has a code, the deviance -2 log m at the drawn and at the observed state,
// its sums per feature and per object, and the state counts of the replicate.  The contract is tests/_ppc_oracle.py;
// DESIGN.md section 22 has the layout, the kernels and the bounds.
//
// A check call holds its n samples on the device and runs
//   k_predict_ids, k_predict_validate   sbe_predict_row.hip.h's, as the posterior predictive runs them;
//   k_ppc_validate_uniforms             a thread per uniform the caller passed;
//   k_ppc_draw<SP, CP>                  (only after the host has read that the kernels above found nothing)
//                       k_predict_accumulate's plan: a workgroup owns a tile of Ft features x Nt = 256 / Ft objects, a thread
//                       one cell of it, the sample's slice of the tables and weights is double-buffered in LDS with one barrier
//                       per sample, and the row arithmetic is sbe_predict_row.hip.h's.  Per sample a thread builds the cdf of
//                       its cell in registers (SP: S padded to a power of two, so the loops unroll), draws the state, and
//                       recomputes m[x] and m[y] from LDS instead of indexing a register array dynamically.  It writes the
//                       replicate's state, the two d values of the cell and one integer atomic on the state's count;
//   k_ppc_sum_objects, k_ppc_sum_features   the d values of a (sample, side, feature) over the objects and of a (sample, side,
//                       object) over the features, in the trees the header fixes: no floating-point atomics, and no bit
//                       depends on the tile, the split of the samples or the call.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "sbe_philox.hip.h"
#include "sbe_predict_row.hip.h"
#include "../../include/sbe_ppc.h"

namespace {

constexpr int kFeatureLanes = 16;        // k_ppc_sum_objects: lanes per feature, and features per workgroup
static_assert(kFeatureLanes * kFeatureLanes == kBlock, "a workgroup of k_ppc_sum_objects is 16 features x 16 lanes");

// ---- validation of the caller's uniforms: a thread per entry -------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_ppc_validate_uniforms(const double* uniforms, int64_t n, int64_t cells, unsigned long long* err,
                                                                  int64_t block0) {
    const int64_t q = (block0 + blockIdx.x) * kBlock + threadIdx.x;
    if (q >= n * cells) return;
    const double u = uniforms[q];
    if (!(u >= 0.0 && u < 1.0)) {                              // negative, 1 or more, NaN
        const int64_t t = q / cells;
        atomicMin(err, error_key(t, kUniform, q - t * cells));
    }
}

// ---- the draws ----------------------------------------------------------------------------------------------------------------
struct DrawArgs {
    const uint8_t* codes;          // [N][F]
    const uint8_t* groups;         // [C-1][N]
    const uint16_t* kid;           // [n][N]
    const double* weights;         // [n][F][C]
    const double* tables;          // [n][R][F][S]
    const double* uniforms;        // [n][N F] or null: Philox
    uint8_t* y_rep;                // [n][N][F] or null
    double* d;                     // [n][2][N][F]: d_obs, d_rep of every cell, or null
    int* count_rep;                // [n][F][S] or null
    unsigned long long* n_skipped;
    uint64_t seed;
    int64_t first_draw;
    int64_t N;
    int F, S, C, R;
    int n;
    int Ft, Nt, f_tiles;
    int64_t block0;                // of this launch
    int row_off[kMaxC];            // first table row of a component's groups (row_off[0] = 0: the clusters)
};

template <int SP, int CP>
__global__ __launch_bounds__(kBlock) void k_ppc_draw(const DrawArgs g) {
    extern __shared__ double lds[];                            // two slices
    const TileCell tc = tile_cell(g);
    const bool live = tc.live;
    const int64_t cell = tc.cell;
    const int64_t cells = g.N * g.F;

    int row[CP];                                               // the object's table row per component (0: not applicable)
    bool has[CP];
#pragma unroll
    for (int c = 0; c < CP; ++c) cell_group(g, tc, c, row[c], has[c]);
    int x = kNA;
    if (live) x = g.codes[cell];
    unsigned long long skipped = 0;

    stage_slice(lds, g, 0, tc.f0, tc.fw);
    __syncthreads();
    for (int t = 0; t < g.n; ++t) {
        const double* cur = lds + (t & 1) * tc.slice;
        if (t + 1 < g.n) stage_slice(lds + ((t + 1) & 1) * tc.slice, g, t + 1, tc.f0, tc.fw);
        if (live) {
            double d_obs = 0.0, d_rep = 0.0;                   // what a cell without a code, or a skipped one, adds
            int y = kNA;
            if (x != kNA) {
                double wn[CP];
                const double* base[CP];
                cell_weights(g, tc, cur, t, row, has, wn, base);
                double cdf[SP], total = 0.0;
                int last = 0;                                  // the last state of positive mass
#pragma unroll
                for (int s = 0; s < SP; ++s) {
                    if (s < g.S) {
                        const double m = cell_state(g.C, wn, base, s);
                        total += m;
                        if (m > 0.0) last = s;
                    }
                    cdf[s] = total;
                }
                if (total > 0.0) {
                    const double u = g.uniforms ? g.uniforms[(int64_t)t * cells + cell]
                                                : sbe::philox_uniform(g.seed, (uint64_t)(g.first_draw + t), (uint64_t)cell);
                    const double v = u * total;
                    int below = 0;
#pragma unroll
                    for (int s = 0; s < SP; ++s) below += s < g.S && cdf[s] <= v ? 1 : 0;
                    y = min(below, last);
                    if (g.d) {
                        d_obs = -2.0 * log(cell_state(g.C, wn, base, x));
                        d_rep = -2.0 * log(cell_state(g.C, wn, base, y));
                    }
                    if (g.count_rep) atomicAdd(g.count_rep + ((int64_t)t * g.F + tc.f) * g.S + y, 1);
                } else {
                    ++skipped;
                }
            }
            if (g.y_rep) g.y_rep[(int64_t)t * cells + cell] = (uint8_t)y;
            if (g.d) {
                g.d[(int64_t)(2 * t) * cells + cell] = d_obs;
                g.d[(int64_t)(2 * t + 1) * cells + cell] = d_rep;
            }
        }
        __syncthreads();                                       // sample t is read, the slice of t + 1 is written
    }
    if (skipped) atomicAdd(g.n_skipped, skipped);
}

using DrawKernel = void (*)(const DrawArgs);

template <int SP>
DrawKernel draw_kernel_c(int C) {
    if (C <= 1) return k_ppc_draw<SP, 1>;
    if (C <= 2) return k_ppc_draw<SP, 2>;
    if (C <= 4) return k_ppc_draw<SP, 4>;
    return k_ppc_draw<SP, 8>;
}

DrawKernel draw_kernel(int S, int C) {
    if (S <= 2) return draw_kernel_c<2>(C);
    if (S <= 4) return draw_kernel_c<4>(C);
    if (S <= 8) return draw_kernel_c<8>(C);
    if (S <= 16) return draw_kernel_c<16>(C);
    return draw_kernel_c<32>(C);
}

// ---- the sums -------------------------------------------------------------------------------------------------------------------
// dev_feature[q][f], q = 2 t + side: a workgroup takes 16 features of one q; lane j of a feature's 16 adds the objects j,
// j + 16, .. in order onto 0; then the lanes' sums are added in order 0 .. 15.  blockIdx.x + block0 = q * f_blocks + feature block.
__global__ __launch_bounds__(kBlock) void k_ppc_sum_objects(const double* d, int64_t N, int F, int f_blocks, double* dev_feature, int64_t block0) {
    __shared__ double part[kFeatureLanes][kFeatureLanes];
    const int64_t b = block0 + blockIdx.x;
    const int64_t q = b / f_blocks;
    const int f = (int)(b - q * f_blocks) * kFeatureLanes + (threadIdx.x % kFeatureLanes);
    const int lane = threadIdx.x / kFeatureLanes;
    double sum = 0.0;
    if (f < F) {
        const double* col = d + q * N * F + f;
        for (int64_t obj = lane; obj < N; obj += kFeatureLanes) sum += col[obj * F];
    }
    part[lane][threadIdx.x % kFeatureLanes] = sum;
    __syncthreads();
    if (lane == 0 && f < F) {
        double total = part[0][threadIdx.x];
        for (int j = 1; j < kFeatureLanes; ++j) total += part[j][threadIdx.x];
        dev_feature[q * F + f] = total;
    }
}

// dev_object[row], row = (2 t + side) N + object: a wave takes one row of d; lane j adds the features j, j + 64, .. in order
// onto 0; then the fixed tree of the unit layer over the lanes
__global__ __launch_bounds__(kBlock) void k_ppc_sum_features(const double* d, int64_t rows, int F, double* dev_object, int64_t block0) {
    const int64_t row = (block0 + blockIdx.x) * (kBlock / 64) + (threadIdx.x >> 6);
    if (row >= rows) return;                                   // (a whole wave)
    const double* v = d + row * F;
    double sum = 0.0;
    for (int f = threadIdx.x & 63; f < F; f += 64) sum += v[f];
    sum = unit_wave_reduce(sum, unit_sum());
    if ((threadIdx.x & 63) == 0) dev_object[row] = sum;
}

}  // namespace

struct sbe_ppc : sbe_unit_handle, sample_store {
    // d_words: [0]: n_skipped of the call, [1]: the first offender's key
    double* d_uniforms = nullptr;       // [n][N F]
    size_t uniforms_bytes = 0;
    uint8_t* d_y = nullptr;             // [n][N][F]
    size_t y_bytes = 0;
    double* d_d = nullptr;              // [n][2][N][F]
    size_t d_bytes = 0;
    double* d_sums = nullptr;           // dev_feature [n][2][F], then dev_object [n][2][N]
    size_t sums_bytes = 0;
    int* d_counts = nullptr;            // [n][F][S]
    size_t counts_bytes = 0;
    std::vector<void*> buffers() const { return buffers_with({d_uniforms, d_y, d_d, d_sums, d_counts}); }
};

namespace {

constexpr char kPrefix[] = "sbe_ppc";

int64_t sample_bytes(int64_t N, int64_t F, int S, int C, int K, int R, bool y_rep, bool uniforms) {
    return (int64_t)K * N + 8 * F * C + 8 * (int64_t)R * F * S + 2 * N + 16 * N * F + 16 * F + 16 * N + 4 * F * S + (y_rep ? N * F : 0) +
           (uniforms ? 8 * N * F : 0);
}

}  // namespace

extern "C" {

int sbe_ppc_abi_version(void) { return SBE_PPC_ABI_VERSION; }

const char* sbe_ppc_last_error(const sbe_ppc* h) { return unit_last_error(h); }

int sbe_ppc_create(sbe_ppc** out, int device) { return unit_create_on_device(out, device, "sbe_ppc_create"); }

int sbe_ppc_destroy(sbe_ppc* h) { return unit_destroy(h, kNullHandle); }

int sbe_ppc_last_kernel_ms(const sbe_ppc* h, float* ms_out) { return unit_last_kernel_ms(h, ms_out, kNullHandle); }

int64_t sbe_ppc_sample_bytes(int64_t n_objects, int64_t n_features, int n_states, int n_components, int n_clusters, int n_rows, int with_y_rep,
                             int with_uniforms) {
    return shape_ok(n_objects, n_features, n_states, n_components, n_clusters, n_rows)
               ? sample_bytes(n_objects, n_features, n_states, n_components, n_clusters, n_rows, with_y_rep != 0, with_uniforms != 0)
               : 0;
}

int sbe_ppc_set_feature_tile(sbe_ppc* h, int features) { return set_feature_tile(h, features); }

int sbe_ppc_set_data(sbe_ppc* h, int64_t N, int64_t F, int S, int C, int K, const uint8_t* codes, const uint8_t* groups, const int* n_groups) {
    CHECK_HANDLE(h, kNullHandle);
    int row_off[kMaxC], R;
    if (const int bad = check_data(h, N, F, S, C, K, codes, groups, n_groups, row_off, R)) return bad;
    return h->upload(h, N, F, S, C, K, R, row_off, codes, groups, no_hook, [&] { return wait_for_stream(h); });
}

int sbe_ppc_check(sbe_ppc* h, int64_t n, int64_t first_draw, uint64_t seed, const uint8_t* clusters, const double* weights, const double* tables,
                  const double* uniforms, uint8_t* y_rep, double* dev_feature, double* dev_object, int32_t* count_rep, int64_t* n_skipped_out) {
    CHECK_HANDLE(h, kNullHandle);
    if (!h->has_data) return no_data(h, kPrefix);
    if (n < 0) return fail(h, SBE_ERR_ARG, "n=%lld is negative", (long long)n);
    if (first_draw < 0) return fail(h, SBE_ERR_ARG, "first_draw=%lld is negative", (long long)first_draw);
    if (n == 0) {
        if (n_skipped_out) *n_skipped_out = 0;
        return SBE_OK;
    }
    const int64_t N = h->N, F = h->F, cells = N * F;
    const int S = h->S;
    const bool sums = dev_feature || dev_object;
    const size_t u_bytes = (size_t)n * cells * sizeof(double), c_bytes = (size_t)n * F * S * sizeof(int);
    unsigned long long* d_err = h->d_words + 1;
    SamplePlan plan;
    int rc = h->stage(
        h, n, clusters, weights, tables, sample_bytes(N, F, S, h->C, h->K, h->R, y_rep != nullptr, uniforms != nullptr), SBE_PPC_MAX_STAGE_BYTES, d_err,
        [&] {
            int own = uniforms ? unit_ensure(h, h->d_uniforms, h->uniforms_bytes, u_bytes) : SBE_OK;
            if (!own && y_rep) own = unit_ensure(h, h->d_y, h->y_bytes, (size_t)n * cells);
            if (!own && sums) own = unit_ensure(h, h->d_d, h->d_bytes, 2 * u_bytes);
            if (!own && sums) own = unit_ensure(h, h->d_sums, h->sums_bytes, (size_t)n * 2 * (size_t)(F + N) * sizeof(double));
            if (!own && count_rep) own = unit_ensure(h, h->d_counts, h->counts_bytes, c_bytes);
            if (!own && uniforms) own = copy_pieces(h, h->d_uniforms, uniforms, u_bytes, hipMemcpyHostToDevice);
            return own;
        },
        [&] {
            if (!uniforms) return SBE_OK;
            return unit_for_grid_chunks(div_up(n * cells, kBlock), [&](int64_t first, int64_t count) {
                k_ppc_validate_uniforms<<<(unsigned)count, kBlock, 0, h->stream>>>(h->d_uniforms, n, cells, d_err, first);
                HIPCHK(h, hipGetLastError());
                return SBE_OK;
            });
        },
        plan);
    if (rc) return rc;
    if (plan.key != kNoError) {                                // (kUniform: the other kinds are worded by the store)
        const long long at = (long long)(plan.key & ((1ull << 36) - 1));
        return fail(h, SBE_ERR_DATA, "sample %lld: uniforms[%lld] (object %lld, feature %lld) is outside [0, 1) or not finite", (long long)(plan.key >> 40),
                    at, at / (long long)F, at % (long long)F);
    }

    HIPCHK(h, hipMemsetAsync(h->d_words, 0, sizeof(unsigned long long), h->stream));
    if (count_rep) HIPCHK(h, hipMemsetAsync(h->d_counts, 0, c_bytes, h->stream));
    DrawArgs args{};
    h->fill(args, n, plan);
    args.uniforms = uniforms ? h->d_uniforms : nullptr;
    args.y_rep = y_rep ? h->d_y : nullptr;
    args.d = sums ? h->d_d : nullptr;
    args.count_rep = count_rep ? h->d_counts : nullptr;
    args.n_skipped = h->d_words;
    args.seed = seed;
    args.first_draw = first_draw;
    if ((rc = launch_tiles(h, draw_kernel(S, h->C), args, plan.lds))) return rc;
    double* d_feature = h->d_sums;
    double* d_object = h->d_sums + (size_t)n * 2 * (size_t)F;
    if (dev_feature) {
        const int f_blocks = div_up(F, kFeatureLanes);
        rc = unit_for_grid_chunks(2 * n * f_blocks, [&](int64_t first, int64_t count) {
            k_ppc_sum_objects<<<(unsigned)count, kBlock, 0, h->stream>>>(h->d_d, N, (int)F, f_blocks, d_feature, first);
            HIPCHK(h, hipGetLastError());
            return SBE_OK;
        });
        if (rc) return rc;
    }
    if (dev_object) {
        const int64_t rows = 2 * n * N;
        rc = unit_for_grid_chunks((rows + kBlock / 64 - 1) / (kBlock / 64), [&](int64_t first, int64_t count) {
            k_ppc_sum_features<<<(unsigned)count, kBlock, 0, h->stream>>>(h->d_d, rows, (int)F, d_object, first);
            HIPCHK(h, hipGetLastError());
            return SBE_OK;
        });
        if (rc) return rc;
    }
    HIPCHK(h, hipEventRecord(h->ev[1], h->stream));
    if (y_rep) rc = copy_pieces(h, y_rep, h->d_y, (size_t)n * cells, hipMemcpyDeviceToHost);
    if (!rc && dev_feature) rc = copy_pieces(h, dev_feature, d_feature, (size_t)n * 2 * (size_t)F * sizeof(double), hipMemcpyDeviceToHost);
    if (!rc && dev_object) rc = copy_pieces(h, dev_object, d_object, (size_t)n * 2 * (size_t)N * sizeof(double), hipMemcpyDeviceToHost);
    if (!rc && count_rep) rc = copy_pieces(h, count_rep, h->d_counts, c_bytes, hipMemcpyDeviceToHost);
    if (rc) return rc;
    unsigned long long skipped = 0;
    HIPCHK(h, hipMemcpyAsync(&skipped, h->d_words, sizeof skipped, hipMemcpyDeviceToHost, h->stream));
    if ((rc = unit_sync_timed(h))) return rc;
    if (n_skipped_out) *n_skipped_out = (int64_t)skipped;
    return SBE_OK;
}

}  // extern "C"
