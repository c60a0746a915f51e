// sbe_contrib.hip -- the per-cluster evidence of the logged samples on the device (include/sbe_contrib.h): per logged sample,
// cluster k and cell that has a code, d = log m_k - log m0, the log-likelihood ratio of the object placed in cluster k against
// the object in no cluster, and its sums per object (affinity) and, over the cluster's members, per feature (gain).  The
// contract is tests/_contrib_oracle.py; DESIGN.md section 24 has the layout, the kernels and the bounds.
//
// An evaluate call holds its n samples on the device and runs
//   k_predict_ids, k_predict_validate   sbe_predict_row.hip.h's, as the posterior predictive runs them;
//   k_contrib_cell<CP>                  (only after the host has read that the kernels above found nothing)
//                       k_predict_accumulate's plan: a workgroup owns a tile of Ft features x Nt = 256 / Ft objects, a thread
//                       one cell of it, the sample's slice of the tables and weights is double-buffered in LDS with one barrier
//                       per sample, and the row arithmetic is sbe_predict_row.hip.h's.  Only the observed state's entry of a
//                       row is needed.  Per sample a thread forms the two sets of weights and the confounders' products once,
//                       m0 and its log once, and in a run-time loop over k the chain of additions of m_k and its log; it
//                       writes the K d values of its cell;
//   k_contrib_sum_features, k_contrib_sum_members   the d values of a (sample, k, object) over the features and of a (sample, k,
//                       feature) over the cluster's members, in the trees the header fixes: no floating-point atomics, and no
//                       bit depends on the tile, the split of the samples or the call.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "sbe_predict_row.hip.h"
#include "../../include/sbe_contrib.h"

namespace {

constexpr int kFeatureLanes = 16;        // k_contrib_sum_members: lanes per feature, and features per workgroup
static_assert(kFeatureLanes * kFeatureLanes == kBlock, "a workgroup of k_contrib_sum_members is 16 features x 16 lanes");

// ---- the cells ----------------------------------------------------------------------------------------------------------------
struct CellArgs {
    const uint8_t* codes;          // [N][F]
    const uint8_t* groups;         // [C-1][N]
    const double* weights;         // [n][F][C]
    const double* tables;          // [n][R][F][S]
    double* d;                     // [n][K][N][F]: d of every (cluster, cell), or null
    unsigned long long* n_skipped;
    int64_t N;
    int F, S, C, R, K;
    int n;
    int Ft, Nt, f_tiles;
    int64_t block0;                // of this launch
    int row_off[kMaxC];            // first table row of a component's groups (row_off[0] = 0: the clusters)
};

template <int CP>
__global__ __launch_bounds__(kBlock) void k_contrib_cell(const CellArgs g) {
    extern __shared__ double lds[];                            // two slices
    const TileCell tc = tile_cell(g);
    const bool live = tc.live;
    const int64_t cell = tc.cell;
    const int64_t cells = g.N * g.F;

    int row[CP];                                               // the object's table row per confounder (row[0] = 0)
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
            double* out = g.d ? g.d + (int64_t)t * g.K * cells + cell : nullptr;   // d[t][k][n][f] = out[k cells]
            bool formed = false;
            double w1[CP], w0[CP], part[CP];
            const double* base[CP];
            double log_m0 = 0.0;
            if (x != kNA) {
                formed = cell_weights_in_and_out(g, tc, cur, row, has, w1, w0, base);
                if (formed) {
                    log_m0 = log(cell_state(g.C, w0, base, x));    // -inf where m0 = 0
#pragma unroll
                    for (int c = 1; c < CP; ++c) part[c] = c < g.C ? w1[c] * base[c][x] : 0.0;
                } else {
                    skipped += (unsigned long long)g.K;
                }
            }
            const double* theta = cur + tc.fl * g.S;               // table[0][f][.] of the slice; a cluster further: Ft S
            for (int k = 0; k < g.K; ++k, theta += g.Ft * g.S) {
                double d = 0.0;                                    // what a cell without a code, or a skipped entry, adds
                if (formed) {
                    const double m = cell_state_in(g.C, w1[0], theta, x, part);
                    if (m > 0.0)
                        d = log(m) - log_m0;
                    else
                        ++skipped;
                }
                if (out) out[(int64_t)k * cells] = d;
            }
        }
        __syncthreads();                                       // sample t is read, the slice of t + 1 is written
    }
    if (skipped) atomicAdd(g.n_skipped, skipped);
}

using CellKernel = void (*)(const CellArgs);

CellKernel cell_kernel(int C) {
    if (C <= 1) return k_contrib_cell<1>;
    if (C <= 2) return k_contrib_cell<2>;
    if (C <= 4) return k_contrib_cell<4>;
    return k_contrib_cell<8>;
}

// ---- the sums -------------------------------------------------------------------------------------------------------------------
// gain_feature[q][f], q = t K + k: a workgroup takes 16 features of one q; lane j of a feature's 16 adds the objects j,
// j + 16, .. in order onto 0, a non-member of k adding +0.0; then the lanes' sums are added in order 0 .. 15.
// blockIdx.x + block0 = q * f_blocks + feature block.
__global__ __launch_bounds__(kBlock) void k_contrib_sum_members(const double* d, const uint16_t* kid, int64_t N, int F, int K, int f_blocks,
                                                                double* gain_feature, int64_t block0) {
    __shared__ double part[kFeatureLanes][kFeatureLanes];
    const int64_t b = block0 + blockIdx.x;
    const int64_t q = b / f_blocks;
    const int f = (int)(b - q * f_blocks) * kFeatureLanes + (threadIdx.x % kFeatureLanes);
    const int lane = threadIdx.x / kFeatureLanes;
    double sum = 0.0;
    if (f < F) {
        const int64_t t = q / K;
        const uint16_t k = (uint16_t)(q - t * K);
        const double* col = d + q * N * F + f;
        const uint16_t* ids = kid + t * N;
        for (int64_t obj = lane; obj < N; obj += kFeatureLanes) sum += ids[obj] == k ? col[obj * F] : 0.0;
    }
    part[lane][threadIdx.x % kFeatureLanes] = sum;
    __syncthreads();
    if (lane == 0 && f < F) {
        double total = part[0][threadIdx.x];
        for (int j = 1; j < kFeatureLanes; ++j) total += part[j][threadIdx.x];
        gain_feature[q * F + f] = total;
    }
}

// affinity[row], row = (t K + k) N + object: a wave takes one row of d; lane j adds the features j, j + 64, .. in order onto 0;
// then the fixed tree of the unit layer over the lanes
__global__ __launch_bounds__(kBlock) void k_contrib_sum_features(const double* d, int64_t rows, int F, double* affinity, int64_t block0) {
    const int64_t row = (block0 + blockIdx.x) * (kBlock / 64) + (threadIdx.x >> 6);
    if (row >= rows) return;                                   // (a whole wave)
    const double* v = d + row * F;
    double sum = 0.0;
    for (int f = threadIdx.x & 63; f < F; f += 64) sum += v[f];
    sum = unit_wave_reduce(sum, unit_sum());
    if ((threadIdx.x & 63) == 0) affinity[row] = sum;
}

}  // namespace

struct sbe_contrib : sbe_unit_handle, sample_store {
    // d_words: [0]: n_skipped of the call, [1]: the first offender's key
    double* d_d = nullptr;              // [n][K][N][F]
    size_t d_bytes = 0;
    double* d_sums = nullptr;           // gain_feature [n][K][F], then affinity [n][K][N]
    size_t sums_bytes = 0;
    std::vector<void*> buffers() const { return buffers_with({d_d, d_sums}); }
};

namespace {

constexpr char kPrefix[] = "sbe_contrib";

int64_t sample_bytes(int64_t N, int64_t F, int S, int C, int K, int R) {
    return (int64_t)K * N + 8 * F * C + 8 * (int64_t)R * F * S + 2 * N + 8 * (int64_t)K * N * F + 8 * (int64_t)K * (N + F);
}

}  // namespace

extern "C" {

int sbe_contrib_abi_version(void) { return SBE_CONTRIB_ABI_VERSION; }

const char* sbe_contrib_last_error(const sbe_contrib* h) { return unit_last_error(h); }

int sbe_contrib_create(sbe_contrib** out, int device) { return unit_create_on_device(out, device, "sbe_contrib_create"); }

int sbe_contrib_destroy(sbe_contrib* h) { return unit_destroy(h, kNullHandle); }

int sbe_contrib_last_kernel_ms(const sbe_contrib* h, float* ms_out) { return unit_last_kernel_ms(h, ms_out, kNullHandle); }

int64_t sbe_contrib_sample_bytes(int64_t n_objects, int64_t n_features, int n_states, int n_components, int n_clusters, int n_rows) {
    return shape_ok(n_objects, n_features, n_states, n_components, n_clusters, n_rows)
               ? sample_bytes(n_objects, n_features, n_states, n_components, n_clusters, n_rows)
               : 0;
}

int sbe_contrib_set_feature_tile(sbe_contrib* h, int features) { return set_feature_tile(h, features); }

int sbe_contrib_set_data(sbe_contrib* h, int64_t N, int64_t F, int S, int C, int K, const uint8_t* codes, const uint8_t* groups, const int* n_groups) {
    CHECK_HANDLE(h, kNullHandle);
    int row_off[kMaxC], R;
    if (const int bad = check_data(h, N, F, S, C, K, codes, groups, n_groups, row_off, R)) return bad;
    return h->upload(h, N, F, S, C, K, R, row_off, codes, groups, no_hook, [&] { return wait_for_stream(h); });
}

int sbe_contrib_evaluate(sbe_contrib* h, int64_t n, const uint8_t* clusters, const double* weights, const double* tables, double* affinity,
                         double* gain_feature, int64_t* n_skipped_out) {
    CHECK_HANDLE(h, kNullHandle);
    if (!h->has_data) return no_data(h, kPrefix);
    if (n < 0) return fail(h, SBE_ERR_ARG, "n=%lld is negative", (long long)n);
    if (n == 0) {
        if (n_skipped_out) *n_skipped_out = 0;
        return SBE_OK;
    }
    const int64_t N = h->N, F = h->F, cells = N * F;
    const int K = h->K;
    const bool sums = affinity || gain_feature;
    const size_t gain_count = (size_t)n * K * (size_t)F, aff_count = (size_t)n * K * (size_t)N;
    SamplePlan plan;
    int rc = h->stage(h, n, clusters, weights, tables, sample_bytes(N, F, h->S, h->C, K, h->R), SBE_CONTRIB_MAX_STAGE_BYTES, h->d_words + 1, [&] {
        if (!sums) return SBE_OK;
        const int own = unit_ensure(h, h->d_d, h->d_bytes, (size_t)n * K * (size_t)cells * sizeof(double));
        return own ? own : unit_ensure(h, h->d_sums, h->sums_bytes, (gain_count + aff_count) * sizeof(double));
    }, no_hook, plan);
    if (rc) return rc;

    HIPCHK(h, hipMemsetAsync(h->d_words, 0, sizeof(unsigned long long), h->stream));
    CellArgs args{};
    h->fill(args, n, plan);
    args.d = sums ? h->d_d : nullptr;
    args.n_skipped = h->d_words;
    args.K = K;
    if ((rc = launch_tiles(h, cell_kernel(h->C), args, plan.lds))) return rc;
    double* d_gain = h->d_sums;
    double* d_affinity = h->d_sums + gain_count;
    if (gain_feature) {
        const int f_blocks = div_up(F, kFeatureLanes);
        rc = unit_for_grid_chunks(n * K * f_blocks, [&](int64_t first, int64_t count) {
            k_contrib_sum_members<<<(unsigned)count, kBlock, 0, h->stream>>>(h->d_d, h->d_kid, N, (int)F, K, f_blocks, d_gain, first);
            HIPCHK(h, hipGetLastError());
            return SBE_OK;
        });
        if (rc) return rc;
    }
    if (affinity) {
        const int64_t rows = n * K * N;
        rc = unit_for_grid_chunks((rows + kBlock / 64 - 1) / (kBlock / 64), [&](int64_t first, int64_t count) {
            k_contrib_sum_features<<<(unsigned)count, kBlock, 0, h->stream>>>(h->d_d, rows, (int)F, d_affinity, first);
            HIPCHK(h, hipGetLastError());
            return SBE_OK;
        });
        if (rc) return rc;
    }
    HIPCHK(h, hipEventRecord(h->ev[1], h->stream));
    if (gain_feature) rc = copy_pieces(h, gain_feature, d_gain, gain_count * sizeof(double), hipMemcpyDeviceToHost);
    if (!rc && affinity) rc = copy_pieces(h, affinity, d_affinity, aff_count * sizeof(double), hipMemcpyDeviceToHost);
    if (rc) return rc;
    unsigned long long skipped = 0;
    HIPCHK(h, hipMemcpyAsync(&skipped, h->d_words, sizeof skipped, hipMemcpyDeviceToHost, h->stream));
    if ((rc = unit_sync_timed(h))) return rc;
    if (n_skipped_out) *n_skipped_out = (int64_t)skipped;
    return SBE_OK;
}

}  // extern "C"
