// sbe_predict.hip -- the posterior predictive of the logged samples on the device (include/sbe_predict.h): per cell the
// mixture row of every sample, summed over the samples, each component's responsibility for the observed cells and the
// pointwise likelihood rows.  The contract is tests/_predict_oracle.py; DESIGN.md section 21 has the layout, the structure
// of the kernels and the limits.
//
// An accumulate call holds its n samples on the device and runs three kernels:
//   k_predict_ids       a thread per (sample, object): the 0 / 1 cluster rows become one cluster id per object, an object in
//                       two clusters is reported;
//   k_predict_validate  a thread per weight row and per table row: entries, positive entry, sum;
//   k_predict_accumulate<SP, CP>  (only after the host has read that the two above found nothing)
//                       a workgroup owns a tile of Ft features x Nt = 256 / Ft objects, a thread one cell of it with the
//                       cell's S + C float64 accumulators in registers (SP, CP: S and C padded to a power of two, so the
//                       loops over them unroll) for all n samples: pred_sum / resp_sum are read once and written once per
//                       call.  Per sample the workgroup stages the tile's slice of the tables, [R][Ft][S], and of the
//                       weights, [Ft][C], into one of two LDS buffers: the slice of sample t + 1 is written while sample t
//                       is computed from the other buffer, one barrier per sample.  The weight normalisation is computed
//                       per cell from the object's h flags (no table over the 2^C patterns).  Threads along the tile's
//                       features are adjacent, so a sample's lik row is written in runs of Ft floats.
// The first two kernels, the staging of a slice and the row arithmetic of a cell are sbe_predict_row.hip.h's, shared with
// sbe_ppc.hip.  The first offender travels as one uint64 key (sample, kind, position) through an integer atomicMin.  No
// floating-point atomics: a cell belongs to one thread, which adds the samples in order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "sbe_predict_row.hip.h"

namespace {

// ---- the accumulation -------------------------------------------------------------------------------------------------------
struct AccArgs {
    const uint8_t* codes;          // [N][F]
    const uint8_t* groups;         // [C-1][N]
    const uint16_t* kid;           // [n][N]
    const double* weights;         // [n][F][C]
    const double* tables;          // [n][R][F][S]
    double* pred;                  // [N][F][S]
    double* resp;                  // [N][F][C]
    float* lik;                    // [n][N F] or null
    unsigned long long* n_zero;
    int64_t N;
    int F, S, C, R;
    int n;
    int Ft, Nt, f_tiles;
    int64_t block0;                // of this launch
    int row_off[kMaxC];            // first table row of a component's groups (row_off[0] = 0: the clusters)
};

template <int SP, int CP>
__global__ __launch_bounds__(kBlock) void k_predict_accumulate(const AccArgs g) {
    extern __shared__ double lds[];                            // two slices
    const TileCell tc = tile_cell(g);
    const bool live = tc.live;
    const int64_t cell = tc.cell;

    double pred[SP], resp[CP];
    int row[CP];                                               // the object's table row per component (0: not applicable)
    bool has[CP];
    int x = kNA;
#pragma unroll
    for (int s = 0; s < SP; ++s) pred[s] = live && s < g.S ? g.pred[cell * g.S + s] : 0.0;
#pragma unroll
    for (int c = 0; c < CP; ++c) {
        resp[c] = live && c < g.C ? g.resp[cell * g.C + c] : 0.0;
        cell_group(g, tc, c, row[c], has[c]);
    }
    if (live) x = g.codes[cell];
    unsigned long long zeros = 0;

    stage_slice(lds, g, 0, tc.f0, tc.fw);
    __syncthreads();
    for (int t = 0; t < g.n; ++t) {
        const double* cur = lds + (t & 1) * tc.slice;
        if (t + 1 < g.n) stage_slice(lds + ((t + 1) & 1) * tc.slice, g, t + 1, tc.f0, tc.fw);
        if (live) {
            double wn[CP];
            const double* base[CP];
            cell_weights(g, tc, cur, t, row, has, wn, base);
#pragma unroll
            for (int s = 0; s < SP; ++s)
                if (s < g.S) pred[s] += cell_state(g.C, wn, base, s);
            float lik = 1.0f;
            if (x != kNA) {
                double part[CP];
                const double mx = cell_state(g.C, wn, base, x, part);
                if (mx > 0.0) {
#pragma unroll
                    for (int c = 0; c < CP; ++c) resp[c] += part[c] / mx;
                } else {
                    ++zeros;
                }
                lik = (float)mx;
            }
            if (g.lik) g.lik[(int64_t)t * g.N * g.F + cell] = lik;
        }
        __syncthreads();                                       // sample t is read, the slice of t + 1 is written
    }
    if (!live) return;
#pragma unroll
    for (int s = 0; s < SP; ++s)
        if (s < g.S) g.pred[cell * g.S + s] = pred[s];
#pragma unroll
    for (int c = 0; c < CP; ++c)
        if (c < g.C) g.resp[cell * g.C + c] = resp[c];
    if (zeros) atomicAdd(g.n_zero, zeros);
}

using AccKernel = void (*)(const AccArgs);

template <int SP>
AccKernel acc_kernel_c(int C) {
    if (C <= 1) return k_predict_accumulate<SP, 1>;
    if (C <= 2) return k_predict_accumulate<SP, 2>;
    if (C <= 4) return k_predict_accumulate<SP, 4>;
    return k_predict_accumulate<SP, 8>;
}

AccKernel acc_kernel(int S, int C) {
    if (S <= 2) return acc_kernel_c<2>(C);
    if (S <= 4) return acc_kernel_c<4>(C);
    if (S <= 8) return acc_kernel_c<8>(C);
    if (S <= 16) return acc_kernel_c<16>(C);
    return acc_kernel_c<32>(C);
}

}  // namespace

struct sbe_predict : sbe_unit_handle, sample_store {
    int64_t n_samples = 0;
    double* d_acc = nullptr;            // pred_sum [N][F][S], then resp_sum [N][F][C]
    size_t acc_bytes = 0;
    float* d_lik = nullptr;             // [n][N F]
    size_t lik_bytes = 0;
    // d_words: [0]: n_zero, [1]: the first offender's key
    std::vector<void*> buffers() const { return buffers_with({d_acc, d_lik}); }
    double* pred() const { return d_acc; }
    double* resp() const { return d_acc + (size_t)N * F * S; }
    size_t acc_doubles() const { return (size_t)N * F * (S + C); }
};

namespace {

constexpr char kPrefix[] = "sbe_predict";

int64_t sample_bytes(int64_t N, int64_t F, int S, int C, int K, int R, bool lik) {
    return (int64_t)K * N + 8 * F * C + 8 * (int64_t)R * F * S + 2 * N + (lik ? 4 * N * F : 0);
}

int zero_accumulators(sbe_predict* h) {
    HIPCHK(h, hipMemsetAsync(h->d_acc, 0, h->acc_doubles() * sizeof(double), h->stream));
    HIPCHK(h, hipMemsetAsync(h->d_words, 0, sizeof(unsigned long long), h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->n_samples = 0;
    return SBE_OK;
}

}  // namespace

extern "C" {

int sbe_predict_abi_version(void) { return SBE_PREDICT_ABI_VERSION; }

const char* sbe_predict_last_error(const sbe_predict* h) { return unit_last_error(h); }

int sbe_predict_create(sbe_predict** out, int device) { return unit_create_on_device(out, device, "sbe_predict_create"); }

int sbe_predict_destroy(sbe_predict* h) { return unit_destroy(h, kNullHandle); }

int sbe_predict_last_kernel_ms(const sbe_predict* h, float* ms_out) { return unit_last_kernel_ms(h, ms_out, kNullHandle); }

int64_t sbe_predict_sample_bytes(int64_t n_objects, int64_t n_features, int n_states, int n_components, int n_clusters, int n_rows, int with_lik) {
    return shape_ok(n_objects, n_features, n_states, n_components, n_clusters, n_rows)
               ? sample_bytes(n_objects, n_features, n_states, n_components, n_clusters, n_rows, with_lik != 0)
               : 0;
}

int sbe_predict_set_feature_tile(sbe_predict* h, int features) { return set_feature_tile(h, features); }

int sbe_predict_set_data(sbe_predict* h, int64_t N, int64_t F, int S, int C, int K, const uint8_t* codes, const uint8_t* groups, const int* n_groups) {
    CHECK_HANDLE(h, kNullHandle);
    int row_off[kMaxC], R;
    if (const int bad = check_data(h, N, F, S, C, K, codes, groups, n_groups, row_off, R)) return bad;
    return h->upload(h, N, F, S, C, K, R, row_off, codes, groups,
                     [&] { return unit_ensure(h, h->d_acc, h->acc_bytes, (size_t)(N * F * (S + C)) * sizeof(double)); },
                     [&] { return zero_accumulators(h); });               // (waits for the copies too)
}

int sbe_predict_reset(sbe_predict* h) {
    CHECK_HANDLE(h, kNullHandle);
    if (!h->has_data) return no_data(h, kPrefix);
    HIPCHK(h, hipSetDevice(h->device));
    return zero_accumulators(h);
}

int sbe_predict_accumulate(sbe_predict* h, int64_t n, const uint8_t* clusters, const double* weights, const double* tables, float* lik_out) {
    CHECK_HANDLE(h, kNullHandle);
    if (!h->has_data) return no_data(h, kPrefix);
    if (n < 0) return fail(h, SBE_ERR_ARG, "n=%lld is negative", (long long)n);
    if (n == 0) return SBE_OK;
    const int64_t N = h->N, F = h->F;
    SamplePlan plan;
    int rc = h->stage(h, n, clusters, weights, tables, sample_bytes(N, F, h->S, h->C, h->K, h->R, lik_out != nullptr), SBE_PREDICT_MAX_STAGE_BYTES,
                      h->d_words + 1, [&] { return lik_out ? unit_ensure(h, h->d_lik, h->lik_bytes, (size_t)n * N * F * sizeof(float)) : SBE_OK; },
                      no_hook, plan);
    if (rc) return rc;

    AccArgs args{};
    h->fill(args, n, plan);
    args.pred = h->pred();
    args.resp = h->resp();
    args.lik = lik_out ? h->d_lik : nullptr;
    args.n_zero = h->d_words;
    rc = launch_tiles(h, acc_kernel(h->S, h->C), args, plan.lds);
    if (rc) return rc;
    HIPCHK(h, hipEventRecord(h->ev[1], h->stream));
    if (lik_out) rc = copy_pieces(h, lik_out, h->d_lik, (size_t)n * N * F * sizeof(float), hipMemcpyDeviceToHost);
    if (!rc) rc = unit_sync_timed(h);
    if (rc) return rc;
    h->n_samples += n;
    return SBE_OK;
}

int sbe_predict_read(sbe_predict* h, double* pred_sum, double* resp_sum, int64_t* n_samples_out, int64_t* n_zero_out) {
    CHECK_HANDLE(h, kNullHandle);
    if (!h->has_data) return no_data(h, kPrefix);
    if (!n_samples_out || !n_zero_out) return fail(h, SBE_ERR_ARG, "null pointer argument: %s", !n_samples_out ? "n_samples_out" : "n_zero_out");
    HIPCHK(h, hipSetDevice(h->device));
    int rc = SBE_OK;
    if (pred_sum) rc = copy_pieces(h, pred_sum, h->pred(), (size_t)h->N * h->F * h->S * sizeof(double), hipMemcpyDeviceToHost);
    if (!rc && resp_sum) rc = copy_pieces(h, resp_sum, h->resp(), (size_t)h->N * h->F * h->C * sizeof(double), hipMemcpyDeviceToHost);
    if (rc) return rc;
    unsigned long long zeros = 0;
    HIPCHK(h, hipMemcpyAsync(&zeros, h->d_words, sizeof zeros, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    *n_samples_out = h->n_samples;
    *n_zero_out = (int64_t)zeros;
    return SBE_OK;
}

}  // extern "C"
