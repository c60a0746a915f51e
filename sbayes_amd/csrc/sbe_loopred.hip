// sbe_loopred.hip -- the leave-one-out predictive of every observed cell on the device (include/sbe_loopred.h): the likelihood
// rows of the logged samples kept column-major, PSIS per column with the smoothed weight of every sample kept, and the samples
// run past the weights a second time.  The contract is tests/_loopred_oracle.py; DESIGN.md section 26 has the layout, the
// choice of the weights' road to the threads and what it measured.
//
// The three phases and their kernels:
//   add         k_predict_ids, k_predict_validate (sbe_predict_row.hip.h), then k_loopred_rows<CP>: a thread per cell of a
//               tile writes lik = float32(m[x]) of every sample of the call into sample-major staging [n][N F] (runs of Ft
//               floats), and k_loopred_to_store gathers the observed cells' columns of it into the store [M][cap] through a
//               32 x 32 LDS tile;
//   weights     k_loopred_weights: a workgroup per column runs psis_column (sbe_psis_column.hip.h) with the sample index in
//               the tail's sort key and a sink that stores exp(x'_t) at w[column][t]; the workgroup then divides its column
//               by A and sums the squares;
//   accumulate  ids and validation again, then k_loopred_accumulate<SP, CP>: sbe_predict.hip's tile and slices, a thread per
//               cell with the cell's S float64 sums in registers for all n samples, one extra operand per (cell, sample): the
//               thread reads the weight and the stored row from its own column of the store, consecutive samples from
//               consecutive addresses (what else was tried).  The sums are read from one buffer and
//               written to the other; the host swaps the two only when no sample's row differed from the stored one, so a
//               refused call leaves them as they were.
// No floating-point atomics: a cell belongs to one thread, which adds the samples in order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

#include "sbe_predict_row.hip.h"
#include "sbe_psis_column.hip.h"
#include "../../include/sbe_loopred.h"

namespace {

using LooKey = psis_key_sample;                      // the tail's positions name their samples (the oracle's stable argsort)

// ---- phase 1: the likelihood rows ---------------------------------------------------------------------------------------------
struct RowArgs {                                     // (the fields sbe_predict_row.hip.h reads, then the unit's own)
    const uint8_t* codes;
    const uint8_t* groups;
    const uint16_t* kid;
    const double* weights;
    const double* tables;
    int64_t N;
    int F, S, C, R;
    int n;
    int Ft, Nt, f_tiles;
    int64_t block0;
    int row_off[kMaxC];
    float* lik;                                      // phase 1: staging [n][N F], written
    const double* p_in;                              // phase 3: the sums [N][F][S], read ..
    double* p_out;                                   // .. and written
    const float* lik_ref;                            // the store's rows [M][cap] ..
    const double* w;                                 // .. and weights [M][cap]
    const int32_t* col_of_cell;                      // [N F] (-1: NA)
    int64_t cap, t_first;                            // the call's first sample
    unsigned long long* err;                         // the first sample whose row differs (atomicMin)
};

template <int CP>
__global__ __launch_bounds__(kBlock) void k_loopred_rows(const RowArgs g) {
    extern __shared__ double lds[];                            // two slices
    const TileCell tc = tile_cell(g);
    int row[CP];
    bool has[CP];
#pragma unroll
    for (int c = 0; c < CP; ++c) cell_group(g, tc, c, row[c], has[c]);
    const int x = tc.live ? g.codes[tc.cell] : kNA;
    const bool observed = x != kNA;

    stage_slice(lds, g, 0, tc.f0, tc.fw);
    __syncthreads();
    for (int t = 0; t < g.n; ++t) {
        const double* cur = lds + (t & 1) * tc.slice;
        if (t + 1 < g.n) stage_slice(lds + ((t + 1) & 1) * tc.slice, g, t + 1, tc.f0, tc.fw);
        if (observed) {
            double wn[CP];
            const double* base[CP];
            cell_weights(g, tc, cur, t, row, has, wn, base);
            g.lik[(int64_t)t * g.N * g.F + tc.cell] = (float)cell_state(g.C, wn, base, x);
        }
        __syncthreads();                                       // sample t is read, the slice of t + 1 is written
    }
}

// staging rows [n][W] (W = N F cells) -> store columns [M][cap] at row offset r0; column j takes the cell cells[j];
// 32 x 32 tiles through LDS; blockIdx.x + ct0: column tile, blockIdx.y: row tile
template <class T>
__global__ __launch_bounds__(256) void k_loopred_to_store(const T* rows, int64_t n, int64_t W, const int32_t* cells, int64_t M, T* store, int64_t cap,
                                                          int64_t r0, int64_t ct0) {
    __shared__ T tile[32][33];
    const int64_t c0 = (ct0 + blockIdx.x) * 32, n0 = (int64_t)blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;     // 32 x 8
    const int64_t mine = c0 + tx < M ? cells[c0 + tx] : 0;
    for (int r = ty; r < 32; r += 8) {
        const int64_t row = n0 + r;
        if (row < n && c0 + tx < M) tile[r][tx] = rows[row * W + mine];
    }
    __syncthreads();
    for (int c = ty; c < 32; c += 8) {
        const int64_t col = c0 + c, row = n0 + tx;
        if (row < n && col < M) store[col * cap + r0 + row] = tile[tx][c];
    }
}

// ---- phase 2: PSIS per column, the weights kept ---------------------------------------------------------------------------------
struct WeightArgs {
    const float* lh;          // store: [M][cap]
    double* w;                // [M][cap]
    int64_t cap;
    int s, tail_n, tail_p;    // T, its tail count, pow2 at or above that
    int staged;
    double* out;              // [3][M]: loo_i, k_i, n_eff
    int64_t M;
    int64_t j0;               // first column of this launch
    unsigned long long* err;  // the first (column, sample) that is not positive and finite: column << 20 | sample (atomicMin)
};

struct WeightSink {
    double* w;                // the column's weights
    __device__ void operator()(int sample, double e) const { w[sample] = e; }
};

__global__ __launch_bounds__(kPsisBlock) void k_loopred_weights(WeightArgs a) {
    extern __shared__ __align__(16) unsigned char dyn[];
    __shared__ PsisScratch sc;
    const int64_t j = a.j0 + blockIdx.x;
    const int tid = threadIdx.x;
    const uint32_t* g = reinterpret_cast<const uint32_t*>(a.lh + j * a.cap);
    double* w = a.w + j * a.cap;
    const PsisColumn c = psis_column<LooKey>(g, a.s, a.tail_n, a.tail_p, a.staged != 0, dyn, sc, WeightSink{w});
    if (c.bad) {                                     // (uniform over the block)
        uint32_t first = 0xFFFFFFFFu;
        for (int i = tid; i < a.s; i += kPsisBlock) {
            const uint32_t u = g[i];
            if (u == 0u || u >= 0x7F800000u) first = min(first, (uint32_t)i);
        }
        first = unit_block_reduce<kPsisWaves>(first, sc.ured, unit_min{});
        if (tid == 0) {
            atomicMin(a.err, ((unsigned long long)j << 20) | first);
            for (int q = 0; q < 3; ++q) a.out[q * a.M + j] = NAN;
        }
        return;
    }
    // every exp(x'_t) of the column is in w (the sink's stores are ordered before this by the barriers of the block's last
    // reductions); divide by A and sum the squares: per-thread partial sums in sample order, then the fixed tree
    double sq = 0.0;
    for (int i = tid; i < a.s; i += kPsisBlock) {
        const double v = w[i] / c.a_all;
        w[i] = v;
        sq += v * v;
    }
    sq = unit_block_reduce<kPsisWaves>(sq, sc.red, unit_sum{});
    if (tid == 0) {
        a.out[j] = c.loo;
        a.out[a.M + j] = c.k_hat;
        a.out[2 * a.M + j] = 1 / sq;
    }
}

// ---- phase 3: the samples past the weights ------------------------------------------------------------------------------------------
template <int SP, int CP>
__global__ __launch_bounds__(kBlock) void k_loopred_accumulate(const RowArgs g) {
    extern __shared__ double lds[];                            // two slices
    const TileCell tc = tile_cell(g);
    double p[SP];
    int row[CP];
    bool has[CP];
#pragma unroll
    for (int c = 0; c < CP; ++c) cell_group(g, tc, c, row[c], has[c]);
    const int x = tc.live ? g.codes[tc.cell] : kNA;
    const bool observed = x != kNA;
#pragma unroll
    for (int s = 0; s < SP; ++s) p[s] = observed && s < g.S ? g.p_in[tc.cell * g.S + s] : 0.0;
    const int64_t at = observed ? (int64_t)g.col_of_cell[tc.cell] * g.cap + g.t_first : 0;   // of the call's first sample in the cell's column
    int differs = INT_MAX;                                     // the first sample of the call whose row differs from the stored one

    stage_slice(lds, g, 0, tc.f0, tc.fw);
    __syncthreads();
    for (int t = 0; t < g.n; ++t) {
        const double* cur = lds + (t & 1) * tc.slice;
        if (t + 1 < g.n) stage_slice(lds + ((t + 1) & 1) * tc.slice, g, t + 1, tc.f0, tc.fw);
        if (observed) {
            const double wt = g.w[at + t];
            const float ref = g.lik_ref[at + t];
            double wn[CP];
            const double* base[CP];
            cell_weights(g, tc, cur, t, row, has, wn, base);
#pragma unroll
            for (int s = 0; s < SP; ++s)
                if (s < g.S) p[s] += wt * cell_state(g.C, wn, base, s);
            const float lik = (float)cell_state(g.C, wn, base, x);
            if (__float_as_uint(lik) != __float_as_uint(ref)) differs = min(differs, t);
        }
        __syncthreads();                                       // sample t is read, the slice of t + 1 is written
    }
    if (!observed) return;
#pragma unroll
    for (int s = 0; s < SP; ++s)
        if (s < g.S) g.p_out[tc.cell * g.S + s] = p[s];
    if (differs != INT_MAX) atomicMin(g.err, (unsigned long long)(g.t_first + differs));
}

using RowKernel = void (*)(const RowArgs);

RowKernel rows_kernel(int C) {
    if (C <= 1) return k_loopred_rows<1>;
    if (C <= 2) return k_loopred_rows<2>;
    if (C <= 4) return k_loopred_rows<4>;
    return k_loopred_rows<8>;
}

template <int SP>
RowKernel acc_kernel_c(int C) {
    if (C <= 1) return k_loopred_accumulate<SP, 1>;
    if (C <= 2) return k_loopred_accumulate<SP, 2>;
    if (C <= 4) return k_loopred_accumulate<SP, 4>;
    return k_loopred_accumulate<SP, 8>;
}

RowKernel acc_kernel(int S, int C) {
    if (S <= 2) return acc_kernel_c<2>(C);
    if (S <= 4) return acc_kernel_c<4>(C);
    if (S <= 8) return acc_kernel_c<8>(C);
    if (S <= 16) return acc_kernel_c<16>(C);
    return acc_kernel_c<32>(C);
}

}  // namespace

struct sbe_loopred : sbe_unit_handle, sample_store {
    bool weighted = false;
    int64_t M = 0, cap = 0;
    int64_t n_rows = 0;                 // T so far
    int64_t next_t = 0;                 // phase 3: the samples accumulated
    int cur = 0;                        // which of the two sums buffers holds the sums
    int32_t* d_cells = nullptr;         // [M]: the cell of a column
    size_t cells_bytes = 0;
    int32_t* d_col = nullptr;           // [N F]: the column of a cell, -1: NA
    size_t col_bytes = 0;
    double* d_p = nullptr;              // two buffers of [N][F][S]
    size_t p_bytes = 0;
    float* d_lh = nullptr;              // the rows [M][cap]
    size_t lh_bytes = 0;
    double* d_w = nullptr;              // the weights [M][cap]
    size_t w_bytes = 0;
    double* d_out = nullptr;            // [3][M]
    size_t out_bytes = 0;
    float* d_lik = nullptr;             // staging [n][N F]
    size_t lik_bytes = 0;
    // d_words: [0]: the first offender's key, [1]: phase 2's and phase 3's first offender
    std::vector<void*> buffers() const { return buffers_with({d_cells, d_col, d_p, d_lh, d_w, d_out, d_lik}); }
    size_t p_doubles() const { return (size_t)N * F * S; }
    double* sums(int which) const { return d_p + (size_t)which * p_doubles(); }
};

namespace {

constexpr char kPrefix[] = "sbe_loopred";

int64_t sample_bytes(int64_t N, int64_t F, int S, int C, int K, int R) {
    return (int64_t)K * N + 8 * F * C + 8 * (int64_t)R * F * S + 2 * N + 4 * N * F;
}

int64_t store_bytes(int64_t M, int64_t cap) { return M * cap * (int64_t)(sizeof(float) + sizeof(double)); }

int forget_rows(sbe_loopred* h) {
    HIPCHK(h, hipMemsetAsync(h->d_p, 0, 2 * h->p_doubles() * sizeof(double), h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->n_rows = h->next_t = 0;
    h->cur = 0;
    h->weighted = false;
    return SBE_OK;
}

// The part add and accumulate share: the store's opening of a call over n samples with the staging rows of the likelihood; on
// SBE_OK args holds what sbe_predict_row.hip.h reads.
int stage_samples(sbe_loopred* h, int64_t n, const uint8_t* clusters, const double* weights, const double* tables, RowArgs& args, size_t& lds) {
    SamplePlan plan;
    const int rc = h->stage(h, n, clusters, weights, tables, sample_bytes(h->N, h->F, h->S, h->C, h->K, h->R), SBE_LOOPRED_MAX_STAGE_BYTES, h->d_words,
                            [&] { return unit_ensure(h, h->d_lik, h->lik_bytes, (size_t)n * h->N * h->F * sizeof(float)); }, no_hook, plan);
    if (rc) return rc;
    args = RowArgs{};
    h->fill(args, n, plan);
    lds = plan.lds;
    return SBE_OK;
}

}  // namespace

extern "C" {

int sbe_loopred_abi_version(void) { return SBE_LOOPRED_ABI_VERSION; }

const char* sbe_loopred_last_error(const sbe_loopred* h) { return unit_last_error(h); }

int sbe_loopred_create(sbe_loopred** out, int device) { return unit_create_on_device(out, device, "sbe_loopred_create"); }

int sbe_loopred_destroy(sbe_loopred* h) { return unit_destroy(h, kNullHandle); }

int sbe_loopred_last_kernel_ms(const sbe_loopred* h, float* ms_out) { return unit_last_kernel_ms(h, ms_out, kNullHandle); }

int64_t sbe_loopred_store_bytes(int64_t n_observed, int64_t capacity) {
    return n_observed < 0 || capacity < 0 || capacity > SBE_LOOPRED_MAX_SAMPLES ? -1 : store_bytes(n_observed, capacity);
}

int64_t sbe_loopred_sample_bytes(int64_t n_objects, int64_t n_features, int n_states, int n_components, int n_clusters, int n_rows) {
    return shape_ok(n_objects, n_features, n_states, n_components, n_clusters, n_rows)
               ? sample_bytes(n_objects, n_features, n_states, n_components, n_clusters, n_rows)
               : 0;
}

int64_t sbe_loopred_lds_max_samples(void) {
    static const int64_t v = psis_lds_max_samples<LooKey>();
    return v;
}

int sbe_loopred_set_feature_tile(sbe_loopred* h, int features) { return set_feature_tile(h, features); }

int sbe_loopred_set_data(sbe_loopred* h, int64_t N, int64_t F, int S, int C, int K, const uint8_t* codes, const uint8_t* groups, const int* n_groups,
                         int64_t capacity) {
    CHECK_HANDLE(h, kNullHandle);
    int row_off[kMaxC], R;
    if (const int bad = check_data(h, N, F, S, C, K, codes, groups, n_groups, row_off, R)) return bad;
    if (capacity < 1 || capacity > SBE_LOOPRED_MAX_SAMPLES)
        return fail(h, SBE_ERR_ARG, "capacity=%lld out of range [1, %d] (2^20 samples)", (long long)capacity, SBE_LOOPRED_MAX_SAMPLES);
    std::vector<int32_t> cells, col((size_t)(N * F), -1);      // (N F (S + C) 8 <= 2^32: a cell's index fits an int32)
    for (int64_t q = 0; q < N * F; ++q)
        if (codes[q] != kNA) {
            col[(size_t)q] = (int32_t)cells.size();
            cells.push_back((int32_t)q);
        }
    const int64_t M = (int64_t)cells.size();
    if (store_bytes(M, capacity) > SBE_LOOPRED_MAX_STORE_BYTES)
        return fail(h, SBE_ERR_ARG, "the rows and weights of %lld observed cells x %lld samples take %lld bytes on the device, the limit is %lld",
                    (long long)M, (long long)capacity, (long long)store_bytes(M, capacity), (long long)SBE_LOOPRED_MAX_STORE_BYTES);
    const size_t store = std::max<size_t>(1, (size_t)M * (size_t)capacity);
    return h->upload(
        h, N, F, S, C, K, R, row_off, codes, groups,
        [&] {
            int rc = unit_ensure(h, h->d_cells, h->cells_bytes, std::max<size_t>(1, (size_t)M) * sizeof(int32_t));
            if (!rc) rc = unit_ensure(h, h->d_col, h->col_bytes, (size_t)(N * F) * sizeof(int32_t));
            if (!rc) rc = unit_ensure(h, h->d_p, h->p_bytes, 2 * (size_t)(N * F * S) * sizeof(double));
            if (!rc) rc = unit_ensure(h, h->d_lh, h->lh_bytes, store * sizeof(float));
            if (!rc) rc = unit_ensure(h, h->d_w, h->w_bytes, store * sizeof(double));
            if (!rc) rc = unit_ensure(h, h->d_out, h->out_bytes, 3 * std::max<size_t>(1, (size_t)M) * sizeof(double));
            if (!rc && M > 0) rc = copy_pieces(h, h->d_cells, cells.data(), (size_t)M * sizeof(int32_t), hipMemcpyHostToDevice);
            if (!rc) rc = copy_pieces(h, h->d_col, col.data(), (size_t)(N * F) * sizeof(int32_t), hipMemcpyHostToDevice);
            return rc;
        },
        [&] {
            h->M = M;
            h->cap = capacity;
            return forget_rows(h);                            // (waits for the copies too: `cells` and `col` live until here)
        });
}

int sbe_loopred_reset(sbe_loopred* h) {
    CHECK_HANDLE(h, kNullHandle);
    if (!h->has_data) return no_data(h, kPrefix);
    HIPCHK(h, hipSetDevice(h->device));
    return forget_rows(h);
}

int sbe_loopred_add(sbe_loopred* h, int64_t n, const uint8_t* clusters, const double* weights, const double* tables) {
    CHECK_HANDLE(h, kNullHandle);
    if (!h->has_data) return no_data(h, kPrefix);
    if (n < 0) return fail(h, SBE_ERR_ARG, "n=%lld is negative", (long long)n);
    if (n == 0) return SBE_OK;
    if (h->n_rows + n > h->cap)
        return fail(h, SBE_ERR_ARG, "store overflow: %lld samples + %lld exceed the capacity of %lld samples", (long long)h->n_rows, (long long)n,
                    (long long)h->cap);
    RowArgs args;
    size_t lds;
    int rc = stage_samples(h, n, clusters, weights, tables, args, lds);
    if (rc) return rc;
    args.lik = h->d_lik;
    if ((rc = launch_tiles(h, rows_kernel(h->C), args, lds))) return rc;
    const int64_t M = h->M, W = h->N * h->F;
    rc = unit_for_grid_chunks((M + 31) / 32, [&](int64_t ct0, int64_t tiles) {
        k_loopred_to_store<<<dim3((unsigned)tiles, (unsigned)((n + 31) / 32)), 256, 0, h->stream>>>((const float*)h->d_lik, n, W, h->d_cells, M, h->d_lh, h->cap,
                                                                                                   h->n_rows, ct0);
        HIPCHK(h, hipGetLastError());
        return SBE_OK;
    });
    if (rc) return rc;
    HIPCHK(h, hipEventRecord(h->ev[1], h->stream));
    if ((rc = unit_sync_timed(h))) return rc;
    h->n_rows += n;
    h->weighted = false;
    return SBE_OK;
}

int sbe_loopred_weights(sbe_loopred* h, double* loo_i, double* k_i, double* n_eff) {
    CHECK_HANDLE(h, kNullHandle);
    if (!h->has_data) return no_data(h, kPrefix);
    if (!loo_i || !k_i || !n_eff) return fail(h, SBE_ERR_ARG, "null pointer argument: %s", !loo_i ? "loo_i" : !k_i ? "k_i" : "n_eff");
    const int64_t s = h->n_rows, M = h->M;
    if (s < SBE_ELPD_MIN_SAMPLES)
        return fail(h, SBE_ERR_STATE, "%lld samples stored; PSIS needs at least %d per observation", (long long)s, SBE_ELPD_MIN_SAMPLES);
    HIPCHK(h, hipSetDevice(h->device));
    h->weighted = false;
    const bool staged = psis_column_staged<LooKey>(s);
    const int tn = psis_tail_count(s), tp = pow2_at_least(std::max(tn, 1));
    const size_t lds = (staged ? (size_t)s * sizeof(uint32_t) : 0) + psis_tail_lds_bytes<LooKey>(s);
    unsigned long long* d_err = h->d_words + 1;
    HIPCHK(h, hipFuncSetAttribute((const void*)k_loopred_weights, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kLdsBudget - kPsisStaticLds)));
    HIPCHK(h, hipMemsetAsync(d_err, 0xFF, sizeof(unsigned long long), h->stream));
    HIPCHK(h, hipMemsetAsync(h->d_p, 0, 2 * h->p_doubles() * sizeof(double), h->stream));
    h->next_t = 0;
    int rc = unit_timed(h, [&] {
        return unit_for_grid_chunks(M, [&](int64_t j0, int64_t columns) {   // one workgroup per column
            const WeightArgs args{h->d_lh, h->d_w, h->cap, (int)s, tn, tp, staged ? 1 : 0, h->d_out, M, j0, d_err};
            k_loopred_weights<<<(unsigned)columns, kPsisBlock, lds, h->stream>>>(args);
            HIPCHK(h, hipGetLastError());
            return SBE_OK;
        });
    });
    unsigned long long key = kNoError;
    if (!rc) rc = unit_copy_back(h, (const unsigned long long*)d_err, 1, {&key});
    if (!rc && M > 0) rc = unit_copy_back(h, (const double*)h->d_out, (size_t)M, {loo_i, k_i, n_eff});
    if (!rc) rc = unit_sync_timed(h);
    if (rc) return rc;
    if (key != kNoError) {
        std::vector<int32_t> cell(1);
        const int64_t j = (int64_t)(key >> 20);
        HIPCHK(h, hipMemcpy(cell.data(), h->d_cells + j, sizeof(int32_t), hipMemcpyDeviceToHost));
        return fail(h, SBE_ERR_DATA, "cell (object %lld, feature %lld), sample %lld: the likelihood of the observed state is zero or not finite; "
                    "its importance weight would be infinite", (long long)(cell[0] / h->F), (long long)(cell[0] % h->F), (long long)(key & ((1ull << 20) - 1)));
    }
    h->weighted = true;
    return SBE_OK;
}

int sbe_loopred_accumulate(sbe_loopred* h, int64_t t0, int64_t n, const uint8_t* clusters, const double* weights, const double* tables) {
    CHECK_HANDLE(h, kNullHandle);
    if (!h->has_data) return no_data(h, kPrefix);
    if (!h->weighted) return fail(h, SBE_ERR_STATE, "no weights yet (sbe_loopred_weights comes before sbe_loopred_accumulate)");
    if (n < 0) return fail(h, SBE_ERR_ARG, "n=%lld is negative", (long long)n);
    if (t0 != h->next_t || t0 + n > h->n_rows)
        return fail(h, SBE_ERR_STATE, "samples [%lld, %lld): the calls cover [0, %lld) in order without gaps, the next sample is %lld", (long long)t0,
                    (long long)(t0 + n), (long long)h->n_rows, (long long)h->next_t);
    if (n == 0) return SBE_OK;
    RowArgs args;
    size_t lds;
    int rc = stage_samples(h, n, clusters, weights, tables, args, lds);
    if (rc) return rc;
    unsigned long long* d_err = h->d_words + 1;
    HIPCHK(h, hipMemsetAsync(d_err, 0xFF, sizeof(unsigned long long), h->stream));
    args.p_in = h->sums(h->cur);
    args.p_out = h->sums(1 - h->cur);
    args.lik_ref = h->d_lh;
    args.w = h->d_w;
    args.col_of_cell = h->d_col;
    args.cap = h->cap;
    args.t_first = t0;
    args.err = d_err;
    if ((rc = launch_tiles(h, acc_kernel(h->S, h->C), args, lds))) return rc;
    HIPCHK(h, hipEventRecord(h->ev[1], h->stream));
    unsigned long long first = kNoError;
    if ((rc = unit_copy_back(h, (const unsigned long long*)d_err, 1, {&first}))) return rc;
    if ((rc = unit_sync_timed(h))) return rc;
    if (first != kNoError)
        return fail(h, SBE_ERR_DATA, "sample %lld: its likelihood row differs from the one sbe_loopred_add stored; the second pass takes the same samples "
                    "in the same order", (long long)first);
    h->cur = 1 - h->cur;
    h->next_t += n;
    return SBE_OK;
}

int sbe_loopred_read(sbe_loopred* h, double* p_loo, int64_t* n_samples_out) {
    CHECK_HANDLE(h, kNullHandle);
    if (!h->has_data) return no_data(h, kPrefix);
    if (!n_samples_out) return fail(h, SBE_ERR_ARG, "null pointer argument: n_samples_out");
    HIPCHK(h, hipSetDevice(h->device));
    if (p_loo) {
        if (const int rc = copy_pieces(h, p_loo, h->sums(h->cur), h->p_doubles() * sizeof(double), hipMemcpyDeviceToHost)) return rc;
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    *n_samples_out = h->next_t;
    return SBE_OK;
}

int sbe_loopred_get_store(sbe_loopred* h, float* lik, double* w) {
    CHECK_HANDLE(h, kNullHandle);
    if (!h->has_data) return no_data(h, kPrefix);
    if (w && !h->weighted) return fail(h, SBE_ERR_STATE, "no weights yet (sbe_loopred_weights comes first)");
    if (h->M == 0 || h->n_rows == 0) return SBE_OK;
    HIPCHK(h, hipSetDevice(h->device));
    const size_t T = (size_t)h->n_rows;
    if (lik)
        HIPCHK(h, hipMemcpy2DAsync(lik, T * sizeof(float), h->d_lh, (size_t)h->cap * sizeof(float), T * sizeof(float), (size_t)h->M, hipMemcpyDeviceToHost,
                                   h->stream));
    if (w)
        HIPCHK(h, hipMemcpy2DAsync(w, T * sizeof(double), h->d_w, (size_t)h->cap * sizeof(double), T * sizeof(double), (size_t)h->M, hipMemcpyDeviceToHost,
                                   h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return SBE_OK;
}

}  // extern "C"
