// sbe_elpd.hip -- on-device model comparison over logged observation likelihoods (include/sbe_elpd.h): the likelihood
// store, its fill kernels, and one workgroup per kept column computing PSIS-LOO (arviz.loo for one chain) and the
// per-observation WAIC terms.  The numerical contract is tests/_elpd_oracle.py; DESIGN.md section 11 has the layout,
// the selection and the limits.
//
// The column's steps (min and check, sums, radix-select cutoff, tail sort, _gpdfit, _gpinv, the tail's and the body's sums) are
// sbe_psis_column.hip.h's, shared with sbe_loopred.hip.  Every sum is a fixed tree over fixed per-thread partial sums: results
// do not depend on the store's capacity or on how the store was filled, so the host path and the engine path give the same bits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "sbe_psis_column.hip.h"
#include "sbe_unit.hip.h"
#include "sbe_engine_internal.hip.h"   // sbe_elpd_append_engine reads the engine's row on the device
#include "../../include/sbe_elpd.h"

namespace {

using ElpdKey = psis_key_plain;                      // equal likelihoods are interchangeable here: the bit pattern alone is sorted

struct ElpdArgs {
    const float* lh;          // store: [M][cap]
    const int32_t* cols;      // [n_kept] column indices
    int64_t cap, burn;
    int s, tail_n, tail_p;    // S, T, pow2 >= T
    int staged;
    double* out;              // [4][n_kept]: loo_i, k_i, lppd_i, v_i
    int64_t n_kept;
    int64_t j0;               // first kept column of this launch (launches are chunked: kMaxGridBlocks)
    int* bad;                 // device word: count of columns holding a value that is not positive and finite
};

__global__ __launch_bounds__(kPsisBlock) void k_elpd_column(ElpdArgs a) {
    extern __shared__ __align__(16) unsigned char dyn[];
    __shared__ PsisScratch sc;
    const int64_t j = a.j0 + blockIdx.x;
    const uint32_t* g = reinterpret_cast<const uint32_t*>(a.lh + (int64_t)a.cols[j] * a.cap + a.burn);
    const PsisColumn c = psis_column<ElpdKey>(g, a.s, a.tail_n, a.tail_p, a.staged != 0, dyn, sc, psis_no_sink{});
    if (threadIdx.x != 0) return;
    if (c.bad) {
        atomicAdd(a.bad, 1);
        for (int q = 0; q < 4; ++q) a.out[q * a.n_kept + j] = NAN;
        return;
    }
    a.out[j] = c.loo;
    a.out[a.n_kept + j] = c.k_hat;
    a.out[2 * a.n_kept + j] = c.lppd;
    a.out[3 * a.n_kept + j] = c.var;
}

// NA rule of elpd.py:31 without a mask: keep[m] = 0 where every stored row is isclose(lh, 1); one wave per column
__global__ __launch_bounds__(256) void k_elpd_isclose(const float* lh, int64_t cap, int64_t n_rows, int64_t M, uint8_t* keep,
                                                      int64_t col0) {
    const int64_t col = col0 + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (col >= M) return;
    const float* c = lh + col * cap;
    int far = 0;
    for (int64_t i = threadIdx.x & 63; i < n_rows; i += 64) far |= !(fabs((double)c[i] - 1.0) <= 1e-8 + 1e-5 * 1.0);
    far = unit_wave_reduce(far, unit_or{});
    if ((threadIdx.x & 63) == 0) keep[col] = (uint8_t)far;
}

// store columns -> host row order [n][M] (rows read back): the reverse of k_unit_transpose
__global__ __launch_bounds__(256) void k_elpd_untranspose(const float* lh, int64_t cap, int64_t r0, int64_t n, int64_t M, float* rows,
                                                          int64_t mt0) {
    __shared__ float tile[32][33];
    const int64_t m0 = (mt0 + blockIdx.x) * 32, n0 = (int64_t)blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int c = ty; c < 32; c += 8) {
        const int64_t col = m0 + c, row = n0 + tx;
        if (row < n && col < M) tile[tx][c] = lh[col * cap + r0 + row];
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int64_t row = n0 + r, col = m0 + tx;
        if (row < n && col < M) rows[row * M + col] = tile[r][tx];
    }
}

// the LikelihoodLogger row of an engine slot (float64 [N*F] in the engine's scratch) into row r of the store
__global__ __launch_bounds__(256) void k_elpd_store_row(const double* row, int64_t M, float* lh, int64_t cap, int64_t r) {
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m < M) lh[m * cap + r] = (float)row[m];
}

}  // namespace

struct sbe_elpd_store : sbe_unit_handle {     // (sbe_unit.hip.h; ev: around the column kernel of the last compute call)
    int64_t M = 0, cap = 0, n = 0;
    float* d_lh = nullptr;              // [M][cap]
    void* d_stage = nullptr;            // host rows in flight / rows read back: one piece (unit_piece_rows)
    size_t stage_bytes = 0;
    int32_t* d_cols = nullptr;          // [M]
    uint8_t* d_keep = nullptr;          // [M]
    double* d_out = nullptr;            // [4][M]
    int* d_bad = nullptr;
    std::vector<void*> buffers() const { return {d_lh, d_stage, d_cols, d_keep, d_out, d_bad}; }
};

namespace {

constexpr sbe_elpd_store* kNone = nullptr;           // (fail without a handle: the type names the unit)
constexpr char kNullHandle[] = "null store handle";

}  // namespace

extern "C" {

int sbe_elpd_abi_version(void) { return SBE_ELPD_ABI_VERSION; }

const char* sbe_elpd_last_error(const sbe_elpd_store* st) { return unit_last_error(st); }

int64_t sbe_elpd_lds_max_samples(void) {
    static const int64_t v = psis_lds_max_samples<ElpdKey>();
    return v;
}

int sbe_elpd_create(sbe_elpd_store** out, int device, int64_t n_columns, int64_t capacity) {
    if (!out) return fail(kNone, SBE_ERR_ARG, "null pointer argument: out");
    *out = nullptr;
    if (n_columns < 1 || n_columns > INT32_MAX)
        return fail(kNone, SBE_ERR_ARG, "n_columns=%lld out of range [1, %d]", (long long)n_columns, INT32_MAX);
    if (capacity < 1) return fail(kNone, SBE_ERR_ARG, "capacity=%lld must be positive", (long long)capacity);
    if (device < 0) return fail(kNone, SBE_ERR_ARG, "device %d out of range", device);
    char shape[96];
    snprintf(shape, sizeof shape, " (%lld x %lld float32 store)", (long long)n_columns, (long long)capacity);
    sbe_elpd_store* st = nullptr;
    const int rc = unit_open(st, device, "sbe_elpd_create", shape);
    if (rc) return rc;
    st->M = n_columns;
    st->cap = capacity;
    auto bail = [&](hipError_t err, const char* what) { return unit_create_failed(st, "sbe_elpd_create", what, err, shape); };
    hipError_t err;
    if ((err = hipMalloc((void**)&st->d_lh, (size_t)n_columns * capacity * sizeof(float))) != hipSuccess) return bail(err, "hipMalloc");
    if ((err = hipMalloc((void**)&st->d_cols, (size_t)n_columns * sizeof(int32_t))) != hipSuccess) return bail(err, "hipMalloc");
    if ((err = hipMalloc((void**)&st->d_keep, (size_t)n_columns)) != hipSuccess) return bail(err, "hipMalloc");
    if ((err = hipMalloc((void**)&st->d_out, (size_t)n_columns * 4 * sizeof(double))) != hipSuccess) return bail(err, "hipMalloc");
    if ((err = hipMalloc((void**)&st->d_bad, sizeof(int))) != hipSuccess) return bail(err, "hipMalloc");
    *out = st;
    return SBE_OK;
}

int sbe_elpd_destroy(sbe_elpd_store* st) { return unit_destroy(st, kNullHandle); }

int sbe_elpd_n_rows(const sbe_elpd_store* st, int64_t* n_rows_out) {
    CHECK_HANDLE(st, kNullHandle);
    if (!n_rows_out) return fail(st, SBE_ERR_ARG, "null pointer argument: n_rows_out");
    *n_rows_out = st->n;
    return SBE_OK;
}

int sbe_elpd_last_kernel_ms(const sbe_elpd_store* st, float* ms_out) { return unit_last_kernel_ms(st, ms_out, kNullHandle); }

int sbe_elpd_reset(sbe_elpd_store* st) {
    CHECK_HANDLE(st, kNullHandle);
    st->n = 0;
    return SBE_OK;
}

int sbe_elpd_append_rows(sbe_elpd_store* st, const float* rows, int64_t n_rows) {
    CHECK_HANDLE(st, kNullHandle);
    if (n_rows < 0) return fail(st, SBE_ERR_ARG, "n_rows=%lld is negative", (long long)n_rows);
    if (n_rows > 0 && !rows) return fail(st, SBE_ERR_ARG, "null pointer argument: rows");
    if (st->n + n_rows > st->cap)
        return fail(st, SBE_ERR_ARG, "store overflow: %lld rows + %lld exceed the capacity of %lld rows", (long long)st->n,
                     (long long)n_rows, (long long)st->cap);
    if (n_rows == 0) return SBE_OK;
    HIPCHK(st, hipSetDevice(st->device));
    const int64_t M = st->M;
    const int rc = unit_append_pieces(st, st->d_stage, st->stage_bytes, rows, n_rows, (int64_t)sizeof(float) * M, st->cap, [&](int64_t k, int64_t r) {
        return unit_for_grid_chunks((M + 31) / 32, [&](int64_t t0, int64_t tiles) {
            k_unit_transpose<<<dim3((unsigned)tiles, (unsigned)((k + 31) / 32)), 256, 0, st->stream>>>((const float*)st->d_stage, k, M, st->d_lh,
                                                                                                      st->cap, st->n + r, t0);
            HIPCHK(st, hipGetLastError());
            return SBE_OK;
        });
    });
    if (rc) return rc;
    st->n += n_rows;
    return SBE_OK;
}

int sbe_elpd_append_engine(sbe_elpd_store* st, sbe_engine* e, int slot) {
    CHECK_HANDLE(st, kNullHandle);
    if (!e) return fail(st, SBE_ERR_ARG, "null engine handle");
    if (slot < 0 || slot >= e->n_slots) return fail(st, SBE_ERR_ARG, "slot %d out of range [0,%d)", slot, e->n_slots);
    if (e->device != st->device)
        return fail(st, SBE_ERR_ARG, "the store lives on device %d, the engine on device %d", st->device, e->device);
    if ((int64_t)e->N * e->F != st->M)
        return fail(st, SBE_ERR_ARG, "the store has %lld columns, the engine's rows have N*F = %lld", (long long)st->M,
                     (long long)e->N * e->F);
    if (st->n + 1 > st->cap) return fail(st, SBE_ERR_ARG, "store overflow: capacity of %lld rows reached", (long long)st->cap);
    int rc = enqueue_lh_exact(e, slot, "sbe_elpd_append_engine");
    if (rc == SBE_OK) {
        k_elpd_store_row<<<div_up(st->M, 256), 256, 0, e->stream>>>((const double*)e->d_scratch, st->M, st->d_lh, st->cap, st->n);
        const hipError_t err = hipGetLastError();
        if (err != hipSuccess) rc = fail(e, SBE_ERR_HIP, "k_elpd_store_row launch: %s", hipGetErrorString(err));
    }
    if (rc == SBE_OK) rc = lh_exact_report(e);            // the engine's stream wait and its status word: nothing else is read back
    if (rc) return fail(st, rc, "%s", e->last_error.c_str());
    ++st->n;
    return SBE_OK;
}

int sbe_elpd_get_rows(sbe_elpd_store* st, int64_t row0, int64_t n_rows, float* out) {
    CHECK_HANDLE(st, kNullHandle);
    if (row0 < 0 || n_rows < 0 || row0 + n_rows > st->n)
        return fail(st, SBE_ERR_ARG, "rows [%lld, %lld) out of range [0, %lld)", (long long)row0, (long long)(row0 + n_rows),
                     (long long)st->n);
    if (n_rows > 0 && !out) return fail(st, SBE_ERR_ARG, "null pointer argument: out");
    if (n_rows == 0) return SBE_OK;
    HIPCHK(st, hipSetDevice(st->device));
    const int64_t M = st->M, piece = unit_piece_rows((int64_t)sizeof(float) * M, st->cap);
    int rc = unit_ensure(st, st->d_stage, st->stage_bytes, (size_t)piece * M * sizeof(float));
    for (int64_t r = 0; !rc && r < n_rows; r += piece) {
        const int64_t k = std::min(piece, n_rows - r);
        rc = unit_for_grid_chunks((M + 31) / 32, [&](int64_t t0, int64_t tiles) {
            k_elpd_untranspose<<<dim3((unsigned)tiles, (unsigned)((k + 31) / 32)), 256, 0, st->stream>>>(st->d_lh, st->cap, row0 + r, k, M,
                                                                                                        (float*)st->d_stage, t0);
            HIPCHK(st, hipGetLastError());
            return SBE_OK;
        });
        if (rc) break;
        HIPCHK(st, hipMemcpyAsync(out + r * M, st->d_stage, (size_t)k * M * sizeof(float), hipMemcpyDeviceToHost, st->stream));
        HIPCHK(st, hipStreamSynchronize(st->stream));
    }
    return rc;
}

int sbe_elpd_compute(sbe_elpd_store* st, int64_t burn_rows, const uint8_t* na_values, int na_isclose,
                     double* loo_i, double* k_i, double* lppd_i, double* v_i, int64_t* n_kept_out) {
    CHECK_HANDLE(st, kNullHandle);
    if (!loo_i || !k_i || !lppd_i || !v_i || !n_kept_out) return fail(st, SBE_ERR_ARG, "null pointer argument: output");
    if (burn_rows < 0 || burn_rows >= st->n)
        return fail(st, SBE_ERR_ARG, "burn_rows=%lld out of range [0, %lld) (rows stored: %lld)", (long long)burn_rows,
                     (long long)st->n, (long long)st->n);
    const int64_t s = st->n - burn_rows;
    if (s < SBE_ELPD_MIN_SAMPLES || s > SBE_ELPD_MAX_SAMPLES)
        return fail(st, SBE_ERR_ARG, "%lld samples after burn-in; PSIS needs %d .. %d (2^20) per observation", (long long)s,
                     SBE_ELPD_MIN_SAMPLES, SBE_ELPD_MAX_SAMPLES);
    *n_kept_out = 0;
    HIPCHK(st, hipSetDevice(st->device));
    std::vector<uint8_t> keep((size_t)st->M, 1);
    if (na_values) {
        for (int64_t m = 0; m < st->M; ++m) keep[m] = na_values[m] == 0;
    } else if (na_isclose) {
        const int rc = unit_for_grid_chunks(div_up(st->M, 4), [&](int64_t b0, int64_t blocks) {
            k_elpd_isclose<<<(unsigned)blocks, 256, 0, st->stream>>>(st->d_lh, st->cap, st->n, st->M, st->d_keep, b0 * 4);
            HIPCHK(st, hipGetLastError());
            return SBE_OK;
        });
        if (rc) return rc;
        HIPCHK(st, hipMemcpyAsync(keep.data(), st->d_keep, (size_t)st->M, hipMemcpyDeviceToHost, st->stream));
        HIPCHK(st, hipStreamSynchronize(st->stream));
    }
    std::vector<int32_t> cols;
    cols.reserve((size_t)st->M);
    for (int64_t m = 0; m < st->M; ++m)
        if (keep[m]) cols.push_back((int32_t)m);
    const int64_t nk = (int64_t)cols.size();
    if (nk == 0) return SBE_OK;
    const bool staged = psis_column_staged<ElpdKey>(s);
    const int tn = psis_tail_count(s), tp = pow2_at_least(std::max(tn, 1));
    const size_t lds = (staged ? (size_t)s * sizeof(uint32_t) : 0) + psis_tail_lds_bytes<ElpdKey>(s);
    HIPCHK(st, hipFuncSetAttribute((const void*)k_elpd_column, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kLdsBudget - kPsisStaticLds)));
    HIPCHK(st, hipMemcpyAsync(st->d_cols, cols.data(), (size_t)nk * sizeof(int32_t), hipMemcpyHostToDevice, st->stream));
    HIPCHK(st, hipMemsetAsync(st->d_bad, 0, sizeof(int), st->stream));
    int rc = unit_timed(st, [&] {
        return unit_for_grid_chunks(nk, [&](int64_t j0, int64_t columns) {   // one workgroup per kept column
            const ElpdArgs args{st->d_lh, st->d_cols, st->cap, burn_rows, (int)s, tn, tp, staged ? 1 : 0, st->d_out, nk, j0, st->d_bad};
            k_elpd_column<<<(unsigned)columns, kPsisBlock, lds, st->stream>>>(args);
            HIPCHK(st, hipGetLastError());
            return SBE_OK;
        });
    });
    int bad = 0;
    if (!rc) rc = unit_copy_back(st, (const int*)st->d_bad, 1, {&bad});
    if (!rc) rc = unit_copy_back(st, (const double*)st->d_out, (size_t)nk, {loo_i, k_i, lppd_i, v_i});
    if (!rc) rc = unit_sync_timed(st);
    if (rc) return rc;
    if (bad) return fail(st, SBE_ERR_DATA, "%d observation column%s hold likelihood values that are not positive and finite "
                          "in rows [%lld, %lld)", bad, bad == 1 ? "" : "s", (long long)burn_rows, (long long)st->n);
    *n_kept_out = nk;
    return SBE_OK;
}

}  // extern "C"
