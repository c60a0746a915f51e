// sbe_elpd.hip -- on-device model comparison over logged observation likelihoods (include/sbe_elpd.h): the likelihood
// store, its fill kernels, and one workgroup per kept column computing PSIS-LOO (arviz.loo for one chain) and the
// per-observation WAIC terms.  The numerical contract is tests/_elpd_oracle.py; DESIGN.md section 11 has the layout,
// the selection and the limits.
//
// Per column (S samples of float32 lh > 0, ll = log(double(lh))):
//   1. min of the bit patterns (positive floats order as uint32) and the data check; column staged in LDS when
//      it fits the budget, else every pass below reads global memory (same code, same order of operations);
//   2. sum of ll (mean, for the variance) and sum of lh (= sum exp(ll): lppd_i);
//   3. _psislw's cutoff: x = -ll - max(-ll) orders as the reverse of lh, so the element at ascending x position S-T-1
//      is the (T+1)-th smallest lh -- found exactly by an 8-bit radix select over the bit patterns (LDS histograms);
//   4. the tail (lh strictly below the cutoff: at most T elements) compacted into LDS and bitonic-sorted;
//   5. _gpdfit in fp64 (the m_est candidates spread over the waves), _gpinv smoothing, the tail's sums;
//   6. variance of ll (second pass about the mean) and the body's sums, then loo_i.
// Every sum is a fixed tree over fixed per-thread partial sums: results do not depend on the store's capacity or on
// how the store was filled, so the host path and the engine path give the same bits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "sbe_unit.hip.h"
#include "sbe_engine_internal.hip.h"   // sbe_elpd_append_engine reads the engine's row on the device
#include "../../include/sbe_elpd.h"

namespace {

constexpr int kElpdBlock = 256;                      // 4 waves per column
constexpr int kElpdWaves = kElpdBlock / 64;
constexpr int kMaxM = 96;                            // _gpdfit candidates: 30 + sqrt(T) <= 85 for S <= 2^20 (T <= 3072)
constexpr size_t kStaticLds = 8192;                  // headroom for the kernel's static LDS (histogram, reductions, fit)

inline int tail_count(int64_t s) { return (int)std::ceil(std::min(0.2 * (double)s, 3.0 * std::sqrt((double)s))); }
// dynamic LDS of a column of S samples: [tail exceedances Tp x f64][tail keys Tp x u32][staged column S x u32]
inline size_t tail_lds_bytes(int64_t s) { return (size_t)pow2_at_least(std::max(tail_count(s), 1)) * (sizeof(uint32_t) + sizeof(double)); }
inline size_t staged_lds_bytes(int64_t s) { return (size_t)s * sizeof(uint32_t) + tail_lds_bytes(s); }
inline bool column_staged(int64_t s) { return staged_lds_bytes(s) + kStaticLds <= kLdsBudget; }

int64_t lds_max_samples() {
    int64_t s = 2;
    while (column_staged(s + 1)) ++s;
    return s;
}

__device__ inline double ll_of(uint32_t bits) { return log((double)__uint_as_float(bits)); }

// rank-th smallest (0-based) of the S keys: MSB-first 8-bit radix select with an LDS histogram per digit
__device__ uint32_t radix_select(const uint32_t* v, int s, int rank, uint32_t* hist, uint32_t* wave_tot, uint32_t* found) {
    uint32_t prefix = 0, mask = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        hist[threadIdx.x] = 0;
        __syncthreads();
        for (int i = threadIdx.x; i < s; i += kElpdBlock) {
            const uint32_t u = v[i];
            if ((u & mask) == prefix) atomicAdd(&hist[(u >> shift) & 0xFF], 1u);
        }
        __syncthreads();
        // exclusive prefix sum over the 256 bins: one bin per thread, a wave scan, then the wave totals
        const uint32_t own = hist[threadIdx.x];
        uint32_t inc = own;
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t up = (uint32_t)__shfl_up((int)inc, o, 64);
            if (lane >= o) inc += up;
        }
        if (lane == 63) wave_tot[wave] = inc;
        __syncthreads();
        uint32_t base = 0;
        for (int w = 0; w < wave; ++w) base += wave_tot[w];
        const uint32_t lo = base + inc - own, hi = base + inc;
        if ((uint32_t)rank >= lo && (uint32_t)rank < hi) { found[0] = (uint32_t)threadIdx.x; found[1] = lo; }
        __syncthreads();
        prefix |= found[0] << shift;
        mask |= 0xFFu << shift;
        rank -= (int)found[1];
        __syncthreads();
    }
    return prefix;
}

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

__global__ __launch_bounds__(kElpdBlock) void k_elpd_column(ElpdArgs a) {
    extern __shared__ __align__(16) unsigned char dyn[];
    __shared__ uint32_t hist[256];
    __shared__ uint32_t ured[kElpdWaves], found[2], n_cand;
    __shared__ double red[kElpdWaves];
    __shared__ double fit_b[kMaxM], fit_k[kMaxM], fit_ls[kMaxM], fit_w[kMaxM];
    __shared__ double fit_post[1];                  // b_post
    const int64_t j = a.j0 + blockIdx.x;
    const int s = a.s, tid = threadIdx.x;
    const uint32_t* g = reinterpret_cast<const uint32_t*>(a.lh + (int64_t)a.cols[j] * a.cap + a.burn);
    double* ary = reinterpret_cast<double*>(dyn);                            // [tail_p] tail exceedances
    uint32_t* keys = reinterpret_cast<uint32_t*>(ary + a.tail_p);            // [tail_p] candidate bit patterns
    uint32_t* staged = keys + a.tail_p;                                      // [S] when staged

    // 1. stage, min, data check
    uint32_t umin = 0xFFFFFFFFu, bad = 0;
    for (int i = tid; i < s; i += kElpdBlock) {
        const uint32_t u = g[i];
        if (a.staged) staged[i] = u;
        bad |= (u == 0u || u >= 0x7F800000u);        // zero, negative (sign bit), inf, NaN
        umin = min(umin, u);
    }
    umin = unit_block_reduce<kElpdWaves>(umin, ured, unit_min{});
    bad = unit_block_reduce<kElpdWaves>(bad, ured, unit_max{});
    const uint32_t* v = a.staged ? staged : g;
    if (bad) {                                       // (uniform over the block)
        if (tid == 0) {
            atomicAdd(a.bad, 1);
            for (int q = 0; q < 4; ++q) a.out[q * a.n_kept + j] = NAN;
        }
        return;
    }
    const double ll_min = ll_of(umin);               // max(-ll) = -ll_min

    // 2. sum ll, sum lh
    double sum_ll = 0.0, sum_lh = 0.0;
    for (int i = tid; i < s; i += kElpdBlock) {
        const uint32_t u = v[i];
        sum_ll += ll_of(u);
        sum_lh += (double)__uint_as_float(u);
    }
    sum_ll = unit_block_reduce<kElpdWaves>(sum_ll, red, unit_sum{});
    sum_lh = unit_block_reduce<kElpdWaves>(sum_lh, red, unit_sum{});
    const double mean = sum_ll / s;
    const double lppd = log(sum_lh) - log((double)s);        // logsumexp(ll) - log S: float32 lh neither over- nor underflows

    // 3. cutoff: the (T+1)-th smallest lh
    const uint32_t ucut = radix_select(v, s, a.tail_n, hist, ured, found);
    const double x_cut = -ll_of(ucut) + ll_min;              // x = -ll - max(-ll)
    const double xcutoff = fmax(x_cut, log(2.2250738585072014e-308));   // (never binds for float32 data: x >= -192)
    const double expxcutoff = exp(xcutoff);

    // 4. candidates (lh < cutoff: at most T of them), sorted by lh ascending = x descending; pads sort last
    if (tid == 0) n_cand = 0;
    for (int i = tid; i < a.tail_p; i += kElpdBlock) keys[i] = 0xFFFFFFFFu;
    __syncthreads();
    for (int i = tid; i < s; i += kElpdBlock) {
        const uint32_t u = v[i];
        if (u < ucut) keys[atomicAdd(&n_cand, 1u)] = u;
    }
    __syncthreads();
    const int nc = (int)n_cand;
    for (int k = 2; k <= a.tail_p; k <<= 1) {
        for (int jj = k >> 1; jj > 0; jj >>= 1) {
            for (int i = tid; i < a.tail_p; i += kElpdBlock) {
                const int p = i ^ jj;
                if (p > i) {
                    const uint32_t ki = keys[i], kp = keys[p];
                    const bool up = (i & k) == 0;
                    if ((ki > kp) == up) { keys[i] = kp; keys[p] = ki; }
                }
            }
            __syncthreads();
        }
    }
    // x-ascending position t of candidate keys[nc - 1 - t]; the tail is the x > xcutoff suffix (all candidates here)
    double in_tail = 0.0;
    for (int t = tid; t < nc; t += kElpdBlock) in_tail += (-ll_of(keys[nc - 1 - t]) + ll_min) > xcutoff;
    const int tail_len = (int)unit_block_reduce<kElpdWaves>(in_tail, red, unit_sum{});
    const int t0 = nc - tail_len;                            // x-ascending index of the first tail element

    // 5. _gpdfit on the exceedances exp(x) - exp(cutoff), ascending
    double k_hat = INFINITY, sigma = 0.0;
    const int n = tail_len;
    if (n > 4) {
        for (int i = tid; i < n; i += kElpdBlock) {
            const double x = -ll_of(keys[nc - 1 - (t0 + i)]) + ll_min;
            ary[i] = exp(x) - expxcutoff;
        }
        __syncthreads();
        const int m = 30 + (int)sqrt((double)n);
        const double q = 3 * ary[(int)(n / 4.0 + 0.5) - 1], inv_last = 1 / ary[n - 1];
        const int lane = tid & 63, wave = tid >> 6;
        for (int c = wave; c < m; c += kElpdWaves) {          // k_ary[c] = mean(log1p(-b[c] * ary)): one wave per candidate
            double b = 1 - sqrt(m / ((double)(c + 1) - 0.5));
            b /= q;
            b += inv_last;
            double acc = 0.0;
            for (int i = lane; i < n; i += 64) acc += log1p(-b * ary[i]);
            acc = unit_wave_reduce(acc, unit_sum{});
            if (lane == 0) { fit_b[c] = b; fit_k[c] = acc / n; }
        }
        __syncthreads();
        if (tid < m) fit_ls[tid] = n * (log(-(fit_b[tid] / fit_k[tid])) - fit_k[tid] - 1);
        __syncthreads();
        if (tid < m) {
            double z = 0.0;
            for (int c = 0; c < m; ++c) z += exp(fit_ls[c] - fit_ls[tid]);
            fit_w[tid] = 1 / z;
        }
        __syncthreads();
        if (tid == 0) {                                       // prune negligible weights (NaN included), normalise, posterior b
            double wsum = 0.0;
            for (int c = 0; c < m; ++c) if (fit_w[c] >= 10 * 2.220446049250313e-16) wsum += fit_w[c];
            double b_post = 0.0;
            for (int c = 0; c < m; ++c) if (fit_w[c] >= 10 * 2.220446049250313e-16) b_post += fit_b[c] * (fit_w[c] / wsum);
            fit_post[0] = b_post;
        }
        __syncthreads();
        const double b_post = fit_post[0];
        double acc = 0.0;
        for (int i = tid; i < n; i += kElpdBlock) acc += log1p(-b_post * ary[i]);
        const double k_post = unit_block_reduce<kElpdWaves>(acc, red, unit_sum{}) / n;
        sigma = -k_post / b_post;
        k_hat = (n * k_post + 10 * 0.5) / (n + 10);
    }

    // the tail's terms of logsumexp(x') and logsumexp(x' + ll): smoothed (_gpinv, clamped to 0) when k is finite
    const bool smooth = n > 4 && isfinite(k_hat);
    double a_tail = 0.0, b_tail = 0.0;
    for (int i = tid; i < n; i += kElpdBlock) {
        const double ll = ll_of(keys[nc - 1 - (t0 + i)]);
        double x = -ll + ll_min;
        if (smooth) {
            const double p = (0.5 + i) / n;
            double gq = NAN;                                   // _gpinv: NaN when sigma <= 0, not repaired
            if (!(sigma <= 0)) {
                gq = fabs(k_hat) < 2.220446049250313e-16 ? -log1p(-p) : expm1(-k_hat * log1p(-p)) / k_hat;
                gq *= sigma;
            }
            x = log(gq + expxcutoff);
            if (x > 0) x = 0;
        }
        a_tail += exp(x);
        b_tail += exp(x + ll);
    }

    // 6. variance about the mean; the body's terms (lh >= cutoff, and candidates at or below xcutoff)
    double var = 0.0, a_body = 0.0, b_body = 0.0;
    for (int i = tid; i < s; i += kElpdBlock) {
        const uint32_t u = v[i];
        const double ll = ll_of(u);
        var += (ll - mean) * (ll - mean);
        if (u >= ucut) {
            const double x = -ll + ll_min;
            a_body += exp(x);
            b_body += exp(x + ll);
        }
    }
    for (int t = tid; t < t0; t += kElpdBlock) {
        const double ll = ll_of(keys[nc - 1 - t]);
        const double x = -ll + ll_min;
        a_body += exp(x);
        b_body += exp(x + ll);
    }
    var = unit_block_reduce<kElpdWaves>(var, red, unit_sum{}) / s;
    const double a_all = unit_block_reduce<kElpdWaves>(a_body + a_tail, red, unit_sum{});
    const double b_all = unit_block_reduce<kElpdWaves>(b_body + b_tail, red, unit_sum{});
    if (tid == 0) {
        a.out[j] = log(b_all) - log(a_all);                   // logsumexp(x' - logsumexp(x') + ll)
        a.out[a.n_kept + j] = k_hat;
        a.out[2 * a.n_kept + j] = lppd;
        a.out[3 * a.n_kept + j] = var;
    }
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
    static const int64_t v = lds_max_samples();
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
    const bool staged = column_staged(s);
    const int tn = tail_count(s), tp = pow2_at_least(std::max(tn, 1));
    const size_t lds = (staged ? (size_t)s * sizeof(uint32_t) : 0) + tail_lds_bytes(s);
    HIPCHK(st, hipFuncSetAttribute((const void*)k_elpd_column, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kLdsBudget - kStaticLds)));
    HIPCHK(st, hipMemcpyAsync(st->d_cols, cols.data(), (size_t)nk * sizeof(int32_t), hipMemcpyHostToDevice, st->stream));
    HIPCHK(st, hipMemsetAsync(st->d_bad, 0, sizeof(int), st->stream));
    int rc = unit_timed(st, [&] {
        return unit_for_grid_chunks(nk, [&](int64_t j0, int64_t columns) {   // one workgroup per kept column
            const ElpdArgs args{st->d_lh, st->d_cols, st->cap, burn_rows, (int)s, tn, tp, staged ? 1 : 0, st->d_out, nk, j0, st->d_bad};
            k_elpd_column<<<(unsigned)columns, kElpdBlock, lds, st->stream>>>(args);
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
