#pragma once
// sbe_diag_column.hip.h -- what the two units that diagnose columns share (sbe_diag.hip, sbe_summary.hip): the float64
// column-major store of M chains with its reset and append, the plan of a compute call (burn-in, cut, split: the chains'
// offsets), the column kernel k_diag_column with its constants and its launch loop.  The kernel was moved here from
// sbe_diag.hip unchanged; the numerical contract is tests/_diag_oracle.py and DESIGN.md section 16.  Everything lives in
// an unnamed namespace: each unit compiles its own copy.
//
// Per column (M chains of n draws after burn-in, cut and split):
//   1. finite check and min / max; the chain means, one wave per chain, in two steps (the sum, then the sum of the
//      residuals added back); the column staged in LDS, centred per chain, when it fits (else every pass below reads
//      the store and subtracts the chain mean: the same values, the same order of operations);
//   2. the pooled mean and sd;
//   3. autocovariances for a block of kLagBlock consecutive lags at a time: each wave takes kLagsPerLane lags, a lane
//      keeps them in registers and strides over i, so one read of d[i] feeds kLagsPerLane multiply-adds; the wave
//      reduces with a fixed exchange tree.  One thread then walks the positive-sequence rule over the block and
//      publishes stop or continue;
//   4. the monotone pass and the sums, in one thread, in the order of the contract.
// Every lag's value is a pure function of the column: it does not depend on the lag's place in its block, on the
// column's place in the launch or on how the store was filled.  No float atomics; no workgroup waits for another.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "sbe_unit.hip.h"
#include "../../include/sbe_diag.h"

namespace {

constexpr int kDiagBlock = 256;                      // 4 waves per column
constexpr int kDiagWaves = kDiagBlock / 64;
constexpr int kLagsPerLane = 8;                      // lags a lane keeps in registers
constexpr int kLagBlock = kDiagWaves * kLagsPerLane; // lags evaluated between two walks of the positive-sequence rule
constexpr int kMaxSplitChains = 2 * SBE_DIAG_MAX_CHAINS;
constexpr int kRhoLds = 2048;                        // rho_t entries kept in LDS; later ones go to the column's scratch
constexpr size_t kStaticLds = 4096;                  // headroom for the kernel's static LDS (chain means, lag block, reductions)
// launch rule: multiply-adds of a launch whose columns all run to the n - 3 bound (M * n * n / 2 each) stay below this,
// but a launch holds at least one column per CU
constexpr double kLaunchWork = 4398046511104.0;      // 2^42
constexpr int64_t kMinLaunchColumns = 256;
constexpr size_t kScratchBytes = (size_t)256 << 20;  // rho_t scratch of one launch (columns with n > kRhoLds)

constexpr int64_t kLdsMaxDraws = (int64_t)((kLdsBudget - kStaticLds - (size_t)kRhoLds * sizeof(double)) / sizeof(double));

struct DiagArgs {
    const double* x;          // store: [chains][P][cap]
    const int64_t* off;       // [M] offset of chain m's first kept draw within column 0 (chain * P * cap + first row)
    int64_t cap;
    int M, n;                 // after the split
    int max_lag;              // 0: none
    int rho_lds;              // rho_t entries in LDS: min(n, kRhoLds)
    double* scratch;          // [columns of the launch][n] when n > kRhoLds, else null
    double* out;              // [5][P]: mean, sd, ess, rhat, mcse_mean
    int32_t* n_lags;          // [P]
    uint8_t* flag;            // [P]
    int64_t P, j0;            // columns; first column of this launch
};

// one workgroup per column; kStaged: the centred column lives in LDS
template <bool kStaged>
__global__ __launch_bounds__(kDiagBlock) void k_diag_column(DiagArgs a) {
    extern __shared__ __align__(16) unsigned char dyn[];
    __shared__ double mu[kMaxSplitChains];
    __shared__ double gblk[kLagBlock];
    __shared__ double red[kDiagWaves];
    __shared__ int ired[kDiagWaves];
    __shared__ int stop_s;
    double* rho_l = reinterpret_cast<double*>(dyn);          // [rho_lds]
    double* d = rho_l + a.rho_lds;                           // [M][n] when staged
    const int64_t j = a.j0 + blockIdx.x;
    const int M = a.M, n = a.n, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double* col = a.x + j * a.cap;
    double* rho_g = a.scratch ? a.scratch + (int64_t)blockIdx.x * n : nullptr;
    auto set_rho = [&](int k, double v) { if (k < kRhoLds) rho_l[k] = v; else rho_g[k] = v; };
    auto get_rho = [&](int k) { return k < kRhoLds ? rho_l[k] : rho_g[k]; };

    // 1. finite check, min / max
    double lo = INFINITY, nhi = INFINITY;                    // nhi: min of -x
    int bad = 0;
    for (int m = 0; m < M; ++m) {
        const double* xm = col + a.off[m];
        for (int i = tid; i < n; i += kDiagBlock) {
            const double v = xm[i];
            bad |= !isfinite(v);
            lo = fmin(lo, v);
            nhi = fmin(nhi, -v);
        }
    }
    bad = unit_block_reduce<kDiagWaves>(bad, ired, unit_or{});
    if (bad) {                                               // (uniform over the block)
        if (tid == 0) {
            for (int q = 0; q < 5; ++q) a.out[q * a.P + j] = NAN;
            a.n_lags[j] = 0;
            a.flag[j] = SBE_DIAG_FLAG_NONFINITE;
        }
        return;
    }
    lo = unit_block_reduce<kDiagWaves>(lo, red, unit_min{});
    nhi = unit_block_reduce<kDiagWaves>(nhi, red, unit_min{});
    const bool constant = (-nhi) - lo < 1e-15;

    // chain means: one wave per chain; the sum, then the sum of the residuals added back
    for (int m = wave; m < M; m += kDiagWaves) {
        const double* xm = col + a.off[m];
        double s = 0.0;
        for (int i = lane; i < n; i += 64) s += xm[i];
        const double mu0 = unit_wave_reduce(s, unit_sum{}) / n;
        double r = 0.0;
        for (int i = lane; i < n; i += 64) r += xm[i] - mu0;
        const double mu1 = mu0 + unit_wave_reduce(r, unit_sum{}) / n;
        if (lane == 0) mu[m] = mu1;
    }
    __syncthreads();
    if (kStaged) {
        for (int m = 0; m < M; ++m) {
            const double* xm = col + a.off[m];
            const double mum = mu[m];
            for (int i = tid; i < n; i += kDiagBlock) d[m * n + i] = xm[i] - mum;
        }
        __syncthreads();
    }

    // 2. pooled mean and sd; the variance of the chain means (every thread, in chain order)
    double mean = 0.0;
    for (int m = 0; m < M; ++m) mean += mu[m];
    mean /= M;
    double between = 0.0;
    if (M > 1) {
        for (int m = 0; m < M; ++m) between += (mu[m] - mean) * (mu[m] - mean);
        between /= (M - 1);
    }
    double ssq = 0.0;
    for (int m = 0; m < M; ++m) {
        const double* xm = col + a.off[m];
        const double mum = mu[m], shift = mum - mean;
        for (int i = tid; i < n; i += kDiagBlock) {
            const double v = (kStaged ? d[m * n + i] : xm[i] - mum) + shift;
            ssq += v * v;
        }
    }
    ssq = unit_block_reduce<kDiagWaves>(ssq, red, unit_sum{});
    const double total = (double)M * (double)n;
    const double sd = sqrt(ssq / (total - 1.0));
    if (constant) {
        if (tid == 0) {
            a.out[j] = mean;
            a.out[a.P + j] = sd;
            a.out[2 * a.P + j] = total;
            a.out[3 * a.P + j] = NAN;
            a.out[4 * a.P + j] = 0.0;
            a.n_lags[j] = 0;
            a.flag[j] = SBE_DIAG_FLAG_CONSTANT;
        }
        return;
    }

    // 3. lag blocks and the positive-sequence rule (the walk's state lives in thread 0)
    double even = 1.0, odd = 0.0, mean_var = 0.0, var_plus = 1.0;
    int t = 1, truncated = 0;
    for (int b = 0; b * kLagBlock < n; ++b) {                // (bounded by n; the walk stops it earlier)
        const int t0 = b * kLagBlock + wave * kLagsPerLane;  // first lag of this wave
        double acc[kLagsPerLane];
#pragma unroll
        for (int r = 0; r < kLagsPerLane; ++r) acc[r] = 0.0;
        for (int m = 0; m < M; ++m) {
            const double* xm = col + a.off[m];
            const double* dm = d + m * n;
            const double mum = mu[m];
            for (int i = lane; i + t0 < n; i += 64) {
                const double di = kStaged ? dm[i] : xm[i] - mum;
#pragma unroll
                for (int r = 0; r < kLagsPerLane; ++r) {
                    const int k = i + t0 + r;
                    if (k < n) acc[r] += di * (kStaged ? dm[k] : xm[k] - mum);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < kLagsPerLane; ++r) {
            const double g = unit_wave_reduce(acc[r], unit_sum{});
            if (lane == 0) gblk[wave * kLagsPerLane + r] = g / n / M;
        }
        __syncthreads();
        if (tid == 0) {
            const int base = b * kLagBlock;
            if (b == 0) {
                mean_var = gblk[0] * n / (n - 1);
                var_plus = mean_var * (n - 1) / n + between;
                odd = 1.0 - (mean_var - gblk[1]) / var_plus;
                set_rho(0, 1.0);
                set_rho(1, odd);
            }
            int stop = 0;
            while (true) {
                if (!(t < n - 3 && even + odd > 0.0)) { stop = 1; break; }
                if (a.max_lag > 0 && t + 2 > a.max_lag) { truncated = 1; stop = 1; break; }
                if (t + 1 >= base + kLagBlock) break;        // the next pair lies in the next block
                even = 1.0 - (mean_var - gblk[t + 1 - base]) / var_plus;
                odd = 1.0 - (mean_var - gblk[t + 2 - base]) / var_plus;
                const bool keep = even + odd >= 0.0;
                set_rho(t + 1, keep ? even : 0.0);
                set_rho(t + 2, keep ? odd : 0.0);
                t += 2;
            }
            stop_s = stop;
        }
        __syncthreads();
        if (stop_s) break;
    }

    // 4. the monotone sequence and the sums
    if (tid == 0) {
        const int max_t = t - 2;
        if (even > 0.0) set_rho(max_t + 1, even);
        for (int k = 1; k <= max_t - 2; k += 2) {
            const double prev = get_rho(k - 1) + get_rho(k);
            if (get_rho(k + 1) + get_rho(k + 2) > prev) {
                set_rho(k + 1, prev / 2);
                set_rho(k + 2, prev / 2);
            }
        }
        double sum = 0.0;
        for (int k = 0; k <= max_t; ++k) sum += get_rho(k);
        double tau = -1.0 + 2.0 * sum + get_rho(max_t + 1);
        tau = fmax(tau, 1.0 / log10(total));
        const double ess = total / tau;
        a.out[j] = mean;
        a.out[a.P + j] = sd;
        a.out[2 * a.P + j] = ess;
        a.out[3 * a.P + j] = sqrt(var_plus / mean_var);
        a.out[4 * a.P + j] = sd / sqrt(ess);
        a.n_lags[j] = max_t + 2;
        a.flag[j] = truncated ? SBE_DIAG_FLAG_TRUNCATED : 0;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------
constexpr char kDiagLane[] = "chain";

int64_t default_launch_columns(int M, int64_t n) {
    const double per_column = 0.5 * (double)M * (double)n * (double)n;
    const double by_work = std::floor(kLaunchWork / per_column);
    int64_t cols = by_work >= (double)kMaxGridBlocks ? kMaxGridBlocks : (int64_t)by_work;
    return std::max(cols, kMinLaunchColumns);
}

// The store a unit's handle holds beside sbe_unit_handle: M chains of rows [S_r][P], column-major per chain.
struct diag_store {
    unit_lanes chains;                  // (empty: no shape yet)
    int64_t P = 0;
    double* d_x = nullptr;              // [chains][P][cap]
    size_t x_bytes = 0;
    void* d_stage = nullptr;            // host rows in flight
    size_t stage_bytes = 0;
    int64_t* d_off = nullptr;           // [kMaxSplitChains]
    double* d_scratch = nullptr;        // rho_t of one launch of the column kernel (n > kRhoLds)
    size_t scratch_bytes = 0;
};

// <prefix>_reset: the argument checks, then the store and the offsets; leaves the store unshaped (the unit's own buffers
// follow, then diag_store_shaped)
template <class H>
int diag_store_reset(H* h, int n_chains, int64_t n_columns, int64_t capacity_rows) {
    if (n_chains < 1 || n_chains > SBE_DIAG_MAX_CHAINS)
        return fail(h, SBE_ERR_ARG, "n_chains=%d out of range [1, %d]", n_chains, SBE_DIAG_MAX_CHAINS);
    if (n_columns < 1 || n_columns > INT32_MAX)
        return fail(h, SBE_ERR_ARG, "n_columns=%lld out of range [1, %d]", (long long)n_columns, INT32_MAX);
    if (capacity_rows < 1) return fail(h, SBE_ERR_ARG, "capacity_rows=%lld must be positive", (long long)capacity_rows);
    const double bytes = (double)n_chains * (double)n_columns * (double)capacity_rows * sizeof(double);
    if (bytes > 1.0e15) return fail(h, SBE_ERR_ARG, "a store of %d x %lld x %lld float64 values is out of range", n_chains,
                                     (long long)n_columns, (long long)capacity_rows);
    h->chains.rows.clear();                               // (a failed allocation leaves an unshaped store)
    HIPCHK(h, hipSetDevice(h->device));
    int rc = unit_ensure(h, h->d_x, h->x_bytes, (size_t)n_chains * (size_t)n_columns * (size_t)capacity_rows * sizeof(double));
    if (!rc) rc = unit_ensure(h, h->d_off, (size_t)kMaxSplitChains * sizeof(int64_t));
    return rc;
}

template <class H>
void diag_store_shaped(H* h, int n_chains, int64_t n_columns, int64_t capacity_rows) {
    h->P = n_columns;
    h->chains.cap = capacity_rows;
    h->chains.rows.assign((size_t)n_chains, 0);
}

// <prefix>_append_rows; `reset`: the name of the call that shapes the store
template <class H>
int diag_store_append(H* h, const char* reset, int chain, const double* rows, int64_t n_rows) {
    int rc = h->chains.check_append(h, kDiagLane, reset, chain, rows, n_rows);
    if (rc || n_rows == 0) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    const int64_t P = h->P, cap = h->chains.cap, have = h->chains.rows[(size_t)chain];
    double* x = h->d_x + (int64_t)chain * P * cap;
    rc = unit_append_pieces(h, h->d_stage, h->stage_bytes, rows, n_rows, (int64_t)sizeof(double) * P, cap, [&](int64_t k, int64_t r) {
        return unit_for_grid_chunks((P + 31) / 32, [&](int64_t t0, int64_t tiles) {
            k_unit_transpose<<<dim3((unsigned)tiles, (unsigned)((k + 31) / 32)), 256, 0, h->stream>>>((const double*)h->d_stage, k, P, x, cap,
                                                                                                     have + r, t0);
            HIPCHK(h, hipGetLastError());
            return SBE_OK;
        });
    });
    if (rc) return rc;
    h->chains.rows[(size_t)chain] = have + n_rows;
    return SBE_OK;
}

// The plan of a compute call: its argument checks (after the handle's and the outputs'), then M and n after the split
// and the offset of every chain's first kept draw within column 0.
template <class H>
int diag_plan(H* h, const char* reset, const int64_t* burn_rows, int split, int64_t max_lag, int* M_out, int64_t* n_out,
              std::vector<int64_t>* off_out) {
    if (const int rc = h->chains.check_shaped(h, reset)) return rc;
    if (!burn_rows) return fail(h, SBE_ERR_ARG, "null pointer argument: burn_rows");
    if (max_lag < 0 || max_lag > INT32_MAX) return fail(h, SBE_ERR_ARG, "max_lag=%lld out of range [0, %d] (0: none)", (long long)max_lag, INT32_MAX);
    const int chains = h->chains.count();
    const int64_t cap = h->chains.cap;
    int64_t len = INT64_MAX;
    for (int c = 0; c < chains; ++c) {
        const int64_t have = h->chains.rows[(size_t)c];
        if (burn_rows[c] < 0 || burn_rows[c] > have)
            return fail(h, SBE_ERR_ARG, "burn_rows[%d]=%lld out of range [0, %lld] (rows stored for the chain)", c, (long long)burn_rows[c],
                        (long long)have);
        len = std::min(len, have - burn_rows[c]);
    }
    const int M = split ? 2 * chains : chains;
    const int64_t n = split ? len / 2 : len;
    if (n < SBE_DIAG_MIN_DRAWS)
        return fail(h, SBE_ERR_ARG, "%lld draws per chain after burn-in%s; at least %d are needed", (long long)n,
                    split ? " and split" : "", SBE_DIAG_MIN_DRAWS);
    if ((int64_t)M * n > SBE_DIAG_MAX_DRAWS)
        return fail(h, SBE_ERR_ARG, "%d chains x %lld draws after burn-in%s exceed %d (2^20) draws per column", M, (long long)n,
                    split ? " and split" : "", SBE_DIAG_MAX_DRAWS);
    off_out->assign((size_t)M, 0);
    for (int c = 0; c < chains; ++c) {
        const int64_t base = (int64_t)c * h->P * cap + burn_rows[c];
        if (split) {
            (*off_out)[(size_t)(2 * c)] = base;                     // x[:h]
            (*off_out)[(size_t)(2 * c + 1)] = base + len - n;       // x[-h:]
        } else {
            (*off_out)[(size_t)c] = base;
        }
    }
    *M_out = M;
    *n_out = n;
    return SBE_OK;
}

inline bool diag_staged(int M, int64_t n) { return (int64_t)M * n <= kLdsMaxDraws; }

// columns per launch of the column kernel: the caller's (0: the default), at most what the rho_t scratch holds, at most P
inline int64_t diag_per_launch(int64_t launch_columns, int M, int64_t n, int64_t P) {
    int64_t per_launch = launch_columns ? launch_columns : default_launch_columns(M, n);
    if (n > kRhoLds) per_launch = std::max<int64_t>(1, std::min<int64_t>(per_launch, (int64_t)(kScratchBytes / ((size_t)n * sizeof(double)))));
    return std::min(per_launch, P);
}

// the rho_t scratch of launches of per_launch columns, and the kernels' dynamic LDS limit (once per compute call)
template <class H>
int diag_prepare_launch(H* h, int M, int64_t n, int64_t per_launch) {
    if (n > kRhoLds) {
        const int rc = unit_ensure(h, h->d_scratch, h->scratch_bytes, (size_t)per_launch * (size_t)n * sizeof(double));
        if (rc) return rc;
    }
    auto kernel = diag_staged(M, n) ? k_diag_column<true> : k_diag_column<false>;
    HIPCHK(h, hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kLdsBudget - kStaticLds)));
    return SBE_OK;
}

// the column kernel over the first `count` of the P columns of a store [.][P][cap] (d_off: the chains' offsets; P is also the
// stride of `out`), per_launch columns at a time
template <class H>
int diag_launch_columns(H* h, const double* x, const int64_t* d_off, int64_t cap, int M, int64_t n, int64_t max_lag, double* out,
                        int32_t* lags, uint8_t* flag, int64_t P, int64_t count, int64_t per_launch, int64_t* launches) {
    const bool staged = diag_staged(M, n), spill = n > kRhoLds;
    const int rho_lds = (int)std::min<int64_t>(n, kRhoLds);
    const size_t lds = (size_t)rho_lds * sizeof(double) + (staged ? (size_t)M * (size_t)n * sizeof(double) : 0);
    auto kernel = staged ? k_diag_column<true> : k_diag_column<false>;
    for (int64_t j0 = 0; j0 < count; j0 += per_launch, ++*launches) {
        const DiagArgs args{x, d_off, cap, M, (int)n, (int)max_lag, rho_lds, spill ? h->d_scratch : nullptr, out, lags, flag, P, j0};
        kernel<<<(unsigned)std::min(per_launch, count - j0), kDiagBlock, lds, h->stream>>>(args);
        HIPCHK(h, hipGetLastError());
    }
    return SBE_OK;
}

}  // namespace
