#pragma once
// sbe_psis_ratio.hip.h -- PSIS over one vector of float64 log ratios by one 256-thread workgroup, written once for the units
// that need it: the power-scaling sensitivity (sbe_psens.hip: the ratios (alpha - 1) x of a logged component) and the
// leave-one-object-out ELPD (sbe_objloo.hip: the ratios -L and -Cnd of an object).  sbe_psis_column.hip.h is the float32
// counterpart for logged likelihoods; here the values are float64 and the whole vector is sorted with its samples.  The
// numerical contract is tests/_elpd_oracle.py:psis_column with tests/_psens_oracle.py's bounds; DESIGN.md sections 28 and 32.
//
// The steps a unit's kernel runs, all threads of the workgroup calling each:
//   keys          x = ratio - max with its sample index into RatioKeys (LDS, or a slice of global memory: the same code);
//   ratio_block_sort   the bitonic network of sbe_summary.hip (every comparator points the same way, so slots >= N act as +inf
//                 without storage) over keys of 12 bytes, a float64 value and an int32 sample, held as two arrays; the order
//                 is lexicographic, so it is unique and equals a stable argsort of the values;
//   ratio_smooth_tail  the cutoff floored at log DBL_MIN, the tail (strictly above the cutoff: a suffix of the sort), _gpdfit on
//                 its exceedances and _gpinv in float64, the truncation at 0, written over the tail's values; returns k;
//   ratio_logsumexp    of the values as they then stand (NaN if any is NaN, as the checker's is).
// What a unit does with the normalised weights is its own.  Every sum is a fixed tree over fixed per-thread partial sums.
// Everything lives in an unnamed namespace, as the unit layer does: every unit compiles its own copy.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "sbe_unit_device.hip.h"

namespace {

constexpr int kRatioBlock = 256;                     // 4 waves per vector
constexpr int kRatioWaves = kRatioBlock / 64;
constexpr int kRatioKeyBytes = (int)(sizeof(double) + sizeof(int32_t));
constexpr int kRatioMaxTail = 3072;                  // the tail count ceil(min(0.2 N, 3 sqrt N)) at N = 2^20
constexpr int kRatioMaxM = 96;                       // _gpdfit candidates: 30 + sqrt(tail) <= 85
constexpr double kLogDblMin = -708.3964185322641;    // log(DBL_MIN)
constexpr double kDblEps = 2.220446049250313e-16;

struct RatioKeys {
    double* val;
    int32_t* idx;
};

// the static LDS of a vector's workgroup (the kernel declares one, __shared__)
struct RatioScratch {
    double red[kRatioWaves];
    int ired[kRatioWaves];
    double fit_b[kRatioMaxM], fit_k[kRatioMaxM], fit_ls[kRatioMaxM], fit_w[kRatioMaxM], fit_post;
};

inline int ratio_tail_count(int64_t N) { return (int)std::ceil(std::min(0.2 * (double)N, 3.0 * std::sqrt((double)N))); }

__device__ inline void ratio_compare_exchange(RatioKeys s, int lo, int hi) {
    const double a = s.val[lo], b = s.val[hi];
    const int32_t ia = s.idx[lo], ib = s.idx[hi];
    if (b < a || (b == a && ib < ia)) {
        s.val[lo] = b;
        s.idx[lo] = ib;
        s.val[hi] = a;
        s.idx[hi] = ia;
    }
}

// keys [0 .. N) ascending by (value, sample), by the whole block; ends with a barrier.  Slots N .. pad - 1 are never touched.
__device__ inline void ratio_block_sort(RatioKeys s, int N) {
    const int tid = threadIdx.x;
    int pad = 2;
    while (pad < N) pad <<= 1;                               // (at most 2^20)
    const int pairs = pad >> 1;                              // (< N)
    for (int k = 2; k <= pad; k <<= 1) {
        const int half = k >> 1;
        for (int t = tid; t < pairs; t += kRatioBlock) {     // the merge's first step: slot o of a block with slot k - 1 - o
            const int o = t & (half - 1), base = (t - o) << 1;
            const int hi = base + k - 1 - o;
            if (hi < N) ratio_compare_exchange(s, base + o, hi);
        }
        __syncthreads();
        for (int j = half >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < pairs; t += kRatioBlock) {
                const int o = t & (j - 1), lo = ((t - o) << 1) | o;
                if (lo + j < N) ratio_compare_exchange(s, lo, lo + j);
            }
            __syncthreads();
        }
    }
}

// The sorted keys' tail smoothed in place; ary: [tail_n] doubles of the workgroup's own (the exceedances).  Returns k (inf
// when the tail has at most four values: nothing is smoothed).  Ends with the smoothed values visible to the block.
__device__ inline double ratio_smooth_tail(RatioKeys s, int N, int tail_n, double* ary, RatioScratch& sc) {
    const int tid = threadIdx.x;
    // the cutoff and the tail: the values strictly above it, a suffix of the sort within its last tail_n places
    const double xcutoff = fmax(s.val[N - tail_n - 1], kLogDblMin);
    const double expxcutoff = exp(xcutoff);
    int above = 0;
    for (int p = N - tail_n + tid; p < N; p += kRatioBlock) above += s.val[p] > xcutoff;
    const int n = unit_block_reduce<kRatioWaves>(above, sc.ired, unit_sum{});
    const int t0 = N - n;

    // _gpdfit on the exceedances exp(x) - exp(cutoff), ascending (sbe_psis_column.hip.h, step 5)
    double k_hat = INFINITY, sigma = 0.0;
    if (n > 4) {
        for (int i = tid; i < n; i += kRatioBlock) ary[i] = exp(s.val[t0 + i]) - expxcutoff;
        __syncthreads();
        const int m = 30 + (int)sqrt((double)n);
        const double q = 3 * ary[(int)(n / 4.0 + 0.5) - 1], inv_last = 1 / ary[n - 1];
        const int lane = tid & 63, wave = tid >> 6;
        for (int c = wave; c < m; c += kRatioWaves) {         // k_ary[c] = mean(log1p(-b[c] * ary)): one wave per candidate
            double b = 1 - sqrt(m / ((double)(c + 1) - 0.5));
            b /= q;
            b += inv_last;
            double acc = 0.0;
            for (int i = lane; i < n; i += 64) acc += log1p(-b * ary[i]);
            acc = unit_wave_reduce(acc, unit_sum{});
            if (lane == 0) { sc.fit_b[c] = b; sc.fit_k[c] = acc / n; }
        }
        __syncthreads();
        if (tid < m) sc.fit_ls[tid] = n * (log(-(sc.fit_b[tid] / sc.fit_k[tid])) - sc.fit_k[tid] - 1);
        __syncthreads();
        if (tid < m) {
            double z = 0.0;
            for (int c = 0; c < m; ++c) z += exp(sc.fit_ls[c] - sc.fit_ls[tid]);
            sc.fit_w[tid] = 1 / z;
        }
        __syncthreads();
        if (tid == 0) {                                       // prune negligible weights (NaN included), normalise, posterior b
            double wsum = 0.0;
            for (int c = 0; c < m; ++c) if (sc.fit_w[c] >= 10 * kDblEps) wsum += sc.fit_w[c];
            double b_post = 0.0;
            for (int c = 0; c < m; ++c) if (sc.fit_w[c] >= 10 * kDblEps) b_post += sc.fit_b[c] * (sc.fit_w[c] / wsum);
            sc.fit_post = b_post;
        }
        __syncthreads();
        const double b_post = sc.fit_post;
        double acc = 0.0;
        for (int i = tid; i < n; i += kRatioBlock) acc += log1p(-b_post * ary[i]);
        const double k_post = unit_block_reduce<kRatioWaves>(acc, sc.red, unit_sum{}) / n;
        sigma = -k_post / b_post;
        k_hat = (n * k_post + 10 * 0.5) / (n + 10);
    }

    // the smoothed tail (_gpinv; NaN when sigma <= 0, not repaired), truncated at 0
    if (n > 4 && isfinite(k_hat)) {
        for (int i = tid; i < n; i += kRatioBlock) {
            const double p = (0.5 + i) / n;
            double gq = NAN;
            if (!(sigma <= 0)) {
                gq = fabs(k_hat) < kDblEps ? -log1p(-p) : expm1(-k_hat * log1p(-p)) / k_hat;
                gq *= sigma;
            }
            double x = log(gq + expxcutoff);
            if (x > 0) x = 0;
            s.val[t0 + i] = x;
        }
        __syncthreads();
    }
    return k_hat;
}

// logsumexp of the N values (a NaN among them makes it NaN, as the checker's does)
__device__ inline double ratio_logsumexp(RatioKeys s, int N, RatioScratch& sc) {
    const int tid = threadIdx.x;
    double top = -INFINITY;
    int nan = 0;
    for (int p = tid; p < N; p += kRatioBlock) {
        top = fmax(top, s.val[p]);
        nan |= isnan(s.val[p]);
    }
    top = unit_block_reduce<kRatioWaves>(top, sc.red, unit_max{});
    nan = unit_block_reduce<kRatioWaves>(nan, sc.ired, unit_or{});
    if (nan) top = NAN;
    double sum = 0.0;
    for (int p = tid; p < N; p += kRatioBlock) sum += exp(s.val[p] - top);
    sum = unit_block_reduce<kRatioWaves>(sum, sc.red, unit_sum{});
    return log(sum) + top;
}

}  // namespace
