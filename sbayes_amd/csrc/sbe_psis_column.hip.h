#pragma once
// sbe_psis_column.hip.h -- PSIS over one column of logged likelihoods by one workgroup, written once for the units that need it:
// the model comparison (sbe_elpd.hip: loo_i, k, lppd_i, v_i) and the leave-one-out predictive (sbe_loopred.hip: the same loo_i
// and k, and the smoothed weight of every sample).  The numerical contract is tests/_elpd_oracle.py; DESIGN.md section 11 has
// the layout, the selection and the limits.
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
// how the store was filled.
//
// Two things differ between the units, and both are template parameters:
//   Key   what the tail sort orders.  psis_key_plain: the bit pattern alone (equal values are interchangeable: every result of
//         the column is a function of the sorted values).  psis_key_sample: the bit pattern, then the sample index descending,
//         in one 64-bit word -- position t of the tail in ascending x is then the sample that the oracle's stable argsort puts
//         there (among equal lh the earlier sample first), and the key names it.  The values at every position are the same
//         under both keys, so loo_i and k are the same bits.
//   Sink  sink(sample, exp(x')) receives the unnormalised smoothed weight of every sample exactly once, as it is added to
//         a_all (psis_no_sink: nothing is kept; its `sample` of a tail position is meaningless under psis_key_plain).
// Everything lives in an unnamed namespace, as the unit layer does: every unit compiles its own copy.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "sbe_unit_device.hip.h"

namespace {

constexpr int kPsisBlock = 256;                      // 4 waves per column
constexpr int kPsisWaves = kPsisBlock / 64;
constexpr int kPsisMaxM = 96;                        // _gpdfit candidates: 30 + sqrt(T) <= 85 for S <= 2^20 (T <= 3072)
constexpr size_t kPsisStaticLds = 8192;              // headroom for the kernel's static LDS (histogram, reductions, fit)

struct psis_key_plain {
    using type = uint32_t;
    static constexpr type pad = 0xFFFFFFFFu;          // (sorts behind every likelihood: those are below 0x7F800000)
    __device__ static type make(uint32_t bits, int) { return bits; }
    __device__ static uint32_t bits(type k) { return k; }
    __device__ static int sample(type) { return 0; }
};

struct psis_key_sample {
    using type = unsigned long long;
    static constexpr type pad = ~0ull;
    __device__ static type make(uint32_t bits, int sample) { return ((type)bits << 32) | (uint32_t)~(uint32_t)sample; }
    __device__ static uint32_t bits(type k) { return (uint32_t)(k >> 32); }
    __device__ static int sample(type k) { return (int)~(uint32_t)k; }
};

struct psis_no_sink {
    __device__ void operator()(int, double) const {}
};

inline int psis_tail_count(int64_t s) { return (int)std::ceil(std::min(0.2 * (double)s, 3.0 * std::sqrt((double)s))); }
// dynamic LDS of a column of S samples: [tail exceedances Tp x f64][tail keys Tp x Key][staged column S x u32]
template <class Key>
inline size_t psis_tail_lds_bytes(int64_t s) {
    return (size_t)pow2_at_least(std::max(psis_tail_count(s), 1)) * (sizeof(typename Key::type) + sizeof(double));
}
template <class Key>
inline bool psis_column_staged(int64_t s) {
    return (size_t)s * sizeof(uint32_t) + psis_tail_lds_bytes<Key>(s) + kPsisStaticLds <= kLdsBudget;
}
template <class Key>
inline int64_t psis_lds_max_samples() {
    int64_t s = 2;
    while (psis_column_staged<Key>(s + 1)) ++s;
    return s;
}

__device__ inline double ll_of(uint32_t bits) { return log((double)__uint_as_float(bits)); }

// the static LDS of a column's workgroup (the kernel declares one, __shared__)
struct PsisScratch {
    uint32_t hist[256];
    uint32_t ured[kPsisWaves], found[2], n_cand;
    double red[kPsisWaves];
    double fit_b[kPsisMaxM], fit_k[kPsisMaxM], fit_ls[kPsisMaxM], fit_w[kPsisMaxM];
    double fit_post[1];                               // b_post
};

// what every thread of the workgroup holds afterwards; bad: the column holds a value that is not positive and finite, and
// nothing else was computed
struct PsisColumn {
    bool bad;
    double loo, k_hat, lppd, var;
    double a_all;                                     // sum over the samples of exp(x'): what the sink's values add up to
};

// rank-th smallest (0-based) of the S keys: MSB-first 8-bit radix select with an LDS histogram per digit
__device__ inline uint32_t radix_select(const uint32_t* v, int s, int rank, uint32_t* hist, uint32_t* wave_tot, uint32_t* found) {
    uint32_t prefix = 0, mask = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        hist[threadIdx.x] = 0;
        __syncthreads();
        for (int i = threadIdx.x; i < s; i += kPsisBlock) {
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

// One column: g its S bit patterns in global memory, tail_n = psis_tail_count(S), tail_p the power of two at or above it,
// dyn the workgroup's dynamic LDS (psis_tail_lds_bytes, and S words more when `stage`).  Called by all kPsisBlock threads.
template <class Key, class Sink>
__device__ inline PsisColumn psis_column(const uint32_t* g, int s, int tail_n, int tail_p, bool stage, unsigned char* dyn, PsisScratch& sc,
                                         const Sink& sink) {
    using key_t = typename Key::type;
    const int tid = threadIdx.x;
    double* ary = reinterpret_cast<double*>(dyn);                            // [tail_p] tail exceedances
    key_t* keys = reinterpret_cast<key_t*>(ary + tail_p);                    // [tail_p] candidate keys
    uint32_t* staged = reinterpret_cast<uint32_t*>(keys + tail_p);           // [S] when staged
    PsisColumn out{};

    // 1. stage, min, data check
    uint32_t umin = 0xFFFFFFFFu, bad = 0;
    for (int i = tid; i < s; i += kPsisBlock) {
        const uint32_t u = g[i];
        if (stage) staged[i] = u;
        bad |= (u == 0u || u >= 0x7F800000u);        // zero, negative (sign bit), inf, NaN
        umin = min(umin, u);
    }
    umin = unit_block_reduce<kPsisWaves>(umin, sc.ured, unit_min{});
    bad = unit_block_reduce<kPsisWaves>(bad, sc.ured, unit_max{});
    const uint32_t* v = stage ? staged : g;
    if (bad) {                                       // (uniform over the block)
        out.bad = true;
        return out;
    }
    const double ll_min = ll_of(umin);               // max(-ll) = -ll_min

    // 2. sum ll, sum lh
    double sum_ll = 0.0, sum_lh = 0.0;
    for (int i = tid; i < s; i += kPsisBlock) {
        const uint32_t u = v[i];
        sum_ll += ll_of(u);
        sum_lh += (double)__uint_as_float(u);
    }
    sum_ll = unit_block_reduce<kPsisWaves>(sum_ll, sc.red, unit_sum{});
    sum_lh = unit_block_reduce<kPsisWaves>(sum_lh, sc.red, unit_sum{});
    const double mean = sum_ll / s;
    out.lppd = log(sum_lh) - log((double)s);         // logsumexp(ll) - log S: float32 lh neither over- nor underflows

    // 3. cutoff: the (T+1)-th smallest lh
    const uint32_t ucut = radix_select(v, s, tail_n, sc.hist, sc.ured, sc.found);
    const double x_cut = -ll_of(ucut) + ll_min;              // x = -ll - max(-ll)
    const double xcutoff = fmax(x_cut, log(2.2250738585072014e-308));   // (never binds for float32 data: x >= -192)
    const double expxcutoff = exp(xcutoff);

    // 4. candidates (lh < cutoff: at most T of them), sorted by lh ascending = x descending; pads sort last
    if (tid == 0) sc.n_cand = 0;
    for (int i = tid; i < tail_p; i += kPsisBlock) keys[i] = Key::pad;
    __syncthreads();
    for (int i = tid; i < s; i += kPsisBlock) {
        const uint32_t u = v[i];
        if (u < ucut) keys[atomicAdd(&sc.n_cand, 1u)] = Key::make(u, i);
    }
    __syncthreads();
    const int nc = (int)sc.n_cand;
    for (int k = 2; k <= tail_p; k <<= 1) {
        for (int jj = k >> 1; jj > 0; jj >>= 1) {
            for (int i = tid; i < tail_p; i += kPsisBlock) {
                const int p = i ^ jj;
                if (p > i) {
                    const key_t ki = keys[i], kp = keys[p];
                    const bool up = (i & k) == 0;
                    if ((ki > kp) == up) { keys[i] = kp; keys[p] = ki; }
                }
            }
            __syncthreads();
        }
    }
    // x-ascending position t of candidate keys[nc - 1 - t]; the tail is the x > xcutoff suffix (all candidates here)
    double in_tail = 0.0;
    for (int t = tid; t < nc; t += kPsisBlock) in_tail += (-ll_of(Key::bits(keys[nc - 1 - t])) + ll_min) > xcutoff;
    const int tail_len = (int)unit_block_reduce<kPsisWaves>(in_tail, sc.red, unit_sum{});
    const int t0 = nc - tail_len;                            // x-ascending index of the first tail element

    // 5. _gpdfit on the exceedances exp(x) - exp(cutoff), ascending
    double k_hat = INFINITY, sigma = 0.0;
    const int n = tail_len;
    if (n > 4) {
        for (int i = tid; i < n; i += kPsisBlock) {
            const double x = -ll_of(Key::bits(keys[nc - 1 - (t0 + i)])) + ll_min;
            ary[i] = exp(x) - expxcutoff;
        }
        __syncthreads();
        const int m = 30 + (int)sqrt((double)n);
        const double q = 3 * ary[(int)(n / 4.0 + 0.5) - 1], inv_last = 1 / ary[n - 1];
        const int lane = tid & 63, wave = tid >> 6;
        for (int c = wave; c < m; c += kPsisWaves) {          // k_ary[c] = mean(log1p(-b[c] * ary)): one wave per candidate
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
            for (int c = 0; c < m; ++c) if (sc.fit_w[c] >= 10 * 2.220446049250313e-16) wsum += sc.fit_w[c];
            double b_post = 0.0;
            for (int c = 0; c < m; ++c) if (sc.fit_w[c] >= 10 * 2.220446049250313e-16) b_post += sc.fit_b[c] * (sc.fit_w[c] / wsum);
            sc.fit_post[0] = b_post;
        }
        __syncthreads();
        const double b_post = sc.fit_post[0];
        double acc = 0.0;
        for (int i = tid; i < n; i += kPsisBlock) acc += log1p(-b_post * ary[i]);
        const double k_post = unit_block_reduce<kPsisWaves>(acc, sc.red, unit_sum{}) / n;
        sigma = -k_post / b_post;
        k_hat = (n * k_post + 10 * 0.5) / (n + 10);
    }

    // the tail's terms of logsumexp(x') and logsumexp(x' + ll): smoothed (_gpinv, clamped to 0) when k is finite
    const bool smooth = n > 4 && isfinite(k_hat);
    double a_tail = 0.0, b_tail = 0.0;
    for (int i = tid; i < n; i += kPsisBlock) {
        const key_t key = keys[nc - 1 - (t0 + i)];
        const double ll = ll_of(Key::bits(key));
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
        const double e = exp(x);
        sink(Key::sample(key), e);
        a_tail += e;
        b_tail += exp(x + ll);
    }

    // 6. variance about the mean; the body's terms (lh >= cutoff, and candidates at or below xcutoff)
    double var = 0.0, a_body = 0.0, b_body = 0.0;
    for (int i = tid; i < s; i += kPsisBlock) {
        const uint32_t u = v[i];
        const double ll = ll_of(u);
        var += (ll - mean) * (ll - mean);
        if (u >= ucut) {
            const double x = -ll + ll_min;
            const double e = exp(x);
            sink(i, e);
            a_body += e;
            b_body += exp(x + ll);
        }
    }
    for (int t = tid; t < t0; t += kPsisBlock) {
        const key_t key = keys[nc - 1 - t];
        const double ll = ll_of(Key::bits(key));
        const double x = -ll + ll_min;
        const double e = exp(x);
        sink(Key::sample(key), e);
        a_body += e;
        b_body += exp(x + ll);
    }
    out.var = unit_block_reduce<kPsisWaves>(var, sc.red, unit_sum{}) / s;
    out.a_all = unit_block_reduce<kPsisWaves>(a_body + a_tail, sc.red, unit_sum{});
    const double b_all = unit_block_reduce<kPsisWaves>(b_body + b_tail, sc.red, unit_sum{});
    out.loo = log(b_all) - log(out.a_all);                    // logsumexp(x' - logsumexp(x') + ll)
    out.k_hat = k_hat;
    return out;
}

}  // namespace
