// sbe_dirichlet.hip.h -- the collapsed Dirichlet-categorical log-pdf (a7 + a8: util.py:1373-1394, likelihood.py:65-101) on the
// device: the term itself, written once, and the kernels that are nothing but that term.  One row (group,
// feature) with counts c_s and concentrations a_s:
//   float32( lgamma(A) - lgamma(n + A) + sum_{s: a_s > 0} (lgamma(c_s + a_s) - lgamma(a_s)) )
// n = the float32 NumPy-order sum of the counts, A = the fp64 NumPy-order sum of the concentrations, the series summed in
// NumPy's pairwise order in fp64.  The sums and the thread mapping belong to the caller, the arithmetic on their results is here.
// Included through sbe_kernels.hip.h; the tile blocks of step_core_body (sbe_kernels_sampling.hip.h) are the one caller outside.
#pragma once
#include "sbe_device_common.hip.h"

namespace sbe {

// lgamma(a_s) as k_conc_lgamma's table stores it: 0 where the state is not applicable (a_s <= 0; no lgamma is taken there)
__device__ __forceinline__ double dcat_lgamma_conc(double a) { return a > 0.0 ? sbe_lgamma_pos(a) : 0.0; }
// lgamma(A) of a row (every row has one: a row without an applicable state is lgamma(0) - lgamma(n) as in the reference)
__device__ __forceinline__ double dcat_lgamma_sum(double sum_a) { return sbe_lgamma_pos(sum_a); }
// The term of one state; `lg_a` = dcat_lgamma_conc(a), from the table or computed in place: the same value either way.
__device__ __forceinline__ double dcat_state_term(float c, double a, double lg_a) {
    return a > 0.0 ? sbe_lgamma_pos((double)c + a) - lg_a : 0.0;
}
// The row: `lg_sum_a` = dcat_lgamma_sum(sum_a), `series` = the NumPy-order fp64 sum of the states' terms.
__device__ __forceinline__ float dcat_row(double lg_sum_a, float n, double sum_a, double series) {
    return (float)((lg_sum_a - sbe_lgamma_pos((double)n + sum_a)) + series);
}

// k_dcl: one thread per (group, feature), nothing tabulated (stateless call; resident tables beyond the one-launch LDS budget).
// k_group_sum_f32: one thread per group: float32 NumPy-order sum over features -> float64 cache.
template <class TC>
__global__ void k_dcl(const TC* __restrict__ counts, const double* __restrict__ conc_in,
                      float* __restrict__ per_feature, int g_lo, int g_hi, int F, int S, int conc_per_group) {
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= (int64_t)(g_hi - g_lo) * F) return;
    const int64_t base = ((int64_t)g_lo * F + row) * S;
    // concentration either per group [G][F][S] or one [F][S] table broadcast over groups
    const double* conc = conc_per_group ? conc_in : conc_in - base + (row % F) * (int64_t)S;
    auto cnt = [&](int s) -> float { return (float)counts[base + s]; };
    auto a = [&](int s) -> double { return conc[base + s]; };
    const float n = np_pairwise_sum<float>(cnt, S);
    const double sum_a = np_pairwise_sum<double>(a, S);
    auto series = [&](int s) -> double {
        const double as = conc[base + s];
        return dcat_state_term((float)counts[base + s], as, dcat_lgamma_conc(as));
    };
    per_feature[row] = dcat_row(dcat_lgamma_sum(sum_a), n, sum_a, np_pairwise_sum<double>(series, S));
}

static __global__ void k_group_sum_f32(const float* __restrict__ per_feature, double* __restrict__ per_group, int n_groups, int F) {
    // one group per octet of lanes (np_pairwise_sum_f32_x8: NumPy's order, an eighth of the dependent chain)
    const int g = (blockIdx.x * blockDim.x + threadIdx.x) >> 3;
    if (g >= n_groups) return;
    const float* p = per_feature + (int64_t)g * F;
    auto get = [&](int i) -> float { return p[i]; };
    const float total = np_pairwise_sum_f32_x8(get, F, (int)(threadIdx.x & 7));
    if ((threadIdx.x & 7) == 0) per_group[g] = (double)total;
}

// The count-independent values of the concentration tables, built once per sbe_set_concentration: per element
// dcat_lgamma_conc, per (group, feature) row sum_a = the NumPy-order sum of the row and dcat_lgamma_sum of it.  The
// one-launch forms below and k_step_core then evaluate ONE lgamma per element and per row instead of k_dcl's two.
static __global__ void k_conc_lgamma(const double* __restrict__ conc, double* __restrict__ lg_conc, double* __restrict__ sum_a,
                              double* __restrict__ lg_sum_a, int g_lo, int g_hi, int F, int S) {
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= (int64_t)(g_hi - g_lo) * F) return;
    const int64_t r = (int64_t)g_lo * F + row, base = r * S;
    for (int s = 0; s < S; ++s) lg_conc[base + s] = dcat_lgamma_conc(conc[base + s]);
    auto conc_at = [&](int k) -> double { return conc[base + k]; };
    const double sa = np_pairwise_sum<double>(conc_at, S);
    sum_a[r] = sa;
    lg_sum_a[r] = dcat_lgamma_sum(sa);
}

// a7 + a8 in ONE launch (round 3: the drop-in Likelihood.__call__ asks for this once or twice per MCMC step, and a
// launch costs more than the arithmetic): block = one group.  Phase 1, one thread per table element: the term of the
// element, its lgamma(a) from k_conc_lgamma's table; phase 2, one thread per feature: the ordered sums over the S states
// and the row; phase 3, eight lanes: the float32 NumPy-order sum over the features (k_group_sum_f32's).  Dynamic LDS
// (collapsed_lds_bytes on the host): F*S doubles + F floats.  `per_feature` (may be null) gets the rows.
template <class TC>
__device__ __forceinline__ void collapsed_group_block(
    const TC* __restrict__ counts, const double* __restrict__ conc, const double* __restrict__ lg_conc,
    const double* __restrict__ sum_a, const double* __restrict__ lg_sum_a, float* __restrict__ per_feature,
    double* __restrict__ per_group, int g_lo, int F, int S, int block /* = group - g_lo */, unsigned char* cg_lds) {
    double* ser = reinterpret_cast<double*>(cg_lds);                       // [F][S]
    float* pf = reinterpret_cast<float*>(cg_lds + (size_t)F * S * sizeof(double));   // [F]
    const int g = g_lo + block;
    const int64_t gbase = (int64_t)g * F * S;
    for (int e = threadIdx.x; e < F * S; e += blockDim.x)
        ser[e] = dcat_state_term((float)counts[gbase + e], conc[gbase + e], lg_conc[gbase + e]);
    __syncthreads();
    for (int f = threadIdx.x; f < F; f += blockDim.x) {
        const int64_t base = gbase + (int64_t)f * S;
        auto cnt = [&](int k) -> float { return (float)counts[base + k]; };
        auto ser_at = [&](int k) -> double { return ser[f * S + k]; };
        const float n = np_pairwise_sum<float>(cnt, S);
        const float v = dcat_row(lg_sum_a[(int64_t)g * F + f], n, sum_a[(int64_t)g * F + f], np_pairwise_sum<double>(ser_at, S));
        pf[f] = v;
        if (per_feature) per_feature[(int64_t)block * F + f] = v;
    }
    __syncthreads();
    if (threadIdx.x < 8) {
        auto get = [&](int i) -> float { return pf[i]; };
        const float total = np_pairwise_sum_f32_x8(get, F, (int)threadIdx.x);
        if (threadIdx.x == 0) per_group[block] = (double)total;
    }
}
template <class TC>
__global__ __launch_bounds__(1024) void k_collapsed_groups(
    const TC* __restrict__ counts, const double* __restrict__ conc, const double* __restrict__ lg_conc,
    const double* __restrict__ sum_a, const double* __restrict__ lg_sum_a, float* __restrict__ per_feature,
    double* __restrict__ per_group, int g_lo, int F, int S, DoneSig done = DoneSig{}) {
    extern __shared__ __align__(16) unsigned char cg_lds[];
    collapsed_group_block<TC>(counts, conc, lg_conc, sum_a, lg_sum_a, per_feature, per_group, g_lo, F, S, (int)blockIdx.x, cg_lds);
    signal_done(done);
}

}  // namespace sbe
