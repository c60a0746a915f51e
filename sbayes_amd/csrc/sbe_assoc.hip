// sbe_assoc.hip -- on-device screening of all feature pairs for dependence (include/sbe_assoc.h): the chi-squared test of
// independence that sbayes/tools/find_correlated_features.py runs per pair through pd.crosstab and
// scipy.stats.chi2_contingency.  The numerical contract is tests/_assoc_oracle.py; DESIGN.md section 13 has the layout
// and the limits.
//
// All contingency tables at once are X^T X of the one-hot matrix.  k_assoc_pairs computes one 32 x 32 tile of it per wave, for
// the tile pairs I <= J, by the four steps of sbe_assoc_pair.hip.h (contraction, margins and dof, Pearson terms, ordered
// sum), evaluates Q(dof/2, statistic/2) per pair and stores the pair and its mirror.
// No table is written to memory.  k_assoc_table counts one caller-named pair per block with integer atomics in LDS.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "sbe_assoc_pair.hip.h"
#include "../../include/sbe_assoc.h"

namespace {

constexpr int kTableBlock = 256;
constexpr int kSeriesMaxIter = 5000;                 // (the series and the fraction end long before at dof <= 961)

// ---- Q(a, x), the regularized upper incomplete gamma function ---------------------------------------------------
// tests/_assoc_oracle.py restates both functions operation for operation.
// x^a e^-x / Gamma(a).  From a = 16 on with Stirling's series for lgamma folded in, mu = (x - a) / a: the terms are then of
// the size of the result's logarithm instead of a log x, whose rounding alone would cost 4e-13 at dof 961
__device__ inline double assoc_prefactor(double a, double x) {
    if (a < 16.0) return exp(a * log(x) - x - lgamma(a));
    const double mu = (x - a) / a, w = 1.0 / (a * a);
    const double st = (1.0 / 12.0 - w * (1.0 / 360.0 - w * (1.0 / 1260.0 - w * (1.0 / 1680.0 - w * (1.0 / 1188.0))))) / a;
    return exp(a * (log1p(mu) - mu) + 0.5 * log(a / 6.283185307179586) - st);
}

// Cephes' igam / igamc in their classical form: the power series of P for x < max(1, a), else the continued fraction of Q
__device__ __attribute__((noinline)) double assoc_gamma_q(double a, double x) {
    if (!(x > 0.0)) return 1.0;
    if (isinf(x)) return 0.0;
    const double ax = assoc_prefactor(a, x);
    if (x < 1.0 || x < a) {
        double r = a, c = 1.0, ans = 1.0;
        for (int it = 0; it < kSeriesMaxIter; ++it) {
            r += 1.0;
            c *= x / r;
            ans += c;
            if (!(c > ans * 0x1p-53)) break;
        }
        return 1.0 - ans * ax / a;
    }
    if (ax == 0.0) return 0.0;
    constexpr double big = 4503599627370496.0, biginv = 2.22044604925031308085e-16;
    double y = 1.0 - a, z = x + y + 1.0, c = 0.0;
    double pkm2 = 1.0, qkm2 = x, pkm1 = x + 1.0, qkm1 = z * x;
    double ans = pkm1 / qkm1;
    for (int it = 0; it < kSeriesMaxIter; ++it) {
        c += 1.0;
        y += 1.0;
        z += 2.0;
        const double yc = y * c;
        const double pk = pkm1 * z - pkm2 * yc, qk = qkm1 * z - qkm2 * yc;
        double t = 1.0;
        if (qk != 0.0) {
            const double r = pk / qk;
            t = fabs((ans - r) / r);
            ans = r;
        }
        pkm2 = pkm1; pkm1 = pk; qkm2 = qkm1; qkm1 = qk;
        if (fabs(pk) > big) { pkm2 *= biginv; pkm1 *= biginv; qkm2 *= biginv; qkm1 *= biginv; }
        if (!(t > 0x1p-53)) break;
    }
    return ans * ax;
}

// ---- the pair kernel --------------------------------------------------------------------------------------------
struct PairArgs {
    const uint8_t* xt;        // codes, feature-major [F][n_pad], padded with 255 behind N
    int64_t n_pad;            // multiple of kPad
    int F, log_s;             // S_pad = 1 << log_s
    int64_t t0, t_end;        // tile pairs [t0, t_end) of the enumeration t = J (J + 1) / 2 + I, I <= J
    double* statistic;        // [F][F] outputs
    double* pvalue;
    int32_t* dof;
    int32_t* n;
    uint8_t* valid;
};

// (at most four waves per SIMD, which the LDS allows anyway: the compiler then keeps a round's sixteen loads in flight instead
// of trading them for registers)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 4))) void k_assoc_pairs(const PairArgs g) {
    extern __shared__ double assoc_lds[];                    // dynamic LDS, pair_lds_bytes(sub)
    const int S = 1 << g.log_s, sub = kTile >> g.log_s;      // states per feature (padded), features per tile edge
    const PairLds l = pair_lds(assoc_lds, sub);

    const int64_t t = g.t0 + blockIdx.x;
    if (t >= g.t_end) return;
    const TilePair pair = tile_pair(t);
    const int64_t I = pair.I, J = pair.J;
    const int lane = threadIdx.x;

    // ---- 1. to 3.: the contraction, the margins, the Pearson terms
    const v16f acc = pair_contract(g.xt, g.n_pad, g.F, g.log_s, I, J, lane);
    pair_terms(l, acc, g.log_s, lane);

    // ---- 4. statistic and p-value per pair; the pair and its mirror
    for (int idx = lane; idx < sub * sub; idx += 64) {
        const int p = idx / sub, q = idx - p * sub;
        const int64_t i = I * sub + p, j = J * sub + q;
        if (i >= j || j >= g.F) continue;                // (i < j: the diagonal tile pairs hold every pair twice)
        const int dof = l.pdof[idx];
        double stat = 0.0, pv = std::numeric_limits<double>::quiet_NaN();
        if (dof > 0) {
            stat = pair_statistic(l, p, q, S);
            pv = assoc_gamma_q(0.5 * (double)dof, 0.5 * stat);
        }
        const int n = (int)l.pn[idx];
        for (int m = 0; m < 2; ++m) {
            const int64_t o = m ? j * g.F + i : i * g.F + j;
            g.statistic[o] = stat;
            g.pvalue[o] = pv;
            g.dof[o] = dof;
            g.n[o] = n;
            g.valid[o] = dof > 0;
        }
    }
}

// the diagonal: no pair (statistic 0, pvalue NaN, dof 0, n 0, not valid)
__global__ void k_assoc_diagonal(int F, double* statistic, double* pvalue, int32_t* dof, int32_t* n, uint8_t* valid) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= F) return;
    const int64_t o = (int64_t)i * F + i;
    statistic[o] = 0.0;
    pvalue[o] = std::numeric_limits<double>::quiet_NaN();
    dof[o] = 0;
    n[o] = 0;
    valid[o] = 0;
}

// ---- the table kernel: one block per pair, integer counts -----------------------------------------------------------
__global__ __launch_bounds__(kTableBlock) void k_assoc_table(const uint8_t* xt, int64_t n_pad, int64_t N, const int32_t* pairs,
                                                             int64_t p0, int S, int32_t* out) {
    __shared__ int tab[SBE_ASSOC_MAX_STATES * SBE_ASSOC_MAX_STATES];
    const int64_t p = p0 + blockIdx.x;
    for (int c = threadIdx.x; c < S * S; c += kTableBlock) tab[c] = 0;
    __syncthreads();
    const uint8_t* xi = xt + (int64_t)pairs[2 * p] * n_pad;
    const uint8_t* xj = xt + (int64_t)pairs[2 * p + 1] * n_pad;
    for (int64_t n = threadIdx.x; n < N; n += kTableBlock) {
        const int a = xi[n], b = xj[n];
        if (a < S && b < S) atomicAdd(&tab[a * S + b], 1);       // (codes were checked on the host: the rest is NA)
    }
    __syncthreads();
    for (int c = threadIdx.x; c < S * S; c += kTableBlock) out[p * S * S + c] = tab[c];
}

}  // namespace

struct sbe_assoc : sbe_unit_handle, unit_tile_launches {   // (sbe_unit.hip.h; ev: around the pair kernel's launches)
    uint8_t* d_xt = nullptr;                     // codes of the last compute call, feature-major [F][n_pad]
    size_t xt_bytes = 0;
    void* d_out = nullptr;                       // the five [F][F] outputs, or the tables of one sbe_assoc_tables call
    size_t out_bytes = 0;
    int32_t* d_pairs = nullptr;
    size_t pairs_bytes = 0;
    int64_t N = 0, n_pad = 0, F = 0;             // shape of the codes held (F == 0: none yet)
    int s_max = 0, s_pad = 0;
    int64_t tile_pairs = 0, launches = 0;
    std::vector<void*> buffers() const { return {d_xt, d_out, d_pairs}; }
};

namespace {

constexpr char kNullHandle[] = "null handle";

}  // namespace

extern "C" {

int sbe_assoc_abi_version(void) { return SBE_ASSOC_ABI_VERSION; }

const char* sbe_assoc_last_error(const sbe_assoc* h) { return unit_last_error(h); }

int sbe_assoc_create(sbe_assoc** out, int device) { return unit_create_on_device(out, device, "sbe_assoc_create"); }

int sbe_assoc_destroy(sbe_assoc* h) { return unit_destroy(h, kNullHandle); }

int sbe_assoc_set_launch_tiles(sbe_assoc* h, int64_t tile_pairs) { return unit_set_launch_tiles(h, tile_pairs, kNullHandle); }

int sbe_assoc_compute(sbe_assoc* h, const uint8_t* x, int64_t n_objects, int64_t n_features, const int32_t* n_states,
                      double* statistic, double* pvalue, int32_t* dof, int32_t* n, uint8_t* valid) {
    CHECK_HANDLE(h, kNullHandle);
    if (!x || !n_states) return fail(h, SBE_ERR_ARG, "null pointer argument: %s", !x ? "x" : "n_states");
    if (!statistic || !pvalue || !dof || !n || !valid) return fail(h, SBE_ERR_ARG, "null pointer argument: output");
    const int64_t N = n_objects, F = n_features;
    int s_max = 1;
    if (const int rc = pair_check_shape(h, N, F, n_states, s_max)) return rc;
    // the codes, checked and turned feature-major, padded to whole rounds of the contraction with NA
    const int64_t n_pad = whole_rounds(N);
    std::vector<uint8_t> xt;
    if (const int rc = pair_feature_major(h, x, N, F, n_states, n_pad, xt)) return rc;
    const int log_s = pair_log_s(s_max);
    const int sub = kTile >> log_s;
    const int64_t tiles = (F + sub - 1) / sub, tile_pairs = tiles * (tiles + 1) / 2;
    const int64_t per_launch = tiles_per_launch(n_pad / kStep, h->launch_tiles);

    HIPCHK(h, hipSetDevice(h->device));
    h->F = 0;                                       // (until the new codes are in place)
    int rc = unit_ensure(h, h->d_xt, h->xt_bytes, xt.size());
    if (rc) return rc;
    const size_t ff = (size_t)F * F;
    if ((rc = unit_ensure(h, h->d_out, h->out_bytes, ff * 25))) return rc;
    double* d_stat = (double*)h->d_out;
    double* d_p = d_stat + ff;
    int32_t* d_dof = (int32_t*)(d_p + ff);
    int32_t* d_n = d_dof + ff;
    uint8_t* d_valid = (uint8_t*)(d_n + ff);
    HIPCHK(h, hipMemcpyAsync(h->d_xt, xt.data(), xt.size(), hipMemcpyHostToDevice, h->stream));
    k_assoc_diagonal<<<div_up(F, 256), 256, 0, h->stream>>>((int)F, d_stat, d_p, d_dof, d_n, d_valid);
    HIPCHK(h, hipGetLastError());
    int64_t launches = 0;
    rc = unit_timed(h, [&] {
        return unit_for_tile_launches(tile_pairs, per_launch, [&](int64_t t0, int64_t t_end) {      // one wave per tile pair
            const PairArgs args{h->d_xt, n_pad, (int)F, log_s, t0, t_end, d_stat, d_p, d_dof, d_n, d_valid};
            k_assoc_pairs<<<(unsigned)(t_end - t0), 64, pair_lds_bytes(sub), h->stream>>>(args);
            HIPCHK(h, hipGetLastError());
            ++launches;
            return SBE_OK;
        });
    });
    if (!rc) rc = unit_copy_back(h, (const double*)d_stat, ff, {statistic, pvalue});
    if (!rc) rc = unit_copy_back(h, (const int32_t*)d_dof, ff, {dof, n});
    if (!rc) rc = unit_copy_back(h, (const uint8_t*)d_valid, ff, {valid});
    if (!rc) rc = unit_sync_timed(h);
    if (rc) return rc;
    h->N = N;
    h->n_pad = n_pad;
    h->F = F;
    h->s_max = s_max;
    h->s_pad = 1 << log_s;
    h->tile_pairs = tile_pairs;
    h->launches = launches;
    return SBE_OK;
}

int sbe_assoc_tables(sbe_assoc* h, const int32_t* pairs, int64_t n_pairs, int32_t* out) {
    CHECK_HANDLE(h, kNullHandle);
    if (n_pairs < 0 || n_pairs > (int64_t)SBE_ASSOC_MAX_FEATURES * SBE_ASSOC_MAX_FEATURES)
        return fail(h, SBE_ERR_ARG, "n_pairs=%lld out of range [0, %lld]", (long long)n_pairs,
                     (long long)SBE_ASSOC_MAX_FEATURES * SBE_ASSOC_MAX_FEATURES);
    if (n_pairs > 0 && (!pairs || !out)) return fail(h, SBE_ERR_ARG, "null pointer argument: %s", !pairs ? "pairs" : "out");
    if (h->F == 0) return fail(h, SBE_ERR_STATE, "sbe_assoc_tables needs the codes of a successful sbe_assoc_compute");
    for (int64_t p = 0; p < 2 * n_pairs; ++p)
        if (pairs[p] < 0 || pairs[p] >= h->F)
            return fail(h, SBE_ERR_ARG, "pairs[%lld][%d]=%d out of range [0, %lld)", (long long)(p / 2), (int)(p & 1), pairs[p],
                         (long long)h->F);
    if (n_pairs == 0) return SBE_OK;
    HIPCHK(h, hipSetDevice(h->device));
    const size_t cells = (size_t)h->s_max * h->s_max;
    int rc = unit_ensure(h, h->d_pairs, h->pairs_bytes, (size_t)n_pairs * 2 * sizeof(int32_t));
    if (rc) return rc;
    if ((rc = unit_ensure(h, h->d_out, h->out_bytes, (size_t)n_pairs * cells * sizeof(int32_t)))) return rc;
    HIPCHK(h, hipMemcpyAsync(h->d_pairs, pairs, (size_t)n_pairs * 2 * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    // a block walks all N objects of its pair: as many pairs per launch as the pair kernel's budget allows steps
    const int64_t per_launch = tiles_per_launch(h->n_pad / kStep);
    for (int64_t p0 = 0; p0 < n_pairs; p0 += per_launch) {
        k_assoc_table<<<(unsigned)std::min(per_launch, n_pairs - p0), kTableBlock, 0, h->stream>>>(h->d_xt, h->n_pad, h->N, h->d_pairs, p0,
                                                                                               h->s_max, (int32_t*)h->d_out);
        HIPCHK(h, hipGetLastError());
    }
    HIPCHK(h, hipMemcpyAsync(out, h->d_out, (size_t)n_pairs * cells * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return SBE_OK;
}

int sbe_assoc_last_shape(const sbe_assoc* h, int32_t* s_pad_out, int64_t* tile_pairs_out, int64_t* launches_out) {
    CHECK_HANDLE(h, kNullHandle);
    if (!s_pad_out || !tile_pairs_out || !launches_out)
        return fail(h, SBE_ERR_ARG, "null pointer argument: output");
    if (h->F == 0) return fail(h, SBE_ERR_STATE, "no successful sbe_assoc_compute yet");
    *s_pad_out = h->s_pad;
    *tile_pairs_out = h->tile_pairs;
    *launches_out = h->launches;
    return SBE_OK;
}

int sbe_assoc_last_kernel_ms(const sbe_assoc* h, float* ms_out) { return unit_last_kernel_ms(h, ms_out, kNullHandle); }

}  // extern "C"
