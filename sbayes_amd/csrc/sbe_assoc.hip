// sbe_assoc.hip -- on-device screening of all feature pairs for dependence (include/sbe_assoc.h): the chi-squared test of
// independence that sbayes/tools/find_correlated_features.py runs per pair through pd.crosstab and
// scipy.stats.chi2_contingency.  The numerical contract is tests/_assoc_oracle.py; DESIGN.md section 13 has the layout
// and the limits.
//
// With X the one-hot matrix [N][F * S_pad] (S_pad: the next power of two >= the largest state count, so that a 32 x 32
// tile holds (32 / S_pad)^2 whole pairs), all contingency tables at once are X^T X.  k_assoc_pairs computes one 32 x 32
// tile of it per wave, for the tile pairs I <= J:
//   1. the FP4 contraction over objects of sbe_unit_tiles.hip.h (the counts are exact in the f32 accumulator while
//      N <= 2^24).  The operands are built in registers from the feature-major codes [F][N_pad]: a lane owns one one-hot
//      column (feature f, state s) and 32 objects of the step; four byte-parallel operations turn four codes into four
//      "code == s" bits (an NA object, 255, matches no state, and neither does the padding behind N);
//   2. the accumulator tile goes to LDS; margins of every sub-table along both tile axes, then per pair its total, the
//      occupied rows R and columns C, dof = (R-1)(C-1);
//   3. per cell the Pearson term in fp64 (expected r c / n, Yates' correction when dof == 1), into LDS;
//   4. per pair one lane sums its terms in the fixed order (a major, b minor) -- empty rows and columns add +0.0, which
//      changes no bit of a non-negative sum -- and evaluates Q(dof/2, statistic/2); the pair and its mirror are stored.
// No table is written to memory.  k_assoc_table counts one caller-named pair per block with integer atomics in LDS.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "sbe_unit_tiles.hip.h"
#include "../../include/sbe_assoc.h"

namespace {

constexpr int kPad = 256;                            // the codes are padded to whole rounds: a lane reads a byte per object
constexpr int kTableBlock = 256;
constexpr int kSeriesMaxIter = 5000;                 // (the series and the fraction end long before at dof <= 961)
static_assert(kPad == kRoundElems, "a round of codes is a round of the contraction");

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

// four "code == s" bits of four codes: codes are < 32 or 255, s < 32 (or 0x40 for a column behind the last feature, which
// matches nothing).  Masked to six bits an NA code is 63; the xor is zero exactly for a match; adding 0x7f sets bit 7 of
// every non-zero byte without a carry (63 + 127 < 256)
__device__ inline uint32_t match4(uint32_t codes, uint32_t s4) {
    return ~(((codes & 0x3f3f3f3fu) ^ s4) + 0x7f7f7f7fu) & 0x80808080u;
}

// FP4 operand of one lane: 32 objects (32 codes) against the lane's state; 1.0 = 0x2 in e2m1, so a match sets bit 1 of its
// nibble.  Object 8 d + b of the 32 goes to nibble 2 b (b < 4) or 2 (b - 4) + 1 of dword d
__device__ inline v8i fp4_operand(const uint4 lo, const uint4 hi, uint32_t s4) {
    v8i v = {};
    v[0] = (int)((match4(lo.x, s4) >> 6) | (match4(lo.y, s4) >> 2));
    v[1] = (int)((match4(lo.z, s4) >> 6) | (match4(lo.w, s4) >> 2));
    v[2] = (int)((match4(hi.x, s4) >> 6) | (match4(hi.y, s4) >> 2));
    v[3] = (int)((match4(hi.z, s4) >> 6) | (match4(hi.w, s4) >> 2));
    return v;
}

// the codes of one lane for one round of kRound contraction steps: q[2 u], q[2 u + 1] are its 32 objects of step u.  A round's
// loads are issued together, so their latency is paid once per round
struct LaneCodes {
    uint4 q[2 * kRound];
};

__device__ inline LaneCodes load_codes(const uint8_t* p) {
    LaneCodes c;
#pragma unroll
    for (int u = 0; u < kRound; ++u) {
        c.q[2 * u] = *reinterpret_cast<const uint4*>(p + u * kStep);
        c.q[2 * u + 1] = *reinterpret_cast<const uint4*>(p + u * kStep + 16);
    }
    return c;
}

// (at most four waves per SIMD, which the LDS allows anyway: the compiler then keeps a round's sixteen loads in flight instead
// of trading them for registers)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 4))) void k_assoc_pairs(const PairArgs g) {
    // dynamic LDS, pair_lds_bytes(sub): the terms (8 KiB) -- whose first half holds the tile of X^T X until step 3 -- then the
    // margins and the per-pair values, sized by the sub-tables per tile edge, so that four waves fit a SIMD from S_pad = 8 on
    extern __shared__ double assoc_lds[];
    const int S = 1 << g.log_s, sub = kTile >> g.log_s;      // states per feature (padded), features per tile edge
    double (*term)[kTile] = reinterpret_cast<double(*)[kTile]>(assoc_lds);
    float (*cnt)[kTile] = reinterpret_cast<float(*)[kTile]>(assoc_lds);   // rows = columns of tile I, columns = of tile J
    float* rm = reinterpret_cast<float*>(assoc_lds + kTile * kTile);       // [row][q]: sum of the row over the states of column feature q
    float* cm = rm + kTile * sub;                                          // [p][col]: sum of the column over the states of row feature p
    float* pn = cm + kTile * sub;                                          // per sub-table: total
    int* pdof = reinterpret_cast<int*>(pn + sub * sub);                    //                dof (0: not valid)

    const int64_t t = g.t0 + blockIdx.x;
    if (t >= g.t_end) return;
    const TilePair pair = tile_pair(t);
    const int64_t I = pair.I, J = pair.J;
    const int lane = threadIdx.x, half = lane >> 5;

    // ---- 1. the contraction
    auto column = [&](int64_t tile, const uint8_t*& base, uint32_t& s4) {
        const int64_t col = tile * kTile + (lane & 31);
        int64_t f = col >> g.log_s;
        uint32_t s = (uint32_t)(col & (S - 1));
        if (f >= g.F) { f = 0; s = 0x40u; }
        base = g.xt + f * g.n_pad + 32 * half;
        s4 = s * 0x01010101u;
    };
    const uint8_t *pa, *pb;
    uint32_t sa, sb;
    column(I, pa, sa);
    column(J, pb, sb);
    v16f acc = {};
    for (int64_t n0 = 0; n0 < g.n_pad; n0 += kPad) {
        const LaneCodes ca = load_codes(pa + n0), cb = load_codes(pb + n0);
#pragma unroll
        for (int u = 0; u < kRound; ++u) {
            const v8i a = fp4_operand(ca.q[2 * u], ca.q[2 * u + 1], sa);
            const v8i b = fp4_operand(cb.q[2 * u], cb.q[2 * u + 1], sb);
            acc = mfma_fp4(a, b, acc);
        }
    }
    for_acc_entries(acc, half, lane & 31, [&](int row, int col, float v) { cnt[row][col] = v; });
    __syncthreads();

    // ---- 2. margins along both tile axes, then total, R, C and dof per sub-table
    for (int idx = lane; idx < kTile * sub; idx += 64) {
        const int row = idx / sub, q = idx - row * sub;
        float s = 0.f;
        for (int b = 0; b < S; ++b) s += cnt[row][q * S + b];
        rm[row * sub + q] = s;
        const int p = idx / kTile, col = idx - p * kTile;
        s = 0.f;
        for (int a = 0; a < S; ++a) s += cnt[p * S + a][col];
        cm[p * kTile + col] = s;
    }
    __syncthreads();
    for (int idx = lane; idx < sub * sub; idx += 64) {
        const int p = idx / sub, q = idx - p * sub;
        float n = 0.f;
        int R = 0, C = 0;
        for (int a = 0; a < S; ++a) {
            const float r = rm[(p * S + a) * sub + q];
            n += r;
            R += r > 0.f;
            C += cm[p * kTile + q * S + a] > 0.f;
        }
        pn[idx] = n;
        pdof[idx] = (R > 1 && C > 1) ? (R - 1) * (C - 1) : 0;
    }
    __syncthreads();

    // ---- 3. the Pearson terms (each lane takes its 16 counts out of the shared buffer before the terms go in)
    float obs[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) obs[k] = cnt[2 * k + half][lane & 31];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int row = 2 * k + half, col = lane & 31, p = row >> g.log_s, q = col >> g.log_s;
        const float r = rm[row * sub + q], c = cm[p * kTile + col];
        const int dof = pdof[p * sub + q];
        double v = 0.0;
        if (dof > 0 && r > 0.f && c > 0.f) {
            const double o = (double)obs[k];
            const double e = (double)r * (double)c / (double)pn[p * sub + q];
            double oc = o;
            if (dof == 1) {                              // Yates: O + sign(E - O) min(0.5, |E - O|)
                const double d = e - o;
                const double sgn = d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0);
                oc = o + fmin(0.5, fabs(d)) * sgn;
            }
            const double diff = oc - e;
            v = diff * diff / e;
        }
        term[row][col] = v;
    }
    __syncthreads();

    // ---- 4. statistic and p-value per pair; the pair and its mirror
    for (int idx = lane; idx < sub * sub; idx += 64) {
        const int p = idx / sub, q = idx - p * sub;
        const int64_t i = I * sub + p, j = J * sub + q;
        if (i >= j || j >= g.F) continue;                // (i < j: the diagonal tile pairs hold every pair twice)
        const int dof = pdof[idx];
        double stat = 0.0, pv = std::numeric_limits<double>::quiet_NaN();
        if (dof > 0) {
            for (int a = 0; a < S; ++a)
#pragma unroll 4
                for (int b = 0; b < S; b += 2) {           // (S is even; the reads run ahead, the adds keep their order)
                    const double t0 = term[p * S + a][q * S + b], t1 = term[p * S + a][q * S + b + 1];
                    stat += t0;
                    stat += t1;
                }
            pv = assoc_gamma_q(0.5 * (double)dof, 0.5 * stat);
        }
        const int n = (int)pn[idx];
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

inline size_t pair_lds_bytes(int sub) { return (size_t)kTile * kTile * sizeof(double) + (size_t)(2 * kTile * sub + 2 * sub * sub) * 4; }

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
    if (N < 1 || N > SBE_ASSOC_MAX_OBJECTS)
        return fail(h, SBE_ERR_ARG, "n_objects=%lld out of range [1, %d] (2^24: counts are exact in the f32 accumulator up to there)",
                     (long long)N, SBE_ASSOC_MAX_OBJECTS);
    if (F < 1 || F > SBE_ASSOC_MAX_FEATURES)
        return fail(h, SBE_ERR_ARG, "n_features=%lld out of range [1, %d] (the [F][F] outputs take 25 bytes per entry)",
                     (long long)F, SBE_ASSOC_MAX_FEATURES);
    if (N * F > SBE_ASSOC_MAX_CODES)
        return fail(h, SBE_ERR_ARG, "n_objects * n_features = %lld exceeds the limit of %lld (2^31) codes", (long long)(N * F),
                     (long long)SBE_ASSOC_MAX_CODES);
    int s_max = 1;
    for (int64_t f = 0; f < F; ++f) {
        if (n_states[f] < 1 || n_states[f] > SBE_ASSOC_MAX_STATES)
            return fail(h, SBE_ERR_ARG, "n_states[%lld]=%d out of range [1, %d] (this unit's limit: a 32 x 32 tile holds whole pairs)",
                         (long long)f, n_states[f], SBE_ASSOC_MAX_STATES);
        s_max = std::max(s_max, (int)n_states[f]);
    }
    // the codes, checked and turned feature-major, padded to whole rounds of the contraction with NA
    const int64_t n_pad = whole_rounds(N);
    std::vector<uint8_t> xt((size_t)(F * n_pad), (uint8_t)SBE_ASSOC_NA);
    for (int64_t i0 = 0; i0 < N; i0 += kStep) {        // (blocks of objects: the block's rows stay in cache, the writes are contiguous)
        const int64_t i1 = std::min(N, i0 + kStep);
        for (int64_t f = 0; f < F; ++f) {
            const int32_t ns = n_states[f];
            uint8_t* dst = xt.data() + (size_t)(f * n_pad);
            for (int64_t i = i0; i < i1; ++i) {
                const uint8_t c = x[i * F + f];
                if (c != SBE_ASSOC_NA && c >= ns)
                    return fail(h, SBE_ERR_DATA, "x[%lld][%lld]=%d is neither below n_states[%lld]=%d nor %d (not observed)", (long long)i,
                                 (long long)f, (int)c, (long long)f, ns, SBE_ASSOC_NA);
                dst[i] = c;
            }
        }
    }
    int log_s = 1;
    while ((1 << log_s) < s_max) ++log_s;
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
