// sbe_summary.hip -- the posterior summary per column on the device (include/sbe_summary.h): quantiles, the highest-density
// interval, the rank-normalised R-hat and the bulk and tail ESS, beside the diagnostics of sbe_diag.h.  The store, the plan
// of a compute call and the column kernel are those of sbe_diag.hip (sbe_diag_column.hip.h); this file adds the rank kernel,
// the kernel that combines the five passes of the column kernel, and the host side.  The numerical contract is
// tests/_summary_oracle.py; DESIGN.md section 18 has the layout, the scratch budget, ndtri's error count and the limits.
//
// k_summary_rank, one 256-thread workgroup per column (N = M n draws after burn-in, cut and split):
//   1. the N values (x + 0.0: -0 folded into +0) into the sort buffer -- LDS when N <= sbe_diag_lds_max_draws(), else the
//      column's slice of a global scratch -- and the finite check (a non-finite column: NaN everywhere, no sort);
//   2. the ascending sort: a bitonic network whose comparators all point the same way (the first step of every merge pairs
//      i with its mirror image in the block), so slots >= N act as +inf without storage and N need be no power of two.
//      The ascending order of values is unique (no -0 is left), so the network cannot change a bit of what follows;
//   3. the quantiles (the caller's, and 0.05 / 0.5 / 0.95 for the derived columns) and the HDI: a (width, index)
//      lexicographic minimum, per thread over a stride, then over the fixed exchange tree;
//   4. per element in its original position: lower and upper bound in s by binary search, the average rank, z by ndtri;
//      zb, i05 and i95 go to the derived store;
//   5. |x - median| into the same buffer, sorted again, ranked again: zf.
// The derived store is laid out [M][4 C][n] (C: the columns of a launch; 4 c + which), so k_diag_column runs on it
// unchanged with cap = n and off[m] = m 4 C n.  Every loop is bounded by N (the network's by its padded size < 2 N); no
// workgroup waits for another; no float atomics.  A column's results do not depend on its place in a launch or on C.
#include <climits>

#include "sbe_diag_column.hip.h"
#include "../../include/sbe_summary.h"

namespace {

// scratch budget of one launch of the rank kernel: the derived store (4 N doubles per column) and, on the global path,
// the sort buffer (N more).  C, the columns of a launch, is the budget over that, at least 1.
constexpr size_t kSummaryScratchBytes = (size_t)1 << 30;
constexpr int kDerived = 4;                          // zb, zf, i05, i95

struct RankArgs {
    const double* x;          // store: [chains][P][cap]
    const int64_t* off;       // [M] as DiagArgs::off
    int64_t cap;
    int M, n;                 // after the split
    int inc;                  // the HDI's span in sorted draws: floor(hdi_prob N) clipped to [1, N - 1]
    int n_probs;
    double probs[SBE_SUMMARY_MAX_PROBS];
    double* work;             // global path: [columns of the launch][N]; LDS path: null
    double* derived;          // [M][4 C][n]
    int64_t C;
    double* q;                // [n_probs + 2][P]: the quantiles, hdi_lo, hdi_hi (null: not wanted)
    double* rank_out;         // [N] average ranks of the launch's first column (null: not wanted)
    int64_t P, j0;            // columns; first column of this launch
};

// AS 241 (Wichura 1988), PPND16, the two branches that 0.625 / (2^20 + 0.25) <= p <= 1 - that can reach (sqrt(-log p) < 3.79,
// the third branch starts at 5).  All coefficients are positive and both arguments (0.180625 - q^2 and sqrt(-log p) - 1.6)
// are non-negative, so neither Horner sum cancels.  DESIGN.md section 18 counts the roundings: |z_dev - z| <= 40 u max(1, |z|).
__device__ inline double summary_ndtri(double p) {
    const double q = p - 0.5;
    if (fabs(q) <= 0.425) {
        const double r = 0.180625 - q * q;
        const double num = (((((((2.5090809287301226727e+3 * r + 3.3430575583588128105e+4) * r + 6.7265770927008700853e+4) * r +
                                4.5921953931549871457e+4) * r + 1.3731693765509461125e+4) * r + 1.9715909503065514427e+3) * r +
                              1.3314166789178437745e+2) * r + 3.3871328727963666080e+0);
        const double den = (((((((5.2264952788528545610e+3 * r + 2.8729085735721942674e+4) * r + 3.9307895800092710610e+4) * r +
                                2.1213794301586595867e+4) * r + 5.3941960214247511077e+3) * r + 6.8718700749205790830e+2) * r +
                              4.2313330701600911252e+1) * r + 1.0);
        return q * (num / den);
    }
    const double r = sqrt(-log(q <= 0.0 ? p : 1.0 - p)) - 1.6;
    const double num = (((((((7.74545014278341407640e-4 * r + 2.27238449892691845833e-2) * r + 2.41780725177450611770e-1) * r +
                            1.27045825245236838258e+0) * r + 3.64784832476320460504e+0) * r + 5.76949722146069140550e+0) * r +
                          4.63033784615654529590e+0) * r + 1.42343711074968357734e+0);
    const double den = (((((((1.05075007164441684324e-9 * r + 5.47593808499534494600e-4) * r + 1.51986665636164571966e-2) * r +
                            1.48103976427480074590e-1) * r + 6.89767334985100004550e-1) * r + 1.67638483018380384940e+0) * r +
                          2.05319162663775882187e+0) * r + 1.0);
    const double z = num / den;
    return q < 0.0 ? -z : z;
}

__device__ inline void summary_compare_exchange(double* s, int lo, int hi) {
    const double a = s[lo], b = s[hi];
    if (b < a) {
        s[lo] = b;
        s[hi] = a;
    }
}

// s[0 .. N) ascending, by the whole block; ends with a barrier.  Slots N .. pad - 1 are never touched: a comparator whose
// upper slot is one of them would leave the pair as it is.
__device__ inline void summary_block_sort(double* s, int N) {
    const int tid = threadIdx.x;
    int pad = 2;
    while (pad < N) pad <<= 1;                               // (at most 2^20)
    const int pairs = pad >> 1;                              // (< N)
    for (int k = 2; k <= pad; k <<= 1) {
        const int half = k >> 1;
        for (int t = tid; t < pairs; t += kDiagBlock) {      // the merge's first step: slot o of a block with slot k - 1 - o
            const int o = t & (half - 1), base = (t - o) << 1;
            const int hi = base + k - 1 - o;
            if (hi < N) summary_compare_exchange(s, base + o, hi);
        }
        __syncthreads();
        for (int j = half >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < pairs; t += kDiagBlock) {
                const int o = t & (j - 1), lo = ((t - o) << 1) | o;
                if (lo + j < N) summary_compare_exchange(s, lo, lo + j);
            }
            __syncthreads();
        }
    }
}

__device__ inline double summary_quantile(const double* s, int N, double p) {
    const double h = (double)(N - 1) * p;
    const double fk = floor(h);
    const int k = (int)fk;
    const double g = h - fk;
    const double lo = s[k], hi = s[min(k + 1, N - 1)];
    return lo + (hi - lo) * g;
}

// the average rank of v in s: (values below + values at most v + 1) / 2
__device__ inline double summary_rank(const double* s, int N, double v) {
    int lo = 0, len = N;
    while (len > 0) {                                        // lower bound: first slot with s >= v
        const int step = len >> 1;
        if (s[lo + step] < v) { lo += step + 1; len -= step + 1; } else len = step;
    }
    int up = lo;
    len = N - lo;
    while (len > 0) {                                        // upper bound: first slot with s > v
        const int step = len >> 1;
        if (!(v < s[up + step])) { up += step + 1; len -= step + 1; } else len = step;
    }
    return 0.5 * (double)(lo + up + 1);
}

template <bool kLds>
__global__ __launch_bounds__(kDiagBlock) void k_summary_rank(RankArgs a) {
    extern __shared__ __align__(16) unsigned char dyn[];
    __shared__ int ired[kDiagWaves];
    __shared__ double wred[kDiagWaves];
    const int c = blockIdx.x, tid = threadIdx.x;
    const int64_t j = a.j0 + c;
    const int M = a.M, n = a.n, N = M * n;
    double* s = kLds ? reinterpret_cast<double*>(dyn) : a.work + (int64_t)c * N;
    const double* col = a.x + j * a.cap;
    auto derived = [&](int m, int which) { return a.derived + (((int64_t)m * kDerived * a.C + (int64_t)kDerived * c + which) * n); };

    // 1. load, fold -0, finite check (bit 0); does any chain hold two values (bit 1)
    int bad = 0;
    for (int m = 0; m < M; ++m) {
        const double* xm = col + a.off[m];
        const double first = xm[0] + 0.0;
        for (int i = tid; i < n; i += kDiagBlock) {
            const double v = xm[i] + 0.0;
            bad |= (!isfinite(v) ? 1 : 0) | (v != first ? 2 : 0);
            s[m * n + i] = v;
        }
    }
    bad = unit_block_reduce<kDiagWaves>(bad, ired, unit_or{});
    // every chain constant: W = 0, so R-hat is +inf and every rho(t) is 1 whatever the chains' values are.  zb and zf then hold
    // twice the average rank, an integer below 2^22 whose chain sums are exact, and the column kernel sees W = 0 exactly
    const bool flat = !(bad & 2);
    bad &= 1;
    if (bad) {                                               // (uniform over the block)
        if (a.q && tid < a.n_probs + 2) a.q[(int64_t)tid * a.P + j] = NAN;
        for (int m = 0; m < M; ++m)
            for (int w = 0; w < kDerived; ++w) {
                double* dw = derived(m, w);
                for (int i = tid; i < n; i += kDiagBlock) dw[i] = NAN;
            }
        if (a.rank_out && c == 0)
            for (int i = tid; i < N; i += kDiagBlock) a.rank_out[i] = NAN;
        return;
    }

    // 2. sort
    summary_block_sort(s, N);

    // 3. quantiles and the HDI
    if (a.q && tid < a.n_probs) a.q[(int64_t)tid * a.P + j] = summary_quantile(s, N, a.probs[tid]);
    const double q05 = summary_quantile(s, N, 0.05), q50 = summary_quantile(s, N, 0.5), q95 = summary_quantile(s, N, 0.95);
    if (a.q) {                                               // (uniform over the block)
        const int inc = a.inc;
        double bw = INFINITY;
        int bi = INT_MAX;
        for (int i = tid; i < N - inc; i += kDiagBlock) {
            const double w = s[i + inc] - s[i];
            if (w < bw || (w == bw && i < bi)) { bw = w; bi = i; }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const double ow = __shfl_xor(bw, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (ow < bw || (ow == bw && oi < bi)) { bw = ow; bi = oi; }
        }
        if ((tid & 63) == 0) { wred[tid >> 6] = bw; ired[tid >> 6] = bi; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < kDiagWaves; ++w)
                if (wred[w] < bw || (wred[w] == bw && ired[w] < bi)) { bw = wred[w]; bi = ired[w]; }
            a.q[(int64_t)a.n_probs * a.P + j] = s[bi];
            a.q[(int64_t)(a.n_probs + 1) * a.P + j] = s[bi + inc];
        }
    }

    // 4. ranks of the values: zb, and the two indicators
    const double denom = (double)N + 0.25;
    for (int m = 0; m < M; ++m) {
        const double* xm = col + a.off[m];
        double *zb = derived(m, SBE_SUMMARY_DERIVED_ZB), *i05 = derived(m, SBE_SUMMARY_DERIVED_I05), *i95 = derived(m, SBE_SUMMARY_DERIVED_I95);
        for (int i = tid; i < n; i += kDiagBlock) {
            const double v = xm[i] + 0.0;
            const double r = summary_rank(s, N, v);
            zb[i] = flat ? 2.0 * r : summary_ndtri((r - 0.375) / denom);
            i05[i] = v <= q05 ? 1.0 : 0.0;
            i95[i] = v <= q95 ? 1.0 : 0.0;
            if (a.rank_out && c == 0) a.rank_out[m * n + i] = r;
        }
    }
    __syncthreads();                                         // (every read of s is done)

    // 5. |x - median|: its own sort, its own ranks: zf
    for (int m = 0; m < M; ++m) {
        const double* xm = col + a.off[m];
        for (int i = tid; i < n; i += kDiagBlock) s[m * n + i] = fabs((xm[i] + 0.0) - q50);
    }
    __syncthreads();
    summary_block_sort(s, N);
    for (int m = 0; m < M; ++m) {
        const double* xm = col + a.off[m];
        double* zf = derived(m, SBE_SUMMARY_DERIVED_ZF);
        for (int i = tid; i < n; i += kDiagBlock) {
            const double r = summary_rank(s, N, fabs((xm[i] + 0.0) - q50));
            zf[i] = flat ? 2.0 * r : summary_ndtri((r - 0.375) / denom);
        }
    }
}

// The five passes of the column kernel into the outputs of `count` columns from j0: dout / dflag hold the derived
// columns' results ([5][4 C] and [4 C], 4 c + which), flag the store's own (updated in place).
__global__ __launch_bounds__(kDiagBlock) void k_summary_combine(const double* dout, const uint8_t* dflag, int64_t C, int64_t count, int64_t j0,
                                                                int64_t P, double total, double* sum, uint8_t* flag) {
    const int64_t c = (int64_t)blockIdx.x * kDiagBlock + threadIdx.x;
    if (c >= count) return;
    const int64_t j = j0 + c, D = kDerived * C;
    const double* ess = dout + 2 * D + kDerived * c;
    const double* rhat = dout + 3 * D + kDerived * c;
    const uint8_t own = flag[j];
    double ess_bulk = ess[SBE_SUMMARY_DERIVED_ZB];
    double ess_tail = fmin(ess[SBE_SUMMARY_DERIVED_I05], ess[SBE_SUMMARY_DERIVED_I95]);
    double rhat_rank = fmax(rhat[SBE_SUMMARY_DERIVED_ZB], rhat[SBE_SUMMARY_DERIVED_ZF]);      // (fmax: a NaN side is ignored)
    int truncated = 0;
    for (int w = 0; w < kDerived; ++w) truncated |= dflag[kDerived * c + w] & SBE_DIAG_FLAG_TRUNCATED;
    if (own & SBE_DIAG_FLAG_NONFINITE) {
        ess_bulk = ess_tail = rhat_rank = NAN;
        truncated = 0;
    } else if (own & SBE_DIAG_FLAG_CONSTANT) {
        ess_bulk = ess_tail = total;
        rhat_rank = NAN;
        truncated = 0;
    }
    sum[j] = ess_bulk;
    sum[P + j] = ess_tail;
    sum[2 * P + j] = rhat_rank;
    flag[j] = (uint8_t)(own | truncated);
}

}  // namespace

struct sbe_summary : sbe_unit_handle, diag_store {   // (sbe_unit.hip.h, sbe_diag_column.hip.h)
    double* d_out = nullptr;            // [5][P]: the store's own pass
    size_t out_bytes = 0;
    int32_t* d_lags = nullptr;          // [P]
    size_t lags_bytes = 0;
    uint8_t* d_flag = nullptr;          // [P]
    size_t flag_bytes = 0;
    double* d_q = nullptr;              // [SBE_SUMMARY_MAX_PROBS + 2][P]
    size_t q_bytes = 0;
    double* d_sum = nullptr;            // [3][P]: ess_bulk, ess_tail, rhat_rank
    size_t sum_bytes = 0;
    double* d_derived = nullptr;        // [M][4 C][n]
    size_t derived_bytes = 0;
    double* d_work = nullptr;           // global path: [C][N]
    size_t work_bytes = 0;
    double* d_dout = nullptr;           // [5][4 C]
    size_t dout_bytes = 0;
    int32_t* d_dlags = nullptr;         // [4 C]
    size_t dlags_bytes = 0;
    uint8_t* d_dflag = nullptr;         // [4 C]
    size_t dflag_bytes = 0;
    int64_t* d_doff = nullptr;          // [kMaxSplitChains]: the chains' offsets in the derived store
    double* d_rank = nullptr;           // [N] (sbe_summary_derived_column)
    size_t rank_bytes = 0;
    std::vector<hipEvent_t> marks;      // between the kernels of a compute call
    int64_t launch_columns = 0;         // 0: the default
    float last_ms[2] = {0.0f, 0.0f};
    bool last_valid = false;            // the store, d_off and the sizes below are those of the last compute call
    int last_M = 0, last_path = 0, last_inc = 1;
    int64_t last_n = 0, last_launches = 0, last_C = 0;
    std::vector<void*> buffers() const {
        return {d_x, d_stage, d_off, d_scratch, d_out, d_lags, d_flag, d_q, d_sum, d_derived, d_work, d_dout, d_dlags, d_dflag, d_doff, d_rank};
    }
};

namespace {

constexpr char kNullHandle[] = "null handle";
constexpr char kReset[] = "sbe_summary_reset";

// columns per launch of the rank kernel: the caller's (0: what the budget holds), at most what the budget holds, at most P
int64_t summary_launch_columns(int64_t wanted, int64_t N, bool lds, int64_t P) {
    const size_t per_column = (size_t)(kDerived + (lds ? 0 : 1)) * (size_t)N * sizeof(double);
    int64_t C = std::max<int64_t>(1, (int64_t)(kSummaryScratchBytes / per_column));
    C = std::min(C, kMaxGridBlocks / kDerived);
    if (wanted) C = std::min(C, wanted);
    return std::min(C, P);
}

int summary_launch_rank(sbe_summary* h, const RankArgs& args, bool lds, int64_t count) {
    const size_t bytes = lds ? (size_t)args.M * (size_t)args.n * sizeof(double) : 0;
    if (lds)
        k_summary_rank<true><<<(unsigned)count, kDiagBlock, bytes, h->stream>>>(args);
    else
        k_summary_rank<false><<<(unsigned)count, kDiagBlock, 0, h->stream>>>(args);
    HIPCHK(h, hipGetLastError());
    return SBE_OK;
}

}  // namespace

extern "C" {

int sbe_summary_abi_version(void) { return SBE_SUMMARY_ABI_VERSION; }

const char* sbe_summary_last_error(const sbe_summary* h) { return unit_last_error(h); }

int sbe_summary_create(sbe_summary** out, int device) { return unit_create_on_device(out, device, "sbe_summary_create"); }

int sbe_summary_destroy(sbe_summary* h) {
    CHECK_HANDLE(h, kNullHandle);
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (hipEvent_t ev : h->marks) (void)hipEventDestroy(ev);
    h->marks.clear();
    return unit_destroy(h, kNullHandle);
}

int sbe_summary_last_kernel_ms(const sbe_summary* h, float* ms_out) {
    CHECK_HANDLE(h, kNullHandle);
    if (!ms_out) return fail(h, SBE_ERR_ARG, "null pointer argument: ms_out");
    ms_out[0] = h->last_ms[0];
    ms_out[1] = h->last_ms[1];
    return SBE_OK;
}

int sbe_summary_set_launch_columns(sbe_summary* h, int64_t columns) {
    CHECK_HANDLE(h, kNullHandle);
    if (columns < 0 || columns > kMaxGridBlocks)
        return fail(h, SBE_ERR_ARG, "columns=%lld out of range [0, %lld] (0: the default)", (long long)columns, (long long)kMaxGridBlocks);
    h->launch_columns = columns;
    return SBE_OK;
}

int sbe_summary_reset(sbe_summary* h, int n_chains, int64_t n_columns, int64_t capacity_rows) {
    CHECK_HANDLE(h, kNullHandle);
    h->last_valid = false;
    int rc = diag_store_reset(h, n_chains, n_columns, capacity_rows);
    const size_t P = (size_t)n_columns;
    if (!rc) rc = unit_ensure(h, h->d_out, h->out_bytes, P * 5 * sizeof(double));
    if (!rc) rc = unit_ensure(h, h->d_lags, h->lags_bytes, P * sizeof(int32_t));
    if (!rc) rc = unit_ensure(h, h->d_flag, h->flag_bytes, P);
    if (!rc) rc = unit_ensure(h, h->d_q, h->q_bytes, P * (SBE_SUMMARY_MAX_PROBS + 2) * sizeof(double));
    if (!rc) rc = unit_ensure(h, h->d_sum, h->sum_bytes, P * 3 * sizeof(double));
    if (!rc) rc = unit_ensure(h, h->d_doff, (size_t)kMaxSplitChains * sizeof(int64_t));
    if (rc) return rc;
    diag_store_shaped(h, n_chains, n_columns, capacity_rows);
    return SBE_OK;
}

int sbe_summary_rows(const sbe_summary* h, int chain, int64_t* n_rows_out) {
    CHECK_HANDLE(h, kNullHandle);
    return h->chains.get(h, kDiagLane, chain, n_rows_out);
}

int sbe_summary_append_rows(sbe_summary* h, int chain, const double* rows, int64_t n_rows) {
    CHECK_HANDLE(h, kNullHandle);
    return diag_store_append(h, kReset, chain, rows, n_rows);
}

int sbe_summary_compute(sbe_summary* h, const int64_t* burn_rows, int split, int64_t max_lag, int n_probs, const double* probs,
                        double hdi_prob, double* quantiles_out, double* hdi_lo_out, double* hdi_hi_out, double* ess_bulk_out,
                        double* ess_tail_out, double* rhat_rank_out, double* mean_out, double* sd_out, double* ess_out,
                        double* rhat_out, double* mcse_mean_out, int32_t* n_lags_out, uint8_t* flag_out) {
    CHECK_HANDLE(h, kNullHandle);
    if (const int rc = h->chains.check_shaped(h, kReset)) return rc;
    if (!burn_rows) return fail(h, SBE_ERR_ARG, "null pointer argument: burn_rows");
    if (n_probs < 0 || n_probs > SBE_SUMMARY_MAX_PROBS)
        return fail(h, SBE_ERR_ARG, "n_probs=%d out of range [0, %d]", n_probs, SBE_SUMMARY_MAX_PROBS);
    if (n_probs > 0 && !probs) return fail(h, SBE_ERR_ARG, "null pointer argument: probs");
    for (int q = 0; q < n_probs; ++q)
        if (!(probs[q] >= 0.0 && probs[q] <= 1.0)) return fail(h, SBE_ERR_ARG, "probs[%d]=%g out of range [0, 1]", q, probs[q]);
    if (!(hdi_prob > 0.0 && hdi_prob < 1.0)) return fail(h, SBE_ERR_ARG, "hdi_prob=%g out of range (0, 1)", hdi_prob);
    if ((n_probs > 0 && !quantiles_out) || !hdi_lo_out || !hdi_hi_out || !ess_bulk_out || !ess_tail_out || !rhat_rank_out || !mean_out ||
        !sd_out || !ess_out || !rhat_out || !mcse_mean_out || !n_lags_out || !flag_out)
        return fail(h, SBE_ERR_ARG, "null pointer argument: output");
    int M = 0;
    int64_t n = 0;
    std::vector<int64_t> off;
    if (const int rc = diag_plan(h, kReset, burn_rows, split, max_lag, &M, &n, &off)) return rc;
    h->last_valid = false;
    const int64_t N = (int64_t)M * n, P = h->P;
    const int inc = (int)std::min<double>((double)(N - 1), std::max(1.0, std::floor(hdi_prob * (double)N)));
    const bool lds = diag_staged(M, n);
    const int64_t C = summary_launch_columns(h->launch_columns, N, lds, P);
    const int64_t D = kDerived * C;
    const int64_t per_launch = diag_per_launch(h->launch_columns, M, n, P);    // the store's own pass
    const int64_t per_launch_d = diag_per_launch(0, M, n, D);                  // the derived store's
    std::vector<int64_t> doff((size_t)M);
    for (int m = 0; m < M; ++m) doff[(size_t)m] = (int64_t)m * D * n;

    HIPCHK(h, hipSetDevice(h->device));
    int rc = diag_prepare_launch(h, M, n, std::max(per_launch, per_launch_d));
    if (!rc) rc = unit_ensure(h, h->d_derived, h->derived_bytes, (size_t)D * (size_t)N * sizeof(double));
    if (!rc && !lds) rc = unit_ensure(h, h->d_work, h->work_bytes, (size_t)C * (size_t)N * sizeof(double));
    if (!rc) rc = unit_ensure(h, h->d_dout, h->dout_bytes, (size_t)D * 5 * sizeof(double));
    if (!rc) rc = unit_ensure(h, h->d_dlags, h->dlags_bytes, (size_t)D * sizeof(int32_t));
    if (!rc) rc = unit_ensure(h, h->d_dflag, h->dflag_bytes, (size_t)D);
    if (rc) return rc;
    if (lds)
        HIPCHK(h, hipFuncSetAttribute((const void*)k_summary_rank<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kLdsBudget - kStaticLds)));
    const int64_t chunks = (P + C - 1) / C;
    while ((int64_t)h->marks.size() < 2 + 2 * chunks) {
        hipEvent_t ev = nullptr;
        HIPCHK(h, hipEventCreate(&ev));
        h->marks.push_back(ev);
    }
    HIPCHK(h, hipMemcpyAsync(h->d_off, off.data(), (size_t)M * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_doff, doff.data(), (size_t)M * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));

    RankArgs ra{};
    ra.x = h->d_x;
    ra.off = h->d_off;
    ra.cap = h->chains.cap;
    ra.M = M;
    ra.n = (int)n;
    ra.inc = inc;
    ra.n_probs = n_probs;
    for (int q = 0; q < n_probs; ++q) ra.probs[q] = probs[q];
    ra.work = lds ? nullptr : h->d_work;
    ra.derived = h->d_derived;
    ra.C = C;
    ra.q = h->d_q;
    ra.rank_out = nullptr;
    ra.P = P;

    int64_t launches = 0, column_launches = 0;
    size_t mark = 0;
    HIPCHK(h, hipEventRecord(h->marks[mark++], h->stream));
    rc = diag_launch_columns(h, h->d_x, h->d_off, h->chains.cap, M, n, max_lag, h->d_out, h->d_lags, h->d_flag, P, P, per_launch, &column_launches);
    if (rc) return rc;
    HIPCHK(h, hipEventRecord(h->marks[mark++], h->stream));
    for (int64_t j0 = 0; j0 < P; j0 += C, ++launches) {
        const int64_t count = std::min(C, P - j0);
        ra.j0 = j0;
        if ((rc = summary_launch_rank(h, ra, lds, count))) return rc;
        HIPCHK(h, hipEventRecord(h->marks[mark++], h->stream));
        rc = diag_launch_columns(h, h->d_derived, h->d_doff, n, M, n, max_lag, h->d_dout, h->d_dlags, h->d_dflag, D, kDerived * count,
                                 per_launch_d, &column_launches);
        if (rc) return rc;
        k_summary_combine<<<(unsigned)div_up(count, kDiagBlock), kDiagBlock, 0, h->stream>>>(h->d_dout, h->d_dflag, C, count, j0, P, (double)N, h->d_sum,
                                                                                             h->d_flag);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipEventRecord(h->marks[mark++], h->stream));
    }
    const size_t Pz = (size_t)P;
    if (n_probs > 0) HIPCHK(h, hipMemcpyAsync(quantiles_out, h->d_q, Pz * (size_t)n_probs * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    rc = unit_copy_back(h, (const double*)(h->d_q + Pz * (size_t)n_probs), Pz, {hdi_lo_out, hdi_hi_out});
    if (!rc) rc = unit_copy_back(h, (const double*)h->d_sum, Pz, {ess_bulk_out, ess_tail_out, rhat_rank_out});
    if (!rc) rc = unit_copy_back(h, (const double*)h->d_out, Pz, {mean_out, sd_out, ess_out, rhat_out, mcse_mean_out});
    if (!rc) rc = unit_copy_back(h, (const int32_t*)h->d_lags, Pz, {n_lags_out});
    if (!rc) rc = unit_copy_back(h, (const uint8_t*)h->d_flag, Pz, {flag_out});
    if (rc) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    float rank_ms = 0.0f, column_ms = 0.0f, ms = 0.0f;
    HIPCHK(h, hipEventElapsedTime(&column_ms, h->marks[0], h->marks[1]));
    for (size_t k = 1; k + 2 < mark; k += 2) {           // marks: start, the store's pass, then per launch: rank, columns
        HIPCHK(h, hipEventElapsedTime(&ms, h->marks[k], h->marks[k + 1]));
        rank_ms += ms;
        HIPCHK(h, hipEventElapsedTime(&ms, h->marks[k + 1], h->marks[k + 2]));
        column_ms += ms;
    }
    h->last_ms[0] = rank_ms;
    h->last_ms[1] = column_ms;
    h->last_kernel_ms = rank_ms + column_ms;
    h->last_M = M;
    h->last_n = n;
    h->last_inc = inc;
    h->last_path = lds ? SBE_DIAG_PATH_LDS : SBE_DIAG_PATH_GLOBAL;
    h->last_launches = launches;
    h->last_C = C;
    h->last_valid = true;
    return SBE_OK;
}

int sbe_summary_last_shape(const sbe_summary* h, int* chains_out, int64_t* draws_out, int* path_out, int64_t* launches_out,
                           int64_t* launch_columns_out) {
    CHECK_HANDLE(h, kNullHandle);
    if (!chains_out || !draws_out || !path_out || !launches_out || !launch_columns_out) return fail(h, SBE_ERR_ARG, "null pointer argument: output");
    *chains_out = h->last_M;
    *draws_out = h->last_n;
    *path_out = h->last_path;
    *launches_out = h->last_launches;
    *launch_columns_out = h->last_C;
    return SBE_OK;
}

int sbe_summary_derived_column(sbe_summary* h, int64_t column, int which, double* out) {
    CHECK_HANDLE(h, kNullHandle);
    if (!h->last_valid) return fail(h, SBE_ERR_STATE, "no compute call since the store was shaped (sbe_summary_compute)");
    if (column < 0 || column >= h->P) return fail(h, SBE_ERR_ARG, "column %lld out of range [0,%lld)", (long long)column, (long long)h->P);
    if (which < 0 || which > SBE_SUMMARY_DERIVED_RANK) return fail(h, SBE_ERR_ARG, "which=%d out of range [0, %d]", which, SBE_SUMMARY_DERIVED_RANK);
    if (!out) return fail(h, SBE_ERR_ARG, "null pointer argument: out");
    const int M = h->last_M;
    const int64_t n = h->last_n, N = (int64_t)M * n;
    const bool lds = h->last_path == SBE_DIAG_PATH_LDS;
    HIPCHK(h, hipSetDevice(h->device));
    if (const int rc = unit_ensure(h, h->d_rank, h->rank_bytes, (size_t)N * sizeof(double))) return rc;
    RankArgs ra{};
    ra.x = h->d_x;
    ra.off = h->d_off;
    ra.cap = h->chains.cap;
    ra.M = M;
    ra.n = (int)n;
    ra.inc = h->last_inc;
    ra.n_probs = 0;
    ra.work = lds ? nullptr : h->d_work;
    ra.derived = h->d_derived;
    ra.C = h->last_C;
    ra.q = nullptr;
    ra.rank_out = h->d_rank;
    ra.P = h->P;
    ra.j0 = column;
    if (const int rc = summary_launch_rank(h, ra, lds, 1)) return rc;
    if (which == SBE_SUMMARY_DERIVED_RANK) {
        HIPCHK(h, hipMemcpyAsync(out, h->d_rank, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    } else {
        for (int m = 0; m < M; ++m)
            HIPCHK(h, hipMemcpyAsync(out + (int64_t)m * n, h->d_derived + ((int64_t)m * kDerived * h->last_C + which) * n, (size_t)n * sizeof(double),
                                     hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return SBE_OK;
}

}  // extern "C"
