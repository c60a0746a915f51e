// sbe_psens.hip -- the power-scaling sensitivity of every logged column on the device (include/sbe_psens.h): PSIS weights of
// a logged component raised to a power near 1, and per (weight vector, column) the sums of the cumulative Jensen-Shannon
// distance between the weighted and the unweighted empirical cdf.  The store is that of sbe_diag.hip (sbe_diag_column.hip.h);
// this file adds the plan (no cut, no split: the chains' kept draws stacked), the sort of (value, sample) keys, the two
// kernels and the host side.  The numerical contract is tests/_psens_oracle.py; DESIGN.md section 28 has the layout, the
// stated order of the prefix sum, the error bound and the limits.
//
// psens_block_sort: sbe_psis_ratio.hip.h's bitonic network over keys of 12 bytes, a float64 value and an int32 sample index,
// held as two arrays; the order is lexicographic, so it is unique and equals a stable argsort of the values (the header has
// the PSIS steps too, which the leave-one-object-out unit shares).  Both kernels keep the keys in LDS when
// N <= sbe_psens_lds_max_draws(), else in their slice of a global scratch: the same code, the same comparisons.
//
// k_psens_weights, one 256-thread workgroup per weight vector: ratios (alpha - 1) x of the component's column, their maximum
// subtracted, sorted with their samples; the tail (strictly above the cutoff: a suffix of the sort), _gpdfit and _gpinv in
// float64 as sbe_psis_column.hip.h has them for float32 likelihoods, the truncation at 0, logsumexp and the weights
// scattered to their samples.
//
// k_psens_column, one 256-thread workgroup per column: load (x + 0.0), finite check and min / max, sort; then per vector and
// per direction (x, and -x read from the same sort backwards) two walks of the thread's chunk of ceil(N / 256) consecutive
// sorted draws: the chunk's total of q, a sequential scan of the 256 totals by one thread, and the walk that forms Q_i, the
// integrals' terms with three log2 each and the moments.  Every loop is bounded by N (the network's by its padded size
// < 2 N); no workgroup waits for another; no float atomics.  A column's results do not depend on its place in a launch, on
// the columns of a launch, on the path or on how the store was filled.
#include <climits>

#include "sbe_diag_column.hip.h"
#include "sbe_psis_ratio.hip.h"
#include "../../include/sbe_psens.h"

namespace {

constexpr size_t kPsensStaticLds = 8192;             // headroom for the kernels' static LDS (the scan's totals, the fit, reductions)
constexpr int kPsensKeyBytes = kRatioKeyBytes;
constexpr int64_t kPsensLdsMaxDraws = (int64_t)((kLdsBudget - kPsensStaticLds) / kPsensKeyBytes);
constexpr size_t kPsensScratchBytes = (size_t)256 << 20;   // the sort keys of one launch on the global path
constexpr int kPsensMaxTail = kRatioMaxTail;
constexpr int kPsensOutputs = 6;                     // js, bound, js_neg, bound_neg, wmean, wsd
constexpr int kStartAt = SBE_DIAG_MAX_CHAINS;        // plan[kStartAt + m]: chain m's first place in the stack; [kStartAt + M] = N
constexpr int kPlanLength = 2 * SBE_DIAG_MAX_CHAINS + 1;
constexpr double kHalfInvLn2 = 0.7213475204444817;   // 0.5 / ln 2
static_assert(kDiagBlock == kRatioBlock, "the shared PSIS steps run in the unit's workgroup");
constexpr int64_t kMaxProbe = (int64_t)1 << 24;

using PsensKeys = RatioKeys;                         // (value, sample) keys and their sort: sbe_psis_ratio.hip.h

__device__ inline void psens_block_sort(PsensKeys s, int N) { ratio_block_sort(s, N); }

template <bool kLds>
__device__ inline PsensKeys psens_keys(unsigned char* dyn, double* work_val, int32_t* work_idx, int N) {
    if (kLds) return {reinterpret_cast<double*>(dyn), reinterpret_cast<int32_t*>(dyn + (size_t)N * sizeof(double))};
    return {work_val + (int64_t)blockIdx.x * N, work_idx + (int64_t)blockIdx.x * N};
}

// f(place in the stack, value) for every kept draw of a column, the block's threads striding over each chain
template <class F>
__device__ inline void psens_for_draws(const double* col, const int64_t* off, int M, F f) {
    for (int m = 0; m < M; ++m) {
        const double* xm = col + off[m];
        const int s0 = (int)off[kStartAt + m], n = (int)off[kStartAt + m + 1] - s0;
        for (int i = threadIdx.x; i < n; i += kDiagBlock) f(s0 + i, xm[i]);
    }
}

// ---- the weights ---------------------------------------------------------------------------------------------------------
struct WeightArgs {
    const double* x;          // store: [chains][P][cap]
    const int64_t* off;       // [M] chain m's first kept draw within column 0; [kStartAt + m]: its place in the stack
    int64_t cap;
    int M, N, tail_n;
    int64_t column[SBE_PSENS_MAX_VECTORS];
    double scale[SBE_PSENS_MAX_VECTORS];                     // alpha - 1
    double* work_val;         // global path: [V][N]
    int32_t* work_idx;
    double* ary;              // [V][kPsensMaxTail]: the tail's exceedances
    double* w;                // [V][N]
    double* k_out;            // [V]
    double* ess_out;          // [V]
    uint8_t* vflag;           // [V]
    int* bad;                 // [V]
};

template <bool kLds>
__global__ __launch_bounds__(kDiagBlock) void k_psens_weights(WeightArgs a) {
    extern __shared__ __align__(16) unsigned char dyn[];
    __shared__ RatioScratch sc;
    const int v = blockIdx.x, tid = threadIdx.x, N = a.N;
    const PsensKeys s = psens_keys<kLds>(dyn, a.work_val, a.work_idx, N);
    const double* col = a.x + a.column[v] * a.cap;
    const double scale = a.scale[v];
    double* w = a.w + (int64_t)v * N;
    double* ary = a.ary + (int64_t)v * kPsensMaxTail;

    // 1. the ratios: finite check, max and min
    int bad = 0;
    double hi = -INFINITY, nlo = -INFINITY;
    psens_for_draws(col, a.off, a.M, [&](int, double x) {
        const double r = scale * x;
        bad |= !isfinite(r);
        hi = fmax(hi, r);
        nlo = fmax(nlo, -r);
    });
    bad = unit_block_reduce<kDiagWaves>(bad, sc.ired, unit_or{});
    if (bad) {                                               // (uniform over the block)
        if (tid == 0) a.bad[v] = 1;
        return;
    }
    hi = unit_block_reduce<kDiagWaves>(hi, sc.red, unit_max{});
    nlo = unit_block_reduce<kDiagWaves>(nlo, sc.red, unit_max{});
    if (hi + nlo == 0.0) {                                   // max - min == 0: uniform weights
        const double u = 1.0 / (double)N;
        for (int i = tid; i < N; i += kDiagBlock) w[i] = u;
        if (tid == 0) {
            a.bad[v] = 0;
            a.k_out[v] = INFINITY;
            a.ess_out[v] = (double)N;
            a.vflag[v] = SBE_PSENS_VFLAG_CONSTANT;
        }
        return;
    }

    // 2. x = ratio - max with its sample, sorted
    psens_for_draws(col, a.off, a.M, [&](int k, double x) {
        s.val[k] = scale * x - hi;
        s.idx[k] = k;
    });
    __syncthreads();
    psens_block_sort(s, N);

    // 3 - 5. the cutoff, the tail, _gpdfit, _gpinv and the truncation at 0; 6. logsumexp, the weights to their samples, ess
    // (a NaN in the tail makes every weight NaN, as the checker's does): sbe_psis_ratio.hip.h
    const double k_hat = ratio_smooth_tail(s, N, a.tail_n, ary, sc);
    const double lse = ratio_logsumexp(s, N, sc);
    double sumsq = 0.0;
    for (int p = tid; p < N; p += kDiagBlock) {
        const double wp = exp(s.val[p] - lse);
        w[s.idx[p]] = wp;
        sumsq += wp * wp;
    }
    sumsq = unit_block_reduce<kDiagWaves>(sumsq, sc.red, unit_sum{});
    if (tid == 0) {
        a.bad[v] = 0;
        a.k_out[v] = k_hat;
        a.ess_out[v] = 1.0 / sumsq;
        a.vflag[v] = k_hat > 0.7 ? SBE_PSENS_VFLAG_UNRELIABLE : 0;
    }
}

// the caller's weights: bad[v] = 1 for a negative or non-finite entry, 2 for a sum that is not positive
__global__ __launch_bounds__(kDiagBlock) void k_psens_check_weights(const double* w, int N, int* bad_out, uint8_t* vflag) {
    __shared__ double red[kDiagWaves];
    __shared__ int ired[kDiagWaves];
    const int v = blockIdx.x;
    const double* wv = w + (int64_t)v * N;
    int bad = 0;
    double sum = 0.0;
    for (int i = threadIdx.x; i < N; i += kDiagBlock) {
        const double q = wv[i];
        bad |= !(q >= 0.0 && isfinite(q));
        sum += q;
    }
    bad = unit_block_reduce<kDiagWaves>(bad, ired, unit_or{});
    sum = unit_block_reduce<kDiagWaves>(sum, red, unit_sum{});
    if (threadIdx.x == 0) {
        bad_out[v] = bad ? 1 : (sum > 0.0 && isfinite(sum) ? 0 : 2);
        vflag[v] = 0;
    }
}

// ---- the columns ---------------------------------------------------------------------------------------------------------
struct ColumnArgs {
    const double* x;          // store: [chains][P][cap]
    const int64_t* off;       // as WeightArgs::off
    int64_t cap;
    int M, N, V;
    const double* w;          // [V][N]
    const uint8_t* vflag;     // [V]
    double* work_val;         // global path: [columns of the launch][N]
    int32_t* work_idx;
    double* out;              // [kPsensOutputs][V][P]
    uint8_t* flag;            // [P]
    double* sorted_val;       // sbe_psens_sorted_column: [N] each (null: a compute call)
    int32_t* sorted_idx;
    int64_t P, j0;            // columns; first column of this launch
};

struct PsensScan {
    double tot[kDiagBlock];   // the chunks' totals of q
    double base[kDiagBlock];  // the totals before each chunk, added in sequence
    double total;
    double red[kDiagWaves];
};

struct PsensSums {
    double js, bound, wmean, wsd;
};

// One vector in one direction (kNeg: -x, the sort read backwards), by the whole block; every thread ends with the sums.
// Element k of the direction is sorted place N - 1 - k or k.  `uniform`: q = 1 (a vector of equal weights).  The moments
// are formed on the way forward only.
template <bool kNeg>
__device__ inline PsensSums psens_pass(PsensKeys s, int N, const double* wv, bool uniform, PsensScan& sc) {
    const int tid = threadIdx.x;
    const int len = (N + kDiagBlock - 1) / kDiagBlock;
    const int k0 = min(tid * len, N), k1 = min(k0 + len, N);
    auto value = [&](int k) { return kNeg ? -s.val[N - 1 - k] : s.val[k]; };
    auto weight = [&](int k) { return uniform ? 1.0 : wv[s.idx[kNeg ? N - 1 - k : k]]; };

    double tot = 0.0;
    for (int k = k0; k < k1; ++k) tot += weight(k);
    __syncthreads();                                         // (the previous pass has read sc)
    sc.tot[tid] = tot;
    __syncthreads();
    if (tid == 0) {
        double run = 0.0;
        for (int t = 0; t < kDiagBlock; ++t) {
            sc.base[t] = run;
            run += sc.tot[t];
        }
        sc.total = run;
    }
    __syncthreads();
    const double total = sc.total, base = sc.base[tid], dn = (double)N;

    double run = 0.0, pint = 0.0, qint = 0.0, spq = 0.0, sqp = 0.0, mom = 0.0;
    for (int k = k0; k < k1; ++k) {
        const double q = weight(k), sk = value(k);
        run += q;
        if (!kNeg) mom += q * sk;
        if (k < N - 1) {
            const double Q = (base + run) / total, P = (double)(k + 1) / dn, M = 0.5 * (P + Q);
            const double b = value(k + 1) - sk;
            const double l2m = log2(M), l2p = log2(P), l2q = Q > 0.0 ? log2(Q) : 0.0;
            const double bp = b * P, bq = b * Q;
            pint += bp;
            qint += bq;
            spq += bp * (l2p - l2m);
            sqp += bq * (l2q - l2m);
        }
    }
    pint = unit_block_reduce<kDiagWaves>(pint, sc.red, unit_sum{});
    qint = unit_block_reduce<kDiagWaves>(qint, sc.red, unit_sum{});
    spq = unit_block_reduce<kDiagWaves>(spq, sc.red, unit_sum{});
    sqp = unit_block_reduce<kDiagWaves>(sqp, sc.red, unit_sum{});
    double pq = spq + kHalfInvLn2 * (qint - pint), qp = sqp + kHalfInvLn2 * (pint - qint);
    if (pq < 0.0) pq = 0.0;
    if (qp < 0.0) qp = 0.0;
    PsensSums r{pq + qp, pint + qint, 0.0, 0.0};
    if (!kNeg) {
        r.wmean = unit_block_reduce<kDiagWaves>(mom, sc.red, unit_sum{}) / total;
        double var = 0.0;
        for (int k = k0; k < k1; ++k) {
            const double d = value(k) - r.wmean;
            var += weight(k) * (d * d);
        }
        r.wsd = sqrt(unit_block_reduce<kDiagWaves>(var, sc.red, unit_sum{}) / total);
    }
    return r;
}

template <bool kLds>
__global__ __launch_bounds__(kDiagBlock) void k_psens_column(ColumnArgs a) {
    extern __shared__ __align__(16) unsigned char dyn[];
    __shared__ PsensScan sc;
    __shared__ int ired[kDiagWaves];
    const int tid = threadIdx.x, N = a.N, V = a.V;
    const int64_t j = a.j0 + blockIdx.x, P = a.P;
    const PsensKeys s = psens_keys<kLds>(dyn, a.work_val, a.work_idx, N);
    const double* col = a.x + j * a.cap;
    auto out = [&](int which, int v) -> double& { return a.out[((int64_t)which * V + v) * P + j]; };

    // 1. load, fold -0, finite check, min / max
    int bad = 0;
    double lo = INFINITY, nhi = INFINITY;                    // nhi: min of -x
    psens_for_draws(col, a.off, a.M, [&](int k, double x) {
        const double v = x + 0.0;
        bad |= !isfinite(v);
        lo = fmin(lo, v);
        nhi = fmin(nhi, -v);
        s.val[k] = v;
        s.idx[k] = k;
    });
    bad = unit_block_reduce<kDiagWaves>(bad, ired, unit_or{});
    if (bad) {                                               // (uniform over the block)
        if (a.sorted_val) {
            for (int i = tid; i < N; i += kDiagBlock) { a.sorted_val[i] = NAN; a.sorted_idx[i] = -1; }
            return;
        }
        for (int t = tid; t < kPsensOutputs * V; t += kDiagBlock) out(t / V, t % V) = NAN;
        if (tid == 0) a.flag[j] = SBE_DIAG_FLAG_NONFINITE;
        return;
    }
    lo = unit_block_reduce<kDiagWaves>(lo, sc.red, unit_min{});
    nhi = unit_block_reduce<kDiagWaves>(nhi, sc.red, unit_min{});
    const bool constant = (-nhi) - lo < 1e-15;

    // 2. sort
    psens_block_sort(s, N);
    if (a.sorted_val) {                                      // (uniform over the block)
        for (int i = tid; i < N; i += kDiagBlock) { a.sorted_val[i] = s.val[i]; a.sorted_idx[i] = s.idx[i]; }
        return;
    }

    // 3. per vector: the sums of x and of -x, the moments
    for (int v = 0; v < V; ++v) {
        const double* wv = a.w + (int64_t)v * N;
        const bool uniform = (a.vflag[v] & SBE_PSENS_VFLAG_CONSTANT) != 0;
        const PsensSums f = psens_pass<false>(s, N, wv, uniform, sc);
        const PsensSums r = psens_pass<true>(s, N, wv, uniform, sc);
        if (tid == 0) {
            out(0, v) = constant ? 0.0 : f.js;
            out(1, v) = constant ? 0.0 : f.bound;
            out(2, v) = constant ? 0.0 : r.js;
            out(3, v) = constant ? 0.0 : r.bound;
            out(4, v) = f.wmean;
            out(5, v) = f.wsd;
        }
    }
    if (tid == 0) a.flag[j] = constant ? SBE_DIAG_FLAG_CONSTANT : 0;
}

__global__ __launch_bounds__(kDiagBlock) void k_psens_log2(const double* in, int64_t n, double* out) {
    const int64_t i = (int64_t)blockIdx.x * kDiagBlock + threadIdx.x;
    if (i < n) out[i] = log2(in[i]);
}

}  // namespace

struct sbe_psens : sbe_unit_handle, diag_store {     // (sbe_unit.hip.h, sbe_diag_column.hip.h)
    double* d_w = nullptr;              // [SBE_PSENS_MAX_VECTORS][N]
    size_t w_bytes = 0;
    double* d_vec = nullptr;            // [2][SBE_PSENS_MAX_VECTORS]: pareto k, ess
    uint8_t* d_vflag = nullptr;         // [SBE_PSENS_MAX_VECTORS]
    int* d_bad = nullptr;               // [SBE_PSENS_MAX_VECTORS]
    double* d_ary = nullptr;            // [SBE_PSENS_MAX_VECTORS][kPsensMaxTail]
    double* d_work_val = nullptr;       // global path: the sort keys of one launch
    size_t work_val_bytes = 0;
    int32_t* d_work_idx = nullptr;
    size_t work_idx_bytes = 0;
    double* d_out = nullptr;            // [kPsensOutputs][V][P]
    size_t out_bytes = 0;
    uint8_t* d_flag = nullptr;          // [P]
    size_t flag_bytes = 0;
    double* d_sorted_val = nullptr;     // [N] (sbe_psens_sorted_column)
    size_t sorted_val_bytes = 0;
    int32_t* d_sorted_idx = nullptr;
    size_t sorted_idx_bytes = 0;
    double* d_probe = nullptr;          // [2][n] (sbe_psens_device_log2)
    size_t probe_bytes = 0;
    int64_t* d_plan = nullptr;          // [kPlanLength]: the chains' offsets within column 0, then their places in the stack
    std::vector<int64_t> plan;          // its host image
    int64_t launch_columns = 0;         // 0: the default
    bool global_path = false;
    bool weights_valid = false;         // d_w, d_vflag and d_plan are those of the last weights call on this store
    int V = 0, M = 0;
    int64_t N = 0;
    float last_ms[2] = {0.0f, 0.0f};
    int64_t last_launches = 0, last_C = 0;
    std::vector<void*> buffers() const {
        return {d_x,   d_stage, d_off,        d_scratch,    d_w,     d_vec,  d_vflag,      d_bad,
                d_ary, d_work_val, d_work_idx, d_out, d_flag, d_sorted_val, d_sorted_idx, d_probe, d_plan};
    }
};

namespace {

constexpr char kNullHandle[] = "null handle";
constexpr char kReset[] = "sbe_psens_reset";

inline bool psens_lds(const sbe_psens* h, int64_t N) { return !h->global_path && N <= kPsensLdsMaxDraws; }

// The plan of a weights call: the kept draws of every chain, stacked.  h->plan, h->M and h->N afterwards.
int psens_plan(sbe_psens* h, const int64_t* burn_rows) {
    if (const int rc = h->chains.check_shaped(h, kReset)) return rc;
    if (!burn_rows) return fail(h, SBE_ERR_ARG, "null pointer argument: burn_rows");
    const int chains = h->chains.count();
    std::vector<int64_t> plan((size_t)kPlanLength, 0);
    int64_t total = 0;
    for (int c = 0; c < chains; ++c) {
        const int64_t have = h->chains.rows[(size_t)c];
        if (burn_rows[c] < 0 || burn_rows[c] > have)
            return fail(h, SBE_ERR_ARG, "burn_rows[%d]=%lld out of range [0, %lld] (rows stored for the chain)", c, (long long)burn_rows[c],
                        (long long)have);
        const int64_t n = have - burn_rows[c];
        if (n < SBE_DIAG_MIN_DRAWS)
            return fail(h, SBE_ERR_ARG, "chain %d has %lld draws after burn-in; at least %d are needed", c, (long long)n, SBE_DIAG_MIN_DRAWS);
        plan[(size_t)c] = (int64_t)c * h->P * h->chains.cap + burn_rows[c];
        plan[(size_t)(kStartAt + c)] = total;
        total += n;
        if (total > SBE_DIAG_MAX_DRAWS)
            return fail(h, SBE_ERR_ARG, "the chains hold more than %d (2^20) draws per column after burn-in", SBE_DIAG_MAX_DRAWS);
    }
    plan[(size_t)(kStartAt + chains)] = total;
    h->weights_valid = false;
    h->plan = plan;
    h->M = chains;
    h->N = total;
    return SBE_OK;
}

// the buffers of a weights call and the plan on the device
int psens_prepare_weights(sbe_psens* h, bool lds) {
    HIPCHK(h, hipSetDevice(h->device));
    const size_t N = (size_t)h->N;
    int rc = unit_ensure(h, h->d_w, h->w_bytes, (size_t)SBE_PSENS_MAX_VECTORS * N * sizeof(double));
    if (!rc) rc = unit_ensure(h, h->d_vec, (size_t)2 * SBE_PSENS_MAX_VECTORS * sizeof(double));
    if (!rc) rc = unit_ensure(h, h->d_vflag, (size_t)SBE_PSENS_MAX_VECTORS);
    if (!rc) rc = unit_ensure(h, h->d_bad, (size_t)SBE_PSENS_MAX_VECTORS * sizeof(int));
    if (!rc) rc = unit_ensure(h, h->d_ary, (size_t)SBE_PSENS_MAX_VECTORS * kPsensMaxTail * sizeof(double));
    if (!rc) rc = unit_ensure(h, h->d_plan, (size_t)kPlanLength * sizeof(int64_t));
    if (!rc && !lds) rc = unit_ensure(h, h->d_work_val, h->work_val_bytes, (size_t)SBE_PSENS_MAX_VECTORS * N * sizeof(double));
    if (!rc && !lds) rc = unit_ensure(h, h->d_work_idx, h->work_idx_bytes, (size_t)SBE_PSENS_MAX_VECTORS * N * sizeof(int32_t));
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(h->d_plan, h->plan.data(), (size_t)kPlanLength * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
    return SBE_OK;
}

// columns per launch of the column kernel: the caller's (0: all), at most what a grid and, on the global path, the scratch hold
int64_t psens_launch_columns(int64_t wanted, int64_t N, bool lds, int64_t P) {
    int64_t C = kMaxGridBlocks;
    if (!lds) C = std::max<int64_t>(1, (int64_t)(kPsensScratchBytes / ((size_t)N * kPsensKeyBytes)));
    if (wanted) C = std::min(C, wanted);
    return std::min(C, P);
}

int psens_launch_column(sbe_psens* h, const ColumnArgs& args, bool lds, int64_t count) {
    if (lds) {
        HIPCHK(h, hipFuncSetAttribute((const void*)k_psens_column<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)(kLdsBudget - kPsensStaticLds)));
        k_psens_column<true><<<(unsigned)count, kDiagBlock, (size_t)args.N * kPsensKeyBytes, h->stream>>>(args);
    } else {
        k_psens_column<false><<<(unsigned)count, kDiagBlock, 0, h->stream>>>(args);
    }
    HIPCHK(h, hipGetLastError());
    return SBE_OK;
}

ColumnArgs psens_column_args(const sbe_psens* h, bool lds) {
    ColumnArgs a{};
    a.x = h->d_x;
    a.off = h->d_plan;
    a.cap = h->chains.cap;
    a.M = h->M;
    a.N = (int)h->N;
    a.V = h->V;
    a.w = h->d_w;
    a.vflag = h->d_vflag;
    a.work_val = lds ? nullptr : h->d_work_val;
    a.work_idx = lds ? nullptr : h->d_work_idx;
    a.out = h->d_out;
    a.flag = h->d_flag;
    a.P = h->P;
    return a;
}

}  // namespace

extern "C" {

int sbe_psens_abi_version(void) { return SBE_PSENS_ABI_VERSION; }

const char* sbe_psens_last_error(const sbe_psens* h) { return unit_last_error(h); }

int64_t sbe_psens_lds_max_draws(void) { return kPsensLdsMaxDraws; }

int sbe_psens_create(sbe_psens** out, int device) { return unit_create_on_device(out, device, "sbe_psens_create"); }

int sbe_psens_destroy(sbe_psens* h) { return unit_destroy(h, kNullHandle); }

int sbe_psens_last_kernel_ms(const sbe_psens* h, float* ms_out) {
    CHECK_HANDLE(h, kNullHandle);
    if (!ms_out) return fail(h, SBE_ERR_ARG, "null pointer argument: ms_out");
    ms_out[0] = h->last_ms[0];
    ms_out[1] = h->last_ms[1];
    return SBE_OK;
}

int sbe_psens_set_launch_columns(sbe_psens* h, int64_t columns) {
    CHECK_HANDLE(h, kNullHandle);
    if (columns < 0 || columns > kMaxGridBlocks)
        return fail(h, SBE_ERR_ARG, "columns=%lld out of range [0, %lld] (0: the default)", (long long)columns, (long long)kMaxGridBlocks);
    h->launch_columns = columns;
    return SBE_OK;
}

int sbe_psens_set_global_path(sbe_psens* h, int on) {
    CHECK_HANDLE(h, kNullHandle);
    h->global_path = on != 0;
    return SBE_OK;
}

int sbe_psens_reset(sbe_psens* h, int n_chains, int64_t n_columns, int64_t capacity_rows) {
    CHECK_HANDLE(h, kNullHandle);
    h->weights_valid = false;
    h->last_launches = h->last_C = 0;
    int rc = diag_store_reset(h, n_chains, n_columns, capacity_rows);
    if (!rc) rc = unit_ensure(h, h->d_flag, h->flag_bytes, (size_t)n_columns);
    if (rc) return rc;
    diag_store_shaped(h, n_chains, n_columns, capacity_rows);
    return SBE_OK;
}

int sbe_psens_rows(const sbe_psens* h, int chain, int64_t* n_rows_out) {
    CHECK_HANDLE(h, kNullHandle);
    return h->chains.get(h, kDiagLane, chain, n_rows_out);
}

int sbe_psens_append_rows(sbe_psens* h, int chain, const double* rows, int64_t n_rows) {
    CHECK_HANDLE(h, kNullHandle);
    h->weights_valid = false;
    return diag_store_append(h, kReset, chain, rows, n_rows);
}

int sbe_psens_weights_from_components(sbe_psens* h, const int64_t* burn_rows, int n_components, const int64_t* component_columns, double delta,
                                      double* pareto_k_out, double* ess_out, uint8_t* vflag_out, double* weights_out) {
    CHECK_HANDLE(h, kNullHandle);
    if (const int rc = h->chains.check_shaped(h, kReset)) return rc;
    if (n_components < 1 || n_components > SBE_PSENS_MAX_COMPONENTS)
        return fail(h, SBE_ERR_ARG, "n_components=%d out of range [1, %d]", n_components, SBE_PSENS_MAX_COMPONENTS);
    if (!component_columns) return fail(h, SBE_ERR_ARG, "null pointer argument: component_columns");
    for (int g = 0; g < n_components; ++g)
        if (component_columns[g] < 0 || component_columns[g] >= h->P)
            return fail(h, SBE_ERR_ARG, "component_columns[%d]=%lld out of range [0,%lld)", g, (long long)component_columns[g], (long long)h->P);
    if (!(delta > 0.0) || !std::isfinite(delta)) return fail(h, SBE_ERR_ARG, "delta=%g must be positive and finite", delta);
    if (!pareto_k_out || !ess_out || !vflag_out) return fail(h, SBE_ERR_ARG, "null pointer argument: output");
    if (const int rc = psens_plan(h, burn_rows)) return rc;
    const int V = 2 * n_components;
    const int64_t N = h->N;
    const bool lds = psens_lds(h, N);
    if (const int rc = psens_prepare_weights(h, lds)) return rc;

    WeightArgs a{};
    a.x = h->d_x;
    a.off = h->d_plan;
    a.cap = h->chains.cap;
    a.M = h->M;
    a.N = (int)N;
    a.tail_n = (int)std::ceil(std::min(0.2 * (double)N, 3.0 * std::sqrt((double)N)));
    const double alpha[2] = {1.0 / (1.0 + delta), 1.0 + delta};
    for (int v = 0; v < V; ++v) {
        a.column[v] = component_columns[v / 2];
        a.scale[v] = alpha[v & 1] - 1.0;
    }
    a.work_val = lds ? nullptr : h->d_work_val;
    a.work_idx = lds ? nullptr : h->d_work_idx;
    a.ary = h->d_ary;
    a.w = h->d_w;
    a.k_out = h->d_vec;
    a.ess_out = h->d_vec + SBE_PSENS_MAX_VECTORS;
    a.vflag = h->d_vflag;
    a.bad = h->d_bad;
    int rc = unit_timed(h, [&] {
        if (lds) {
            HIPCHK(h, hipFuncSetAttribute((const void*)k_psens_weights<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)(kLdsBudget - kPsensStaticLds)));
            k_psens_weights<true><<<(unsigned)V, kDiagBlock, (size_t)N * kPsensKeyBytes, h->stream>>>(a);
        } else {
            k_psens_weights<false><<<(unsigned)V, kDiagBlock, 0, h->stream>>>(a);
        }
        HIPCHK(h, hipGetLastError());
        return SBE_OK;
    });
    if (rc) return rc;
    int bad[SBE_PSENS_MAX_VECTORS] = {0};
    HIPCHK(h, hipMemcpyAsync(bad, h->d_bad, (size_t)V * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int v = 0; v < V; ++v)
        if (bad[v])
            return fail(h, SBE_ERR_ARG, "component column %lld holds a non-finite value, or its log ratios at delta=%g overflow",
                        (long long)component_columns[v / 2], delta);
    HIPCHK(h, hipMemcpyAsync(pareto_k_out, h->d_vec, (size_t)V * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(ess_out, h->d_vec + SBE_PSENS_MAX_VECTORS, (size_t)V * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(vflag_out, h->d_vflag, (size_t)V, hipMemcpyDeviceToHost, h->stream));
    if (weights_out) HIPCHK(h, hipMemcpyAsync(weights_out, h->d_w, (size_t)V * (size_t)N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if ((rc = unit_sync_timed(h))) return rc;
    h->last_ms[0] = h->last_kernel_ms;
    h->V = V;
    h->last_launches = h->last_C = 0;
    h->weights_valid = true;
    return SBE_OK;
}

int sbe_psens_set_weights(sbe_psens* h, const int64_t* burn_rows, int n_vectors, const double* weights) {
    CHECK_HANDLE(h, kNullHandle);
    if (const int rc = h->chains.check_shaped(h, kReset)) return rc;
    if (n_vectors < 1 || n_vectors > SBE_PSENS_MAX_VECTORS)
        return fail(h, SBE_ERR_ARG, "n_vectors=%d out of range [1, %d]", n_vectors, SBE_PSENS_MAX_VECTORS);
    if (!weights) return fail(h, SBE_ERR_ARG, "null pointer argument: weights");
    if (const int rc = psens_plan(h, burn_rows)) return rc;
    const int64_t N = h->N;
    if (const int rc = psens_prepare_weights(h, true)) return rc;
    HIPCHK(h, hipMemcpyAsync(h->d_w, weights, (size_t)n_vectors * (size_t)N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    k_psens_check_weights<<<(unsigned)n_vectors, kDiagBlock, 0, h->stream>>>(h->d_w, (int)N, h->d_bad, h->d_vflag);
    HIPCHK(h, hipGetLastError());
    int bad[SBE_PSENS_MAX_VECTORS] = {0};
    HIPCHK(h, hipMemcpyAsync(bad, h->d_bad, (size_t)n_vectors * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int v = 0; v < n_vectors; ++v) {
        if (bad[v] == 1) return fail(h, SBE_ERR_ARG, "weights[%d] holds a negative or non-finite value", v);
        if (bad[v] == 2) return fail(h, SBE_ERR_ARG, "weights[%d] has no positive finite sum", v);
    }
    h->last_ms[0] = 0.0f;
    h->V = n_vectors;
    h->last_launches = h->last_C = 0;
    h->weights_valid = true;
    return SBE_OK;
}

int sbe_psens_compute(sbe_psens* h, double* js_out, double* bound_out, double* js_neg_out, double* bound_neg_out, double* wmean_out,
                      double* wsd_out, uint8_t* flag_out) {
    CHECK_HANDLE(h, kNullHandle);
    if (const int rc = h->chains.check_shaped(h, kReset)) return rc;
    if (!js_out || !bound_out || !js_neg_out || !bound_neg_out || !wmean_out || !wsd_out || !flag_out)
        return fail(h, SBE_ERR_ARG, "null pointer argument: output");
    if (!h->weights_valid)
        return fail(h, SBE_ERR_STATE, "no weights for the rows of the store (sbe_psens_weights_from_components, sbe_psens_set_weights)");
    const int64_t N = h->N, P = h->P;
    const int V = h->V;
    const bool lds = psens_lds(h, N);
    const int64_t C = psens_launch_columns(h->launch_columns, N, lds, P);
    HIPCHK(h, hipSetDevice(h->device));
    int rc = unit_ensure(h, h->d_out, h->out_bytes, (size_t)kPsensOutputs * (size_t)V * (size_t)P * sizeof(double));
    if (!rc && !lds) rc = unit_ensure(h, h->d_work_val, h->work_val_bytes, (size_t)C * (size_t)N * sizeof(double));
    if (!rc && !lds) rc = unit_ensure(h, h->d_work_idx, h->work_idx_bytes, (size_t)C * (size_t)N * sizeof(int32_t));
    if (rc) return rc;
    ColumnArgs a = psens_column_args(h, lds);
    int64_t launches = 0;
    rc = unit_timed(h, [&] {
        for (int64_t j0 = 0; j0 < P; j0 += C, ++launches) {
            a.j0 = j0;
            if (const int lrc = psens_launch_column(h, a, lds, std::min(C, P - j0))) return lrc;
        }
        return (int)SBE_OK;
    });
    if (rc) return rc;
    rc = unit_copy_back(h, (const double*)h->d_out, (size_t)V * (size_t)P, {js_out, bound_out, js_neg_out, bound_neg_out, wmean_out, wsd_out});
    if (!rc) rc = unit_copy_back(h, (const uint8_t*)h->d_flag, (size_t)P, {flag_out});
    if (!rc) rc = unit_sync_timed(h);
    if (rc) return rc;
    h->last_ms[1] = h->last_kernel_ms;
    h->last_launches = launches;
    h->last_C = C;
    return SBE_OK;
}

int sbe_psens_last_shape(const sbe_psens* h, int* chains_out, int64_t* draws_out, int* vectors_out, int* path_out, int64_t* launches_out,
                         int64_t* launch_columns_out) {
    CHECK_HANDLE(h, kNullHandle);
    if (!chains_out || !draws_out || !vectors_out || !path_out || !launches_out || !launch_columns_out)
        return fail(h, SBE_ERR_ARG, "null pointer argument: output");
    if (!h->weights_valid)
        return fail(h, SBE_ERR_STATE, "no weights for the rows of the store (sbe_psens_weights_from_components, sbe_psens_set_weights)");
    *chains_out = h->M;
    *draws_out = h->N;
    *vectors_out = h->V;
    *path_out = psens_lds(h, h->N) ? SBE_DIAG_PATH_LDS : SBE_DIAG_PATH_GLOBAL;
    *launches_out = h->last_launches;
    *launch_columns_out = h->last_C;
    return SBE_OK;
}

int sbe_psens_sorted_column(sbe_psens* h, int64_t column, double* values_out, int32_t* samples_out) {
    CHECK_HANDLE(h, kNullHandle);
    if (const int rc = h->chains.check_shaped(h, kReset)) return rc;
    if (!h->weights_valid)
        return fail(h, SBE_ERR_STATE, "no weights for the rows of the store (sbe_psens_weights_from_components, sbe_psens_set_weights)");
    if (column < 0 || column >= h->P) return fail(h, SBE_ERR_ARG, "column %lld out of range [0,%lld)", (long long)column, (long long)h->P);
    if (!values_out || !samples_out) return fail(h, SBE_ERR_ARG, "null pointer argument: output");
    const size_t N = (size_t)h->N;
    const bool lds = psens_lds(h, h->N);
    HIPCHK(h, hipSetDevice(h->device));
    int rc = unit_ensure(h, h->d_sorted_val, h->sorted_val_bytes, N * sizeof(double));
    if (!rc) rc = unit_ensure(h, h->d_sorted_idx, h->sorted_idx_bytes, N * sizeof(int32_t));
    if (!rc && !lds) rc = unit_ensure(h, h->d_work_val, h->work_val_bytes, N * sizeof(double));
    if (!rc && !lds) rc = unit_ensure(h, h->d_work_idx, h->work_idx_bytes, N * sizeof(int32_t));
    if (rc) return rc;
    ColumnArgs a = psens_column_args(h, lds);
    a.sorted_val = h->d_sorted_val;
    a.sorted_idx = h->d_sorted_idx;
    a.j0 = column;
    if ((rc = psens_launch_column(h, a, lds, 1))) return rc;
    HIPCHK(h, hipMemcpyAsync(values_out, h->d_sorted_val, N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(samples_out, h->d_sorted_idx, N * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return SBE_OK;
}

int sbe_psens_device_log2(sbe_psens* h, int64_t n, const double* in, double* out) {
    CHECK_HANDLE(h, kNullHandle);
    if (n < 1 || n > kMaxProbe) return fail(h, SBE_ERR_ARG, "n=%lld out of range [1, %lld]", (long long)n, (long long)kMaxProbe);
    if (!in || !out) return fail(h, SBE_ERR_ARG, "null pointer argument: %s", in ? "out" : "in");
    HIPCHK(h, hipSetDevice(h->device));
    if (const int rc = unit_ensure(h, h->d_probe, h->probe_bytes, (size_t)2 * (size_t)n * sizeof(double))) return rc;
    HIPCHK(h, hipMemcpyAsync(h->d_probe, in, (size_t)n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    k_psens_log2<<<(unsigned)div_up(n, kDiagBlock), kDiagBlock, 0, h->stream>>>(h->d_probe, n, h->d_probe + n);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(out, h->d_probe + n, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return SBE_OK;
}

}  // extern "C"
