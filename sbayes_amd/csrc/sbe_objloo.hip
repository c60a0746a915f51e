// sbe_objloo.hip -- the leave-one-object-out ELPD with the cluster membership integrated out, on the device
// (include/sbe_objloo.h): per logged sample and object the log likelihood of the object's cells under every membership
// hypothesis, mixed with the conditional prior into the object's marginal log likelihood; PSIS per object over the marginal and
// over the conditional column with the marginal weights kept; and the samples run past the weights a second time for the
// zero-shot predictive of every cell.  The contract is tests/_objloo_oracle.py; DESIGN.md section 32 has the layout, the launch
// plan and the bounds.
//
// The three phases and their kernels:
//   add         k_predict_ids, k_predict_validate (sbe_predict_row.hip.h), k_objloo_validate_prior, then
//               k_objloo_rows<CP>: sbe_contrib.hip's plan -- a thread per cell of a tile, the sample's slice double-buffered in
//               LDS, the two sets of weights and the confounders' products once, then m0 and the chain of m_k -- writing
//               log m_j of every (hypothesis, cell) to staging [n][K+1][N][F] (+0.0 for a cell without a code);
//               k_objloo_sum_features: a wave per (sample, hypothesis, object), lane i adds the features i, i + 64, .. in order,
//               then the unit layer's xor tree: H of the call, [n][K+1][N];
//               k_objloo_mix: a thread per (object, sample) forms a_j = log prior_j + H_j, L and Cnd and writes the object's
//               columns of the store (consecutive threads write consecutive samples);
//   weights     k_objloo_weights<kLds>: a 256-thread workgroup per (object, kind), kind 0 the marginal column L and kind 1 the
//               conditional column Cnd: sbe_psis_ratio.hip.h's steps over the ratios -ll (keys in LDS, or past
//               sbe_objloo_lds_max_samples in the workgroup's slice of a global scratch, the launches in chunks of as many
//               workgroups as the scratch has slices), then loo_i, lppd_i and, for kind 0, the weights to their samples, n_eff
//               and the membership probabilities;
//   accumulate  the first two kernels of add again into the staging buffers, k_objloo_compare (the call's H and a against
//               the store, bit for bit), then k_objloo_accumulate<SP, CP>: sbe_predict.hip's tile and slices, a thread per cell,
//               with or without a code, with the cell's S float64 sums in registers for all n samples.  The sums are read from
//               one buffer and written to the other; the host swaps the two only when no sample differed, so a refused call
//               leaves them as they were.
// No floating-point atomics: a cell belongs to one thread, which adds the samples in order; no workgroup waits for another.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

#include "sbe_predict_row.hip.h"
#include "sbe_psis_ratio.hip.h"
#include "../../include/sbe_objloo.h"

namespace {

constexpr int kPriorRow = kUniform;                  // the seventh kind's slot of the offender's key: stage() leaves it to the unit
constexpr size_t kObjlooStaticLds = 8192;            // headroom for the weights kernel's static LDS (the fit, the reductions)
constexpr size_t kObjlooScratchBytes = (size_t)256 << 20;   // the sort keys of one launch on the global path
constexpr int kOutputs = 7;                          // loo_i, k_i, n_eff_i, lppd_i, loo_cond_i, k_cond_i, lppd_cond_i

// ---- phase 1: the rows ----------------------------------------------------------------------------------------------------------
struct RowArgs {                                     // (the fields sbe_predict_row.hip.h reads, then the unit's own)
    const uint8_t* codes;
    const uint8_t* groups;
    const uint16_t* kid;
    const double* weights;
    const double* tables;
    int64_t N;
    int F, S, C, R;
    int n;
    int Ft, Nt, f_tiles;
    int64_t block0;
    int row_off[kMaxC];
    int K;
    const double* prior;                             // [n][N][K+1], or null: `uniform` everywhere
    double uniform;                                  // 1.0 / (K + 1)
    double* lg;                                      // phase 1: staging [n][K+1][N][F], written
    const double* p_in;                              // phase 3: the sums [N][F][S], read ..
    double* p_out;                                   // .. and written
    const double* w;                                 // the store's weights [N][cap]
    int64_t cap, t_first;                            // the call's first sample in the store
    unsigned long long* err;                         // the first observed cell without a confounder: sample << 40 | cell (atomicMin)
};

template <int CP>
__global__ __launch_bounds__(kBlock) void k_objloo_rows(const RowArgs g) {
    extern __shared__ double lds[];                            // two slices
    const TileCell tc = tile_cell(g);
    const int64_t cells = g.N * g.F;
    int row[CP];
    bool has[CP];
#pragma unroll
    for (int c = 0; c < CP; ++c) cell_group(g, tc, c, row[c], has[c]);
    const int x = tc.live ? g.codes[tc.cell] : kNA;
    unsigned long long first = kNoError;

    stage_slice(lds, g, 0, tc.f0, tc.fw);
    __syncthreads();
    for (int t = 0; t < g.n; ++t) {
        const double* cur = lds + (t & 1) * tc.slice;
        if (t + 1 < g.n) stage_slice(lds + ((t + 1) & 1) * tc.slice, g, t + 1, tc.f0, tc.fw);
        if (tc.live) {
            double* out = g.lg + (int64_t)t * (g.K + 1) * cells + tc.cell;     // lg[t][j][n][f] = out[j cells]
            bool formed = false;
            double w1[CP], w0[CP], part[CP];
            const double* base[CP];
            if (x != kNA) {
                formed = cell_weights_in_and_out(g, tc, cur, row, has, w1, w0, base);
                if (!formed) first = min(first, ((unsigned long long)(g.t_first + t) << 40) | (unsigned long long)tc.cell);
            }
            if (formed) {
                out[0] = log(cell_state(g.C, w0, base, x));        // -inf where m0 = 0
#pragma unroll
                for (int c = 1; c < CP; ++c) part[c] = c < g.C ? w1[c] * base[c][x] : 0.0;
            } else {
                out[0] = 0.0;
            }
            const double* theta = cur + tc.fl * g.S;               // table[0][f][.] of the slice; a cluster further: Ft S
            for (int k = 0; k < g.K; ++k, theta += g.Ft * g.S)
                out[(int64_t)(k + 1) * cells] = formed ? log(cell_state_in(g.C, w1[0], theta, x, part)) : 0.0;
        }
        __syncthreads();                                       // sample t is read, the slice of t + 1 is written
    }
    if (first != kNoError) atomicMin(g.err, first);
}

// H[row], row = (t (K + 1) + j) N + object: a wave takes one row of lg; lane i adds the features i, i + 64, .. in order onto 0;
// then the fixed tree of the unit layer over the lanes
__global__ __launch_bounds__(kBlock) void k_objloo_sum_features(const double* lg, int64_t rows, int F, double* sums, int64_t block0) {
    const int64_t row = (block0 + blockIdx.x) * (kBlock / 64) + (threadIdx.x >> 6);
    if (row >= rows) return;                                   // (a whole wave)
    const double* v = lg + row * F;
    double sum = 0.0;
    for (int f = threadIdx.x & 63; f < F; f += 64) sum += v[f];
    sum = unit_wave_reduce(sum, unit_sum());
    if ((threadIdx.x & 63) == 0) sums[row] = sum;
}

// the prior rows of a call: one thread per (sample, object)
__global__ __launch_bounds__(kBlock) void k_objloo_validate_prior(const double* prior, int64_t n, int64_t N, int K, unsigned long long* err) {
    const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (q >= n * N) return;
    const int64_t t = q / N, obj = q - t * N;
    const double* v = prior + q * (K + 1);
    double sum = 0.0;
    for (int j = 0; j <= K; ++j) {
        const double x = v[j];
        if (!(x >= 0.0) || isinf(x)) {                       // negative, NaN or infinite
            atomicMin(err, error_key(t, kPriorRow, obj));
            return;
        }
        sum += x;
    }
    if (fabs(sum - 1.0) > SBE_PREDICT_SUM_TOL) atomicMin(err, error_key(t, kPriorRow, obj));
}

struct MixArgs {
    const double* sums;                              // H of the call: [n][K+1][N]
    const uint16_t* kid;                             // [n][N]
    const double* prior;                             // [n][N][K+1] or null
    double uniform;
    int64_t N, n, cap, r0;                           // r0: the call's first sample in the store
    int K;
    double* H;                                       // the store: [N][K+1][cap]
    double* A;                                       // [N][K+1][cap]
    double* L;                                       // [N][cap]
    double* Cnd;                                     // [N][cap]
    unsigned long long* err;                         // add: the first (object, sample) whose L or Cnd is not finite: object << 21 |
                                                     // sample << 1 | (L is finite); compare: the first sample that differs
};

__device__ inline double mix_a(const MixArgs& a, int64_t t, int64_t obj, int j, double h) {
    const double pj = a.prior ? a.prior[(t * a.N + obj) * (a.K + 1) + j] : a.uniform;
    return log(pj) + h;
}

// thread q: object q / n, sample q % n of the call
__global__ __launch_bounds__(kBlock) void k_objloo_mix(const MixArgs a) {
    const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (q >= a.N * a.n) return;
    const int64_t obj = q / a.n, t = q - obj * a.n;
    const uint16_t id = a.kid[t * a.N + obj];
    const int z = id == kNoCluster ? 0 : (int)id + 1;
    const double* hs = a.sums + t * (a.K + 1) * a.N + obj;   // H_j = hs[j N]
    const int64_t col = obj * (a.K + 1) * a.cap + a.r0 + t;    // of hypothesis 0; a hypothesis further: cap
    double mx = -INFINITY, cnd = 0.0;
    for (int j = 0; j <= a.K; ++j) {
        const double h = hs[(int64_t)j * a.N], aj = mix_a(a, t, obj, j, h);
        a.H[col + (int64_t)j * a.cap] = h;
        a.A[col + (int64_t)j * a.cap] = aj;
        mx = fmax(mx, aj);
        if (j == z) cnd = h;
    }
    double sum = 0.0;
    for (int j = 0; j <= a.K; ++j) sum += exp(a.A[col + (int64_t)j * a.cap] - mx);
    const double l = mx + log(sum);
    a.L[obj * a.cap + a.r0 + t] = l;
    a.Cnd[obj * a.cap + a.r0 + t] = cnd;
    if (!isfinite(l) || !isfinite(cnd))
        atomicMin(a.err, ((unsigned long long)obj << 21) | ((unsigned long long)(a.r0 + t) << 1) | (isfinite(l) ? 1ull : 0ull));
}

// phase 3: the call's H and a against the store's, bit for bit
__global__ __launch_bounds__(kBlock) void k_objloo_compare(const MixArgs a) {
    const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (q >= a.N * a.n) return;
    const int64_t obj = q / a.n, t = q - obj * a.n;
    const double* hs = a.sums + t * (a.K + 1) * a.N + obj;
    const int64_t col = obj * (a.K + 1) * a.cap + a.r0 + t;
    bool differs = false;
    for (int j = 0; j <= a.K; ++j) {
        const double h = hs[(int64_t)j * a.N], aj = mix_a(a, t, obj, j, h);
        differs |= __double_as_longlong(h) != __double_as_longlong(a.H[col + (int64_t)j * a.cap]);
        differs |= __double_as_longlong(aj) != __double_as_longlong(a.A[col + (int64_t)j * a.cap]);
    }
    if (differs) atomicMin(a.err, (unsigned long long)(a.r0 + t));
}

// ---- phase 2: PSIS per (object, kind), the marginal weights kept ----------------------------------------------------------------
struct WeightArgs {
    const double* L;          // store: [N][cap]
    const double* Cnd;        // [N][cap]
    const double* A;          // [N][K+1][cap]
    double* w;                // [N][cap]
    int64_t cap, N;
    int T, tail_n, K;
    double* work;             // global path: a slice per workgroup of the launch
    int64_t slice;            // its doubles: val [T], ary [tail_n], idx [T] int32
    double* out;              // [kOutputs][N]
    double* member;           // [N][K+1]
    int64_t b0;               // first workgroup of this launch: 2 object + kind
};

template <bool kLds>
__global__ __launch_bounds__(kRatioBlock) void k_objloo_weights(WeightArgs a) {
    extern __shared__ __align__(16) unsigned char dyn[];
    __shared__ RatioScratch sc;
    const int tid = threadIdx.x, T = a.T;
    const int64_t b = a.b0 + blockIdx.x, obj = b >> 1;
    const int kind = (int)(b & 1);
    double* base = kLds ? reinterpret_cast<double*>(dyn) : a.work + (int64_t)blockIdx.x * a.slice;
    double* ary = base;                                      // [tail_n] the tail's exceedances
    const RatioKeys s{base + a.tail_n, reinterpret_cast<int32_t*>(base + a.tail_n + T)};
    const double* col = (kind ? a.Cnd : a.L) + obj * a.cap;

    // 1. the ratios -ll: their maximum; the maximum of ll for lppd
    double hi = -INFINITY, top = -INFINITY;
    for (int i = tid; i < T; i += kRatioBlock) {
        hi = fmax(hi, -col[i]);
        top = fmax(top, col[i]);
    }
    hi = unit_block_reduce<kRatioWaves>(hi, sc.red, unit_max{});
    top = unit_block_reduce<kRatioWaves>(top, sc.red, unit_max{});

    // 2. x = ratio - max with its sample, sorted; 3. the smoothed tail and logsumexp (sbe_psis_ratio.hip.h)
    for (int i = tid; i < T; i += kRatioBlock) {
        s.val[i] = -col[i] - hi;
        s.idx[i] = i;
    }
    __syncthreads();
    ratio_block_sort(s, T);
    const double k_hat = ratio_smooth_tail(s, T, a.tail_n, ary, sc);
    const double lse = ratio_logsumexp(s, T, sc);

    // 4. lw = x' - logsumexp(x'): loo_i = logsumexp(lw + ll); the marginal column's weights to their samples and n_eff
    double best = -INFINITY;
    int nan = 0;
    for (int p = tid; p < T; p += kRatioBlock) {
        const double v = (s.val[p] - lse) + col[s.idx[p]];
        best = fmax(best, v);
        nan |= isnan(v);
    }
    best = unit_block_reduce<kRatioWaves>(best, sc.red, unit_max{});
    nan = unit_block_reduce<kRatioWaves>(nan, sc.ired, unit_or{});
    if (nan) best = NAN;
    double sum = 0.0, sumsq = 0.0;
    for (int p = tid; p < T; p += kRatioBlock) {
        const double lw = s.val[p] - lse;
        const int t = s.idx[p];
        sum += exp((lw + col[t]) - best);
        if (kind == 0) {
            const double wt = exp(lw);
            a.w[obj * a.cap + t] = wt;
            sumsq += wt * wt;
        }
    }
    sum = unit_block_reduce<kRatioWaves>(sum, sc.red, unit_sum{});
    sumsq = unit_block_reduce<kRatioWaves>(sumsq, sc.red, unit_sum{});

    // 5. lppd_i = logsumexp(ll) - log T
    double plain = 0.0;
    for (int i = tid; i < T; i += kRatioBlock) plain += exp(col[i] - top);
    plain = unit_block_reduce<kRatioWaves>(plain, sc.red, unit_sum{});
    if (tid == 0) {
        double* out = a.out + (kind ? 4 : 0) * a.N + obj;
        out[0] = log(sum) + best;
        out[a.N] = k_hat;
        if (kind == 0) {
            out[2 * a.N] = 1 / sumsq;
            out[3 * a.N] = (log(plain) + top) - log((double)T);
        } else {
            out[2 * a.N] = (log(plain) + top) - log((double)T);
        }
    }
    if (kind != 0) return;                                   // (uniform over the block)

    // 6. the membership probabilities: the mean over the samples of exp(a_j - L)
    for (int j = 0; j <= a.K; ++j) {
        const double* aj = a.A + (obj * (a.K + 1) + j) * a.cap;
        double r = 0.0;
        for (int i = tid; i < T; i += kRatioBlock) r += exp(aj[i] - col[i]);
        r = unit_block_reduce<kRatioWaves>(r, sc.red, unit_sum{});
        if (tid == 0) a.member[obj * (a.K + 1) + j] = r / (double)T;
    }
}

// ---- phase 3: the samples past the weights ------------------------------------------------------------------------------------------
template <int SP, int CP>
__global__ __launch_bounds__(kBlock) void k_objloo_accumulate(const RowArgs g) {
    extern __shared__ double lds[];                            // two slices
    const TileCell tc = tile_cell(g);
    double p[SP];
    int row[CP];
    bool has[CP];
#pragma unroll
    for (int c = 0; c < CP; ++c) cell_group(g, tc, c, row[c], has[c]);
#pragma unroll
    for (int s = 0; s < SP; ++s) p[s] = tc.live && s < g.S ? g.p_in[tc.cell * g.S + s] : 0.0;
    const int64_t at = tc.live ? tc.obj * g.cap + g.t_first : 0;  // of the call's first sample in the object's column

    stage_slice(lds, g, 0, tc.f0, tc.fw);
    __syncthreads();
    for (int t = 0; t < g.n; ++t) {
        const double* cur = lds + (t & 1) * tc.slice;
        if (t + 1 < g.n) stage_slice(lds + ((t + 1) & 1) * tc.slice, g, t + 1, tc.f0, tc.fw);
        if (tc.live) {
            const double wt = g.w[at + t];
            const double* pr = g.prior ? g.prior + ((int64_t)t * g.N + tc.obj) * (g.K + 1) : nullptr;
            double w1[CP], w0[CP], part[CP];
            const double* base[CP];
            cell_weights_in_and_out(g, tc, cur, row, has, w1, w0, base);
#pragma unroll
            for (int s = 0; s < SP; ++s)
                if (s < g.S) {
                    double mz = 0.0;
                    mz += (pr ? pr[0] : g.uniform) * cell_state(g.C, w0, base, s);
#pragma unroll
                    for (int c = 1; c < CP; ++c) part[c] = c < g.C ? w1[c] * base[c][s] : 0.0;
                    const double* theta = cur + tc.fl * g.S;
                    for (int k = 0; k < g.K; ++k, theta += g.Ft * g.S) mz += (pr ? pr[k + 1] : g.uniform) * cell_state_in(g.C, w1[0], theta, s, part);
                    p[s] += wt * mz;
                }
        }
        __syncthreads();                                       // sample t is read, the slice of t + 1 is written
    }
    if (!tc.live) return;
#pragma unroll
    for (int s = 0; s < SP; ++s)
        if (s < g.S) g.p_out[tc.cell * g.S + s] = p[s];
}

using RowKernel = void (*)(const RowArgs);

RowKernel rows_kernel(int C) {
    if (C <= 1) return k_objloo_rows<1>;
    if (C <= 2) return k_objloo_rows<2>;
    if (C <= 4) return k_objloo_rows<4>;
    return k_objloo_rows<8>;
}

template <int SP>
RowKernel acc_kernel_c(int C) {
    if (C <= 1) return k_objloo_accumulate<SP, 1>;
    if (C <= 2) return k_objloo_accumulate<SP, 2>;
    if (C <= 4) return k_objloo_accumulate<SP, 4>;
    return k_objloo_accumulate<SP, 8>;
}

RowKernel acc_kernel(int S, int C) {
    if (S <= 2) return acc_kernel_c<2>(C);
    if (S <= 4) return acc_kernel_c<4>(C);
    if (S <= 8) return acc_kernel_c<8>(C);
    if (S <= 16) return acc_kernel_c<16>(C);
    return acc_kernel_c<32>(C);
}

}  // namespace

struct sbe_objloo : sbe_unit_handle, sample_store {
    bool weighted = false;
    int64_t cap = 0;
    int64_t n_rows = 0;                 // T so far
    int64_t next_t = 0;                 // phase 3: the samples accumulated
    int cur = 0;                        // which of the two sums buffers holds the sums
    double* d_p = nullptr;              // two buffers of [N][F][S]
    size_t p_bytes = 0;
    double* d_H = nullptr;              // the store: H [N][K+1][cap]
    size_t H_bytes = 0;
    double* d_A = nullptr;              // a [N][K+1][cap]
    size_t A_bytes = 0;
    double* d_cols = nullptr;           // L, Cnd, w: [3][N][cap]
    size_t cols_bytes = 0;
    double* d_out = nullptr;            // [kOutputs][N], then membership [N][K+1]
    size_t out_bytes = 0;
    double* d_lg = nullptr;             // staging [n][K+1][N][F]
    size_t lg_bytes = 0;
    double* d_sums = nullptr;           // H of the call [n][K+1][N]
    size_t sums_bytes = 0;
    double* d_prior = nullptr;          // [n][N][K+1]
    size_t prior_bytes = 0;
    double* d_work = nullptr;           // the global path's sort keys of one launch
    size_t work_bytes = 0;
    unsigned long long* d_err = nullptr;   // [0]: the first observed cell without a confounder, [1]: the first (object, sample)
                                           // whose L or Cnd is not finite (add), the first sample that differs (accumulate)
    // d_words: [0]: stage()'s first offender's key
    std::vector<void*> buffers() const { return buffers_with({d_p, d_H, d_A, d_cols, d_out, d_lg, d_sums, d_prior, d_work, d_err}); }
    size_t p_doubles() const { return (size_t)N * F * S; }
    double* sums(int which) const { return d_p + (size_t)which * p_doubles(); }
    double* L() const { return d_cols; }
    double* Cnd() const { return d_cols + (size_t)N * (size_t)cap; }
    double* w() const { return d_cols + 2 * (size_t)N * (size_t)cap; }
};

namespace {

constexpr char kPrefix[] = "sbe_objloo";

int64_t sample_bytes(int64_t N, int64_t F, int S, int C, int K, int R) {
    return (int64_t)K * N + 8 * F * C + 8 * (int64_t)R * F * S + 2 * N + 8 * (int64_t)(K + 1) * N * F + 16 * (int64_t)(K + 1) * N;
}

int64_t store_bytes(int64_t N, int K, int64_t cap) { return N * cap * 8 * (2 * ((int64_t)K + 1) + 3); }

// dynamic LDS of a column of T samples: [tail exceedances][values][samples]
size_t weights_lds_bytes(int64_t T) { return (size_t)ratio_tail_count(T) * sizeof(double) + (size_t)T * kRatioKeyBytes; }

bool weights_in_lds(int64_t T) { return weights_lds_bytes(T) + kObjlooStaticLds <= kLdsBudget; }

int forget_rows(sbe_objloo* h) {
    HIPCHK(h, hipMemsetAsync(h->d_p, 0, 2 * h->p_doubles() * sizeof(double), h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->n_rows = h->next_t = 0;
    h->cur = 0;
    h->weighted = false;
    return SBE_OK;
}

// The part add and accumulate share: the store's opening of a call over n samples with the prior rows validated, then the log
// rows and their sums over the features into the staging buffers.  t_first: the call's first sample in the store.  On SBE_OK
// the kernels are queued, args holds what sbe_predict_row.hip.h reads, and d_err is set to "none" ahead of them.
int form_rows(sbe_objloo* h, int64_t n, int64_t t_first, const uint8_t* clusters, const double* weights, const double* tables, const double* prior,
              RowArgs& args, size_t& lds) {
    SamplePlan plan;
    const int64_t N = h->N, F = h->F;
    const int K = h->K;
    const size_t prior_count = (size_t)n * (size_t)N * (size_t)(K + 1);
    const int rc = h->stage(
        h, n, clusters, weights, tables, sample_bytes(N, F, h->S, h->C, K, h->R), SBE_OBJLOO_MAX_STAGE_BYTES, h->d_words,
        [&] {
            int own = unit_ensure(h, h->d_lg, h->lg_bytes, (size_t)n * (size_t)(K + 1) * (size_t)(N * F) * sizeof(double));
            if (!own) own = unit_ensure(h, h->d_sums, h->sums_bytes, prior_count * sizeof(double));
            if (!own) own = unit_ensure(h, h->d_prior, h->prior_bytes, prior_count * sizeof(double));
            if (!own && prior) own = copy_pieces(h, h->d_prior, prior, prior_count * sizeof(double), hipMemcpyHostToDevice);
            return own;
        },
        [&] {
            if (!prior) return (int)SBE_OK;
            k_objloo_validate_prior<<<(unsigned)div_up(n * N, kBlock), kBlock, 0, h->stream>>>(h->d_prior, n, N, K, h->d_words);
            HIPCHK(h, hipGetLastError());
            return (int)SBE_OK;
        },
        plan);
    if (rc) return rc;
    if (plan.key != kNoError)
        return fail(h, SBE_ERR_DATA, "sample %lld: the prior row of object %lld has an entry that is negative or not finite, or sums further than %g from 1",
                    (long long)(plan.key >> 40), (long long)(plan.key & ((1ull << 36) - 1)), SBE_PREDICT_SUM_TOL);
    args = RowArgs{};
    h->fill(args, n, plan);
    lds = plan.lds;
    args.K = K;
    args.prior = prior ? h->d_prior : nullptr;
    args.uniform = 1.0 / (double)(K + 1);
    args.lg = h->d_lg;
    args.t_first = t_first;
    args.cap = h->cap;
    args.err = h->d_err;
    HIPCHK(h, hipMemsetAsync(h->d_err, 0xFF, 2 * sizeof(unsigned long long), h->stream));
    if (const int launched = launch_tiles(h, rows_kernel(h->C), args, lds)) return launched;
    const int64_t rows = n * (K + 1) * N;
    return unit_for_grid_chunks((rows + kBlock / 64 - 1) / (kBlock / 64), [&](int64_t first, int64_t count) {
        k_objloo_sum_features<<<(unsigned)count, kBlock, 0, h->stream>>>(h->d_lg, rows, (int)F, h->d_sums, first);
        HIPCHK(h, hipGetLastError());
        return SBE_OK;
    });
}

MixArgs mix_args(const sbe_objloo* h, const RowArgs& rows, int64_t n) {
    MixArgs a{};
    a.sums = h->d_sums;
    a.kid = h->d_kid;
    a.prior = rows.prior;
    a.uniform = rows.uniform;
    a.N = h->N;
    a.n = n;
    a.cap = h->cap;
    a.r0 = rows.t_first;
    a.K = h->K;
    a.H = h->d_H;
    a.A = h->d_A;
    a.L = h->L();
    a.Cnd = h->Cnd();
    a.err = h->d_err + 1;
    return a;
}

// the message of a call whose rows kernel met an observed cell to which no confounder applies
int no_confounder(sbe_objloo* h, unsigned long long key) {
    const long long cell = (long long)(key & ((1ull << 40) - 1));
    return fail(h, SBE_ERR_DATA, "cell (object %lld, feature %lld), sample %lld: no confounder applies to the object, so \"in no cluster\" gives the "
                "observed cell no likelihood", cell / h->F, cell % h->F, (long long)(key >> 40));
}

}  // namespace

extern "C" {

int sbe_objloo_abi_version(void) { return SBE_OBJLOO_ABI_VERSION; }

const char* sbe_objloo_last_error(const sbe_objloo* h) { return unit_last_error(h); }

int sbe_objloo_create(sbe_objloo** out, int device) { return unit_create_on_device(out, device, "sbe_objloo_create"); }

int sbe_objloo_destroy(sbe_objloo* h) { return unit_destroy(h, kNullHandle); }

int sbe_objloo_last_kernel_ms(const sbe_objloo* h, float* ms_out) { return unit_last_kernel_ms(h, ms_out, kNullHandle); }

int64_t sbe_objloo_store_bytes(int64_t n_objects, int n_clusters, int64_t capacity) {
    return n_objects < 0 || n_clusters < 1 || capacity < 0 || capacity > SBE_OBJLOO_MAX_SAMPLES ? -1 : store_bytes(n_objects, n_clusters, capacity);
}

int64_t sbe_objloo_sample_bytes(int64_t n_objects, int64_t n_features, int n_states, int n_components, int n_clusters, int n_rows) {
    return shape_ok(n_objects, n_features, n_states, n_components, n_clusters, n_rows)
               ? sample_bytes(n_objects, n_features, n_states, n_components, n_clusters, n_rows)
               : 0;
}

int64_t sbe_objloo_lds_max_samples(void) {
    static const int64_t v = [] {
        int64_t lo = 2, hi = SBE_OBJLOO_MAX_SAMPLES;             // (weights_lds_bytes grows with T)
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) / 2;
            if (weights_in_lds(mid)) lo = mid; else hi = mid - 1;
        }
        return lo;
    }();
    return v;
}

int sbe_objloo_set_feature_tile(sbe_objloo* h, int features) { return set_feature_tile(h, features); }

int sbe_objloo_set_data(sbe_objloo* h, int64_t N, int64_t F, int S, int C, int K, const uint8_t* codes, const uint8_t* groups, const int* n_groups,
                        int64_t capacity) {
    CHECK_HANDLE(h, kNullHandle);
    int row_off[kMaxC], R;
    if (const int bad = check_data(h, N, F, S, C, K, codes, groups, n_groups, row_off, R)) return bad;
    if (capacity < 1 || capacity > SBE_OBJLOO_MAX_SAMPLES)
        return fail(h, SBE_ERR_ARG, "capacity=%lld out of range [1, %d] (2^20 samples)", (long long)capacity, SBE_OBJLOO_MAX_SAMPLES);
    if (store_bytes(N, K, capacity) > SBE_OBJLOO_MAX_STORE_BYTES)
        return fail(h, SBE_ERR_ARG, "the rows and weights of %lld objects x %d hypotheses x %lld samples take %lld bytes on the device, the limit is %lld",
                    (long long)N, K + 1, (long long)capacity, (long long)store_bytes(N, K, capacity), (long long)SBE_OBJLOO_MAX_STORE_BYTES);
    const size_t columns = (size_t)N * (size_t)capacity, hyp = columns * (size_t)(K + 1);
    return h->upload(
        h, N, F, S, C, K, R, row_off, codes, groups,
        [&] {
            int rc = unit_ensure(h, h->d_p, h->p_bytes, 2 * (size_t)(N * F * S) * sizeof(double));
            if (!rc) rc = unit_ensure(h, h->d_H, h->H_bytes, hyp * sizeof(double));
            if (!rc) rc = unit_ensure(h, h->d_A, h->A_bytes, hyp * sizeof(double));
            if (!rc) rc = unit_ensure(h, h->d_cols, h->cols_bytes, 3 * columns * sizeof(double));
            if (!rc) rc = unit_ensure(h, h->d_out, h->out_bytes, (size_t)N * (size_t)(kOutputs + K + 1) * sizeof(double));
            if (!rc) rc = unit_ensure(h, h->d_err, 2 * sizeof(unsigned long long));
            return rc;
        },
        [&] {
            h->cap = capacity;
            return forget_rows(h);
        });
}

int sbe_objloo_reset(sbe_objloo* h) {
    CHECK_HANDLE(h, kNullHandle);
    if (!h->has_data) return no_data(h, kPrefix);
    HIPCHK(h, hipSetDevice(h->device));
    return forget_rows(h);
}

int sbe_objloo_add(sbe_objloo* h, int64_t n, const uint8_t* clusters, const double* weights, const double* tables, const double* prior) {
    CHECK_HANDLE(h, kNullHandle);
    if (!h->has_data) return no_data(h, kPrefix);
    if (n < 0) return fail(h, SBE_ERR_ARG, "n=%lld is negative", (long long)n);
    if (n == 0) return SBE_OK;
    if (h->n_rows + n > h->cap)
        return fail(h, SBE_ERR_ARG, "store overflow: %lld samples + %lld exceed the capacity of %lld samples", (long long)h->n_rows, (long long)n,
                    (long long)h->cap);
    RowArgs args;
    size_t lds;
    int rc = form_rows(h, n, h->n_rows, clusters, weights, tables, prior, args, lds);
    if (rc) return rc;
    const MixArgs mix = mix_args(h, args, n);
    k_objloo_mix<<<(unsigned)div_up(h->N * n, kBlock), kBlock, 0, h->stream>>>(mix);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipEventRecord(h->ev[1], h->stream));
    unsigned long long cell = kNoError, column = kNoError;
    if ((rc = unit_copy_back(h, (const unsigned long long*)h->d_err, 1, {&cell, &column}))) return rc;
    if ((rc = unit_sync_timed(h))) return rc;
    if (cell != kNoError) return no_confounder(h, cell);
    if (column != kNoError) {
        const long long obj = (long long)(column >> 21), t = (long long)((column >> 1) & ((1ull << 20) - 1));
        if (column & 1)
            return fail(h, SBE_ERR_DATA, "object %lld, sample %lld: the likelihood of its observed cells under the logged membership is zero; its "
                        "conditional importance weight would be infinite", obj, t);
        return fail(h, SBE_ERR_DATA, "object %lld, sample %lld: the marginal likelihood of its observed cells is zero or not finite: no membership "
                    "with a positive prior gives every observed cell a positive probability", obj, t);
    }
    h->n_rows += n;
    h->weighted = false;
    return SBE_OK;
}

int sbe_objloo_weights(sbe_objloo* h, double* loo_i, double* k_i, double* n_eff_i, double* lppd_i, double* loo_cond_i, double* k_cond_i,
                       double* lppd_cond_i, double* membership) {
    CHECK_HANDLE(h, kNullHandle);
    if (!h->has_data) return no_data(h, kPrefix);
    if (!loo_i || !k_i || !n_eff_i || !lppd_i || !loo_cond_i || !k_cond_i || !lppd_cond_i || !membership)
        return fail(h, SBE_ERR_ARG, "null pointer argument: %s", !loo_i ? "loo_i" : !k_i ? "k_i" : !n_eff_i ? "n_eff_i" : !lppd_i ? "lppd_i" :
                    !loo_cond_i ? "loo_cond_i" : !k_cond_i ? "k_cond_i" : !lppd_cond_i ? "lppd_cond_i" : "membership");
    const int64_t T = h->n_rows, N = h->N;
    if (T < SBE_ELPD_MIN_SAMPLES)
        return fail(h, SBE_ERR_STATE, "%lld samples stored; PSIS needs at least %d per object", (long long)T, SBE_ELPD_MIN_SAMPLES);
    HIPCHK(h, hipSetDevice(h->device));
    h->weighted = false;
    const bool lds = weights_in_lds(T);
    const int tail_n = ratio_tail_count(T);
    WeightArgs a{};
    a.L = h->L();
    a.Cnd = h->Cnd();
    a.A = h->d_A;
    a.w = h->w();
    a.cap = h->cap;
    a.N = N;
    a.T = (int)T;
    a.tail_n = tail_n;
    a.K = h->K;
    a.slice = T + tail_n + (T + 1) / 2;
    a.out = h->d_out;
    a.member = h->d_out + (size_t)kOutputs * (size_t)N;
    // workgroups per launch: what a grid holds and, on the global path, what the scratch has slices for
    int64_t per_launch = kMaxGridBlocks;
    if (!lds) {
        per_launch = std::min(2 * N, std::max<int64_t>(1, (int64_t)(kObjlooScratchBytes / ((size_t)a.slice * sizeof(double)))));
        if (const int rc = unit_ensure(h, h->d_work, h->work_bytes, (size_t)per_launch * (size_t)a.slice * sizeof(double))) return rc;
        a.work = h->d_work;
    }
    if (lds) HIPCHK(h, hipFuncSetAttribute((const void*)k_objloo_weights<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kLdsBudget - kObjlooStaticLds)));
    HIPCHK(h, hipMemsetAsync(h->d_p, 0, 2 * h->p_doubles() * sizeof(double), h->stream));
    h->next_t = 0;
    h->cur = 0;
    int rc = unit_timed(h, [&] {
        for (int64_t b0 = 0; b0 < 2 * N; b0 += per_launch) {
            const int64_t count = std::min(per_launch, 2 * N - b0);
            a.b0 = b0;
            if (lds)
                k_objloo_weights<true><<<(unsigned)count, kRatioBlock, weights_lds_bytes(T), h->stream>>>(a);
            else
                k_objloo_weights<false><<<(unsigned)count, kRatioBlock, 0, h->stream>>>(a);
            HIPCHK(h, hipGetLastError());
        }
        return (int)SBE_OK;
    });
    if (!rc) rc = unit_copy_back(h, (const double*)h->d_out, (size_t)N, {loo_i, k_i, n_eff_i, lppd_i, loo_cond_i, k_cond_i, lppd_cond_i});
    if (!rc) rc = unit_copy_back(h, (const double*)a.member, (size_t)N * (size_t)(h->K + 1), {membership});
    if (!rc) rc = unit_sync_timed(h);
    if (rc) return rc;
    h->weighted = true;
    return SBE_OK;
}

int sbe_objloo_accumulate(sbe_objloo* h, int64_t t0, int64_t n, const uint8_t* clusters, const double* weights, const double* tables,
                          const double* prior) {
    CHECK_HANDLE(h, kNullHandle);
    if (!h->has_data) return no_data(h, kPrefix);
    if (!h->weighted) return fail(h, SBE_ERR_STATE, "no weights yet (sbe_objloo_weights comes before sbe_objloo_accumulate)");
    if (n < 0) return fail(h, SBE_ERR_ARG, "n=%lld is negative", (long long)n);
    if (t0 != h->next_t || t0 + n > h->n_rows)
        return fail(h, SBE_ERR_STATE, "samples [%lld, %lld): the calls cover [0, %lld) in order without gaps, the next sample is %lld", (long long)t0,
                    (long long)(t0 + n), (long long)h->n_rows, (long long)h->next_t);
    if (n == 0) return SBE_OK;
    RowArgs args;
    size_t lds;
    int rc = form_rows(h, n, t0, clusters, weights, tables, prior, args, lds);
    if (rc) return rc;
    const MixArgs mix = mix_args(h, args, n);
    k_objloo_compare<<<(unsigned)div_up(h->N * n, kBlock), kBlock, 0, h->stream>>>(mix);
    HIPCHK(h, hipGetLastError());
    args.p_in = h->sums(h->cur);
    args.p_out = h->sums(1 - h->cur);
    args.w = h->w();
    if ((rc = launch_tiles(h, acc_kernel(h->S, h->C), args, lds))) return rc;
    HIPCHK(h, hipEventRecord(h->ev[1], h->stream));
    unsigned long long cell = kNoError, first = kNoError;
    if ((rc = unit_copy_back(h, (const unsigned long long*)h->d_err, 1, {&cell, &first}))) return rc;
    if ((rc = unit_sync_timed(h))) return rc;
    if (cell != kNoError) return no_confounder(h, cell);
    if (first != kNoError)
        return fail(h, SBE_ERR_DATA, "sample %lld: its rows differ from the ones sbe_objloo_add stored; the second pass takes the same samples and "
                    "priors in the same order", (long long)first);
    h->cur = 1 - h->cur;
    h->next_t += n;
    return SBE_OK;
}

int sbe_objloo_read(sbe_objloo* h, double* p_loo, int64_t* n_samples_out) {
    CHECK_HANDLE(h, kNullHandle);
    if (!h->has_data) return no_data(h, kPrefix);
    if (!n_samples_out) return fail(h, SBE_ERR_ARG, "null pointer argument: n_samples_out");
    HIPCHK(h, hipSetDevice(h->device));
    if (p_loo) {
        if (const int rc = copy_pieces(h, p_loo, h->sums(h->cur), h->p_doubles() * sizeof(double), hipMemcpyDeviceToHost)) return rc;
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    *n_samples_out = h->next_t;
    return SBE_OK;
}

int sbe_objloo_get_store(sbe_objloo* h, double* H, double* L, double* Cnd, double* w) {
    CHECK_HANDLE(h, kNullHandle);
    if (!h->has_data) return no_data(h, kPrefix);
    if (w && !h->weighted) return fail(h, SBE_ERR_STATE, "no weights yet (sbe_objloo_weights comes first)");
    if (h->n_rows == 0) return SBE_OK;
    HIPCHK(h, hipSetDevice(h->device));
    const size_t T = (size_t)h->n_rows * sizeof(double), pitch = (size_t)h->cap * sizeof(double), N = (size_t)h->N;
    if (H) HIPCHK(h, hipMemcpy2DAsync(H, T, h->d_H, pitch, T, N * (size_t)(h->K + 1), hipMemcpyDeviceToHost, h->stream));
    if (L) HIPCHK(h, hipMemcpy2DAsync(L, T, h->L(), pitch, T, N, hipMemcpyDeviceToHost, h->stream));
    if (Cnd) HIPCHK(h, hipMemcpy2DAsync(Cnd, T, h->Cnd(), pitch, T, N, hipMemcpyDeviceToHost, h->stream));
    if (w) HIPCHK(h, hipMemcpy2DAsync(w, T, h->w(), pitch, T, N, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return SBE_OK;
}

}  // extern "C"
