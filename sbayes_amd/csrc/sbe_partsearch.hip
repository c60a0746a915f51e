// sbe_partsearch.hip -- the search for the partition that minimises the expected VI or Binder loss (include/sbe_partsearch.h):
// the label store, the kernel that turns appended rows into labels, the persistent search kernel (one workgroup per start)
// and the evaluate kernel, which is what a search ends with.  The contract is tests/_partsearch_oracle.py; DESIGN.md section
// 27 has the layout, the kernels and the limits.
//
//   store:   lab[N][cap] uint8, object-major: the threads of a workgroup read one object's labels of 256 samples coalesced.
//   scratch: E[start][B][B][T_pad] uint16, B = K + 1, sample-minor.  Thread j of a start's workgroup owns the samples
//            t = j, j + 256, ..: nobody else reads or writes their columns, so the tables need no barrier.
//   LDS:     the candidate [N] and, while the tables are built, 256 columns of counters (two uint16 counts to a word).
//   order:   read from global memory, one step ahead (the header says so).
// Every thread of a workgroup ends a block reduction with the same values and so takes the same decision: the sizes a_q
// and the counters of a search live in registers, the same in every thread.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "sbe_unit.hip.h"
#include "../../include/sbe_partsearch.h"

namespace {

constexpr int kMaxK = SBE_PARTSEARCH_MAX_CLUSTERS;
constexpr int kMaxB = kMaxK + 1;                       // blocks of a partition: block 0 and the areas
constexpr int kMaxN = SBE_PARTSEARCH_MAX_OBJECTS;
constexpr int kBlock = SBE_PARTSEARCH_THREADS;
constexpr int kWaves = kBlock / 64;
constexpr int kCellWords = (kMaxB * kMaxB + 1) / 2;    // counter words of one sample while its tables are built
constexpr int kBatch = 8;                              // reads of a thread that are in flight together (a workgroup has one wave per SIMD)
static_assert(kBlock == 256 && kWaves == 4, "the contract's tree is 256 threads: four waves added in index order");
static_assert(kMaxN < (1 << 16), "a count fits a uint16, and two of them a counter word without a carry");
static_assert(kMaxN + (size_t)kCellWords * kBlock * 4 + 3 * kMaxB * kWaves * 8 < ((size_t)64 << 10), "the kernels' static LDS");

struct SearchArgs {
    const uint8_t* lab;       // [N][cap]
    int64_t cap, T_pad;
    int T, N, K;
    const double* L;          // [N + 1]
    const double* dL;         // [N]
    uint16_t* E;              // [n][B][B][T_pad]
    const uint8_t* init;      // [n][N]: the starts of a search, the candidates of an evaluation
    const int32_t* order;     // [n][N]                          (search)
    int max_sweeps;
    uint8_t* labels;          // [n][N]                          (search)
    int32_t* sweeps;          // [n]
    long long* moves;
    uint8_t* converged;
    double* trace;            // [n][max_sweeps] or null
    long long* bsum;          // [n]
    double* vsum;
    double* vi;               // [n][T] or null                  (evaluate)
    int32_t* binder;
};

// the LDS of a workgroup
struct Shared {
    uint32_t cnt[kCellWords * kBlock];
    double red_d[kMaxB * kWaves];
    long long red_l[kMaxB * kWaves];
    int red_i[kMaxB * kWaves];
    uint8_t cand[kMaxN];
};

// unit_block_reduce<kWaves> with unit_sum of the B values v[0 .. B), with one pair of barriers for all of them: per value
// the same tree, the lanes by xor exchanges, then the waves in index order.  red: [kMaxB][kWaves]
template <class T>
__device__ inline void reduce_blocks(T (&v)[kMaxB], int B, T* red) {
#pragma unroll
    for (int q = 0; q < kMaxB; ++q)
        if (q < B) v[q] = unit_wave_reduce(v[q], unit_sum());
    __syncthreads();                                   // (red may still be read by the previous reduction)
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int q = 0; q < kMaxB; ++q)
            if (q < B) red[q * kWaves + (threadIdx.x >> 6)] = v[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kMaxB; ++q) {
        if (q >= B) continue;
        T t = red[q * kWaves];
        for (int w = 1; w < kWaves; ++w) t = t + red[q * kWaves + w];
        v[q] = t;
    }
}

// ---- dL[m] = L[m + 1] - L[m], m < N --------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_partsearch_dl(const double* L, int N, double* dL) {
    const int m = blockIdx.x * kBlock + threadIdx.x;
    if (m < N) dL[m] = L[m + 1] - L[m];
}

// ---- host bytes [n][K][N] (staging) -> label rows [n][N]: 0 for no area, k + 1 for area k -------------------------------------
// blockIdx.x + s0: the sample within the piece, blockIdx.y: kBlock objects
__global__ __launch_bounds__(kBlock) void k_partsearch_labels(const uint8_t* rows, int64_t n, int K, int N, uint8_t* out, int64_t s0) {
    const int64_t s = s0 + blockIdx.x;
    const int i = blockIdx.y * kBlock + threadIdx.x;
    if (s >= n || i >= N) return;
    uint8_t label = 0;
    for (int k = 0; k < K; ++k)
        if (rows[(s * K + k) * N + i]) label = (uint8_t)(k + 1);
    out[s * N + i] = label;
}

// the candidate of workgroup s into LDS (a label beyond K cannot index a table: the host has refused it)
__device__ inline void load_candidate(const SearchArgs& g, int64_t s, Shared& sh) {
    for (int i = threadIdx.x; i < g.N; i += kBlock) sh.cand[i] = (uint8_t)min((int)g.init[s * g.N + i], g.K);
    __syncthreads();
}

// The tables of the candidate in LDS against every sample, and its sizes a[0 .. B).  256 samples at a time: a thread counts
// its sample's (q, l) cells in its own column of counter words (adds without a return value: the LDS runs them in order).
__device__ inline void build_tables(const SearchArgs& g, uint16_t* E, Shared& sh, int (&a)[kMaxB]) {
    const int B = g.K + 1, cells = B * B, words = (cells + 1) / 2;
    for (int64_t t0 = 0; t0 < g.T_pad; t0 += kBlock) {
        const int64_t t = t0 + threadIdx.x;
        for (int w = 0; w < words; ++w) sh.cnt[w * kBlock + threadIdx.x] = 0;
        if (t < g.T)
            for (int i0 = 0; i0 < g.N; i0 += kBatch) {   // (the labels of kBatch objects are in flight together)
                int y[kBatch];
#pragma unroll
                for (int u = 0; u < kBatch; ++u) y[u] = i0 + u < g.N ? min((int)g.lab[(i0 + u) * g.cap + t], g.K) : 0;
#pragma unroll
                for (int u = 0; u < kBatch; ++u) {
                    if (i0 + u >= g.N) continue;
                    const int cell = (int)sh.cand[i0 + u] * B + y[u];
                    atomicAdd(&sh.cnt[(cell >> 1) * kBlock + threadIdx.x], 1u << (16 * (cell & 1)));
                }
            }
        for (int cell = 0; cell < cells; ++cell)        // (the columns behind T hold zeros)
            E[cell * g.T_pad + t] = (uint16_t)(sh.cnt[(cell >> 1) * kBlock + threadIdx.x] >> (16 * (cell & 1)));
    }
#pragma unroll
    for (int q = 0; q < kMaxB; ++q) a[q] = 0;
    for (int i = threadIdx.x; i < g.N; i += kBlock) {
        const int c = sh.cand[i];
#pragma unroll
        for (int q = 0; q < kMaxB; ++q) a[q] += c == q;
    }
    reduce_blocks(a, B, sh.red_i);
}

// The losses of the tables' candidate against every sample, in the contract's order; vsum in the contract's tree, bsum
// exact: in every thread.  s: the row of the per-sample outputs, where they are asked for.
__device__ inline void evaluate_tables(const SearchArgs& g, const uint16_t* E, Shared& sh, const int (&a)[kMaxB], int64_t s, double& vsum, long long& bsum) {
    const int B = g.K + 1, N = g.N;
    const double* L = g.L;
    auto lx = [&](int e) { return L[e < 0 ? 0 : e > N ? N : e]; };      // (a count lies in [0, N])
    double hc = 0.0;
    int a_squares = 0;
#pragma unroll
    for (int q = 0; q < kMaxB; ++q) {
        if (q >= B) continue;
        hc += lx(a[q]);
        if (q >= 1) a_squares += a[q] * a[q];
    }
    double v = 0.0;
    long long b = 0;
    for (int t = threadIdx.x; t < g.T; t += kBlock) {
        int bl[kMaxB];
#pragma unroll
        for (int l = 0; l < kMaxB; ++l) bl[l] = 0;
        double j = 0.0;
        int n2 = 0;
#pragma unroll
        for (int q = 0; q < kMaxB; ++q) {
            if (q >= B) continue;
#pragma unroll
            for (int l = 0; l < kMaxB; ++l) {
                if (l >= B) continue;
                const int e = (int)E[(q * B + l) * g.T_pad + t];
                j += lx(e);
                bl[l] += e;
                if (q >= 1 && l >= 1) n2 += e * e;
            }
        }
        double ht = 0.0;
        int b_squares = 0;
#pragma unroll
        for (int l = 0; l < kMaxB; ++l) {
            if (l >= B) continue;
            ht += lx(bl[l]);
            if (l >= 1) b_squares += bl[l] * bl[l];
        }
        const double vi = fmax(0.0, ((hc + ht) - 2.0 * j) / (double)N);
        const int binder = a_squares + b_squares - 2 * n2;
        if (g.vi) g.vi[s * g.T + t] = vi;
        if (g.binder) g.binder[s * g.T + t] = binder;
        v += vi;
        b += binder;
    }
    vsum = unit_block_reduce<kWaves>(v, sh.red_d, unit_sum());
    bsum = unit_block_reduce<kWaves>(b, sh.red_l, unit_sum());
}

// ---- evaluate: one workgroup per candidate ----------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_partsearch_evaluate(const SearchArgs g, int64_t s0) {
    __shared__ Shared sh;
    const int64_t s = s0 + blockIdx.x;
    const int B = g.K + 1;
    uint16_t* E = g.E + s * B * B * g.T_pad;
    int a[kMaxB];
    load_candidate(g, s, sh);
    build_tables(g, E, sh, a);
    double vsum;
    long long bsum;
    evaluate_tables(g, E, sh, a, s, vsum, bsum);
    if (threadIdx.x == 0) {
        g.vsum[s] = vsum;
        g.bsum[s] = bsum;
    }
}

// ---- search: one workgroup per start, persistent over all sweeps ------------------------------------------------------------
// The scores of the contract for an object with label p and the labels y[t] of the thread's samples read again from the
// store: g(q) from the entries E_t[q][y[t]] less the object itself where q = p (the tables are written only when it moves).
template <int kLoss>
__device__ inline int choose_block(const SearchArgs& g, const uint16_t* E, Shared& sh, const int (&a)[kMaxB], int i, int p) {
    const int B = g.K + 1, T = g.T;
    const uint8_t* y_of = g.lab + (int64_t)i * g.cap;
    int best = 0;
    if constexpr (kLoss == SBE_PARTSEARCH_LOSS_VI) {
        const double* dL = g.dL;
        const int top = g.N - 1;
        double part[kMaxB];
#pragma unroll
        for (int q = 0; q < kMaxB; ++q) part[q] = 0.0;
        // kBatch samples of the thread at a time: their labels, then their entries, then the entries' dL are in flight
        // together (a step is three dependent reads deep); the sums take them in the order of t
        for (int t0 = threadIdx.x; t0 < T; t0 += kBatch * kBlock) {
            int y[kBatch];
            double d[kBatch][kMaxB];
#pragma unroll
            for (int u = 0; u < kBatch; ++u) y[u] = t0 + u * kBlock < T ? min((int)y_of[t0 + u * kBlock], g.K) : 0;
#pragma unroll
            for (int u = 0; u < kBatch; ++u) {
                const int t = t0 + u * kBlock;
#pragma unroll
                for (int q = 0; q < kMaxB; ++q) {
                    if (q >= B || t >= T) continue;
                    const int e = (int)E[(q * B + y[u]) * g.T_pad + t] - (q == p);
                    d[u][q] = dL[e < 0 ? 0 : e > top ? top : e];
                }
            }
#pragma unroll
            for (int u = 0; u < kBatch; ++u) {
                if (t0 + u * kBlock >= T) continue;
#pragma unroll
                for (int q = 0; q < kMaxB; ++q)
                    if (q < B) part[q] += d[u][q];
            }
        }
        reduce_blocks(part, B, sh.red_d);
        double least = 0.0, mine = 0.0;
#pragma unroll
        for (int q = 0; q < kMaxB; ++q) {
            if (q >= B) continue;
            const int size = a[q] - (q == p);
            const double gq = (double)T * dL[size < 0 ? 0 : size > top ? top : size] - 2.0 * part[q];
            if (q == 0 || gq < least) {
                least = gq;
                best = q;
            }
            if (q == p) mine = gq;
        }
        if (mine == least) best = p;
    } else {
        long long part[kMaxB];
#pragma unroll
        for (int q = 0; q < kMaxB; ++q) part[q] = 0;
        for (int t0 = threadIdx.x; t0 < T; t0 += kBatch * kBlock) {
            int y[kBatch];
#pragma unroll
            for (int u = 0; u < kBatch; ++u) y[u] = t0 + u * kBlock < T ? min((int)y_of[t0 + u * kBlock], g.K) : 0;
#pragma unroll
            for (int u = 0; u < kBatch; ++u) {
                if (y[u] == 0) continue;                // (a sample behind T, or the object in no area: no term)
#pragma unroll
                for (int q = 1; q < kMaxB; ++q) {
                    if (q >= B) continue;
                    part[q] += 2 * ((int)E[(q * B + y[u]) * g.T_pad + t0 + u * kBlock] - (q == p)) + 1;
                }
            }
        }
        reduce_blocks(part, B, sh.red_l);
        long long least = 0, mine = 0;                  // g(0) = 0
#pragma unroll
        for (int q = 1; q < kMaxB; ++q) {
            if (q >= B) continue;
            const long long gq = (long long)T * (2 * (a[q] - (q == p)) + 1) - 2 * part[q];
            if (gq < least) {
                least = gq;
                best = q;
            }
            if (q == p) mine = gq;
        }
        if (mine == least) best = p;
    }
    return best;
}

template <int kLoss>
__global__ __launch_bounds__(kBlock) void k_partsearch_search(const SearchArgs g, int64_t s0) {
    __shared__ Shared sh;
    const int64_t s = s0 + blockIdx.x;
    const int B = g.K + 1, N = g.N;
    uint16_t* E = g.E + s * B * B * g.T_pad;
    const int32_t* order = g.order + s * N;
    int a[kMaxB];
    load_candidate(g, s, sh);
    build_tables(g, E, sh, a);
    int sweeps = 0, converged = 0;
    long long moves = 0;
    double vsum;
    long long bsum;
    while (sweeps < g.max_sweeps) {
        int moved = 0;
        int next = order[0];
        for (int step = 0; step < N; ++step) {
            const int i = next;
            if (step + 1 < N) next = order[step + 1];
            const int p = sh.cand[i];
            const int q = choose_block<kLoss>(g, E, sh, a, i, p);      // (the same in every thread)
            if (q == p) continue;
            const uint8_t* y_of = g.lab + (int64_t)i * g.cap;
#pragma unroll 4
            for (int t = threadIdx.x; t < g.T; t += kBlock) {
                const int y = min((int)y_of[t], g.K);
                E[(p * B + y) * g.T_pad + t] -= 1;
                E[(q * B + y) * g.T_pad + t] += 1;
            }
#pragma unroll
            for (int k = 0; k < kMaxB; ++k) a[k] += (k == q) - (k == p);
            // (every thread has read cand[i] before the barriers of the reduction, and an object comes once per sweep)
            if (threadIdx.x == 0) sh.cand[i] = (uint8_t)q;
            ++moved;
        }
        __syncthreads();                                // the candidate as the sweep left it, for the next sweep's reads
        moves += moved;
        if (g.trace) {
            evaluate_tables(g, E, sh, a, s, vsum, bsum);
            if (threadIdx.x == 0) g.trace[s * g.max_sweeps + sweeps] = kLoss == SBE_PARTSEARCH_LOSS_VI ? vsum : (double)bsum;
        }
        ++sweeps;
        if (!moved) {
            converged = 1;
            break;
        }
    }
    evaluate_tables(g, E, sh, a, s, vsum, bsum);
    for (int i = threadIdx.x; i < N; i += kBlock) g.labels[s * N + i] = sh.cand[i];
    if (g.trace)
        for (int w = sweeps + threadIdx.x; w < g.max_sweeps; w += kBlock) g.trace[s * g.max_sweeps + w] = __longlong_as_double(0x7ff8000000000000ll);
    if (threadIdx.x == 0) {
        g.sweeps[s] = sweeps;
        g.moves[s] = moves;
        g.converged[s] = (uint8_t)converged;
        g.vsum[s] = vsum;
        g.bsum[s] = bsum;
    }
}

template <class T>
struct Buffer {
    T* d = nullptr;
    size_t bytes = 0;
};

}  // namespace

struct sbe_partsearch : sbe_unit_handle {              // (ev: around the kernel of the last search or evaluate)
    bool shaped = false;
    int K = 0;
    int64_t N = 0, cap = 0, rows = 0;
    Buffer<uint8_t> lab;                // [N][cap]
    Buffer<uint8_t> row_labels;         // [piece][N]: the labels of a piece before they are filed
    void* d_stage = nullptr;            // host rows in flight
    size_t stage_bytes = 0;
    Buffer<double> xlogx, dl;           // [N + 1], [N]
    Buffer<uint16_t> tables;            // [n][B][B][T_pad]
    Buffer<uint8_t> init, labels, converged;
    Buffer<int32_t> order, sweeps, binder;
    Buffer<long long> moves, bsum;
    Buffer<double> vsum, trace, vi;
    std::vector<void*> buffers() const {
        return {lab.d, row_labels.d, d_stage, xlogx.d, dl.d, tables.d, init.d, labels.d, converged.d, order.d, sweeps.d, binder.d, moves.d, bsum.d, vsum.d,
                trace.d, vi.d};
    }
};

namespace {

constexpr char kNullHandle[] = "null handle";
constexpr char kReset[] = "sbe_partsearch_reset";

int64_t padded_samples(int64_t T) { return (T + kBlock - 1) / kBlock * kBlock; }

bool scratch_shape_ok(int K, int64_t T, int64_t n) {
    return K >= 1 && K <= kMaxK && T >= 1 && T <= SBE_PARTSEARCH_MAX_ROWS && n >= 1 && n <= kMaxGridBlocks;
}

int64_t scratch_bytes(int K, int64_t T, int64_t n) { return n * (K + 1) * (K + 1) * padded_samples(T) * (int64_t)sizeof(uint16_t); }

template <class T>
int ensure(sbe_partsearch* h, Buffer<T>& b, size_t count) { return unit_ensure(h, b.d, b.bytes, std::max<size_t>(count, 1) * sizeof(T)); }

// the state and count checks search and evaluate share; `what` names the count's argument and its things
int check_call(sbe_partsearch* h, const char* what, const char* things, int64_t n) {
    if (!h->shaped) return fail(h, SBE_ERR_STATE, "the store has no shape yet (%s)", kReset);
    if (h->rows == 0) return fail(h, SBE_ERR_STATE, "the store holds no rows");
    if (n < 1 || n > kMaxGridBlocks) return fail(h, SBE_ERR_ARG, "%s=%lld out of range [1, %lld]", what, (long long)n, (long long)kMaxGridBlocks);
    const int64_t need = scratch_bytes(h->K, h->rows, n);
    if (need > SBE_PARTSEARCH_MAX_SCRATCH_BYTES)
        return fail(h, SBE_ERR_ARG, "the tables of %lld %s against %lld samples of %d clusters take %lld bytes, the limit of one call is %lld", (long long)n,
                    things, (long long)h->rows, h->K, (long long)need, (long long)SBE_PARTSEARCH_MAX_SCRATCH_BYTES);
    return SBE_OK;
}

// labels [n][N] in 0..K; `name`: the argument
int check_labels(sbe_partsearch* h, const char* name, const uint8_t* labels, int64_t n) {
    for (int64_t s = 0; s < n; ++s)
        for (int64_t i = 0; i < h->N; ++i)
            if (labels[s * h->N + i] > h->K)
                return fail(h, SBE_ERR_DATA, "%s[%lld][%lld]=%d is not a label in [0, %d]", name, (long long)s, (long long)i, (int)labels[s * h->N + i], h->K);
    return SBE_OK;
}

int check_orders(sbe_partsearch* h, const int32_t* order, int64_t n) {
    std::vector<uint8_t> seen((size_t)h->N);
    for (int64_t s = 0; s < n; ++s) {
        std::fill(seen.begin(), seen.end(), (uint8_t)0);
        for (int64_t i = 0; i < h->N; ++i) {
            const int32_t at = order[s * h->N + i];
            if (at < 0 || at >= h->N)
                return fail(h, SBE_ERR_DATA, "order[%lld][%lld]=%d is not an object in [0, %lld): the order of a start must be a permutation", (long long)s,
                            (long long)i, (int)at, (long long)h->N);
            if (seen[(size_t)at])
                return fail(h, SBE_ERR_DATA, "order[%lld][%lld]=%d comes a second time: the order of a start must be a permutation", (long long)s, (long long)i,
                            (int)at);
            seen[(size_t)at] = 1;
        }
    }
    return SBE_OK;
}

// the host scan of an appended call: 0 / 1 bytes and disjoint areas per sample
int scan_rows(sbe_partsearch* h, const uint8_t* rows, int64_t n_rows) {
    const int K = h->K;
    const int64_t N = h->N;
    std::vector<uint8_t> held((size_t)N);
    for (int64_t s = 0; s < n_rows; ++s) {
        const uint8_t* sample = rows + s * K * N;
        std::fill(held.begin(), held.end(), (uint8_t)0);
        uint8_t any = 0;
        for (int k = 0; k < K; ++k)
            for (int64_t i = 0; i < N; ++i) {
                any |= sample[k * N + i];
                held[(size_t)i] = (uint8_t)(held[(size_t)i] + (sample[k * N + i] != 0));
            }
        if (any > 1) {
            int64_t q = 0;
            while (sample[q] <= 1) ++q;
            return fail(h, SBE_ERR_DATA, "rows[%lld][%lld][%lld]=%d is neither 0 nor 1", (long long)s, (long long)(q / N), (long long)(q % N), (int)sample[q]);
        }
        for (int64_t i = 0; i < N; ++i)
            if (held[(size_t)i] > 1)
                return fail(h, SBE_ERR_DATA, "rows[%lld]: object %lld is in %d areas of the sample (the areas of a sample must be disjoint)", (long long)s,
                            (long long)i, (int)held[(size_t)i]);
    }
    return SBE_OK;
}

SearchArgs common_args(const sbe_partsearch* h) {
    SearchArgs g{};
    g.lab = h->lab.d;
    g.cap = h->cap;
    g.T = (int)h->rows;
    g.T_pad = padded_samples(h->rows);
    g.N = (int)h->N;
    g.K = h->K;
    g.L = h->xlogx.d;
    g.dL = h->dl.d;
    g.E = h->tables.d;
    g.init = h->init.d;
    g.bsum = h->bsum.d;
    g.vsum = h->vsum.d;
    return g;
}

}  // namespace

extern "C" {

int sbe_partsearch_abi_version(void) { return SBE_PARTSEARCH_ABI_VERSION; }

const char* sbe_partsearch_last_error(const sbe_partsearch* h) { return unit_last_error(h); }

int64_t sbe_partsearch_scratch_bytes(int n_clusters, int64_t n_samples, int64_t n_starts) {
    return scratch_shape_ok(n_clusters, n_samples, n_starts) ? scratch_bytes(n_clusters, n_samples, n_starts) : 0;
}

int sbe_partsearch_create(sbe_partsearch** out, int device) { return unit_create_on_device(out, device, "sbe_partsearch_create"); }

int sbe_partsearch_destroy(sbe_partsearch* h) { return unit_destroy(h, kNullHandle); }

int sbe_partsearch_last_kernel_ms(const sbe_partsearch* h, float* ms_out) { return unit_last_kernel_ms(h, ms_out, kNullHandle); }

int sbe_partsearch_reset(sbe_partsearch* h, int n_clusters, int64_t n_objects, int64_t capacity_rows, const double* xlogx) {
    CHECK_HANDLE(h, kNullHandle);
    if (n_clusters < 1 || n_clusters > kMaxK) return fail(h, SBE_ERR_ARG, "n_clusters=%d out of range [1, %d]", n_clusters, kMaxK);
    if (n_objects < 1 || n_objects > kMaxN)
        return fail(h, SBE_ERR_ARG, "n_objects=%lld out of range [1, %d] (a count fits a uint16, 2 N^2 an int32)", (long long)n_objects, kMaxN);
    if (capacity_rows < 1 || capacity_rows > SBE_PARTSEARCH_MAX_ROWS)
        return fail(h, SBE_ERR_ARG, "capacity_rows=%lld out of range [1, %d]", (long long)capacity_rows, SBE_PARTSEARCH_MAX_ROWS);
    if (!xlogx) return fail(h, SBE_ERR_ARG, "null pointer argument: xlogx");
    h->shaped = false;                                    // (a failed allocation leaves an unshaped store)
    h->rows = 0;
    HIPCHK(h, hipSetDevice(h->device));
    int rc = ensure(h, h->lab, (size_t)n_objects * (size_t)capacity_rows);
    if (!rc) rc = ensure(h, h->xlogx, (size_t)n_objects + 1);
    if (!rc) rc = ensure(h, h->dl, (size_t)n_objects);
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(h->xlogx.d, xlogx, ((size_t)n_objects + 1) * sizeof(double), hipMemcpyHostToDevice, h->stream));
    k_partsearch_dl<<<(unsigned)div_up(n_objects, kBlock), kBlock, 0, h->stream>>>(h->xlogx.d, (int)n_objects, h->dl.d);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->K = n_clusters;
    h->N = n_objects;
    h->cap = capacity_rows;
    h->shaped = true;
    return SBE_OK;
}

int sbe_partsearch_rows(const sbe_partsearch* h, int64_t* n_rows_out) {
    CHECK_HANDLE(h, kNullHandle);
    if (!n_rows_out) return fail(h, SBE_ERR_ARG, "null pointer argument: n_rows_out");
    if (!h->shaped) return fail(h, SBE_ERR_STATE, "the store has no shape yet (%s)", kReset);
    *n_rows_out = h->rows;
    return SBE_OK;
}

int sbe_partsearch_append_rows(sbe_partsearch* h, const uint8_t* rows, int64_t n_rows) {
    CHECK_HANDLE(h, kNullHandle);
    if (!h->shaped) return fail(h, SBE_ERR_STATE, "the store has no shape yet (%s)", kReset);
    if (n_rows < 0) return fail(h, SBE_ERR_ARG, "n_rows=%lld is negative", (long long)n_rows);
    if (n_rows > 0 && !rows) return fail(h, SBE_ERR_ARG, "null pointer argument: rows");
    if (h->rows + n_rows > h->cap)
        return fail(h, SBE_ERR_ARG, "store overflow: the store holds %lld rows, %lld more exceed the capacity of %lld rows", (long long)h->rows,
                    (long long)n_rows, (long long)h->cap);
    if (n_rows == 0) return SBE_OK;
    if (const int rc = scan_rows(h, rows, n_rows)) return rc;     // (before the first piece: a refused call leaves the store as it was)
    HIPCHK(h, hipSetDevice(h->device));
    const int64_t N = h->N, row_bytes = (int64_t)h->K * N;
    int rc = ensure(h, h->row_labels, (size_t)unit_piece_rows(row_bytes, h->cap) * (size_t)N);
    if (!rc)
        rc = unit_append_pieces(h, h->d_stage, h->stage_bytes, rows, n_rows, row_bytes, h->cap, [&](int64_t k, int64_t r) {
            const int lrc = unit_for_grid_chunks(k, [&](int64_t s0, int64_t n) {
                k_partsearch_labels<<<dim3((unsigned)n, (unsigned)div_up(N, kBlock)), kBlock, 0, h->stream>>>((const uint8_t*)h->d_stage, k, h->K, (int)N,
                                                                                                           h->row_labels.d, s0);
                HIPCHK(h, hipGetLastError());
                return SBE_OK;
            });
            if (lrc) return lrc;
            return unit_for_grid_chunks((N + 31) / 32, [&](int64_t t0, int64_t tiles) {
                k_unit_transpose<<<dim3((unsigned)tiles, (unsigned)((k + 31) / 32)), 256, 0, h->stream>>>((const uint8_t*)h->row_labels.d, k, N, h->lab.d, h->cap,
                                                                                                         h->rows + r, t0);
                HIPCHK(h, hipGetLastError());
                return SBE_OK;
            });
        });
    // a piece may be in the store already while the row count is not: the store is unshaped instead (reset comes next)
    if (rc) {
        h->shaped = false;
        return rc;
    }
    h->rows += n_rows;
    return SBE_OK;
}

int sbe_partsearch_search(sbe_partsearch* h, int loss, int64_t n_starts, const uint8_t* init, const int32_t* order, int max_sweeps,
                          uint8_t* labels_out, int32_t* sweeps_out, int64_t* moves_out, uint8_t* converged_out, int64_t* binder_sum_out,
                          double* vi_sum_out, double* trace_out) {
    CHECK_HANDLE(h, kNullHandle);
    if (loss != SBE_PARTSEARCH_LOSS_VI && loss != SBE_PARTSEARCH_LOSS_BINDER)
        return fail(h, SBE_ERR_ARG, "loss=%d is neither SBE_PARTSEARCH_LOSS_VI (0) nor SBE_PARTSEARCH_LOSS_BINDER (1)", loss);
    if (max_sweeps < 1 || max_sweeps > SBE_PARTSEARCH_MAX_SWEEPS)
        return fail(h, SBE_ERR_ARG, "max_sweeps=%d out of range [1, %d]", max_sweeps, SBE_PARTSEARCH_MAX_SWEEPS);
    if (const int rc = check_call(h, "n_starts", "starts", n_starts)) return rc;
    const char* null_arg = !init ? "init" : !order ? "order" : !labels_out ? "labels_out" : !sweeps_out ? "sweeps_out" : !moves_out ? "moves_out"
                           : !converged_out ? "converged_out" : !binder_sum_out ? "binder_sum_out" : !vi_sum_out ? "vi_sum_out" : nullptr;
    if (null_arg) return fail(h, SBE_ERR_ARG, "null pointer argument: %s", null_arg);
    if (const int rc = check_labels(h, "init", init, n_starts)) return rc;
    if (const int rc = check_orders(h, order, n_starts)) return rc;
    const size_t n = (size_t)n_starts, cells = n * (size_t)h->N, steps = n * (size_t)max_sweeps;
    HIPCHK(h, hipSetDevice(h->device));
    int rc = ensure(h, h->tables, (size_t)scratch_bytes(h->K, h->rows, n_starts) / sizeof(uint16_t));
    if (!rc) rc = ensure(h, h->init, cells);
    if (!rc) rc = ensure(h, h->order, cells);
    if (!rc) rc = ensure(h, h->labels, cells);
    if (!rc) rc = ensure(h, h->sweeps, n);
    if (!rc) rc = ensure(h, h->moves, n);
    if (!rc) rc = ensure(h, h->converged, n);
    if (!rc) rc = ensure(h, h->bsum, n);
    if (!rc) rc = ensure(h, h->vsum, n);
    if (!rc && trace_out) rc = ensure(h, h->trace, steps);
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(h->init.d, init, cells, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->order.d, order, cells * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    SearchArgs g = common_args(h);
    g.order = h->order.d;
    g.max_sweeps = max_sweeps;
    g.labels = h->labels.d;
    g.sweeps = h->sweeps.d;
    g.moves = h->moves.d;
    g.converged = h->converged.d;
    g.trace = trace_out ? h->trace.d : nullptr;
    rc = unit_timed(h, [&] {
        return unit_for_grid_chunks(n_starts, [&](int64_t s0, int64_t count) {
            if (loss == SBE_PARTSEARCH_LOSS_VI)
                k_partsearch_search<SBE_PARTSEARCH_LOSS_VI><<<(unsigned)count, kBlock, 0, h->stream>>>(g, s0);
            else
                k_partsearch_search<SBE_PARTSEARCH_LOSS_BINDER><<<(unsigned)count, kBlock, 0, h->stream>>>(g, s0);
            HIPCHK(h, hipGetLastError());
            return SBE_OK;
        });
    });
    if (!rc) rc = unit_copy_back(h, (const uint8_t*)h->labels.d, cells, {labels_out});
    if (!rc) rc = unit_copy_back(h, (const int32_t*)h->sweeps.d, n, {sweeps_out});
    if (!rc) rc = unit_copy_back(h, (const int64_t*)h->moves.d, n, {moves_out});
    if (!rc) rc = unit_copy_back(h, (const uint8_t*)h->converged.d, n, {converged_out});
    if (!rc) rc = unit_copy_back(h, (const int64_t*)h->bsum.d, n, {binder_sum_out});
    if (!rc) rc = unit_copy_back(h, (const double*)h->vsum.d, n, {vi_sum_out});
    if (!rc && trace_out) rc = unit_copy_back(h, (const double*)h->trace.d, steps, {trace_out});
    if (!rc) rc = unit_sync_timed(h);
    return rc;
}

int sbe_partsearch_evaluate(sbe_partsearch* h, int64_t n, const uint8_t* labels, double* vi_out, int32_t* binder_out, double* vi_sum_out,
                            int64_t* binder_sum_out) {
    CHECK_HANDLE(h, kNullHandle);
    if (const int rc = check_call(h, "n", "candidates", n)) return rc;
    if (!labels) return fail(h, SBE_ERR_ARG, "null pointer argument: labels");
    if (!vi_out && !binder_out && !vi_sum_out && !binder_sum_out)
        return fail(h, SBE_ERR_ARG, "null pointer argument: vi_out, binder_out, vi_sum_out and binder_sum_out (at least one is needed)");
    if (const int rc = check_labels(h, "labels", labels, n)) return rc;
    const size_t count = (size_t)n, cells = count * (size_t)h->N, entries = count * (size_t)h->rows;
    HIPCHK(h, hipSetDevice(h->device));
    int rc = ensure(h, h->tables, (size_t)scratch_bytes(h->K, h->rows, n) / sizeof(uint16_t));
    if (!rc) rc = ensure(h, h->init, cells);
    if (!rc) rc = ensure(h, h->bsum, count);
    if (!rc) rc = ensure(h, h->vsum, count);
    if (!rc && vi_out) rc = ensure(h, h->vi, entries);
    if (!rc && binder_out) rc = ensure(h, h->binder, entries);
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(h->init.d, labels, cells, hipMemcpyHostToDevice, h->stream));
    SearchArgs g = common_args(h);
    g.vi = vi_out ? h->vi.d : nullptr;
    g.binder = binder_out ? h->binder.d : nullptr;
    rc = unit_timed(h, [&] {
        return unit_for_grid_chunks(n, [&](int64_t s0, int64_t chunk) {
            k_partsearch_evaluate<<<(unsigned)chunk, kBlock, 0, h->stream>>>(g, s0);
            HIPCHK(h, hipGetLastError());
            return SBE_OK;
        });
    });
    if (!rc && vi_out) rc = unit_copy_back(h, (const double*)h->vi.d, entries, {vi_out});
    if (!rc && binder_out) rc = unit_copy_back(h, (const int32_t*)h->binder.d, entries, {binder_out});
    if (!rc && vi_sum_out) rc = unit_copy_back(h, (const double*)h->vsum.d, count, {vi_sum_out});
    if (!rc && binder_sum_out) rc = unit_copy_back(h, (const int64_t*)h->bsum.d, count, {binder_sum_out});
    if (!rc) rc = unit_sync_timed(h);
    return rc;
}

}  // extern "C"
