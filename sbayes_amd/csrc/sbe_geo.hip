// sbe_geo.hip -- the cost-based geo prior on the device (include/sbe_geo.h): per cluster mask the minimum spanning tree of
// the members' cost sub-matrix (or the whole sub-matrix), its aggregate and the prior's probability function, and per
// object the change of that log-probability if the object joined.  The numerical contract is tests/_geo_oracle.py;
// DESIGN.md section 14 has the layout, the limits and the measurements.
//
// k_geo_skeleton, one workgroup of 256 threads per mask:
//   1. the member indices are compacted in ascending order into the launch's scratch (a count per thread over its
//      stretch of the mask, a scan over the workgroup, then the writes);
//   2. MST skeleton: Prim's algorithm from member 0.  Thread t owns the keys of members t, t + 256, ...; in a step it
//      lowers them by the row of the member added last and takes its own smallest, the wave reduces (key, member) by
//      cross-lane exchange, the four waves meet through one LDS exchange (double-buffered: one barrier per step), and
//      every thread knows the next member.  Ties go to the lowest member, so the order of the edges, and with it the
//      sum, is fixed.  A mask of up to SBE_GEO_LDS_MEMBERS members first stages its m x m sub-matrix in LDS with all
//      loads in flight at once (every entry is read once either way: what the staging removes is m dependent trips to
//      memory); a larger one reads one cost row per step from memory and keeps its keys in scratch.  Both paths do the
//      same arithmetic in the same order;
//      complete skeleton: thread t adds entries t, t + 256, ... of the sub-matrix in order, then a fixed tree over LDS;
//   3. thread 0 writes m, n_edges, sum, max and the probability function of the aggregate.
// k_geo_per_object: 64 objects per workgroup, the member rows dealt to its four waves (coalesced along the row), the four
// minima joined through LDS (a minimum is exact in any order), then after and f(after) - f(before) per object.
// Every loop is bounded by m or N; no workgroup waits for another.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <limits>
#include <vector>

#include "sbe_unit.hip.h"
#include "../../include/sbe_geo.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kCols = 64;                           // objects per workgroup of k_geo_per_object
constexpr int64_t kScratchEntries = (int64_t)1 << 24;   // masks * N per launch by default: 13 bytes of scratch each
constexpr size_t kPerObjectOffset = 24;             // the per-object outputs start 64 bytes into the output buffer of one mask

// ---- the probability function ---------------------------------------------------------------------------------------
__device__ inline double geo_log_expit(double t) { return t < 0.0 ? t - log1p(exp(t)) : -log1p(exp(-t)); }

__device__ inline double geo_log_prob(double x, int pf, double scale, double x0) {
    if (pf == SBE_GEO_PROB_EXPONENTIAL) return -x / scale;
    return geo_log_expit(-(x - x0) / scale) - geo_log_expit(x0 / scale);
}

__device__ inline double geo_aggregate(int agg, int64_t n_edges, double sum, double mx) {
    if (agg == SBE_GEO_AGG_SUM) return sum;
    if (agg == SBE_GEO_AGG_MAX) return mx;
    return sum / (double)(n_edges > 0 ? n_edges : 1);
}

__global__ void k_geo_log_expit(const double* t, int64_t n, double* out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = geo_log_expit(t[i]);
}

// ---- the cost matrix: finite? symmetric? ----------------------------------------------------------------------------
__global__ void k_geo_check(const double* cost, int N, int* flags) {
    const int64_t total = (int64_t)N * N;
    int found = 0;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = e / N, j = e - i * N;
        const double c = cost[e];
        if (!isfinite(c)) found |= 1;
        else if (j > i && c != cost[j * N + i]) found |= 2;
    }
    if (found) atomicOr(flags, found);
}

// ---- the skeleton kernel ----------------------------------------------------------------------------------------------
struct SkeletonArgs {
    const double* cost;       // [N][N]
    int N;
    int symmetric;            // cost[a][b] == cost[b][a] everywhere: one read per edge
    const uint8_t* masks;     // [n][N] of this launch
    int32_t* idx;             // scratch [n][N]: the members of each mask, ascending
    double* keys;             // scratch [n][N]: Prim's keys of the masks above the LDS threshold
    int skeleton, agg, pf;
    double scale, x0;
    int lds_members;          // sub-matrices of up to this many members fit the launch's LDS
    int32_t* m_out;           // [n] outputs of this launch
    int64_t* ne_out;
    double* sum_out;
    double* max_out;
    double* logp_out;
};

// lexicographic minimum of (key, member) over the wave, a butterfly in which every lane ends with the result (the
// comparison is symmetric, so both lanes of an exchange keep the same pair).  Not unit_wave_reduce (sbe_unit_device.hip.h):
// that one exchanges a single value, this one a pair, and the waves meet through a double-buffered LDS exchange
__device__ inline void keep_smaller(double& k, int& v, double ok, int ov) {
    if (ok < k || (ok == k && ov < v)) { k = ok; v = ov; }
}

__device__ inline void wave_argmin(double& k, int& v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) keep_smaller(k, v, __shfl_xor(k, off), __shfl_xor(v, off));
}

// Prim's algorithm over m >= 2 members.  LDS: sub (m x m, edge weights) and key (m) in LDS; else the rows come from memory
// and the keys live in scratch.  A key of +inf marks a member of the tree (costs are finite).
template <bool LDS>
__device__ inline void prim(const SkeletonArgs& g, const int32_t* idx, int m, const double* sub, double* key, double (*red_k)[kWaves],
                            int (*red_v)[kWaves], int64_t& n_edges, double& sum, double& mx) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double inf = std::numeric_limits<double>::infinity();
    for (int v = tid; v < m; v += kBlock) key[v] = v == 0 ? inf : DBL_MAX;
    int u = 0;
    for (int step = 0; step + 1 < m; ++step) {
        const int64_t iu = LDS ? 0 : (int64_t)idx[u];
        const double* row = LDS ? sub + (size_t)u * m : g.cost + iu * g.N;
        double best = inf;
        int best_v = 0x7fffffff;
        for (int v = tid; v < m; v += kBlock) {
            double k = key[v];
            if (k == inf) continue;
            double c;
            if (LDS) {
                c = row[v];
            } else {
                const int64_t iv = idx[v];
                c = row[iv];
                if (!g.symmetric) c = fmin(c, g.cost[iv * g.N + iu]);
            }
            k = fmin(k, c);
            key[v] = k;
            if (k < best) { best = k; best_v = v; }
        }
        wave_argmin(best, best_v);
        const int p = step & 1;
        if (lane == 0) { red_k[p][wave] = best; red_v[p][wave] = best_v; }
        __syncthreads();
        best = red_k[p][0];
        best_v = red_v[p][0];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) {
            keep_smaller(best, best_v, red_k[p][w], red_v[p][w]);
        }
        if (best_v >= m) break;                               // (cannot happen with finite costs; uniform over the workgroup)
        u = best_v;
        if ((u & (kBlock - 1)) == tid) key[u] = inf;          // (its owner: nobody else reads or writes this key)
        if (best != 0.0) {
            ++n_edges;
            sum += best;
            mx = fmax(mx, best);
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_geo_skeleton(const SkeletonArgs g) {
    extern __shared__ double geo_lds[];              // LDS path: sub [lds_members^2], key [lds_members]
    __shared__ int s_wave_total[kWaves];
    __shared__ double red_k[2][kWaves];
    __shared__ int red_v[2][kWaves];
    __shared__ double s_sum[kBlock];
    __shared__ double s_max[kBlock];

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, N = g.N;
    const uint8_t* mask = g.masks + (size_t)b * N;
    int32_t* idx = g.idx + (size_t)b * N;

    // ---- 1. the members, ascending
    const int stretch = (N + kBlock - 1) / kBlock, n0 = min(N, tid * stretch), n1 = min(N, n0 + stretch);
    int mine = 0;
    for (int n = n0; n < n1; ++n) mine += mask[n] != 0;
    int incl = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(incl, off);
        if (lane >= off) incl += o;
    }
    if (lane == 63) s_wave_total[wave] = incl;
    __syncthreads();
    int pos = incl - mine, m = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        if (w < wave) pos += s_wave_total[w];
        m += s_wave_total[w];
    }
    for (int n = n0; n < n1; ++n)
        if (mask[n] != 0) idx[pos++] = n;
    __threadfence_block();
    __syncthreads();

    int64_t n_edges = 0;
    double sum = 0.0, mx = -std::numeric_limits<double>::infinity();
    if (g.skeleton == SBE_GEO_SKELETON_COMPLETE) {
        // ---- 2b. every entry of the sub-matrix: thread t takes entries t, t + 256, ... in order, then a fixed tree
        const int64_t total = (int64_t)m * m;
        for (int64_t e = tid; e < total; e += kBlock) {
            const int a = (int)(e / m), c = (int)(e - (int64_t)a * m);
            const double w = g.cost[(int64_t)idx[a] * N + idx[c]];
            sum += w;
            mx = fmax(mx, w);
        }
        s_sum[tid] = sum;
        s_max[tid] = mx;
        __syncthreads();
        for (int half = kBlock / 2; half > 0; half >>= 1) {
            if (tid < half) {
                s_sum[tid] += s_sum[tid + half];
                s_max[tid] = fmax(s_max[tid], s_max[tid + half]);
            }
            __syncthreads();
        }
        sum = s_sum[0];
        mx = s_max[0];
        n_edges = total;
    } else if (m >= 2) {
        // ---- 2a. the minimum spanning tree
        if (m <= g.lds_members) {
            double* sub = geo_lds;
            double* key = geo_lds + (size_t)g.lds_members * g.lds_members;
            for (int e = tid; e < m * m; e += kBlock) {
                const int a = e / m, c = e - a * m;
                const int64_t ia = idx[a], ic = idx[c];
                double w = g.cost[ia * N + ic];
                if (!g.symmetric) w = fmin(w, g.cost[ic * N + ia]);
                sub[e] = w;
            }
            __syncthreads();
            prim<true>(g, idx, m, sub, key, red_k, red_v, n_edges, sum, mx);
        } else {
            prim<false>(g, idx, m, nullptr, g.keys + (size_t)b * N, red_k, red_v, n_edges, sum, mx);
        }
    }
    // ---- 3. the outputs
    if (tid == 0) {
        if (n_edges == 0) mx = 0.0;                  // (no non-zero edge: the edge set is {0})
        g.m_out[b] = m;
        g.ne_out[b] = n_edges;
        g.sum_out[b] = sum;
        g.max_out[b] = mx;
        g.logp_out[b] = m > 0 ? geo_log_prob(geo_aggregate(g.agg, n_edges, sum, mx), g.pf, g.scale, g.x0)
                              : std::numeric_limits<double>::quiet_NaN();
    }
}

// ---- the per-object kernel (after k_geo_skeleton of the one mask, on the same stream) -----------------------------------
struct PerObjectArgs {
    const double* cost;
    int N;
    const int32_t* idx;       // the members (scratch of mask 0)
    const int32_t* m;         // the skeleton kernel's outputs of mask 0
    const int64_t* ne;
    const double* sum;
    const double* mx;
    int agg, pf;
    double scale, x0;
    double* ctc;              // [N] outputs
    double* out;
};

__global__ __launch_bounds__(kBlock) void k_geo_per_object(const PerObjectArgs g) {
    __shared__ double s_min[kWaves][kCols];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = g.m[0];
    const int col = blockIdx.x * kCols + lane;
    double best = std::numeric_limits<double>::infinity();
    if (col < g.N) {
#pragma unroll 4
        for (int a = wave; a < m; a += kWaves) best = fmin(best, g.cost[(int64_t)g.idx[a] * g.N + col]);
    }
    s_min[wave][lane] = best;
    __syncthreads();
    if (wave != 0 || col >= g.N) return;
#pragma unroll
    for (int w = 1; w < kWaves; ++w) best = fmin(best, s_min[w][lane]);
    const double before = geo_aggregate(g.agg, g.ne[0], g.sum[0], g.mx[0]);
    double after;
    if (g.agg == SBE_GEO_AGG_MEAN) after = (best + (double)m * before) / (double)(1 + m);
    else if (g.agg == SBE_GEO_AGG_SUM) after = best + before;
    else after = fmax(best, before);
    g.ctc[col] = best;
    g.out[col] = geo_log_prob(after, g.pf, g.scale, g.x0) - geo_log_prob(before, g.pf, g.scale, g.x0);
}

inline size_t skeleton_lds_bytes(int lds_members) { return ((size_t)lds_members * lds_members + lds_members) * sizeof(double); }

}  // namespace

struct sbe_geo : sbe_unit_handle {              // (sbe_unit.hip.h; ev: around the kernels of the last call)
    double* d_cost = nullptr;                   // [N][N]
    size_t cost_bytes = 0;
    int64_t N = 0;                              // 0: no cost matrix yet
    int symmetric = 1;
    int* d_flags = nullptr;
    uint8_t* d_masks = nullptr;                 // the masks of one launch
    size_t masks_bytes = 0;
    int32_t* d_idx = nullptr;                   // scratch: members
    size_t idx_bytes = 0;
    double* d_keys = nullptr;                   // scratch: keys of the memory path
    size_t keys_bytes = 0;
    void* d_out = nullptr;                      // the five outputs of one launch, then the two [N] outputs of the per-object kernel
    size_t out_bytes = 0;
    int64_t launch_masks = 0;                   // 0: the default
    int64_t launches = 0, lds_masks = 0;
    bool ran = false;
    size_t lds_allowed = 0;                     // dynamic LDS the skeleton kernel was last allowed
    std::vector<void*> buffers() const { return {d_cost, d_flags, d_masks, d_idx, d_keys, d_out}; }
};

namespace {

constexpr char kNullHandle[] = "null handle";

int check_function(sbe_geo* h, int aggregation, int probability_function, double scale, double x0) {
    if (aggregation < SBE_GEO_AGG_MEAN || aggregation > SBE_GEO_AGG_MAX)
        return fail(h, SBE_ERR_ARG, "aggregation=%d is none of mean (0), sum (1), max (2)", aggregation);
    if (probability_function != SBE_GEO_PROB_EXPONENTIAL && probability_function != SBE_GEO_PROB_SIGMOID)
        return fail(h, SBE_ERR_ARG, "probability_function=%d is neither exponential (0) nor sigmoid (1)", probability_function);
    if (!(std::isfinite(scale) && scale > 0.0)) return fail(h, SBE_ERR_ARG, "scale=%g must be positive and finite", scale);
    if (!std::isfinite(x0)) return fail(h, SBE_ERR_ARG, "inflection_point=%g must be finite", x0);
    return SBE_OK;
}

// The skeleton kernel over n_masks masks in launches of bounded size; every output pointer may be null.  The members and
// the outputs of the last launch stay on the device (the per-object kernel reads those of its one mask); with
// close_events false the caller goes on in the stream and closes the timing itself.
int run_skeleton(sbe_geo* h, const uint8_t* masks, int64_t n_masks, int skeleton, int agg, int pf, double scale, double x0,
                 int32_t* m_out, int64_t* ne_out, double* sum_out, double* max_out, double* logp_out, bool close_events) {
    const int64_t N = h->N;
    // members per mask, on the host: an empty mask is refused before any device call, and the LDS of a launch is sized
    // by the largest mask of it that takes the LDS path
    std::vector<int32_t> count((size_t)n_masks);
    for (int64_t b = 0; b < n_masks; ++b) {
        const uint8_t* row = masks + (size_t)(b * N);
        int32_t c = 0;
        for (int64_t n = 0; n < N; ++n) c += row[n] != 0;
        if (c == 0) return fail(h, SBE_ERR_DATA, "mask %lld has no member", (long long)b);
        count[(size_t)b] = c;
    }
    const int64_t per_launch = h->launch_masks > 0
        ? h->launch_masks
        : std::max<int64_t>(1, std::min<int64_t>(SBE_GEO_MAX_LAUNCH_MASKS, kScratchEntries / N));
    const int64_t cap = std::min(per_launch, n_masks);
    HIPCHK(h, hipSetDevice(h->device));
    int rc;
    if ((rc = unit_ensure(h, h->d_masks, h->masks_bytes, (size_t)(cap * N)))) return rc;
    if ((rc = unit_ensure(h, h->d_idx, h->idx_bytes, (size_t)(cap * N) * sizeof(int32_t)))) return rc;
    bool any_memory_path = false;
    if (skeleton == SBE_GEO_SKELETON_MST)
        for (int32_t c : count) any_memory_path |= c > SBE_GEO_LDS_MEMBERS;
    if (any_memory_path && (rc = unit_ensure(h, h->d_keys, h->keys_bytes, (size_t)(cap * N) * sizeof(double)))) return rc;
    if ((rc = unit_ensure(h, h->d_out, h->out_bytes, (size_t)cap * 40 + kPerObjectOffset + (size_t)N * 16))) return rc;
    double* d_sum = (double*)h->d_out;
    double* d_max = d_sum + cap;
    double* d_logp = d_max + cap;
    int64_t* d_ne = (int64_t*)(d_logp + cap);
    int32_t* d_m = (int32_t*)(d_ne + cap);

    HIPCHK(h, hipEventRecord(h->ev[0], h->stream));
    int64_t launches = 0, lds_masks = 0;
    for (int64_t b0 = 0; b0 < n_masks; b0 += per_launch, ++launches) {
        const int64_t n = std::min(per_launch, n_masks - b0);
        int lds_members = 0;
        if (skeleton == SBE_GEO_SKELETON_MST)
            for (int64_t b = b0; b < b0 + n; ++b) {
                const int32_t c = count[(size_t)b];
                if (c >= 2 && c <= SBE_GEO_LDS_MEMBERS) lds_members = std::max(lds_members, (int)c);
                lds_masks += c <= SBE_GEO_LDS_MEMBERS;
            }
        const size_t lds = skeleton_lds_bytes(lds_members);
        if (lds > h->lds_allowed) {
            HIPCHK(h, hipFuncSetAttribute((const void*)k_geo_skeleton, hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)skeleton_lds_bytes(SBE_GEO_LDS_MEMBERS)));
            h->lds_allowed = skeleton_lds_bytes(SBE_GEO_LDS_MEMBERS);
        }
        HIPCHK(h, hipMemcpyAsync(h->d_masks, masks + (size_t)(b0 * N), (size_t)(n * N), hipMemcpyHostToDevice, h->stream));
        const SkeletonArgs args{h->d_cost, (int)N, h->symmetric, h->d_masks, h->d_idx, h->d_keys, skeleton, agg, pf, scale, x0,
                                lds_members, d_m, d_ne, d_sum, d_max, d_logp};
        k_geo_skeleton<<<(unsigned)n, kBlock, lds, h->stream>>>(args);
        HIPCHK(h, hipGetLastError());
        if (m_out) HIPCHK(h, hipMemcpyAsync(m_out + b0, d_m, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        if (ne_out) HIPCHK(h, hipMemcpyAsync(ne_out + b0, d_ne, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
        if (sum_out) HIPCHK(h, hipMemcpyAsync(sum_out + b0, d_sum, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        if (max_out) HIPCHK(h, hipMemcpyAsync(max_out + b0, d_max, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        if (logp_out) HIPCHK(h, hipMemcpyAsync(logp_out + b0, d_logp, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    }
    h->launches = launches;
    h->lds_masks = lds_masks;
    if (close_events) {
        HIPCHK(h, hipEventRecord(h->ev[1], h->stream));
        if ((rc = unit_sync_timed(h))) return rc;
        h->ran = true;
    }
    return SBE_OK;
}

int check_masks(sbe_geo* h, const uint8_t* masks, int64_t n_masks, const char* who) {
    if (h->N == 0) return fail(h, SBE_ERR_STATE, "%s needs the cost matrix of a successful sbe_geo_set_cost", who);
    if (n_masks < 0 || n_masks > SBE_GEO_MAX_MASKS)
        return fail(h, SBE_ERR_ARG, "n_masks=%lld out of range [0, %d] (2^20 masks per call)", (long long)n_masks, SBE_GEO_MAX_MASKS);
    if (n_masks > 0 && !masks) return fail(h, SBE_ERR_ARG, "null pointer argument: masks");
    return SBE_OK;
}

}  // namespace

extern "C" {

int sbe_geo_abi_version(void) { return SBE_GEO_ABI_VERSION; }

const char* sbe_geo_last_error(const sbe_geo* h) { return unit_last_error(h); }

int sbe_geo_create(sbe_geo** out, int device) { return unit_create_on_device(out, device, "sbe_geo_create"); }

int sbe_geo_destroy(sbe_geo* h) { return unit_destroy(h, kNullHandle); }

int sbe_geo_set_launch_masks(sbe_geo* h, int64_t masks) {
    CHECK_HANDLE(h, kNullHandle);
    if (masks < 0 || masks > SBE_GEO_MAX_LAUNCH_MASKS)
        return fail(h, SBE_ERR_ARG, "masks=%lld out of range [0, %d]", (long long)masks, SBE_GEO_MAX_LAUNCH_MASKS);
    h->launch_masks = masks;
    return SBE_OK;
}

int sbe_geo_set_cost(sbe_geo* h, const double* cost, int64_t n_objects) {
    CHECK_HANDLE(h, kNullHandle);
    if (!cost) return fail(h, SBE_ERR_ARG, "null pointer argument: cost");
    const int64_t N = n_objects;
    if (N < 1 || N > SBE_GEO_MAX_OBJECTS)
        return fail(h, SBE_ERR_ARG, "n_objects=%lld out of range [1, %d] (the cost matrix takes N * N * 8 bytes, 8 GiB at the limit)",
                     (long long)N, SBE_GEO_MAX_OBJECTS);
    HIPCHK(h, hipSetDevice(h->device));
    h->N = 0;                                       // (until the new matrix is in place and checked)
    h->ran = false;
    const size_t bytes = (size_t)N * N * sizeof(double);
    int rc = unit_ensure(h, h->d_cost, h->cost_bytes, bytes);
    if (rc) return rc;
    if ((rc = unit_ensure(h, h->d_flags, sizeof(int)))) return rc;
    HIPCHK(h, hipMemcpyAsync(h->d_cost, cost, bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(h->d_flags, 0, sizeof(int), h->stream));
    const int blocks = (int)std::min<int64_t>(4096, div_up(N * N, kBlock));
    k_geo_check<<<blocks, kBlock, 0, h->stream>>>(h->d_cost, (int)N, h->d_flags);
    HIPCHK(h, hipGetLastError());
    int flags = 0;
    HIPCHK(h, hipMemcpyAsync(&flags, h->d_flags, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (flags & 1) {
        for (int64_t e = 0; e < N * N; ++e)
            if (!std::isfinite(cost[e]))
                return fail(h, SBE_ERR_DATA, "cost[%lld][%lld]=%g is not finite", (long long)(e / N), (long long)(e % N), cost[e]);
        return fail(h, SBE_ERR_DATA, "the cost matrix holds a value that is not finite");
    }
    h->symmetric = (flags & 2) ? 0 : 1;
    h->N = N;
    return SBE_OK;
}

int sbe_geo_skeleton(sbe_geo* h, const uint8_t* masks, int64_t n_masks, int skeleton, int32_t* m_out, int64_t* n_edges_out,
                     double* sum_out, double* max_out) {
    CHECK_HANDLE(h, kNullHandle);
    int rc = check_masks(h, masks, n_masks, "sbe_geo_skeleton");
    if (rc) return rc;
    if (skeleton != SBE_GEO_SKELETON_MST && skeleton != SBE_GEO_SKELETON_COMPLETE)
        return fail(h, SBE_ERR_ARG, "skeleton=%d is neither mst (0) nor complete_graph (1)", skeleton);
    if (n_masks > 0 && (!m_out || !n_edges_out || !sum_out || !max_out)) return fail(h, SBE_ERR_ARG, "null pointer argument: output");
    if (n_masks == 0) return SBE_OK;
    return run_skeleton(h, masks, n_masks, skeleton, SBE_GEO_AGG_SUM, SBE_GEO_PROB_EXPONENTIAL, 1.0, 0.0, m_out, n_edges_out, sum_out,
                        max_out, nullptr, true);
}

int sbe_geo_prior(sbe_geo* h, const uint8_t* masks, int64_t n_masks, int skeleton, int aggregation, int probability_function,
                  double scale, double inflection_point, double* out) {
    CHECK_HANDLE(h, kNullHandle);
    int rc = check_masks(h, masks, n_masks, "sbe_geo_prior");
    if (rc) return rc;
    if (skeleton != SBE_GEO_SKELETON_MST && skeleton != SBE_GEO_SKELETON_COMPLETE)
        return fail(h, SBE_ERR_ARG, "skeleton=%d is neither mst (0) nor complete_graph (1)", skeleton);
    if ((rc = check_function(h, aggregation, probability_function, scale, inflection_point))) return rc;
    if (n_masks > 0 && !out) return fail(h, SBE_ERR_ARG, "null pointer argument: out");
    if (n_masks == 0) return SBE_OK;
    return run_skeleton(h, masks, n_masks, skeleton, aggregation, probability_function, scale, inflection_point, nullptr, nullptr,
                        nullptr, nullptr, out, true);
}

int sbe_geo_costs_per_object(sbe_geo* h, const uint8_t* mask, int aggregation, int probability_function, double scale,
                             double inflection_point, double* ctc_out, double* out) {
    CHECK_HANDLE(h, kNullHandle);
    int rc = check_masks(h, mask, 1, "sbe_geo_costs_per_object");
    if (rc) return rc;
    if ((rc = check_function(h, aggregation, probability_function, scale, inflection_point))) return rc;
    if (!out) return fail(h, SBE_ERR_ARG, "null pointer argument: out");
    const int64_t N = h->N;
    // the skeleton of the one mask (always the MST, as in the reference); its members and outputs stay on the device
    if ((rc = run_skeleton(h, mask, 1, SBE_GEO_SKELETON_MST, aggregation, probability_function, scale, inflection_point, nullptr,
                           nullptr, nullptr, nullptr, nullptr, false)))
        return rc;
    double* d_sum = (double*)h->d_out;              // (the layout of run_skeleton with one mask per launch)
    double* d_max = d_sum + 1;
    double* d_logp = d_max + 1;
    int64_t* d_ne = (int64_t*)(d_logp + 1);
    int32_t* d_m = (int32_t*)(d_ne + 1);
    double* d_ctc = (double*)((char*)h->d_out + 40 + kPerObjectOffset);
    double* d_res = d_ctc + N;
    const PerObjectArgs args{h->d_cost, (int)N, h->d_idx, d_m, d_ne, d_sum, d_max, aggregation, probability_function, scale,
                             inflection_point, d_ctc, d_res};
    k_geo_per_object<<<div_up(N, kCols), kBlock, 0, h->stream>>>(args);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipEventRecord(h->ev[1], h->stream));
    if (ctc_out) HIPCHK(h, hipMemcpyAsync(ctc_out, d_ctc, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(out, d_res, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if ((rc = unit_sync_timed(h))) return rc;
    h->ran = true;
    return SBE_OK;
}

int sbe_geo_log_expit(sbe_geo* h, const double* t, int64_t n, double* out) {
    CHECK_HANDLE(h, kNullHandle);
    if (n < 0 || n > SBE_GEO_MAX_MASKS) return fail(h, SBE_ERR_ARG, "n=%lld out of range [0, %d]", (long long)n, SBE_GEO_MAX_MASKS);
    if (n > 0 && (!t || !out)) return fail(h, SBE_ERR_ARG, "null pointer argument: %s", !t ? "t" : "out");
    if (n == 0) return SBE_OK;
    HIPCHK(h, hipSetDevice(h->device));
    int rc = unit_ensure(h, h->d_keys, h->keys_bytes, (size_t)n * 2 * sizeof(double));
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(h->d_keys, t, (size_t)n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    k_geo_log_expit<<<div_up(n, kBlock), kBlock, 0, h->stream>>>(h->d_keys, n, h->d_keys + n);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(out, h->d_keys + n, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return SBE_OK;
}

int sbe_geo_last_shape(const sbe_geo* h, int64_t* launches_out, int64_t* lds_masks_out) {
    CHECK_HANDLE(h, kNullHandle);
    if (!launches_out || !lds_masks_out) return fail(h, SBE_ERR_ARG, "null pointer argument: output");
    if (!h->ran) return fail(h, SBE_ERR_STATE, "no successful call on the current cost matrix yet");
    *launches_out = h->launches;
    *lds_masks_out = h->lds_masks;
    return SBE_OK;
}

int sbe_geo_last_kernel_ms(const sbe_geo* h, float* ms_out) { return unit_last_kernel_ms(h, ms_out, kNullHandle); }

}  // extern "C"
