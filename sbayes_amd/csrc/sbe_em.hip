// sbe_em.hip -- the on-device EM cluster initializer (include/sbe_em.h): the data of one initializer resident on the
// device and the kernels of one EM step, enqueued back to back on the handle's stream for every step of a call.  The
// numerical contract is tests/_em_oracle.py; DESIGN.md section 12 has the layout, the kernels and the limits.
//
// Per step (everything fp64; every sum in a fixed order, no float atomics):
//   k_em_table  one wave per (f, g): counts[g,f,s] by a sequential sum over the objects of state s of feature f in
//               ascending n (a per-feature bucket list built at create), then p, logp and the NA column log sum_s p;
//   k_em_ll     one thread per (g, n) with g available at n: ll[g,n] = sum_f logp[g,f,x_nf] in ascending f;
//   k_em_peaky, k_em_geo, k_em_fill   (cost-based geo prior only) softmax(N z[k]) over n, its product with the cost
//               matrix (ascending m per (k, n)), and the scalar that replaces the rows g >= K;
//   k_em_update one thread per object: softmax over the available groups of geo + ll / T_i.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "sbe_unit.hip.h"
#include "../../include/sbe_em.h"

namespace {

constexpr int kEmBlock = 256;
constexpr int kEmWaves = kEmBlock / 64;                // (the block reductions: every kernel that reduces is launched with kEmBlock)
constexpr int kEmTableThreads = 64;                  // one wave per (feature, group): thread s sums the objects of state s
constexpr int kEmGeoRows = 8;                        // cluster rows per thread of k_em_geo (one read of a cost column each)

// counts, p and logp of one (feature f = blockIdx.x, group g = blockIdx.y); logp: [G][F][S+1]
__global__ __launch_bounds__(kEmTableThreads) void k_em_table(const double* __restrict__ z, const int32_t* __restrict__ perm,
                                                              const int32_t* __restrict__ off, const uint8_t* __restrict__ app,
                                                              int64_t n, int f_total, int s_total, double* __restrict__ logp) {
    __shared__ double c[SBE_EM_MAX_STATES];
    const int f = blockIdx.x, g = blockIdx.y, tid = threadIdx.x;
    const double* zg = z + (int64_t)g * n;
    const int32_t* pf = perm + (int64_t)f * n;
    const int32_t* of = off + (int64_t)f * (s_total + 1);
    for (int s = tid; s < s_total; s += kEmTableThreads) {
        double acc = 0.0;
        for (int32_t i = of[s]; i < of[s + 1]; ++i) acc += zg[pf[i]];
        c[s] = acc + (app[(int64_t)f * s_total + s] ? 0.5 : 0.0);
    }
    __syncthreads();
    double tot = 0.0;
    for (int s = 0; s < s_total; ++s) tot += c[s];
    double* lp = logp + ((int64_t)g * f_total + f) * (s_total + 1);
    for (int s = tid; s < s_total; s += kEmTableThreads) lp[s] = log(c[s] / tot);
    if (tid == 0) {
        double sp = 0.0;
        for (int s = 0; s < s_total; ++s) sp += c[s] / tot;
        lp[s_total] = log(sp);
    }
}

// ll[g,n] = sum_f logp[g,f,x_nf] over the (g, n) with g available at n; x: [F][N] (NA = S)
__global__ __launch_bounds__(kEmBlock) void k_em_ll(const double* __restrict__ logp, const uint8_t* __restrict__ xt,
                                                    const uint8_t* __restrict__ avail, int64_t n, int f_total, int s_total,
                                                    double* __restrict__ ll) {
    const int64_t i = (int64_t)blockIdx.x * kEmBlock + threadIdx.x;
    const int g = blockIdx.y;
    if (i >= n || !avail[(int64_t)g * n + i]) return;
    const double* lp = logp + (int64_t)g * f_total * (s_total + 1);
    double acc = 0.0;
    for (int f = 0; f < f_total; ++f) acc += lp[(int64_t)f * (s_total + 1) + xt[(int64_t)f * n + i]];
    ll[(int64_t)g * n + i] = acc;
}

// zp[k] = softmax(N z[k]) over the objects, one block per cluster row k
__global__ __launch_bounds__(kEmBlock) void k_em_peaky(const double* __restrict__ z, int64_t n, double* __restrict__ zp) {
    __shared__ double red[kEmWaves];
    const double* zk = z + (int64_t)blockIdx.x * n;
    const double dn = (double)n;
    double m = -INFINITY;
    for (int64_t i = threadIdx.x; i < n; i += kEmBlock) m = fmax(m, dn * zk[i]);
    m = unit_block_reduce<kEmWaves>(m, red, unit_max{});
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += kEmBlock) s += exp(dn * zk[i] - m);
    s = unit_block_reduce<kEmWaves>(s, red, unit_sum{});
    double* out = zp + (int64_t)blockIdx.x * n;
    for (int64_t i = threadIdx.x; i < n; i += kEmBlock) out[i] = exp(dn * zk[i] - m) / s;
}

// geo[k,i] = -(sum_m zp[k,m] cost[m,i]) / scale / 2 for kEmGeoRows cluster rows per thread (ascending m)
__global__ __launch_bounds__(kEmBlock) void k_em_geo(const double* __restrict__ zp, const double* __restrict__ cost, int64_t n,
                                                     int k_total, double scale, double* __restrict__ geo) {
    const int64_t i = (int64_t)blockIdx.x * kEmBlock + threadIdx.x;
    const int k0 = blockIdx.y * kEmGeoRows;
    if (i >= n) return;
    const int rows = min(kEmGeoRows, k_total - k0);
    double acc[kEmGeoRows];
#pragma unroll
    for (int r = 0; r < kEmGeoRows; ++r) acc[r] = 0.0;
    for (int64_t m = 0; m < n; ++m) {
        const double c = cost[m * n + i];
#pragma unroll
        for (int r = 0; r < kEmGeoRows; ++r)
            if (r < rows) acc[r] += zp[(int64_t)(k0 + r) * n + m] * c;
    }
#pragma unroll
    for (int r = 0; r < kEmGeoRows; ++r)
        if (r < rows) geo[(int64_t)(k0 + r) * n + i] = -acc[r] / scale / 2.0;
}

// fill = logsumexp(geo[:K]) - log(K N): the value of every row g >= K (one block)
__global__ __launch_bounds__(kEmBlock) void k_em_fill(const double* __restrict__ geo, int64_t kn, double* __restrict__ fill) {
    __shared__ double red[kEmWaves];
    double m = -INFINITY;
    for (int64_t i = threadIdx.x; i < kn; i += kEmBlock) m = fmax(m, geo[i]);
    m = unit_block_reduce<kEmWaves>(m, red, unit_max{});
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < kn; i += kEmBlock) s += exp(geo[i] - m);
    s = unit_block_reduce<kEmWaves>(s, red, unit_sum{});
    if (threadIdx.x == 0) fill[0] = (log(s) + m) - log((double)kn);
}

// z[:,i] = softmax over the available g of geo[g,i] + ll[g,i] / t; geo == nullptr: no geo prior
__global__ __launch_bounds__(kEmBlock) void k_em_update(const double* __restrict__ ll, const uint8_t* __restrict__ avail,
                                                        const double* __restrict__ geo, const double* __restrict__ fill,
                                                        int64_t n, int g_total, int k_total, double t, double* __restrict__ z,
                                                        int* __restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * kEmBlock + threadIdx.x;
    if (i >= n) return;
    const double fv = geo ? fill[0] : 0.0;
    auto value = [&](int g) {
        const double lg = geo ? (g < k_total ? geo[(int64_t)g * n + i] : fv) : 0.0;
        return lg + ll[(int64_t)g * n + i] / t;
    };
    double m = -INFINITY;
    for (int g = 0; g < g_total; ++g)
        if (avail[(int64_t)g * n + i]) m = fmax(m, value(g));
    double s = 0.0;
    for (int g = 0; g < g_total; ++g)
        if (avail[(int64_t)g * n + i]) s += exp(value(g) - m);
    for (int g = 0; g < g_total; ++g) z[(int64_t)g * n + i] = avail[(int64_t)g * n + i] ? exp(value(g) - m) / s : 0.0;
    if (!(s > 0.0) || !isfinite(s) || !isfinite(m)) atomicOr(status, 1);
}

}  // namespace

struct sbe_em : sbe_unit_handle {       // (sbe_unit.hip.h; ev: around the steps of the last run)
    int64_t N = 0, F = 0, S = 0, G = 0, K = 0;
    uint8_t* d_xt = nullptr;            // [F][N] state index, NA = S
    int32_t* d_perm = nullptr;          // [F][N] objects ordered by state, ascending n within a state
    int32_t* d_off = nullptr;           // [F][S+1] start of each state's objects in d_perm (bucket S = NA is not summed)
    uint8_t* d_app = nullptr;           // [F][S]
    uint8_t* d_avail = nullptr;         // [G][N]
    double* d_z = nullptr;              // [G][N]
    double* d_logp = nullptr;           // [G][F][S+1]
    double* d_ll = nullptr;             // [G][N]
    int* d_status = nullptr;
    double* d_cost = nullptr;           // [N][N] (geo prior on)
    double* d_zp = nullptr;             // [K][N]
    double* d_geo = nullptr;            // [K][N]
    double* d_fill = nullptr;
    bool geo = false;
    double scale = 0.0;
    std::vector<void*> buffers() const {
        return {d_xt, d_perm, d_off, d_app, d_avail, d_z, d_logp, d_ll, d_status, d_cost, d_zp, d_geo, d_fill};
    }
};

namespace {

constexpr sbe_em* kNone = nullptr;                   // (fail without a handle: the type names the unit)
constexpr char kNullHandle[] = "null EM handle";

int enqueue_step(sbe_em* h, double t) {
    const unsigned n_tiles = (unsigned)div_up(h->N, kEmBlock);
    k_em_table<<<dim3((unsigned)h->F, (unsigned)h->G), kEmTableThreads, 0, h->stream>>>(h->d_z, h->d_perm, h->d_off, h->d_app, h->N,
                                                                                        (int)h->F, (int)h->S, h->d_logp);
    HIPCHK(h, hipGetLastError());
    k_em_ll<<<dim3(n_tiles, (unsigned)h->G), kEmBlock, 0, h->stream>>>(h->d_logp, h->d_xt, h->d_avail, h->N, (int)h->F, (int)h->S,
                                                                       h->d_ll);
    HIPCHK(h, hipGetLastError());
    if (h->geo) {
        k_em_peaky<<<(unsigned)h->K, kEmBlock, 0, h->stream>>>(h->d_z, h->N, h->d_zp);
        HIPCHK(h, hipGetLastError());
        k_em_geo<<<dim3(n_tiles, (unsigned)div_up(h->K, kEmGeoRows)), kEmBlock, 0, h->stream>>>(h->d_zp, h->d_cost, h->N, (int)h->K,
                                                                                                 h->scale, h->d_geo);
        HIPCHK(h, hipGetLastError());
        k_em_fill<<<1, kEmBlock, 0, h->stream>>>(h->d_geo, h->K * h->N, h->d_fill);
        HIPCHK(h, hipGetLastError());
    }
    k_em_update<<<n_tiles, kEmBlock, 0, h->stream>>>(h->d_ll, h->d_avail, h->geo ? h->d_geo : nullptr, h->d_fill, h->N, (int)h->G,
                                                      (int)h->K, t, h->d_z, h->d_status);
    HIPCHK(h, hipGetLastError());
    return SBE_OK;
}

}  // namespace

extern "C" {

int sbe_em_abi_version(void) { return SBE_EM_ABI_VERSION; }

const char* sbe_em_last_error(const sbe_em* h) { return unit_last_error(h); }

int sbe_em_create(sbe_em** out, int device, int64_t n_objects, int64_t n_features, int64_t n_states, const uint8_t* state_idx,
                  const uint8_t* applicable, int64_t n_groups, int64_t n_clusters, const uint8_t* groups_available) {
    if (!out) return fail(kNone, SBE_ERR_ARG, "null pointer argument: out");
    *out = nullptr;
    const int64_t N = n_objects, F = n_features, S = n_states, G = n_groups, K = n_clusters;
    if (N < 1 || N > SBE_EM_MAX_OBJECTS)
        return fail(kNone, SBE_ERR_ARG, "n_objects=%lld out of range [1, %d]", (long long)N, SBE_EM_MAX_OBJECTS);
    if (F < 1 || F > SBE_EM_MAX_FEATURES)
        return fail(kNone, SBE_ERR_ARG, "n_features=%lld out of range [1, %d]", (long long)F, SBE_EM_MAX_FEATURES);
    if (S < 1 || S > SBE_EM_MAX_STATES)
        return fail(kNone, SBE_ERR_ARG, "n_states=%lld out of range [1, %d]", (long long)S, SBE_EM_MAX_STATES);
    if (G < 1 || G > SBE_EM_MAX_GROUPS)
        return fail(kNone, SBE_ERR_ARG, "n_groups=%lld out of range [1, %d]", (long long)G, SBE_EM_MAX_GROUPS);
    if (K < 1 || K > G) return fail(kNone, SBE_ERR_ARG, "n_clusters=%lld out of range [1, n_groups=%lld]", (long long)K, (long long)G);
    if (!state_idx || !applicable || !groups_available) return fail(kNone, SBE_ERR_ARG, "null pointer argument: data");
    if (device < 0) return fail(kNone, SBE_ERR_ARG, "device %d out of range", device);
    // data checks and the per-feature object lists (host, before any device call)
    std::vector<uint8_t> xt((size_t)(F * N));
    std::vector<int32_t> off((size_t)(F * (S + 1))), perm((size_t)(F * N));
    std::vector<int32_t> cnt((size_t)S + 1);
    for (int64_t f = 0; f < F; ++f) {
        bool any = false;
        for (int64_t s = 0; s < S; ++s) any |= applicable[f * S + s] != 0;
        if (!any) return fail(kNone, SBE_ERR_DATA, "feature %lld has no applicable state", (long long)f);
        std::fill(cnt.begin(), cnt.end(), 0);
        for (int64_t i = 0; i < N; ++i) {
            const uint8_t x = state_idx[i * F + f];
            if (x > S)
                return fail(kNone, SBE_ERR_DATA, "state_idx[%lld][%lld] = %d exceeds n_states=%lld (NA is n_states)", (long long)i,
                             (long long)f, (int)x, (long long)S);
            xt[(size_t)(f * N + i)] = x;
            ++cnt[x];
        }
        int32_t at = 0;
        for (int64_t s = 0; s <= S; ++s) {
            off[(size_t)(f * (S + 1) + s)] = at;         // (entry S = start of the NA bucket = end of state S-1)
            at += cnt[(size_t)s];
            cnt[(size_t)s] = off[(size_t)(f * (S + 1) + s)];
        }
        for (int64_t i = 0; i < N; ++i) {
            const uint8_t x = state_idx[i * F + f];
            perm[(size_t)(f * N + cnt[x]++)] = (int32_t)i;
        }
    }
    for (int64_t i = 0; i < N; ++i) {
        bool any = false;
        for (int64_t g = 0; g < G && !any; ++g) any = groups_available[g * N + i] != 0;
        if (!any) return fail(kNone, SBE_ERR_DATA, "object %lld has no available group", (long long)i);
    }
    char shape[96];
    snprintf(shape, sizeof shape, " (N=%lld F=%lld S=%lld G=%lld)", (long long)N, (long long)F, (long long)S, (long long)G);
    sbe_em* h = nullptr;
    const int rc = unit_open(h, device, "sbe_em_create", shape);
    if (rc) return rc;
    h->N = N, h->F = F, h->S = S, h->G = G, h->K = K;
    auto bail = [&](hipError_t err, const char* what) { return unit_create_failed(h, "sbe_em_create", what, err, shape); };
    std::vector<uint8_t> app((size_t)(F * S)), avail((size_t)(G * N));
    for (int64_t q = 0; q < F * S; ++q) app[(size_t)q] = applicable[q] != 0;
    for (int64_t q = 0; q < G * N; ++q) avail[(size_t)q] = groups_available[q] != 0;
    hipError_t err;
    struct { void** p; size_t bytes; const void* src; } bufs[] = {
        {(void**)&h->d_xt, (size_t)(F * N), xt.data()},
        {(void**)&h->d_perm, (size_t)(F * N) * sizeof(int32_t), perm.data()},
        {(void**)&h->d_off, (size_t)(F * (S + 1)) * sizeof(int32_t), off.data()},
        {(void**)&h->d_app, (size_t)(F * S), app.data()},
        {(void**)&h->d_avail, (size_t)(G * N), avail.data()},
        {(void**)&h->d_z, (size_t)(G * N) * sizeof(double), nullptr},
        {(void**)&h->d_logp, (size_t)(G * F * (S + 1)) * sizeof(double), nullptr},
        {(void**)&h->d_ll, (size_t)(G * N) * sizeof(double), nullptr},
        {(void**)&h->d_status, sizeof(int), nullptr},
    };
    for (auto& b : bufs) {
        if ((err = hipMalloc(b.p, b.bytes)) != hipSuccess) return bail(err, "hipMalloc");
        if (b.src && (err = hipMemcpy(*b.p, b.src, b.bytes, hipMemcpyHostToDevice)) != hipSuccess) return bail(err, "hipMemcpy");
    }
    // (ll of an unavailable (g, n) is never written nor read; zero it once all the same)
    if ((err = hipMemset(h->d_ll, 0, (size_t)(G * N) * sizeof(double))) != hipSuccess) return bail(err, "hipMemset");
    *out = h;
    return SBE_OK;
}

int sbe_em_destroy(sbe_em* h) { return unit_destroy(h, kNullHandle); }

int sbe_em_set_geo_cost(sbe_em* h, const double* cost, double scale) {
    CHECK_HANDLE(h, kNullHandle);
    if (!cost) {
        h->geo = false;
        return SBE_OK;
    }
    if (!(scale > 0.0) || !std::isfinite(scale)) return fail(h, SBE_ERR_ARG, "scale=%g must be positive and finite", scale);
    const int64_t bytes = h->N * h->N * (int64_t)sizeof(double);
    if (bytes > SBE_EM_MAX_COST_BYTES)
        return fail(h, SBE_ERR_ARG, "the cost matrix of N=%lld objects needs %lld bytes; the limit is %lld (N <= 32768)",
                     (long long)h->N, (long long)bytes, (long long)SBE_EM_MAX_COST_BYTES);
    for (int64_t q = 0; q < h->N * h->N; ++q)
        if (!std::isfinite(cost[q]))
            return fail(h, SBE_ERR_DATA, "cost[%lld][%lld] = %g is not finite", (long long)(q / h->N), (long long)(q % h->N), cost[q]);
    HIPCHK(h, hipSetDevice(h->device));
    const size_t kn_bytes = (size_t)(h->K * h->N) * sizeof(double);
    int rc;                                           // (each buffer on its own: one that failed is tried again by the next call)
    if ((rc = unit_ensure(h, h->d_cost, (size_t)bytes)) || (rc = unit_ensure(h, h->d_zp, kn_bytes)) ||
        (rc = unit_ensure(h, h->d_geo, kn_bytes)) || (rc = unit_ensure(h, h->d_fill, sizeof(double))))
        return rc;
    HIPCHK(h, hipMemcpyAsync(h->d_cost, cost, (size_t)bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->geo = true;
    h->scale = scale;
    return SBE_OK;
}

int sbe_em_run(sbe_em* h, const double* z_in, int64_t n_steps, const double* temperatures, double* z_out) {
    CHECK_HANDLE(h, kNullHandle);
    if (!z_in || !z_out) return fail(h, SBE_ERR_ARG, "null pointer argument: z_in / z_out");
    if (n_steps < 0 || n_steps > SBE_EM_MAX_STEPS)
        return fail(h, SBE_ERR_ARG, "n_steps=%lld out of range [0, %d]", (long long)n_steps, SBE_EM_MAX_STEPS);
    if (n_steps > 0 && !temperatures) return fail(h, SBE_ERR_ARG, "null pointer argument: temperatures");
    for (int64_t i = 0; i < n_steps; ++i)
        if (!(temperatures[i] > 0.0) || !std::isfinite(temperatures[i]))
            return fail(h, SBE_ERR_ARG, "temperatures[%lld] = %g must be positive and finite", (long long)i, temperatures[i]);
    const int64_t N = h->N, G = h->G;
    for (int64_t i = 0; i < N; ++i) {
        double s = 0.0;
        for (int64_t g = 0; g < G; ++g) {
            const double v = z_in[g * N + i];
            if (!std::isfinite(v))
                return fail(h, SBE_ERR_DATA, "z_in[%lld][%lld] = %g is not finite", (long long)g, (long long)i, v);
            s += v;
        }
        if (s == 0.0) return fail(h, SBE_ERR_DATA, "column %lld of z_in sums to 0", (long long)i);
    }
    if (n_steps == 0) {
        if (z_out != z_in) std::memmove(z_out, z_in, (size_t)(G * N) * sizeof(double));
        h->last_kernel_ms = 0.0f;
        return SBE_OK;
    }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpyAsync(h->d_z, z_in, (size_t)(G * N) * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(h->d_status, 0, sizeof(int), h->stream));
    int rc = unit_timed(h, [&] {
        for (int64_t i = 0; i < n_steps; ++i)
            if (const int step_rc = enqueue_step(h, temperatures[i])) {
                (void)hipStreamSynchronize(h->stream);
                return step_rc;
            }
        return SBE_OK;
    });
    int status = 0;
    if (!rc) rc = unit_copy_back(h, (const int*)h->d_status, 1, {&status});
    if (!rc) rc = unit_copy_back(h, (const double*)h->d_z, (size_t)(G * N), {z_out});
    if (!rc) rc = unit_sync_timed(h);
    if (rc) return rc;
    if (status) return fail(h, SBE_ERR_DATA, "an EM step produced a non-finite z (an object whose available groups all have "
                             "likelihood 0, or a non-finite geo prior)");
    return SBE_OK;
}

int sbe_em_last_kernel_ms(const sbe_em* h, float* ms_out) { return unit_last_kernel_ms(h, ms_out, kNullHandle); }

}  // extern "C"
