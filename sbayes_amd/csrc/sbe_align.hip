// sbe_align.hip -- alignment of cluster labels within a run and across runs on the device (include/sbe_align.h): the bit
// store of R runs of cluster samples (sbe_unit.hip.h has it), the within-run kernel (one permutation per sample against the
// running sum of the aligned samples so far), the counts kernel and the across-run kernel.  The contract is
// tests/_align_oracle.py; DESIGN.md section 17 has the layout, the structure of the kernels and the limits.
//
// The within-run kernel is one dependency chain per run: each step needs the sums the step before wrote.  One workgroup
// of 256 threads takes a run and keeps the int32 sums [K][N] in LDS for the whole run.  Per step:
//   A. a lane owns a slice of an object word (W words of 32 objects, each cut into G slices so that W * G fills the
//      block), reads the sample's K bit words (the next sample's are already on their way) and walks the set bits only:
//      d[i][j] += sum[i][n] for every object n of cluster j, in K * K int64 registers;
//   B. the wave reduces the K * K partial sums with a transposing exchange tree (lane l ends with entry l), the four
//      waves meet in LDS;                                                                                 -- barrier 1
//   C. wave 0 solves the assignment by a DP over the 2^K subsets of columns (a lane owns 1 .. 4 subsets, supersets are
//      one lane exchange away), keeping the smallest column that attains each subset's maximum: following those from
//      the empty set gives the lexicographically smallest maximiser.  It stores P_s and publishes its inverse;
//                                                                                                          -- barrier 2
//   D. every lane adds w to sum[i][n] for the objects n of its slice of cluster P_s[i].
// A lane reads and writes the sums of its own objects only, so the sums need no barrier of their own; no workgroup waits
// for another.  The sums are laid out [K][32][W] (object n at (n & 31) * W + (n >> 5)): lanes that are at the same bit
// of neighbouring words touch neighbouring banks.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <vector>

#include "sbe_unit.hip.h"
#include "../../include/sbe_align.h"

namespace {

constexpr int kAlignBlock = 256;
constexpr int kAlignWaves = kAlignBlock / 64;
constexpr int kMaxK = SBE_ALIGN_MAX_CLUSTERS;
constexpr uint64_t kIdentityPack = 0x0706050403020100ull;   // byte i holds i

// ---- the K * K partial sums of a wave: lane l ends with the wave's total of entry l & (L - 1) -----------------------
template <int L>
__device__ inline long long wave_reduce_entries(long long (&v)[L], int lane) {
#pragma unroll
    for (int o = 1, len = L; len > 1; o <<= 1, len >>= 1) {
        const bool up = (lane & o) != 0;
#pragma unroll
        for (int t = 0; t < len / 2; ++t) {
            const long long keep = up ? v[2 * t + 1] : v[2 * t];
            const long long send = up ? v[2 * t] : v[2 * t + 1];
            v[t] = keep + __shfl_xor(send, o, 64);
        }
    }
    long long r = v[0];
#pragma unroll
    for (int o = L; o < 64; o <<= 1) r += __shfl_xor(r, o, 64);
    return r;
}

// the four waves' totals, through LDS: afterwards every lane of every wave holds entry lane & (L - 1).  One barrier; the
// caller keeps `red` from being written again before every wave has read it.
template <int L>
__device__ inline long long block_reduce_entries(long long (&v)[L], long long (*red)[64], int lane, int wave) {
    const long long r = wave_reduce_entries<L>(v, lane);
    if (lane < L) red[wave][lane] = r;
    __syncthreads();
    long long t = red[0][lane & (L - 1)];
#pragma unroll
    for (int w = 1; w < kAlignWaves; ++w) t += red[w][lane & (L - 1)];
    return t;
}

// ---- the assignment rule, by one whole wave -------------------------------------------------------------------------
// d: lane i * K + j holds d[i][j].  f[mask]: the best value of rows popcount(mask) .. K-1 over the columns outside mask;
// a lane owns the masks lane + 64 * slot.  Returns the permutation, byte i = p[i], the same in every lane.
template <int K>
__device__ inline uint64_t solve_assignment(long long d, int lane) {
    constexpr int kSlots = (1 << K) > 64 ? (1 << K) / 64 : 1;
    long long f[kSlots];
    int arg[kSlots];
#pragma unroll
    for (int s = 0; s < kSlots; ++s) {
        f[s] = 0;                                             // (the full mask: nothing left to assign)
        arg[s] = 0;
    }
    const int dlo = (int)(d & 0xffffffffll), dhi = (int)(d >> 32);
#pragma unroll
    for (int level = K - 1; level >= 0; --level) {
#pragma unroll
        for (int s = 0; s < kSlots; ++s) {
            const int mask = lane + 64 * s;
            long long best = LLONG_MIN / 2;                     // (below every sum of K agreements, and safe to add to)
            int best_j = 0;
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const long long dij = ((long long)__builtin_amdgcn_readlane(dhi, level * K + j) << 32) |
                                      (long long)(unsigned)__builtin_amdgcn_readlane(dlo, level * K + j);
                const long long rest = j < 6 ? __shfl_xor(f[s], 1 << (j < 6 ? j : 0), 64) : f[(s ^ (1 << (j >= 6 ? j - 6 : 0))) & (kSlots - 1)];
                const long long cand = dij + rest;
                if (!((mask >> j) & 1) && cand > best) {       // (ascending j, strict: the smallest column of the maximum)
                    best = cand;
                    best_j = j;
                }
            }
            if (__popc(mask) == level) {                       // (what this level reads has popcount level + 1)
                f[s] = best;
                arg[s] = best_j;
            }
        }
    }
    uint64_t pack = 0;
    int mask = 0;
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const int src = __builtin_amdgcn_readfirstlane(mask & 63), slot = __builtin_amdgcn_readfirstlane(mask >> 6);
        int j = __builtin_amdgcn_readlane(arg[0], src);
#pragma unroll
        for (int s = 1; s < kSlots; ++s) {
            const int js = __builtin_amdgcn_readlane(arg[s], src);
            j = slot == s ? js : j;
        }
        pack |= (uint64_t)j << (8 * i);
        mask |= 1 << j;
    }
    return pack;
}

__device__ inline uint64_t invert_pack(uint64_t pack, int K) {
    uint64_t inv = 0;
    for (int i = 0; i < K; ++i) inv |= (uint64_t)i << (8 * ((pack >> (8 * i)) & 0xff));
    return inv;
}

// ---- the within-run kernel ------------------------------------------------------------------------------------------
struct WithinArgs {
    const uint32_t* bits;     // [runs][cap][K][W]
    const int32_t* rows;      // [runs]
    int8_t* perm;             // [runs][cap][K]
    int64_t cap;
    int N, W, G;              // objects, words, slices per word (a power of two up to 32)
    int seed_rows;
};

template <int K>
__device__ inline void load_words(uint32_t (&c)[K], const uint32_t* sample, int W, int w) {
#pragma unroll
    for (int j = 0; j < K; ++j) c[j] = sample[j * W + w];
}

// d[i][j] += sum[i][n] over the objects n of cluster j in this slice
template <int K, int L>
__device__ inline void add_agreement(long long (&acc)[L], const uint32_t (&c)[K], uint32_t slice, const int32_t* sums, int Np, int W, int w) {
#pragma unroll
    for (int j = 0; j < K; ++j) {
        uint32_t m = c[j] & slice;
        while (m) {
            const int at = (__ffs(m) - 1) * W + w;
            m &= m - 1;
#pragma unroll
            for (int i = 0; i < K; ++i) acc[i * K + j] += sums[i * Np + at];
        }
    }
}

// sum[inv[j]][n] += weight over the objects n of cluster j in this slice
template <int K>
__device__ inline void add_sample(int32_t* sums, const uint32_t (&c)[K], uint32_t slice, uint64_t inv, int weight, int Np, int W, int w) {
#pragma unroll
    for (int j = 0; j < K; ++j) {
        int32_t* row = sums + (int)((inv >> (8 * j)) & 0xff) * Np;
        uint32_t m = c[j] & slice;
        while (m) {
            row[(__ffs(m) - 1) * W + w] += weight;
            m &= m - 1;
        }
    }
}

__device__ inline uint32_t slice_mask(int g, int G) {
    const int bits = 32 / G;
    return bits == 32 ? 0xffffffffu : ((1u << bits) - 1u) << (g * bits);
}

template <int K>
__global__ __launch_bounds__(kAlignBlock) void k_align_within(WithinArgs a) {
    constexpr int L = pow2_at_least(K * K);
    extern __shared__ __align__(16) unsigned char dyn[];
    __shared__ long long red[kAlignWaves][64];
    __shared__ uint64_t inv_s;
    int32_t* sums = reinterpret_cast<int32_t*>(dyn);          // [K][32][W]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int W = a.W, G = a.G, Np = 32 * W, items = W * G;
    const int run = blockIdx.x;
    const int S = a.rows[run];
    const uint32_t* bits = a.bits + (int64_t)run * a.cap * K * W;
    int8_t* perm = a.perm + (int64_t)run * a.cap * K;
    const int64_t stride = (int64_t)K * W;                    // words per sample

    for (int q = tid; q < K * Np; q += kAlignBlock) sums[q] = 0;
    __syncthreads();
    const int m = min(a.seed_rows, S), weight = max(m, 1);
    for (int s = 0; s < m; ++s)                               // the seed: the raw first m samples
        for (int it = tid; it < items; it += kAlignBlock) {
            uint32_t c[K];
            load_words<K>(c, bits + s * stride, W, it % W);
            add_sample<K>(sums, c, slice_mask(it / W, G), kIdentityPack, 1, Np, W, it % W);
        }
    // (a lane reads and writes the sums of its own objects only: item it, it + 256, ... in every phase)

    const bool own = tid < items;
    const int w0 = own ? tid % W : 0;
    const uint32_t slice0 = own ? slice_mask(tid / W, G) : 0u;
    uint32_t cur[K], nxt[K];
#pragma unroll
    for (int j = 0; j < K; ++j) cur[j] = nxt[j] = 0;
    if (own && S > 0) load_words<K>(cur, bits, W, w0);
    for (int s = 0; s < S; ++s) {
        const uint32_t* sample = bits + s * stride;
        if (own && s + 1 < S) load_words<K>(nxt, sample + stride, W, w0);
        long long acc[L];
#pragma unroll
        for (int q = 0; q < L; ++q) acc[q] = 0;
        add_agreement<K, L>(acc, cur, slice0, sums, Np, W, w0);
        for (int it = tid + kAlignBlock; it < items; it += kAlignBlock) {
            uint32_t c[K];
            load_words<K>(c, sample, W, it % W);
            add_agreement<K, L>(acc, c, slice_mask(it / W, G), sums, Np, W, it % W);
        }
        const long long d = block_reduce_entries<L>(acc, red, lane, wave);      // barrier 1
        if (wave == 0) {
            const uint64_t pack = solve_assignment<K>(d, lane);
            if (lane == 0) inv_s = invert_pack(pack, K);
            if (lane < K) perm[(int64_t)s * K + lane] = (int8_t)((pack >> (8 * lane)) & 0xff);
        }
        __syncthreads();                                                         // barrier 2 (red is free again, inv_s is set)
        const uint64_t inv = inv_s;
        add_sample<K>(sums, cur, slice0, inv, weight, Np, W, w0);
        for (int it = tid + kAlignBlock; it < items; it += kAlignBlock) {
            uint32_t c[K];
            load_words<K>(c, sample, W, it % W);
            add_sample<K>(sums, c, slice_mask(it / W, G), inv, weight, Np, W, it % W);
        }
#pragma unroll
        for (int j = 0; j < K; ++j) cur[j] = nxt[j];
        // (inv_s is written again only after barrier 1 of the next step, which every wave reaches after reading it)
    }
}

// ---- counts: one thread per (run, label, word), over the rows from the run's burn-in on -----------------------------
__global__ __launch_bounds__(kAlignBlock) void k_align_counts(const uint32_t* bits, const int8_t* perm, const int32_t* rows, const int64_t* burn,
                                                              int aligned, int R, int K, int N, int W, int64_t cap, int32_t* cnt) {
    const int64_t t = (int64_t)blockIdx.x * kAlignBlock + threadIdx.x;
    if (t >= (int64_t)R * K * W) return;
    const int w = (int)(t % W), i = (int)((t / W) % K), r = (int)(t / ((int64_t)W * K));
    int c[32];
#pragma unroll
    for (int b = 0; b < 32; ++b) c[b] = 0;
    const int S = rows[r];
    for (int64_t s = burn[r]; s < S; ++s) {
        const int64_t row = (int64_t)r * cap + s;
        const int j = aligned ? perm[row * K + i] : i;
        const uint32_t word = bits[(row * K + j) * W + w];
#pragma unroll
        for (int b = 0; b < 32; ++b) c[b] += (word >> b) & 1u;
    }
#pragma unroll
    for (int b = 0; b < 32; ++b) {
        const int n = 32 * w + b;
        if (n < N) cnt[((int64_t)r * K + i) * N + n] = c[b];
    }
}

// ---- across runs: one workgroup per run b against the pivot ---------------------------------------------------------
template <int K>
__global__ __launch_bounds__(kAlignBlock) void k_align_runs(const int32_t* cnt, int pivot, int N, int8_t* run_perm, long long* agreement) {
    constexpr int L = pow2_at_least(K * K);
    __shared__ long long red[kAlignWaves][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
    const int32_t* ca = cnt + (int64_t)pivot * K * N;
    const int32_t* cb = cnt + (int64_t)b * K * N;
    long long acc[L];
#pragma unroll
    for (int q = 0; q < L; ++q) acc[q] = 0;
    for (int n = tid; n < N; n += kAlignBlock) {
        long long vb[K];
#pragma unroll
        for (int j = 0; j < K; ++j) vb[j] = cb[j * N + n];
#pragma unroll
        for (int i = 0; i < K; ++i) {
            const long long va = ca[i * N + n];
#pragma unroll
            for (int j = 0; j < K; ++j) acc[i * K + j] += va * vb[j];
        }
    }
    const long long d = block_reduce_entries<L>(acc, red, lane, wave);
    if (wave == 0) {
        if (lane < K * K) agreement[(int64_t)b * K * K + lane] = d;
        const uint64_t pack = solve_assignment<K>(d, lane);
        if (lane < K) run_perm[b * K + lane] = (int8_t)((pack >> (8 * lane)) & 0xff);
    }
}

}  // namespace

struct sbe_align : sbe_unit_handle, unit_bit_store {   // (sbe_unit.hip.h; ev: around the within-run kernel of the last sbe_align_within)
    bool perm_valid = false;
    int8_t* d_perm = nullptr;           // [runs][cap][K]
    size_t perm_bytes = 0;
    int32_t* d_cnt = nullptr;           // [runs][K][N]
    size_t cnt_bytes = 0;
    int32_t* d_rows = nullptr;          // [SBE_ALIGN_MAX_RUNS]
    int64_t* d_burn = nullptr;          // [SBE_ALIGN_MAX_RUNS]
    int8_t* d_run_perm = nullptr;       // [SBE_ALIGN_MAX_RUNS][kMaxK]
    long long* d_agree = nullptr;       // [SBE_ALIGN_MAX_RUNS][kMaxK][kMaxK]
    std::vector<void*> buffers() const { return {d_bits, d_perm, d_stage, d_cnt, d_rows, d_burn, d_run_perm, d_agree}; }
};

namespace {

constexpr char kNullHandle[] = "null handle";
constexpr char kLane[] = "run", kReset[] = "sbe_align_reset";

int64_t max_objects(int K) {
    if (K < 1 || K > kMaxK) return 0;
    return (int64_t)(SBE_ALIGN_LDS_BYTES - SBE_ALIGN_STATIC_LDS) / (4 * K);
}

int upload_rows(sbe_align* h) {
    int32_t rows32[SBE_ALIGN_MAX_RUNS];
    for (int r = 0; r < h->runs.count(); ++r) rows32[r] = (int32_t)h->runs.rows[(size_t)r];
    HIPCHK(h, hipMemcpyAsync(h->d_rows, rows32, (size_t)h->runs.count() * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));              // (rows32 lives on this frame)
    return SBE_OK;
}

template <int K>
int launch_within(sbe_align* h, const WithinArgs& args, size_t lds) {
    HIPCHK(h, hipFuncSetAttribute((const void*)k_align_within<K>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)(SBE_ALIGN_LDS_BYTES - SBE_ALIGN_STATIC_LDS + 4 * 31 * kMaxK)));
    k_align_within<K><<<(unsigned)h->runs.count(), kAlignBlock, lds, h->stream>>>(args);
    HIPCHK(h, hipGetLastError());
    return SBE_OK;
}

template <int K>
int launch_runs(sbe_align* h, int pivot) {
    k_align_runs<K><<<(unsigned)h->runs.count(), kAlignBlock, 0, h->stream>>>(h->d_cnt, pivot, (int)h->N, h->d_run_perm, h->d_agree);
    HIPCHK(h, hipGetLastError());
    return SBE_OK;
}

// fn(std::integral_constant<int, K>()) for the store's K in 1 .. kMaxK: the kernels are compiled per K
template <class Fn>
int for_clusters(int K, Fn fn) {
    switch (K) {
        case 1: return fn(std::integral_constant<int, 1>());
        case 2: return fn(std::integral_constant<int, 2>());
        case 3: return fn(std::integral_constant<int, 3>());
        case 4: return fn(std::integral_constant<int, 4>());
        case 5: return fn(std::integral_constant<int, 5>());
        case 6: return fn(std::integral_constant<int, 6>());
        case 7: return fn(std::integral_constant<int, 7>());
        default: return fn(std::integral_constant<int, 8>());
    }
}

// the counts of every run into d_cnt (arguments checked by the caller)
int run_counts(sbe_align* h, int aligned, const int64_t* burn_rows) {
    HIPCHK(h, hipSetDevice(h->device));
    int rc = upload_rows(h);
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(h->d_burn, burn_rows, (size_t)h->runs.count() * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
    const int64_t threads = (int64_t)h->runs.count() * h->K * h->W;
    k_align_counts<<<(unsigned)div_up(threads, kAlignBlock), kAlignBlock, 0, h->stream>>>(h->d_bits, h->d_perm, h->d_rows, h->d_burn, aligned ? 1 : 0,
                                                                                        h->runs.count(), h->K, (int)h->N, (int)h->W, h->runs.cap, h->d_cnt);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));              // (burn_rows is the caller's)
    return SBE_OK;
}

int check_counts_args(sbe_align* h, int aligned, const int64_t* burn_rows) {
    if (const int rc = h->runs.check_shaped(h, kReset)) return rc;
    if (!burn_rows) return fail(h, SBE_ERR_ARG, "null pointer argument: burn_rows");
    for (int r = 0; r < h->runs.count(); ++r)
        if (burn_rows[r] < 0 || burn_rows[r] > h->runs.rows[(size_t)r])
            return fail(h, SBE_ERR_ARG, "burn_rows[%d]=%lld out of range [0, %lld] (rows stored for the run)", r, (long long)burn_rows[r],
                        (long long)h->runs.rows[(size_t)r]);
    if (aligned && !h->perm_valid)
        return fail(h, SBE_ERR_STATE, "no permutations for the rows stored (sbe_align_within comes first, after the last append)");
    return SBE_OK;
}

}  // namespace

extern "C" {

int sbe_align_abi_version(void) { return SBE_ALIGN_ABI_VERSION; }

const char* sbe_align_last_error(const sbe_align* h) { return unit_last_error(h); }

int64_t sbe_align_max_objects(int n_clusters) { return max_objects(n_clusters); }

int sbe_align_create(sbe_align** out, int device) { return unit_create_on_device(out, device, "sbe_align_create"); }

int sbe_align_destroy(sbe_align* h) { return unit_destroy(h, kNullHandle); }

int sbe_align_last_kernel_ms(const sbe_align* h, float* ms_out) { return unit_last_kernel_ms(h, ms_out, kNullHandle); }

int sbe_align_reset(sbe_align* h, int n_runs, int n_clusters, int64_t n_objects, int64_t capacity_rows) {
    CHECK_HANDLE(h, kNullHandle);
    if (n_runs < 1 || n_runs > SBE_ALIGN_MAX_RUNS) return fail(h, SBE_ERR_ARG, "n_runs=%d out of range [1, %d]", n_runs, SBE_ALIGN_MAX_RUNS);
    if (n_clusters < 1 || n_clusters > kMaxK) return fail(h, SBE_ERR_ARG, "n_clusters=%d out of range [1, %d]", n_clusters, kMaxK);
    if (n_objects < 1 || n_objects > max_objects(n_clusters))
        return fail(h, SBE_ERR_ARG, "n_objects=%lld out of range [1, %lld] for %d clusters (the running sums live in LDS)", (long long)n_objects,
                    (long long)max_objects(n_clusters), n_clusters);
    if (capacity_rows < 1 || capacity_rows > SBE_ALIGN_MAX_ROWS)
        return fail(h, SBE_ERR_ARG, "capacity_rows=%lld out of range [1, %d]", (long long)capacity_rows, SBE_ALIGN_MAX_ROWS);
    h->runs.rows.clear();                                 // (a failed allocation leaves an unshaped store)
    h->perm_valid = false;
    HIPCHK(h, hipSetDevice(h->device));
    int rc = h->alloc_bits(h, n_runs, n_clusters, n_objects, capacity_rows);
    if (!rc) rc = unit_ensure(h, h->d_perm, h->perm_bytes, (size_t)n_runs * (size_t)capacity_rows * (size_t)n_clusters);
    if (!rc) rc = unit_ensure(h, h->d_cnt, h->cnt_bytes, (size_t)n_runs * (size_t)n_clusters * (size_t)n_objects * sizeof(int32_t));
    if (!rc) rc = unit_ensure(h, h->d_rows, (size_t)SBE_ALIGN_MAX_RUNS * sizeof(int32_t));
    if (!rc) rc = unit_ensure(h, h->d_burn, (size_t)SBE_ALIGN_MAX_RUNS * sizeof(int64_t));
    if (!rc) rc = unit_ensure(h, h->d_run_perm, (size_t)SBE_ALIGN_MAX_RUNS * kMaxK);
    if (!rc) rc = unit_ensure(h, h->d_agree, (size_t)SBE_ALIGN_MAX_RUNS * kMaxK * kMaxK * sizeof(long long));
    if (rc) return rc;
    h->set_shape(n_runs, n_clusters, n_objects, capacity_rows);
    return SBE_OK;
}

int sbe_align_rows(const sbe_align* h, int run, int64_t* n_rows_out) {
    CHECK_HANDLE(h, kNullHandle);
    return h->runs.get(h, kLane, run, n_rows_out);
}

int sbe_align_append_rows(sbe_align* h, int run, const uint8_t* rows, int64_t n_rows) {
    CHECK_HANDLE(h, kNullHandle);
    return h->append(h, kLane, kReset, run, rows, n_rows, [&](int64_t, int64_t) {
        h->perm_valid = false;                            // (the store changes from the first piece on)
        return SBE_OK;
    });
}

int sbe_align_within(sbe_align* h, int seed_rows, int8_t* perm_out) {
    CHECK_HANDLE(h, kNullHandle);
    if (const int rc = h->runs.check_shaped(h, kReset)) return rc;
    if (seed_rows < 0 || seed_rows > SBE_ALIGN_MAX_SEED_ROWS)
        return fail(h, SBE_ERR_ARG, "seed_rows=%d out of range [0, %d]", seed_rows, SBE_ALIGN_MAX_SEED_ROWS);
    if (!perm_out) return fail(h, SBE_ERR_ARG, "null pointer argument: perm_out");
    HIPCHK(h, hipSetDevice(h->device));
    int rc = upload_rows(h);
    if (rc) return rc;
    int G = 1;                                            // slices per word: the items fill the block where they can
    while (G < 32 && h->W * G * 2 <= kAlignBlock) G *= 2;
    const WithinArgs args{h->d_bits, h->d_rows, h->d_perm, h->runs.cap, (int)h->N, (int)h->W, G, seed_rows};
    const size_t lds = (size_t)h->K * 32 * (size_t)h->W * sizeof(int32_t);
    rc = unit_timed(h, [&] { return for_clusters(h->K, [&](auto k) { return launch_within<k()>(h, args, lds); }); });
    if (rc) return rc;
    for (int r = 0; r < h->runs.count(); ++r) {
        const size_t bytes = (size_t)h->runs.rows[(size_t)r] * (size_t)h->K;
        if (bytes)
            HIPCHK(h, hipMemcpyAsync(perm_out + (int64_t)r * h->runs.cap * h->K, h->d_perm + (int64_t)r * h->runs.cap * h->K, bytes, hipMemcpyDeviceToHost, h->stream));
    }
    if ((rc = unit_sync_timed(h))) return rc;
    h->perm_valid = true;
    return SBE_OK;
}

int sbe_align_counts(sbe_align* h, int aligned, const int64_t* burn_rows, int32_t* counts_out) {
    CHECK_HANDLE(h, kNullHandle);
    int rc = check_counts_args(h, aligned, burn_rows);
    if (rc) return rc;
    if (!counts_out) return fail(h, SBE_ERR_ARG, "null pointer argument: counts_out");
    rc = run_counts(h, aligned, burn_rows);
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(counts_out, h->d_cnt, (size_t)h->runs.count() * (size_t)h->K * (size_t)h->N * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return SBE_OK;
}

int sbe_align_runs(sbe_align* h, int pivot, int aligned, const int64_t* burn_rows, int8_t* run_perm_out, int64_t* agreement_out) {
    CHECK_HANDLE(h, kNullHandle);
    int rc = check_counts_args(h, aligned, burn_rows);
    if (rc) return rc;
    if (pivot < 0 || pivot >= h->runs.count()) return fail(h, SBE_ERR_ARG, "pivot %d out of range [0,%d)", pivot, h->runs.count());
    if (!run_perm_out || !agreement_out) return fail(h, SBE_ERR_ARG, "null pointer argument: output");
    rc = run_counts(h, aligned, burn_rows);
    if (rc) return rc;
    rc = for_clusters(h->K, [&](auto k) { return launch_runs<k()>(h, pivot); });
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(run_perm_out, h->d_run_perm, (size_t)h->runs.count() * (size_t)h->K, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(agreement_out, h->d_agree, (size_t)h->runs.count() * (size_t)h->K * (size_t)h->K * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return SBE_OK;
}

}  // extern "C"
