// sbe_pairppc.hip -- the pairwise posterior predictive check (include/sbe_pairppc.h): the screening's chi-squared statistic of
// every feature pair on the data and on a stream of replicated data sets, and per pair where the observed value falls among
// the replicated ones.  The numerical contract is tests/_pairppc_oracle.py; DESIGN.md section 25 has the layout.
//
// The arithmetic of a tile pair is sbe_assoc_pair.hip.h's, shared with sbe_assoc.hip.  k_pairppc_observed is the screening's
// pair kernel without the p-value.  k_pairppc_replicates<false> (the sequential form) runs one wave per tile pair I <= J over all
// replicates of the call in order: the pairs' stat_obs and their six accumulators come from the handle's [F][F] buffers into LDS
// once, every replicate's tile goes through steps 1 to 4 and one lane per sub-table compares and adds, and the accumulators go
// back once.  The order over replicates is the loop's, so nothing depends on how a stream is split over calls or tile pairs over
// launches; apart from the optional stat_rep nothing is written per replicate.  Below kSpreadBelow tile pairs one wave
// each leaves the device idle or unevenly loaded, and a call of several replicates takes the spread form: k_pairppc_replicates<true>
// deals the replicates out over waves, which hold each statistic back (8 bytes per pair and replicate), and k_pairppc_accumulate
// adds them per pair in replicate order by the same tally() -- the same bits.  k_pairppc_fill checks the uploaded codes and turns them
// feature-major (the 32 x 32 transpose of sbe_unit_device.hip.h with the replicate on the grid's z axis and the check folded in).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "sbe_assoc_pair.hip.h"
#include "../../include/sbe_pairppc.h"

namespace {

constexpr unsigned long long kNoOffender = ~0ull;
constexpr int kMaxGridZ = 65535;
constexpr int64_t kMinLaunchTiles = 1024;            // SIMDs of an MI355X
constexpr int64_t kSpreadWaves = 8 * 4096;           // the spread form's waves per group: eight rounds of four waves per SIMD
constexpr int64_t kHeldBytes = SBE_PAIRPPC_HELD_BYTES;   // ... and the statistics it holds back at a time (a fixed buffer of the handle)
constexpr int64_t kSpreadBelow = 8192;               // tile pairs below which a call of several replicates takes the spread form by itself

// ---- the fill: y [n][N][F] (staging) -> img [n][F][n_pad] (set to NA before), and the first code that is neither below its
// feature's state count nor NA, by its index in y (an integer atomic minimum).  blockIdx.x: object tile, y: feature tile,
// z + r0: replicate
__global__ __launch_bounds__(256) void k_pairppc_fill(const uint8_t* y, int64_t N, int64_t F, int64_t n_pad, const int32_t* n_states, int64_t r0,
                                                      uint8_t* img, unsigned long long* offender) {
    __shared__ uint8_t tile[32][33];
    const int64_t r = r0 + blockIdx.z, n0 = (int64_t)blockIdx.x * 32, f0 = (int64_t)blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;     // 32 x 8
    const uint8_t* src = y + r * N * F;
    uint8_t* dst = img + r * F * n_pad;
    for (int k = ty; k < 32; k += 8) {
        const int64_t row = n0 + k, col = f0 + tx;
        if (row < N && col < F) {
            const uint8_t c = src[row * F + col];
            if (c != SBE_PAIRPPC_NA && (int32_t)c >= n_states[col]) atomicMin(offender, (unsigned long long)((r * N + row) * F + col));
            tile[k][tx] = c;
        }
    }
    __syncthreads();
    for (int c = ty; c < 32; c += 8) {
        const int64_t col = f0 + c, row = n0 + tx;
        if (row < N && col < F) dst[col * n_pad + row] = tile[tx][c];
    }
}

// ---- the observed statistic: the screening's pair kernel without the p-value -------------------------------------------------
struct ObservedArgs {
    const uint8_t* xt;        // codes, feature-major [F][n_pad], padded with 255 behind N
    int64_t n_pad;            // multiple of kPad
    int F, log_s;             // S_pad = 1 << log_s
    int64_t t0, t_end;        // tile pairs [t0, t_end) of the enumeration t = J (J + 1) / 2 + I, I <= J
    double* statistic;        // [F][F] outputs (zeroed before: the diagonal is no pair)
    int32_t* dof;
    int32_t* n;
    uint8_t* valid;
};

__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 4))) void k_pairppc_observed(const ObservedArgs g) {
    extern __shared__ double pairppc_lds[];                  // dynamic LDS, pair_lds_bytes(sub)
    const int S = 1 << g.log_s, sub = kTile >> g.log_s;
    const PairLds l = pair_lds(pairppc_lds, sub);
    const int64_t t = g.t0 + blockIdx.x;
    if (t >= g.t_end) return;
    const TilePair pair = tile_pair(t);
    const int64_t I = pair.I, J = pair.J;
    const int lane = threadIdx.x;
    const v16f acc = pair_contract(g.xt, g.n_pad, g.F, g.log_s, I, J, lane);
    pair_terms(l, acc, g.log_s, lane);
    for (int idx = lane; idx < sub * sub; idx += 64) {
        const int p = idx / sub, q = idx - p * sub;
        const int64_t i = I * sub + p, j = J * sub + q;
        if (i >= j || j >= g.F) continue;                // (i < j: the diagonal tile pairs hold every pair twice)
        const int dof = l.pdof[idx];
        const double stat = dof > 0 ? pair_statistic(l, p, q, S) : 0.0;
        const int n = (int)l.pn[idx];
        for (int m = 0; m < 2; ++m) {
            const int64_t o = m ? j * g.F + i : i * g.F + j;
            g.statistic[o] = stat;
            g.dof[o] = dof;
            g.n[o] = n;
            g.valid[o] = dof > 0;
        }
    }
}

// ---- the replicates ------------------------------------------------------------------------------------------------------
// one replicate's statistic s of a pair into the pair's six accumulators: the contract's step, written once for both forms
__device__ inline void tally(double s, bool degenerate, double obs, int& n_greater, int& n_equal, int& n_less, int& n_degenerate, double& sum,
                             double& sumsq) {
    if (degenerate) n_degenerate += 1;
    if (s > obs)
        n_greater += 1;
    else if (s == obs)
        n_equal += 1;
    else
        n_less += 1;
    sum += s;
    const double sq = s * s;                                 // (rounded, then added: the build keeps -ffp-contract=off)
    sumsq += sq;
}

struct ReplicateArgs {
    const uint8_t* img;       // [n_rep][F][n_pad]: the replicates of this launch
    int64_t n_pad, n_rep;
    int F, log_s;
    int64_t t0, t_end;
    const double* stat_obs;   // [F][F] of the data
    const uint8_t* valid_obs;
    int32_t* counts;          // [4][F][F]: n_greater, n_equal, n_less, n_degenerate
    double* sum;              // [F][F]
    double* sumsq;
    double* stat_rep;         // null or [n_rep][F][F] (zeroed before)
    // the spread form only: replicates per workgroup along y, and where the statistics wait for k_pairppc_accumulate,
    // [tile pair][n_rep][sub-table], kDegenerate for a table without degrees of freedom
    int64_t chunk;
    double* held;
};

constexpr double kDegenerate = -1.0;                         // (a statistic is never negative)

// what a wave keeps per sub-table of its tile pair behind pair_lds_bytes(sub): 44 bytes each in the sequential form (stat_obs,
// the six accumulators, whether the pair is live), 4 in the spread form (live)
constexpr size_t kKeptBytes = 3 * sizeof(double) + 5 * sizeof(int);
inline size_t replicate_lds_bytes(int sub, bool spread) { return pair_lds_bytes(sub) + (size_t)sub * sub * (spread ? sizeof(int) : kKeptBytes); }

// Two forms, the same bits.  Sequential (kSpread false): a wave walks all replicates of the call and keeps its pairs'
// accumulators in LDS.  Spread (kSpread true): blockIdx.y deals the replicates in chunks to as many waves, which only hold the
// statistics back for k_pairppc_accumulate to add in replicate order -- for shapes with too few tile pairs to fill the device.
template <bool kSpread>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 4))) void k_pairppc_replicates(const ReplicateArgs g) {
    extern __shared__ double pairppc_lds[];                  // dynamic LDS, replicate_lds_bytes(sub, kSpread)
    const int S = 1 << g.log_s, sub = kTile >> g.log_s, ss = sub * sub;
    const PairLds l = pair_lds(pairppc_lds, sub);
    // (pair_lds_bytes is a multiple of 8.)  A sub-table's entries are read and written by one lane alone, the lane idx & 63
    double* k_obs = pairppc_lds + pair_lds_bytes(sub) / sizeof(double);
    double* k_sum = k_obs + ss;
    double* k_sumsq = k_sum + ss;
    int* k_count = reinterpret_cast<int*>(k_sumsq + ss);     // [4][ss]
    int* k_live = kSpread ? reinterpret_cast<int*>(k_obs) : k_count + 4 * ss;      // the pair i < j exists and is valid on the data

    const int64_t t = g.t0 + blockIdx.x;
    if (t >= g.t_end) return;
    const TilePair pair = tile_pair(t);
    const int64_t I = pair.I, J = pair.J, ff = (int64_t)g.F * g.F;
    const int lane = threadIdx.x;

    for (int idx = lane; idx < ss; idx += 64) {
        const int p = idx / sub, q = idx - p * sub;
        const int64_t i = I * sub + p, j = J * sub + q, o = i * g.F + j;
        const bool live = i < j && j < g.F && g.valid_obs[o] != 0;
        k_live[idx] = live;
        if (kSpread || !live) continue;
        k_obs[idx] = g.stat_obs[o];
        k_sum[idx] = g.sum[o];
        k_sumsq[idx] = g.sumsq[o];
        for (int c = 0; c < 4; ++c) k_count[c * ss + idx] = g.counts[c * ff + o];
    }

    const int64_t r_first = kSpread ? (int64_t)blockIdx.y * g.chunk : 0, r_end = kSpread ? min(g.n_rep, r_first + g.chunk) : g.n_rep;
    for (int64_t r = r_first; r < r_end; ++r) {
        const v16f acc = pair_contract(g.img + r * g.F * g.n_pad, g.n_pad, g.F, g.log_s, I, J, lane);
        // (the lane index behind an empty asm: the compiler then forms the LDS addresses of steps 2 to 4 per replicate instead of
        // keeping some seventy of them in registers across the loop, which would halve the waves per SIMD)
        int ln = lane;
        asm volatile("" : "+v"(ln));
        pair_terms(l, acc, g.log_s, ln);
        for (int idx = ln; idx < ss; idx += 64) {
            if (!k_live[idx]) continue;
            const int p = idx / sub, q = idx - p * sub;
            const bool degenerate = l.pdof[idx] == 0;
            const double s = degenerate ? 0.0 : pair_statistic(l, p, q, S);
            if (kSpread)
                g.held[(t * g.n_rep + r) * ss + idx] = degenerate ? kDegenerate : s;
            else
                tally(s, degenerate, k_obs[idx], k_count[idx], k_count[ss + idx], k_count[2 * ss + idx], k_count[3 * ss + idx], k_sum[idx], k_sumsq[idx]);
            if (g.stat_rep) {
                const int64_t i = I * sub + p, j = J * sub + q;
                g.stat_rep[r * ff + i * g.F + j] = s;
                g.stat_rep[r * ff + j * g.F + i] = s;
            }
        }
        __syncthreads();                                     // (the next replicate's counts go where these terms lie)
    }
    if (kSpread) return;

    for (int idx = lane; idx < ss; idx += 64) {
        if (!k_live[idx]) continue;
        const int p = idx / sub, q = idx - p * sub;
        const int64_t i = I * sub + p, j = J * sub + q;
        for (int m = 0; m < 2; ++m) {
            const int64_t o = m ? j * g.F + i : i * g.F + j;
            g.sum[o] = k_sum[idx];
            g.sumsq[o] = k_sumsq[idx];
            for (int c = 0; c < 4; ++c) g.counts[c * ff + o] = k_count[c * ss + idx];
        }
    }
}

// the spread form's second step: a thread per sub-table of the tile pairs [t0, t_end) adds what the waves held back, one
// replicate after the other
__global__ __launch_bounds__(256) void k_pairppc_accumulate(const ReplicateArgs g) {
    const int sub = kTile >> g.log_s, ss = sub * sub;
    const int64_t at = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, t = g.t0 + at / ss, ff = (int64_t)g.F * g.F;
    if (t >= g.t_end) return;
    const int idx = (int)(at % ss), p = idx / sub, q = idx - p * sub;
    const TilePair pair = tile_pair(t);
    const int64_t i = pair.I * sub + p, j = pair.J * sub + q, o = i * g.F + j;
    if (!(i < j && j < g.F && g.valid_obs[o] != 0)) return;
    const double obs = g.stat_obs[o];
    double sum = g.sum[o], sumsq = g.sumsq[o];
    int n_greater = g.counts[o], n_equal = g.counts[ff + o], n_less = g.counts[2 * ff + o], n_degenerate = g.counts[3 * ff + o];
    for (int64_t r = 0; r < g.n_rep; ++r) {
        const double v = g.held[(t * g.n_rep + r) * ss + idx];
        const bool degenerate = v == kDegenerate;
        tally(degenerate ? 0.0 : v, degenerate, obs, n_greater, n_equal, n_less, n_degenerate, sum, sumsq);
    }
    for (int m = 0; m < 2; ++m) {
        const int64_t w = m ? j * g.F + i : o;
        g.sum[w] = sum;
        g.sumsq[w] = sumsq;
        g.counts[w] = n_greater;
        g.counts[ff + w] = n_equal;
        g.counts[2 * ff + w] = n_less;
        g.counts[3 * ff + w] = n_degenerate;
    }
}

}  // namespace

struct sbe_pairppc : sbe_unit_handle, unit_tile_launches {   // (sbe_unit.hip.h; ev: around the pair kernel's launches)
    uint8_t* d_xt = nullptr;                     // the data's codes, feature-major [F][n_pad] (read by k_pairppc_observed)
    size_t xt_bytes = 0;
    int32_t* d_states = nullptr;                 // n_states [F]
    size_t states_bytes = 0;
    void* d_obs = nullptr;                       // stat_obs (8), dof_obs (4), n_obs (4), valid_obs (1) per entry of [F][F]
    size_t obs_bytes = 0;
    void* d_acc = nullptr;                       // sum (8), sumsq (8), the four counts (16) per entry of [F][F]
    size_t acc_bytes = 0;
    uint8_t* d_stage = nullptr;                  // the replicates of one add call as uploaded, [n][N][F]
    size_t stage_bytes = 0;
    uint8_t* d_img = nullptr;                    // ... feature-major [n][F][n_pad]
    size_t img_bytes = 0;
    double* d_rep = nullptr;                     // stat_rep of one add call
    size_t rep_bytes = 0;
    double* d_held = nullptr;                    // the spread form: the statistics of a group of replicates, [tile pair][replicate][sub-table]
    size_t held_bytes = 0;
    unsigned long long* d_offender = nullptr;
    int64_t N = 0, n_pad = 0, F = 0;             // shape of the data (F == 0: none yet)
    int log_s = 1;
    int64_t n_replicates = 0;
    int form = SBE_PAIRPPC_FORM_AUTO;
    int64_t tile_pairs = 0, launches = 0;
    std::vector<void*> buffers() const { return {d_xt, d_states, d_obs, d_acc, d_stage, d_img, d_rep, d_held, d_offender}; }

    size_t ff() const { return (size_t)F * (size_t)F; }
    double* stat_obs() const { return (double*)d_obs; }
    int32_t* dof_obs() const { return (int32_t*)(stat_obs() + ff()); }
    int32_t* n_obs() const { return dof_obs() + ff(); }
    uint8_t* valid_obs() const { return (uint8_t*)(n_obs() + ff()); }
    double* sum() const { return (double*)d_acc; }
    double* sumsq() const { return sum() + ff(); }
    int32_t* counts() const { return (int32_t*)(sumsq() + ff()); }
};

namespace {

constexpr char kNullHandle[] = "null handle";
constexpr size_t kObsEntry = 17, kAccEntry = 32;

bool shape_in_limits(int64_t N, int64_t F) {
    return N >= 1 && N <= SBE_ASSOC_MAX_OBJECTS && F >= 1 && F <= SBE_ASSOC_MAX_FEATURES && N * F <= SBE_ASSOC_MAX_CODES;
}

int64_t replicate_bytes(int64_t N, int64_t F, bool with_stat_rep) { return N * F + F * whole_rounds(N) + (with_stat_rep ? 8 * F * F : 0); }

int64_t tile_pairs_of(int64_t F, int log_s) {
    const int64_t sub = kTile >> log_s, tiles = (F + sub - 1) / sub;
    return tiles * (tiles + 1) / 2;
}

}  // namespace

extern "C" {

int sbe_pairppc_abi_version(void) { return SBE_PAIRPPC_ABI_VERSION; }

const char* sbe_pairppc_last_error(const sbe_pairppc* h) { return unit_last_error(h); }

int sbe_pairppc_create(sbe_pairppc** out, int device) { return unit_create_on_device(out, device, "sbe_pairppc_create"); }

int sbe_pairppc_destroy(sbe_pairppc* h) { return unit_destroy(h, kNullHandle); }

int sbe_pairppc_set_launch_tiles(sbe_pairppc* h, int64_t tile_pairs) { return unit_set_launch_tiles(h, tile_pairs, kNullHandle); }

int sbe_pairppc_set_form(sbe_pairppc* h, int form) {
    CHECK_HANDLE(h, kNullHandle);
    if (form < SBE_PAIRPPC_FORM_AUTO || form > SBE_PAIRPPC_FORM_SPREAD)
        return fail(h, SBE_ERR_ARG, "form=%d is none of %d (auto), %d (sequential), %d (spread)", form, SBE_PAIRPPC_FORM_AUTO, SBE_PAIRPPC_FORM_SEQUENTIAL,
                     SBE_PAIRPPC_FORM_SPREAD);
    h->form = form;
    return SBE_OK;
}

int64_t sbe_pairppc_replicate_bytes(int64_t n_objects, int64_t n_features, int with_stat_rep) {
    return shape_in_limits(n_objects, n_features) ? replicate_bytes(n_objects, n_features, with_stat_rep != 0) : 0;
}

int sbe_pairppc_set_data(sbe_pairppc* h, const uint8_t* x, int64_t n_objects, int64_t n_features, const int32_t* n_states) {
    CHECK_HANDLE(h, kNullHandle);
    if (!x || !n_states) return fail(h, SBE_ERR_ARG, "null pointer argument: %s", !x ? "x" : "n_states");
    const int64_t N = n_objects, F = n_features;
    int s_max = 1;
    if (const int rc = pair_check_shape(h, N, F, n_states, s_max)) return rc;
    const int64_t n_pad = whole_rounds(N);
    std::vector<uint8_t> xt;
    if (const int rc = pair_feature_major(h, x, N, F, n_states, n_pad, xt)) return rc;
    const int log_s = pair_log_s(s_max), sub = kTile >> log_s;
    const int64_t tile_pairs = tile_pairs_of(F, log_s);
    const int64_t per_launch = tiles_per_launch(n_pad / kStep, h->launch_tiles);

    HIPCHK(h, hipSetDevice(h->device));
    h->F = 0;                                       // (until the new data is in place)
    const size_t ff = (size_t)F * F;
    int rc = unit_ensure(h, h->d_xt, h->xt_bytes, xt.size());
    if (!rc) rc = unit_ensure(h, h->d_states, h->states_bytes, (size_t)F * sizeof(int32_t));
    if (!rc) rc = unit_ensure(h, h->d_obs, h->obs_bytes, ff * kObsEntry);
    if (!rc) rc = unit_ensure(h, h->d_acc, h->acc_bytes, ff * kAccEntry);
    if (!rc) rc = unit_ensure(h, h->d_offender, sizeof(unsigned long long));
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(h->d_xt, xt.data(), xt.size(), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_states, n_states, (size_t)F * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(h->d_obs, 0, ff * kObsEntry, h->stream));       // (all-zero bytes: statistic 0, dof 0, n 0, not valid)
    HIPCHK(h, hipMemsetAsync(h->d_acc, 0, ff * kAccEntry, h->stream));
    double* d_stat = (double*)h->d_obs;
    int32_t* d_dof = (int32_t*)(d_stat + ff);
    int32_t* d_n = d_dof + ff;
    uint8_t* d_valid = (uint8_t*)(d_n + ff);
    int64_t launches = 0;
    rc = unit_timed(h, [&] {
        return unit_for_tile_launches(tile_pairs, per_launch, [&](int64_t t0, int64_t t_end) {      // one wave per tile pair
            const ObservedArgs args{h->d_xt, n_pad, (int)F, log_s, t0, t_end, d_stat, d_dof, d_n, d_valid};
            k_pairppc_observed<<<(unsigned)(t_end - t0), 64, pair_lds_bytes(sub), h->stream>>>(args);
            HIPCHK(h, hipGetLastError());
            ++launches;
            return SBE_OK;
        });
    });
    if (!rc) rc = unit_sync_timed(h);
    if (rc) return rc;
    h->N = N;
    h->n_pad = n_pad;
    h->F = F;
    h->log_s = log_s;
    h->n_replicates = 0;
    h->tile_pairs = tile_pairs;
    h->launches = launches;
    return SBE_OK;
}

int sbe_pairppc_add(sbe_pairppc* h, int64_t n, const uint8_t* y_rep, double* stat_rep_out) {
    CHECK_HANDLE(h, kNullHandle);
    if (h->F == 0) return fail(h, SBE_ERR_STATE, "sbe_pairppc_add needs the data of a successful sbe_pairppc_set_data");
    if (n < 0) return fail(h, SBE_ERR_ARG, "n=%lld is negative", (long long)n);
    if (n == 0) return SBE_OK;
    if (!y_rep) return fail(h, SBE_ERR_ARG, "null pointer argument: y_rep");
    const int64_t N = h->N, F = h->F, n_pad = h->n_pad, each = replicate_bytes(N, F, stat_rep_out != nullptr);
    if (n > SBE_PAIRPPC_MAX_STAGE_BYTES / each)
        return fail(h, SBE_ERR_ARG, "%lld replicates of %lld bytes each exceed the %lld bytes one call holds on the device (split the block)",
                     (long long)n, (long long)each, (long long)SBE_PAIRPPC_MAX_STAGE_BYTES);
    const int log_s = h->log_s, sub = kTile >> log_s;
    const int64_t tile_pairs = tile_pairs_of(F, log_s);
    // Spread form: too few tile pairs to fill the device with one wave each, and more than one replicate to deal out.  The
    // replicates go in groups whose held statistics fit kHeldBytes, each group in chunks over about kSpreadWaves waves.
    const bool spread = h->form == SBE_PAIRPPC_FORM_AUTO ? (tile_pairs < kSpreadBelow && n > 1) : h->form == SBE_PAIRPPC_FORM_SPREAD;
    const int64_t ss = (int64_t)sub * sub;
    const int64_t group = spread ? std::max<int64_t>(1, std::min<int64_t>(n, kHeldBytes / (tile_pairs * ss * (int64_t)sizeof(double)))) : n;
    const int64_t chunks = spread ? std::min<int64_t>(std::min<int64_t>(group, kMaxGridZ), div_up(kSpreadWaves, tile_pairs)) : 1;
    const int64_t chunk = (group + chunks - 1) / chunks;
    // (a wave walks its replicates of the call, which the staging limit bounds: at least a wave per SIMD and launch)
    const int64_t per_launch = h->launch_tiles > 0 ? h->launch_tiles : std::max(kMinLaunchTiles, tiles_per_launch(chunk * (n_pad / kStep)));
    const size_t ff = h->ff();

    HIPCHK(h, hipSetDevice(h->device));
    int rc = unit_ensure(h, h->d_stage, h->stage_bytes, (size_t)(n * N * F));
    if (!rc) rc = unit_ensure(h, h->d_img, h->img_bytes, (size_t)(n * F * n_pad));
    if (!rc && stat_rep_out) rc = unit_ensure(h, h->d_rep, h->rep_bytes, (size_t)n * ff * sizeof(double));
    if (!rc && spread) rc = unit_ensure(h, h->d_held, h->held_bytes, (size_t)(tile_pairs * group * ss) * sizeof(double));
    if (rc) return rc;
    // the upload, checked and turned feature-major; nothing of the accumulators is touched before the codes have passed
    unsigned long long offender = kNoOffender;
    HIPCHK(h, hipMemcpyAsync(h->d_stage, y_rep, (size_t)(n * N * F), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_offender, &offender, sizeof offender, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(h->d_img, SBE_PAIRPPC_NA, (size_t)(n * F * n_pad), h->stream));
    for (int64_t r0 = 0; r0 < n; r0 += kMaxGridZ) {
        const dim3 grid((unsigned)div_up(N, 32), (unsigned)div_up(F, 32), (unsigned)std::min<int64_t>(kMaxGridZ, n - r0));
        k_pairppc_fill<<<grid, 256, 0, h->stream>>>(h->d_stage, N, F, n_pad, h->d_states, r0, h->d_img, h->d_offender);
        HIPCHK(h, hipGetLastError());
    }
    HIPCHK(h, hipMemcpyAsync(&offender, h->d_offender, sizeof offender, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (offender != kNoOffender) {
        const int64_t at = (int64_t)offender, f = at % F, i = at / F % N, r = at / (N * F);
        return fail(h, SBE_ERR_DATA, "y_rep[%lld][%lld][%lld]=%d is neither below n_states[%lld] nor %d (not observed)", (long long)r, (long long)i,
                     (long long)f, (int)y_rep[at], (long long)f, SBE_PAIRPPC_NA);
    }
    if (stat_rep_out) HIPCHK(h, hipMemsetAsync(h->d_rep, 0, (size_t)n * ff * sizeof(double), h->stream));
    int64_t launches = 0;
    rc = unit_timed(h, [&] {
        for (int64_t r0 = 0; r0 < n; r0 += group) {                  // (the sequential form: one group)
            const int64_t n_rep = std::min(group, n - r0);
            const int rc_group = unit_for_tile_launches(tile_pairs, per_launch, [&](int64_t t0, int64_t t_end) {
                const ReplicateArgs args{h->d_img + r0 * F * n_pad, n_pad, n_rep, (int)F, log_s, t0, t_end, h->stat_obs(), h->valid_obs(), h->counts(),
                                         h->sum(), h->sumsq(), stat_rep_out ? h->d_rep + r0 * (int64_t)ff : nullptr, chunk, h->d_held};
                if (spread) {
                    const dim3 grid((unsigned)(t_end - t0), (unsigned)div_up(n_rep, chunk));
                    k_pairppc_replicates<true><<<grid, 64, replicate_lds_bytes(sub, true), h->stream>>>(args);
                    HIPCHK(h, hipGetLastError());
                    k_pairppc_accumulate<<<(unsigned)div_up((t_end - t0) * ss, 256), 256, 0, h->stream>>>(args);
                } else {
                    k_pairppc_replicates<false><<<(unsigned)(t_end - t0), 64, replicate_lds_bytes(sub, false), h->stream>>>(args);
                }
                HIPCHK(h, hipGetLastError());
                ++launches;
                return SBE_OK;
            });
            if (rc_group) return rc_group;
        }
        return SBE_OK;
    });
    if (!rc && stat_rep_out) rc = unit_copy_back(h, (const double*)h->d_rep, (size_t)n * ff, {stat_rep_out});
    if (!rc) rc = unit_sync_timed(h);
    if (rc) return rc;
    h->n_replicates += n;
    h->tile_pairs = tile_pairs;
    h->launches = launches;
    return SBE_OK;
}

int sbe_pairppc_read(sbe_pairppc* h, double* stat_obs, int32_t* dof_obs, int32_t* n_obs, uint8_t* valid_obs, int32_t* n_greater,
                     int32_t* n_equal, int32_t* n_less, int32_t* n_degenerate, double* sum, double* sumsq, int64_t* n_replicates_out) {
    CHECK_HANDLE(h, kNullHandle);
    if (!stat_obs || !dof_obs || !n_obs || !valid_obs || !n_greater || !n_equal || !n_less || !n_degenerate || !sum || !sumsq || !n_replicates_out)
        return fail(h, SBE_ERR_ARG, "null pointer argument: output");
    if (h->F == 0) return fail(h, SBE_ERR_STATE, "sbe_pairppc_read needs the data of a successful sbe_pairppc_set_data");
    HIPCHK(h, hipSetDevice(h->device));
    const size_t ff = h->ff();
    int rc = unit_copy_back(h, (const double*)h->stat_obs(), ff, {stat_obs});
    if (!rc) rc = unit_copy_back(h, (const int32_t*)h->dof_obs(), ff, {dof_obs, n_obs});
    if (!rc) rc = unit_copy_back(h, (const uint8_t*)h->valid_obs(), ff, {valid_obs});
    if (!rc) rc = unit_copy_back(h, (const double*)h->sum(), ff, {sum, sumsq});
    if (!rc) rc = unit_copy_back(h, (const int32_t*)h->counts(), ff, {n_greater, n_equal, n_less, n_degenerate});
    if (rc) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    *n_replicates_out = h->n_replicates;
    return SBE_OK;
}

int sbe_pairppc_reset(sbe_pairppc* h) {
    CHECK_HANDLE(h, kNullHandle);
    if (h->F == 0) return fail(h, SBE_ERR_STATE, "sbe_pairppc_reset needs the data of a successful sbe_pairppc_set_data");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemsetAsync(h->d_acc, 0, h->ff() * kAccEntry, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->n_replicates = 0;
    return SBE_OK;
}

int sbe_pairppc_last_shape(const sbe_pairppc* h, int32_t* s_pad_out, int64_t* tile_pairs_out, int64_t* launches_out) {
    CHECK_HANDLE(h, kNullHandle);
    if (!s_pad_out || !tile_pairs_out || !launches_out) return fail(h, SBE_ERR_ARG, "null pointer argument: output");
    if (h->F == 0) return fail(h, SBE_ERR_STATE, "no successful sbe_pairppc_set_data yet");
    *s_pad_out = 1 << h->log_s;
    *tile_pairs_out = h->tile_pairs;
    *launches_out = h->launches;
    return SBE_OK;
}

int sbe_pairppc_last_kernel_ms(const sbe_pairppc* h, float* ms_out) { return unit_last_kernel_ms(h, ms_out, kNullHandle); }

}  // extern "C"
