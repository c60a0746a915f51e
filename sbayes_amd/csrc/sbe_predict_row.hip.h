#pragma once
// sbe_predict_row.hip.h -- the mixture row of a cell, m_t[n,f,.], written once for the units that put the logged samples back
// on the data: the posterior predictive (sbe_predict.hip), the posterior predictive check (sbe_ppc.hip), the per-cluster
// evidence (sbe_contrib.hip), the leave-one-out predictive (sbe_loopred.hip) and the leave-one-object-out ELPD
// (sbe_objloo.hip).  All take the data
// and a sample of include/sbe_predict.h word for word, so they share what reads them.  Device side: the
// ids kernel, the validation kernel with the offender's key, the staging of a sample's slice
// into one of two LDS buffers and the w~ / m arithmetic of a cell.  A unit's kernel
// calls, per workgroup, tile_cell and cell_group once and, per sample, stage_slice, cell_weights and cell_state
// (sbe_contrib.hip and sbe_objloo.hip: cell_weights_in_and_out, cell_state and cell_state_in, the object placed in every cluster
// and in none).
// Host side: the checks of the data's arguments, the plan of the feature tile, the messages of the offender's key, and the
// sample store, which a unit's handle derives from: the data and the samples of the call in flight on the device, the whole of
// <prefix>_set_feature_tile, the device part of <prefix>_set_data (upload), the opening of a compute call up to the offender's
// key (stage), the common fields of a kernel's argument struct (fill), the tile launch (launch_tiles) and the "no data yet"
// message.  A unit keeps its own checks, buffers, sample_bytes and what follows the key; DESIGN.md section 7.1.
// Everything lives in an unnamed namespace, as the unit layer does: every unit compiles its own copy.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "sbe_unit.hip.h"
#include "../../include/sbe_predict.h"

namespace {

constexpr int kBlock = 256;
constexpr int kMaxS = SBE_PREDICT_MAX_STATES;
constexpr int kMaxC = SBE_PREDICT_MAX_COMPONENTS;
constexpr int kMaxR = SBE_PREDICT_MAX_ROWS;
constexpr int kMaxTile = SBE_PREDICT_MAX_TILE;
constexpr uint16_t kNoCluster = 0xFFFF;
constexpr uint8_t kNA = SBE_PREDICT_NA;
constexpr unsigned long long kNoError = ~0ull;
constexpr int kDefaultTile = 16;                     // features per tile, where the slice allows it
constexpr size_t kSmallSlices = (size_t)40 << 10;    // the default plan keeps the two slices under this: four workgroups per CU
static_assert(kMaxTile <= kBlock, "a tile of Ft features gives every thread of a row of Ft a feature");

// kinds of offender, in the order the headers list them (the seventh is the unit's to word: sbe_ppc.h's uniforms, kUniform, and
// sbe_objloo.h's prior rows, which take the same slot)
enum : int { kOverlap = 0, kWeightEntry = 1, kWeightSum = 2, kTableEntry = 3, kTableRowEmpty = 4, kTableSum = 5, kUniform = 6 };

__host__ __device__ inline unsigned long long error_key(int64_t sample, int kind, int64_t at) {
    return ((unsigned long long)sample << 40) | ((unsigned long long)kind << 36) | (unsigned long long)at;
}

// ---- preparation: cluster rows -> cluster id per object --------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_predict_ids(const uint8_t* clusters, int64_t n, int64_t N, int K, uint16_t* kid,
                                                        unsigned long long* err) {
    const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (q >= n * N) return;
    const int64_t t = q / N, obj = q - t * N;
    const uint8_t* rows = clusters + t * K * N + obj;
    int found = 0;
    uint16_t id = kNoCluster;
    for (int k = 0; k < K; ++k)
        if (rows[(int64_t)k * N]) {
            if (!found) id = (uint16_t)k;
            ++found;
        }
    kid[q] = id;
    if (found > 1) atomicMin(err, error_key(t, kOverlap, obj));
}

// ---- validation: one thread per row (a sample's F weight rows, then its R F table rows) -----------------------------------
__global__ __launch_bounds__(kBlock) void k_predict_validate(const double* weights, const double* tables, int64_t n, int F, int S, int C, int R,
                                                             unsigned long long* err) {
    const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t per_sample = (int64_t)F * (1 + R);
    if (q >= n * per_sample) return;
    const int64_t t = q / per_sample, j = q - t * per_sample;
    const bool is_weight = j < F;
    const int64_t row = is_weight ? j : j - F;               // f, or r F + f
    const int len = is_weight ? C : S;
    const double* v = is_weight ? weights + (t * F + row) * C : tables + (t * (int64_t)R * F + row) * S;
    double sum = 0.0;
    bool positive = false;
    for (int i = 0; i < len; ++i) {
        const double x = v[i];
        if (!(x >= 0.0) || isinf(x)) {                       // negative, NaN or infinite
            atomicMin(err, error_key(t, is_weight ? kWeightEntry : kTableEntry, row * len + i));
            return;
        }
        positive |= x > 0.0;
        sum += x;
    }
    if (!is_weight && !positive) {
        atomicMin(err, error_key(t, kTableRowEmpty, row));
        return;
    }
    if (fabs(sum - 1.0) > SBE_PREDICT_SUM_TOL) atomicMin(err, error_key(t, is_weight ? kWeightSum : kTableSum, row));
}

// ---- a cell of a tile over the samples of a call ----------------------------------------------------------------------------
// G is the argument struct of a unit's kernel over tiles of Ft features x Nt = 256 / Ft objects.  The functions below read
// these fields of it, and the unit adds its own:
//     const uint8_t* codes [N][F], * groups [C-1][N];  const uint16_t* kid [n][N];  const double* weights [n][F][C], * tables [n][R][F][S];
//     int64_t N;  int F, S, C, R;  int n;  int Ft, Nt, f_tiles;  int64_t block0 (of this launch);
//     int row_off[kMaxC] (first table row of a component's groups; row_off[0] = 0: the clusters)

// the tile's slice of sample t into `buf`: [R][Ft][S] of the tables, then [Ft][C] of the weights; the features of the last
// tile behind F are zero
template <class G>
__device__ inline void stage_slice(double* buf, const G& g, int t, int f0, int fw) {
    const int row_len = g.Ft * g.S, have = fw * g.S, total = g.R * row_len;
    const double* tab = g.tables + ((int64_t)t * g.R * g.F + f0) * g.S;
    for (int j = threadIdx.x; j < total; j += kBlock) {
        const int r = j / row_len, q = j - r * row_len;
        buf[j] = q < have ? tab[(int64_t)r * g.F * g.S + q] : 0.0;
    }
    const double* w = g.weights + ((int64_t)t * g.F + f0) * g.C;
    for (int j = threadIdx.x; j < g.Ft * g.C; j += kBlock) buf[total + j] = j < fw * g.C ? w[j] : 0.0;
}

// the thread's cell of the workgroup's tile
struct TileCell {
    int f0, fw;                    // the tile's first feature and its features below F
    int fl;                        // the thread's feature within the tile
    int f;
    int64_t obj;
    bool live;                     // the thread has a cell
    int64_t cell;                  // obj F + f (0 for a thread without one)
    int slice;                     // doubles of one LDS buffer
    int w_at;                      // of the feature's weights within a buffer
};

template <class G>
__device__ inline TileCell tile_cell(const G& g) {
    TileCell c;
    const int64_t b = g.block0 + blockIdx.x;
    const int ft = (int)(b % g.f_tiles);
    const int64_t nt = b / g.f_tiles;
    c.f0 = ft * g.Ft;
    c.fw = min(g.Ft, g.F - c.f0);
    c.fl = threadIdx.x % g.Ft;
    const int nl = threadIdx.x / g.Ft;
    c.obj = nt * g.Nt + nl;
    c.f = c.f0 + c.fl;
    c.live = nl < g.Nt && c.obj < g.N && c.f < g.F;
    c.slice = g.R * g.Ft * g.S + g.Ft * g.C;
    c.w_at = g.R * g.Ft * g.S + c.fl * g.C;
    c.cell = c.live ? c.obj * g.F + c.f : 0;
    return c;
}

// the object's table row for component k (0: not applicable) and whether it has one: fixed for the call for the confounders,
// k >= 1; component 0, the clusters, is read per sample by cell_weights
template <class G>
__device__ inline void cell_group(const G& g, const TileCell& c, int k, int& row, bool& has) {
    has = false;
    row = 0;
    if (c.live && k >= 1 && k < g.C) {
        const int grp = g.groups[(int64_t)(k - 1) * g.N + c.obj];
        has = grp != kNA;
        row = has ? g.row_off[k] + grp : 0;
    }
}

// sample t from the LDS buffer `cur`: the cell's normalised weights w~ (the sum over c in order, then one division; 0 where
// the sum is 0) and where its table rows start
template <int CP, class G>
__device__ inline void cell_weights(const G& g, const TileCell& c, const double* cur, int t, const int (&row)[CP], const bool (&has)[CP],
                                    double (&wn)[CP], const double* (&base)[CP]) {
    const uint16_t id = g.kid[(int64_t)t * g.N + c.obj];
    const bool in = id != kNoCluster;
    double wsum = 0.0;
#pragma unroll
    for (int k = 0; k < CP; ++k) {
        const bool h = k == 0 ? in : has[k];
        const int r = k == 0 ? (in ? id : 0) : row[k];
        wn[k] = k < g.C && h ? cur[c.w_at + k] : 0.0;
        if (k < g.C) wsum += wn[k];
        base[k] = cur + (r * g.Ft + c.fl) * g.S;
    }
#pragma unroll
    for (int k = 0; k < CP; ++k) wn[k] = wsum > 0.0 ? wn[k] / wsum : 0.0;
}

// The counterfactual weights of a cell (include/sbe_contrib.h), whatever the object's own membership in sample t: a_0 = w[f][0],
// a_c = w[f][c] where confounder c applies; w1 = a / (a_0 + a_1 + ..) is cell_weights' w~ of a member of any cluster, w0 = a /
// (a_1 + a_2 + ..), with w0[0] = 0, its w~ of an object in no cluster -- the same operations in the same order, so the rows
// they weigh have cell_state's bits.  base[c], c >= 1: where the confounder's table row starts.  False where no confounder
// applies (a_1 + a_2 + .. is not > 0): w0 is then zero.
template <int CP, class G>
__device__ inline bool cell_weights_in_and_out(const G& g, const TileCell& c, const double* cur, const int (&row)[CP], const bool (&has)[CP],
                                               double (&w1)[CP], double (&w0)[CP], const double* (&base)[CP]) {
    double wsum1 = 0.0, wsum0 = 0.0;
#pragma unroll
    for (int k = 0; k < CP; ++k) {
        w1[k] = k < g.C && (k == 0 || has[k]) ? cur[c.w_at + k] : 0.0;
        w0[k] = k == 0 ? 0.0 : w1[k];
        if (k < g.C) {
            wsum1 += w1[k];
            wsum0 += w0[k];
        }
        base[k] = cur + (row[k] * g.Ft + c.fl) * g.S;
    }
#pragma unroll
    for (int k = 0; k < CP; ++k) {
        w1[k] = wsum1 > 0.0 ? w1[k] / wsum1 : 0.0;
        w0[k] = wsum0 > 0.0 ? w0[k] / wsum0 : 0.0;
    }
    return wsum0 > 0.0;
}

// m_k at state s of an object placed in the cluster whose table row starts at `theta`: cell_state's chain of additions with
// the cluster's term first, over the confounders' products part[c] = w1_c table_c[s], c >= 1, which do not depend on k
template <int CP>
__device__ inline double cell_state_in(int C, double w1_0, const double* theta, int s, const double (&part)[CP]) {
    double m = 0.0;
    m += w1_0 * theta[s];
#pragma unroll
    for (int k = 1; k < CP; ++k)
        if (k < C) m += part[k];
    return m;
}

// m[s] = sum_c w~_c table_c[s], c in order, every product rounded, then added (the build contracts nothing); part: the products
template <int CP>
__device__ inline double cell_state(int C, const double (&wn)[CP], const double* const (&base)[CP], int s, double (&part)[CP]) {
    double m = 0.0;
#pragma unroll
    for (int k = 0; k < CP; ++k) {
        part[k] = k < C ? wn[k] * base[k][s] : 0.0;
        if (k < C) m += part[k];
    }
    return m;
}

template <int CP>
__device__ inline double cell_state(int C, const double (&wn)[CP], const double* const (&base)[CP], int s) {
    double m = 0.0;                                            // (the same sum without the products kept)
#pragma unroll
    for (int k = 0; k < CP; ++k)
        if (k < C) m += wn[k] * base[k][s];
    return m;
}

// ---- host side: the data's arguments, the plan of the tile ---------------------------------------------------------------------
inline bool shape_ok(int64_t N, int64_t F, int S, int C, int K, int R) {
    return N >= 1 && N <= SBE_PREDICT_MAX_OBJECTS && F >= 1 && F <= SBE_PREDICT_MAX_FEATURES && S >= 1 && S <= kMaxS && C >= 1 && C <= kMaxC &&
           K >= 1 && R >= K && R <= kMaxR && N * F * (S + C) * 8 <= SBE_PREDICT_MAX_ACC_BYTES;
}

// host bytes <-> device in pieces of at most kStageBytes, on the handle's stream
template <class H>
int copy_pieces(H* h, void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
    for (size_t at = 0; at < bytes; at += (size_t)kStageBytes)
        HIPCHK(h, hipMemcpyAsync((char*)dst + at, (const char*)src + at, std::min((size_t)kStageBytes, bytes - at), kind, h->stream));
    return SBE_OK;
}

// The checks of <unit>_set_data's arguments, before any device call; on SBE_OK row_off and R are the table's layout.
template <class H>
int check_data(H* h, int64_t N, int64_t F, int S, int C, int K, const uint8_t* codes, const uint8_t* groups, const int* n_groups, int (&row_off)[kMaxC],
               int& R) {
    if (N < 1 || N > SBE_PREDICT_MAX_OBJECTS) return fail(h, SBE_ERR_ARG, "n_objects=%lld out of range [1, %d]", (long long)N, SBE_PREDICT_MAX_OBJECTS);
    if (F < 1 || F > SBE_PREDICT_MAX_FEATURES) return fail(h, SBE_ERR_ARG, "n_features=%lld out of range [1, %d]", (long long)F, SBE_PREDICT_MAX_FEATURES);
    if (S < 1 || S > kMaxS) return fail(h, SBE_ERR_ARG, "n_states=%d out of range [1, %d]", S, kMaxS);
    if (C < 1 || C > kMaxC) return fail(h, SBE_ERR_ARG, "n_components=%d out of range [1, %d]", C, kMaxC);
    if (K < 1 || K > kMaxR) return fail(h, SBE_ERR_ARG, "n_clusters=%d out of range [1, %d]", K, kMaxR);
    if (!codes) return fail(h, SBE_ERR_ARG, "null pointer argument: codes");
    if (C > 1 && (!groups || !n_groups)) return fail(h, SBE_ERR_ARG, "null pointer argument: %s", !groups ? "groups" : "n_groups");
    std::fill(row_off, row_off + kMaxC, 0);
    R = K;
    for (int c = 1; c < C; ++c) {
        if (n_groups[c - 1] < 1 || n_groups[c - 1] > kMaxR)
            return fail(h, SBE_ERR_ARG, "n_groups[%d]=%d out of range [1, %d]", c - 1, n_groups[c - 1], kMaxR);
        row_off[c] = R;
        R += n_groups[c - 1];
    }
    if (R > kMaxR) return fail(h, SBE_ERR_ARG, "%d clusters and the confounders' groups make %d table rows, the limit is %d", K, R, kMaxR);
    if (N * F * (S + C) * 8 > SBE_PREDICT_MAX_ACC_BYTES)
        return fail(h, SBE_ERR_ARG, "the accumulators of %lld objects x %lld features x (%d states + %d components) take %lld bytes on the device, the limit is %lld",
                    (long long)N, (long long)F, S, C, (long long)(N * F * (S + C) * 8), (long long)SBE_PREDICT_MAX_ACC_BYTES);
    for (int64_t q = 0; q < N * F; ++q)
        if (codes[q] >= S && codes[q] != kNA)
            return fail(h, SBE_ERR_DATA, "codes[%lld][%lld]=%d is neither a state below %d nor 255", (long long)(q / F), (long long)(q % F), (int)codes[q], S);
    for (int c = 1; c < C; ++c)
        for (int64_t i = 0; i < N; ++i) {
            const uint8_t g = groups[(int64_t)(c - 1) * N + i];
            if (g >= n_groups[c - 1] && g != kNA)
                return fail(h, SBE_ERR_DATA, "groups[%d][%lld]=%d is neither a group below %d nor 255", c - 1, (long long)i, (int)g, n_groups[c - 1]);
        }
    return SBE_OK;
}

inline size_t slices_bytes(int R, int S, int C, int Ft) { return 2 * (size_t)Ft * ((size_t)R * S + C) * sizeof(double); }

// The features of a workgroup's tile (`forced`, or the default: 16, halved until the two slices are small) and the LDS the
// two slices take; SBE_ERR_ARG if they do not fit.
template <class H>
int plan_tile(H* h, int forced, int64_t F, int R, int S, int C, int& Ft, size_t& lds) {
    Ft = forced;
    if (Ft == 0) {
        Ft = std::min(kDefaultTile, pow2_at_least((int)F));
        while (Ft > 1 && slices_bytes(R, S, C, Ft) > kSmallSlices) Ft /= 2;
    }
    lds = slices_bytes(R, S, C, Ft);
    if (lds > kLdsBudget)
        return fail(h, SBE_ERR_ARG, "a tile of %d features takes two slices of %d rows x %d states: %lld bytes of LDS, the limit is %lld", Ft, R, S,
                    (long long)lds, (long long)kLdsBudget);
    return SBE_OK;
}

// the message of a validation failure of one of the six kinds of include/sbe_predict.h
template <class H>
int data_error(H* h, unsigned long long key, int F, int S, int C) {
    const long long t = (long long)(key >> 40), at = (long long)(key & ((1ull << 36) - 1));
    switch ((int)((key >> 36) & 15)) {
    case kOverlap: return fail(h, SBE_ERR_DATA, "sample %lld: object %lld is in more than one cluster", t, at);
    case kWeightEntry: return fail(h, SBE_ERR_DATA, "sample %lld: weights[%lld][%lld] is negative or not finite", t, at / C, at % C);
    case kWeightSum: return fail(h, SBE_ERR_DATA, "sample %lld: the weights of feature %lld sum further than %g from 1", t, at, SBE_PREDICT_SUM_TOL);
    case kTableEntry:
        return fail(h, SBE_ERR_DATA, "sample %lld: tables[%lld][%lld][%lld] (row, feature, state) is negative or not finite", t, at / S / F,
                    at / S % F, at % S);
    case kTableRowEmpty: return fail(h, SBE_ERR_DATA, "sample %lld: table row %lld, feature %lld has no positive entry", t, at / F, at % F);
    default: return fail(h, SBE_ERR_DATA, "sample %lld: table row %lld, feature %lld sums further than %g from 1", t, at / F, at % F, SBE_PREDICT_SUM_TOL);
    }
}

// The first two kernels of a call over n samples held on the device: ids, validation (the unit adds its own before it reads
// the key).  d_err is set to kNoError first.
template <class H>
int launch_ids_and_validation(H* h, int64_t n, int64_t N, int64_t F, int S, int C, int K, int R, const uint8_t* d_clusters, const double* d_weights,
                              const double* d_tables, uint16_t* d_kid, unsigned long long* d_err) {
    HIPCHK(h, hipMemsetAsync(d_err, 0xFF, sizeof(unsigned long long), h->stream));
    HIPCHK(h, hipEventRecord(h->ev[0], h->stream));
    k_predict_ids<<<(unsigned)div_up(n * N, kBlock), kBlock, 0, h->stream>>>(d_clusters, n, N, K, d_kid, d_err);
    HIPCHK(h, hipGetLastError());
    k_predict_validate<<<(unsigned)div_up(n * F * (1 + R), kBlock), kBlock, 0, h->stream>>>(d_weights, d_tables, n, (int)F, S, C, R, d_err);
    HIPCHK(h, hipGetLastError());
    return SBE_OK;
}

// ---- host side: the sample store -----------------------------------------------------------------------------------------------
constexpr char kNullHandle[] = "null handle";

// the state message of a call that needs data; prefix: "sbe_<unit>"
template <class H>
int no_data(H* h, const char* prefix) { return fail(h, SBE_ERR_STATE, "no data yet (%s_set_data comes first)", prefix); }

inline int no_hook() { return SBE_OK; }

template <class H>
int wait_for_stream(H* h) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return SBE_OK;
}

// what stage() leaves for a call's launches; key: kNoError, or an offender of kind kUniform, which is the unit's to word
struct SamplePlan {
    int Ft = 0;                         // features of a tile
    size_t lds = 0;                     // of the two slices
    unsigned long long key = kNoError;
};

// The data and the samples of the call in flight, as every unit of this header holds them.  A unit's handle derives from it
// beside sbe_unit_handle and lists its pointers through buffers_with(its own).  The methods take the handle for its stream,
// its events and its error message.
struct sample_store {
    bool has_data = false;
    int64_t N = 0;
    int F = 0, S = 0, C = 0, K = 0, R = 0;
    int row_off[kMaxC] = {};
    int forced_tile = 0;                // 0: the default
    uint8_t* d_codes = nullptr;         // [N][F]
    size_t codes_bytes = 0;
    uint8_t* d_groups = nullptr;        // [C-1][N]
    size_t groups_bytes = 0;
    unsigned long long* d_words = nullptr;   // two words; the unit's handle says what each holds (one is stage()'s d_err)
    uint8_t* d_clusters = nullptr;      // the samples of the call in flight: [n][K][N]
    size_t clusters_bytes = 0;
    double* d_weights = nullptr;        // [n][F][C]
    size_t weights_bytes = 0;
    double* d_tables = nullptr;         // [n][R][F][S]
    size_t tables_bytes = 0;
    uint16_t* d_kid = nullptr;          // [n][N]
    size_t kid_bytes = 0;

    std::vector<void*> buffers_with(std::initializer_list<void*> own) const {
        std::vector<void*> all{d_codes, d_groups, d_words, d_clusters, d_weights, d_tables, d_kid};
        all.insert(all.end(), own.begin(), own.end());
        return all;
    }

    // The device part of <prefix>_set_data, after check_data and the unit's own checks: the data and the two words onto the
    // device, own() (the unit's allocations and copies), the shape, last() (the unit's zeroing; it waits for the stream).  A
    // failure leaves a handle without data.
    template <class H, class Own, class Last>
    int upload(H* h, int64_t n_objects, int64_t n_features, int n_states, int n_components, int n_clusters, int n_rows, const int (&offsets)[kMaxC],
               const uint8_t* codes, const uint8_t* groups, Own own, Last last) {
        has_data = false;
        HIPCHK(h, hipSetDevice(h->device));
        const size_t code_bytes = (size_t)(n_objects * n_features), group_bytes = (size_t)(n_components - 1) * (size_t)n_objects;
        int rc = unit_ensure(h, d_codes, codes_bytes, code_bytes);
        if (!rc) rc = unit_ensure(h, d_groups, groups_bytes, std::max<size_t>(1, group_bytes));
        if (!rc) rc = unit_ensure(h, d_words, 2 * sizeof(unsigned long long));
        if (!rc) rc = copy_pieces(h, d_codes, codes, code_bytes, hipMemcpyHostToDevice);
        if (!rc && n_components > 1) rc = copy_pieces(h, d_groups, groups, group_bytes, hipMemcpyHostToDevice);
        if (!rc) rc = own();
        if (rc) return rc;
        N = n_objects;
        F = (int)n_features;
        S = n_states;
        C = n_components;
        K = n_clusters;
        R = n_rows;
        std::copy(offsets, offsets + kMaxC, row_off);
        if ((rc = last())) return rc;
        has_data = true;
        return SBE_OK;
    }

    // The opening of a compute call over n > 0 samples: the argument checks, the tile, the samples onto the device, extra() (the
    // unit's allocations and copies), ids and validation (before them the handle's first event), validate() (the unit's own
    // validation, reported through d_err as well), the offender's key read.  per_sample, max_stage: the unit's bytes per sample
    // and its limit.  On SBE_OK the samples stand on the device and `plan` is set.
    template <class H, class Extra, class Validate>
    int stage(H* h, int64_t n, const uint8_t* clusters, const double* weights, const double* tables, int64_t per_sample, int64_t max_stage,
              unsigned long long* d_err, Extra extra, Validate validate, SamplePlan& plan) {
        if (!clusters || !weights || !tables)
            return fail(h, SBE_ERR_ARG, "null pointer argument: %s", !clusters ? "clusters" : !weights ? "weights" : "tables");
        if (n > max_stage / per_sample)
            return fail(h, SBE_ERR_ARG, "n=%lld samples of %lld bytes each exceed the %lld bytes one call holds on the device (at most %lld samples per call here)",
                        (long long)n, (long long)per_sample, (long long)max_stage, (long long)(max_stage / per_sample));
        if (const int bad = plan_tile(h, forced_tile, F, R, S, C, plan.Ft, plan.lds)) return bad;
        HIPCHK(h, hipSetDevice(h->device));
        const size_t cl_bytes = (size_t)n * K * N, w_bytes = (size_t)n * F * C * sizeof(double), t_bytes = (size_t)n * R * F * S * sizeof(double);
        int rc = unit_ensure(h, d_clusters, clusters_bytes, cl_bytes);
        if (!rc) rc = unit_ensure(h, d_weights, weights_bytes, w_bytes);
        if (!rc) rc = unit_ensure(h, d_tables, tables_bytes, t_bytes);
        if (!rc) rc = unit_ensure(h, d_kid, kid_bytes, (size_t)n * N * sizeof(uint16_t));
        if (!rc) rc = copy_pieces(h, d_clusters, clusters, cl_bytes, hipMemcpyHostToDevice);
        if (!rc) rc = copy_pieces(h, d_weights, weights, w_bytes, hipMemcpyHostToDevice);
        if (!rc) rc = copy_pieces(h, d_tables, tables, t_bytes, hipMemcpyHostToDevice);
        if (!rc) rc = extra();
        if (!rc) rc = launch_ids_and_validation(h, n, N, F, S, C, K, R, d_clusters, d_weights, d_tables, d_kid, d_err);
        if (!rc) rc = validate();
        if (rc) return rc;
        HIPCHK(h, hipMemcpyAsync(&plan.key, d_err, sizeof plan.key, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if (plan.key != kNoError && (int)((plan.key >> 36) & 15) != kUniform) return data_error(h, plan.key, F, S, C);
        return SBE_OK;
    }

    // the fields of a kernel's argument struct that the device part of this header reads (kid: where the struct has it)
    template <class G>
    void fill(G& g, int64_t n, const SamplePlan& plan) const {
        g.codes = d_codes;
        g.groups = d_groups;
        set_kid(g, 0);
        g.weights = d_weights;
        g.tables = d_tables;
        g.N = N;
        g.F = F;
        g.S = S;
        g.C = C;
        g.R = R;
        g.n = (int)n;
        g.Ft = plan.Ft;
        g.Nt = kBlock / plan.Ft;
        g.f_tiles = div_up(F, plan.Ft);
        std::copy(row_off, row_off + kMaxC, g.row_off);
    }
    template <class G>
    auto set_kid(G& g, int) const -> decltype((void)g.kid) { g.kid = d_kid; }
    template <class G>
    void set_kid(G&, long) const {}
};

// the whole of <prefix>_set_feature_tile
template <class H>
int set_feature_tile(H* h, int features) {
    CHECK_HANDLE(h, kNullHandle);
    if (features < 0 || features > kMaxTile) return fail(h, SBE_ERR_ARG, "features=%d out of range [0, %d]", features, kMaxTile);
    h->forced_tile = features;
    return SBE_OK;
}

// a kernel over the tiles of the data, in grid chunks; args: filled, its block0 is set per launch
template <class H, class G>
int launch_tiles(H* h, void (*kernel)(const G), G& args, size_t lds) {
    HIPCHK(h, hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBudget));
    const int64_t blocks = (int64_t)args.f_tiles * ((args.N + args.Nt - 1) / args.Nt);
    return unit_for_grid_chunks(blocks, [&](int64_t first, int64_t count) {
        args.block0 = first;
        kernel<<<(unsigned)count, kBlock, lds, h->stream>>>(args);
        HIPCHK(h, hipGetLastError());
        return SBE_OK;
    });
}

}  // namespace
