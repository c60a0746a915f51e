// sbe_spatial.hip -- the spatial posterior predictive check (include/sbe_spatial.h): join counts per class of pairs on the data
// and on a stream of replicated data sets, and where the observed counts fall among the replicated ones.  The contract is
// tests/_spatial_oracle.py; DESIGN.md section 29 has the layout.  Integers only: there is no floating-point number here.
//
// A pair is never compared cell by cell.  set_data packs the classes once into bit rows, rows [B][W][n_pad] of 64-bit words:
// bit j % 64 of rows[b][j / 64][i] says that the pair (i, j), j != i, is in class b (object-minor, so that a wave's loads are
// contiguous).  Per data set, k_spatial_fill checks the codes, turns them feature-major and builds by wave ballots the state
// masks of every feature over the objects, masks [F][S + 1][W]: mask s holds the objects in state s, mask S the observed ones.
// k_spatial_count then gives each lane an object i, a class b and 16 words (or fewer) of that object's bit row in registers,
// and walks a tile of features whose masks lie in LDS: the joins of i in the feature are popcount(mask[y_if] & row), the
// comparable pairs popcount(mask[S] & row).  Summed over the tile they go to local_agree[b][i], summed over the wave to
// agree[b][f], both by integer atomics; every pair is counted from both ends, so the feature counts are even and are halved
// afterwards.  k_spatial_totals adds the features up and k_spatial_tally, a thread per entry, walks the replicates of the call.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "sbe_unit.hip.h"
#include "../../include/sbe_spatial.h"

namespace {

constexpr unsigned long long kNoOffender = ~0ull;
constexpr int kCountBlock = 128;                     // threads (objects) of a count block
constexpr int kChunk = 16;                           // words of a bit row a lane holds at most
constexpr int kDefaultTile = 16;                     // features per tile
constexpr size_t kTileLdsBytes = (size_t)64 << 10;   // what a tile's masks may take
constexpr int kMaxGridZ = 65535;
constexpr int kFillFeatures = 32;                    // features a fill wave walks (a divisor of 64)

// ---- the fill: y [n][N][F] (staging) -> img [n][F][n_pad] (NA behind N) and masks [n][F][S1][W], and the first code that is
// neither below its feature's state count nor NA, by its index in y (an integer atomic minimum).  A wave per 64 objects:
// blockIdx.x: the word, y: kFillFeatures features, z + r0: the replicate.  The codes come through LDS: an object's features
// are contiguous in y, so half a wave reads one object's part of the tile and every cache line is fetched once
__global__ __launch_bounds__(64) void k_spatial_fill(const uint8_t* y, int N, int F, int n_pad, int W, int S1, const int32_t* n_states, int64_t r0,
                                                     uint8_t* img, unsigned long long* masks, unsigned long long* offender) {
    __shared__ uint8_t tile[64][kFillFeatures + 1];
    const int64_t r = r0 + blockIdx.z;
    const int w = blockIdx.x, lane = threadIdx.x, i0 = w * 64, i = i0 + lane;
    const int f0 = blockIdx.y * kFillFeatures, nf = min(kFillFeatures, F - f0);
    const int col = lane % kFillFeatures;
    for (int k = lane / kFillFeatures; k < 64; k += 64 / kFillFeatures) {
        uint8_t c = SBE_SPATIAL_NA;
        if (i0 + k < N && col < nf) {
            const int64_t at = (r * N + i0 + k) * F + f0 + col;
            c = y[at];
            if (c != SBE_SPATIAL_NA && (int32_t)c >= n_states[f0 + col]) {
                atomicMin(offender, (unsigned long long)at);
                c = SBE_SPATIAL_NA;
            }
        }
        tile[k][col] = c;
    }
    __syncthreads();
    for (int t = 0; t < nf; ++t) {
        const int f = f0 + t;
        const uint8_t c = tile[lane][t];
        img[(r * F + f) * n_pad + i] = c;
        unsigned long long mine = 0;
        for (int s = 0; s < S1 - 1; ++s) {
            const unsigned long long m = __ballot(c == s);
            if (lane == s) mine = m;
        }
        const unsigned long long observed = __ballot(c != SBE_SPATIAL_NA);
        if (lane == S1 - 1) mine = observed;
        if (lane < S1) masks[((r * F + f) * S1 + lane) * W + w] = mine;
    }
}

// ---- the counts of n_rep data sets --------------------------------------------------------------------------------------
struct CountArgs {
    const uint8_t* img;                  // [n_rep][F][n_pad]
    const unsigned long long* masks;     // [n_rep][F][S1][W]
    const unsigned long long* rows;      // [B][W][n_pad]
    int32_t* cnt;                        // [n_rep][E], E = B (F + N): twice agree [B][F], then local_agree [B][N] (zeroed before)
    int32_t* cmp;                        // the same of the comparable pairs (kCmp only)
    int N, F, n_pad, W, S1, B, tile, ftiles, chunks;
};

// blockIdx.x: replicate * ftiles + feature tile, y: kCountBlock objects, z: class * chunks + word chunk.  kWords: the words of a
// chunk, a power of two up to kChunk (W = chunks * kWords).  LDS: the tile's masks of this chunk, [tile][S1][kWords | 1] (the
// odd stride keeps the lanes' rows, picked by their codes, on different banks)
template <int kWords, bool kCmp>
__global__ __launch_bounds__(kCountBlock) void k_spatial_count(const CountArgs g) {
    extern __shared__ unsigned long long spatial_lds[];
    constexpr int kStride = kWords | 1;
    const int64_t r = blockIdx.x / g.ftiles;
    const int f0 = (int)(blockIdx.x % g.ftiles) * g.tile, nt = min(g.tile, g.F - f0);
    const int b = blockIdx.z / g.chunks, w0 = (int)(blockIdx.z % g.chunks) * kWords;
    const int i = blockIdx.y * kCountBlock + threadIdx.x;
    const int64_t E = (int64_t)g.B * (g.F + g.N);

    const unsigned long long* src = g.masks + (r * g.F + f0) * g.S1 * g.W;
    for (int idx = threadIdx.x; idx < nt * g.S1 * kWords; idx += kCountBlock) {
        const int line = idx / kWords, w = idx - line * kWords;                 // line: feature of the tile * S1 + state
        spatial_lds[line * kStride + w] = src[(int64_t)line * g.W + w0 + w];
    }
    unsigned long long row[kWords];
#pragma unroll
    for (int w = 0; w < kWords; ++w) row[w] = i < g.n_pad ? g.rows[((int64_t)b * g.W + w0 + w) * g.n_pad + i] : 0ull;
    __syncthreads();

    int local = 0, local_cmp = 0;
    int32_t* cnt = g.cnt + r * E;
    int32_t* cmp = kCmp ? g.cmp + r * E : nullptr;
    for (int t = 0; t < nt; ++t) {
        const uint8_t c = i < g.n_pad ? g.img[(r * g.F + f0 + t) * g.n_pad + i] : (uint8_t)SBE_SPATIAL_NA;
        const bool on = c != SBE_SPATIAL_NA;
        const unsigned long long* mine = spatial_lds + (t * g.S1 + (on ? min((int)c, g.S1 - 2) : 0)) * kStride;
        const unsigned long long* observed = spatial_lds + (t * g.S1 + g.S1 - 1) * kStride;
        int a = 0, q = 0;
#pragma unroll
        for (int w = 0; w < kWords; ++w) {
            a += __popcll(mine[w] & row[w]);
            if (kCmp) q += __popcll(observed[w] & row[w]);
        }
        a = on ? a : 0;
        local += a;
        a = unit_wave_reduce(a, unit_sum());
        if ((threadIdx.x & 63) == 0 && a) atomicAdd(cnt + b * g.F + f0 + t, a);
        if (kCmp) {
            q = on ? q : 0;
            local_cmp += q;
            q = unit_wave_reduce(q, unit_sum());
            if ((threadIdx.x & 63) == 0 && q) atomicAdd(cmp + b * g.F + f0 + t, q);
        }
    }
    if (i < g.N) {
        const int64_t at = (int64_t)g.B * g.F + (int64_t)b * g.N + i;
        if (local) atomicAdd(cnt + at, local);
        if (kCmp && local_cmp) atomicAdd(cmp + at, local_cmp);
    }
}

// total[r][b] = half the sum over f of the doubled agree[r][b][f]; first + blockIdx.x: r * B + b
__global__ __launch_bounds__(256) void k_spatial_totals(const int32_t* cnt, int F, int N, int B, int64_t first, long long* total) {
    __shared__ long long red[4];
    const int64_t at = first + blockIdx.x, r = at / B, E = (int64_t)B * (F + N);
    const int b = (int)(at % B);
    long long s = 0;
    for (int f = threadIdx.x; f < F; f += 256) s += cnt[r * E + (int64_t)b * F + f];
    s = unit_block_reduce<4>(s, red, unit_sum());
    if (threadIdx.x == 0) total[at] = s / 2;
}

// The replicates of a call into the accumulators, one after the other: thread e < E an entry of agree (halved here, in place,
// with its comparable) or local_agree, threads E .. E + B the totals.  counts: [3][E + B] n_greater, n_equal, n_less
__global__ __launch_bounds__(256) void k_spatial_tally(int32_t* cnt, int32_t* cmp, const long long* total, int64_t n_rep, int F, int N, int B,
                                                       const int32_t* obs, const long long* total_obs, int32_t* counts, long long* sum, long long* sumsq) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x, BF = (int64_t)B * F, E = BF + (int64_t)B * N;
    if (e >= E + B) return;
    const bool is_total = e >= E;
    const long long observed = is_total ? total_obs[e - E] : (long long)obs[e];
    int n_greater = counts[e], n_equal = counts[E + B + e], n_less = counts[2 * (E + B) + e];
    long long s1 = is_total ? 0 : sum[e], s2 = is_total ? 0 : sumsq[e];
    for (int64_t r = 0; r < n_rep; ++r) {
        long long v;
        if (is_total) {
            v = total[r * B + (e - E)];
        } else {
            v = cnt[r * E + e];
            if (e < BF) {
                v >>= 1;
                cnt[r * E + e] = (int32_t)v;
                if (cmp) cmp[r * E + e] >>= 1;
            }
            s1 += v;
            s2 += v * v;
        }
        if (v > observed)
            n_greater += 1;
        else if (v == observed)
            n_equal += 1;
        else
            n_less += 1;
    }
    counts[e] = n_greater;
    counts[E + B + e] = n_equal;
    counts[2 * (E + B) + e] = n_less;
    if (!is_total) {
        sum[e] = s1;
        sumsq[e] = s2;
    }
}

}  // namespace

struct sbe_spatial : sbe_unit_handle {               // (sbe_unit.hip.h; ev: around the count kernels' launches)
    unsigned long long* d_rows = nullptr;        // the classes' bit rows [B][W][n_pad]
    size_t rows_bytes = 0;
    int32_t* d_states = nullptr;                 // n_states [F]
    size_t states_bytes = 0;
    void* d_obs = nullptr;                       // total_obs int64 [B], then agree_obs [B][F] and local_obs [B][N] int32
    size_t obs_bytes = 0;
    void* d_acc = nullptr;                       // sum, sumsq int64 [E], then the counts int32 [3][E + B]
    size_t acc_bytes = 0;
    uint8_t* d_stage = nullptr;                  // the data sets of one call as uploaded, [n][N][F]
    size_t stage_bytes = 0;
    uint8_t* d_img = nullptr;                    // ... feature-major [n][F][n_pad]
    size_t img_bytes = 0;
    unsigned long long* d_masks = nullptr;       // ... their state masks [n][F][S1][W]
    size_t masks_bytes = 0;
    int32_t* d_cnt = nullptr;                    // ... their counts [n][E]
    size_t cnt_bytes = 0;
    int32_t* d_cmp = nullptr;                    // ... their comparable pairs [n][E]
    size_t cmp_bytes = 0;
    long long* d_total = nullptr;                // ... their totals [n][B]
    size_t total_bytes = 0;
    unsigned long long* d_offender = nullptr;
    int64_t N = 0, F = 0;                        // shape of the data (F == 0: none yet)
    int B = 0, S1 = 0, W = 0, n_pad = 0;
    int tile = 0;                                // features per tile asked for (0: the default)
    int64_t n_replicates = 0;
    std::vector<int32_t> obs, obs_cmp;           // [E] each: agree | local_agree of the data, and their comparable pairs
    std::vector<int64_t> total_obs;              // [B]
    std::vector<void*> buffers() const {
        return {d_rows, d_states, d_obs, d_acc, d_stage, d_img, d_masks, d_cnt, d_cmp, d_total, d_offender};
    }

    int64_t E() const { return (int64_t)B * (F + N); }
    long long* total_obs_d() const { return (long long*)d_obs; }
    int32_t* obs_d() const { return (int32_t*)(total_obs_d() + B); }
    long long* sum() const { return (long long*)d_acc; }
    long long* sumsq() const { return sum() + E(); }
    int32_t* counts() const { return (int32_t*)(sumsq() + E()); }
    size_t acc_size() const { return (size_t)E() * 16 + (size_t)(E() + B) * 12; }
};

namespace {

constexpr char kNullHandle[] = "null handle";

bool shape_in_limits(int64_t N, int64_t F) { return N >= 1 && N <= SBE_SPATIAL_MAX_OBJECTS && F >= 1 && F <= SBE_SPATIAL_MAX_FEATURES; }

// the 64-bit words of N objects, padded: a power of two up to kChunk, a multiple of kChunk beyond
int padded_words(int64_t N) {
    const int w = (int)((N + 63) / 64);
    return w <= kChunk ? pow2_at_least(w) : (w + kChunk - 1) / kChunk * kChunk;
}

int64_t replicate_bytes(int64_t N, int64_t F, int S, int B) {
    const int64_t W = padded_words(N);
    return N * F + 64 * W * F + 8 * W * F * (S + 1) + 2 * 4 * B * (F + N) + 8 * B;
}

int64_t max_replicates(int64_t N, int64_t F) {
    const int64_t most = std::max(N * (N - 1) / 2, (N - 1) * F);
    return most == 0 ? INT32_MAX : std::min<int64_t>(INT32_MAX, INT64_MAX / (most * most));
}

// features per tile: what was asked for (or the default), shortened until the tile's masks fit kTileLdsBytes
int tile_features(const sbe_spatial* h, int S1, int words) {
    const size_t each = (size_t)S1 * (words | 1) * sizeof(unsigned long long);
    return (int)std::max<size_t>(1, std::min<size_t>(h->tile > 0 ? h->tile : kDefaultTile, kTileLdsBytes / each));
}

template <bool kCmp>
void launch_count(const CountArgs& a, int words, dim3 grid, size_t lds, hipStream_t stream) {
    switch (words) {
        case 1: k_spatial_count<1, kCmp><<<grid, kCountBlock, lds, stream>>>(a); break;
        case 2: k_spatial_count<2, kCmp><<<grid, kCountBlock, lds, stream>>>(a); break;
        case 4: k_spatial_count<4, kCmp><<<grid, kCountBlock, lds, stream>>>(a); break;
        case 8: k_spatial_count<8, kCmp><<<grid, kCountBlock, lds, stream>>>(a); break;
        default: k_spatial_count<16, kCmp><<<grid, kCountBlock, lds, stream>>>(a); break;
    }
}

// The n data sets in d_stage [n][N][F]: checked and filled (`offender_out`: the first bad code's index, or kNoOffender; nothing
// further runs then), counted into d_cnt (and d_cmp, with_cmp) between the handle's events, and their totals into d_total.
// The feature counts are still doubled afterwards.  The handle's shape members are set; its device is current.
int count_staged(sbe_spatial* h, int64_t n, bool with_cmp, unsigned long long& offender_out) {
    const int N = (int)h->N, F = (int)h->F, B = h->B, S1 = h->S1, W = h->W, n_pad = h->n_pad;
    const int64_t E = h->E();
    int rc = unit_ensure(h, h->d_img, h->img_bytes, (size_t)n * F * n_pad);
    if (!rc) rc = unit_ensure(h, h->d_masks, h->masks_bytes, (size_t)n * F * S1 * W * sizeof(unsigned long long));
    if (!rc) rc = unit_ensure(h, h->d_cnt, h->cnt_bytes, (size_t)(n * E) * sizeof(int32_t));
    if (!rc && with_cmp) rc = unit_ensure(h, h->d_cmp, h->cmp_bytes, (size_t)(n * E) * sizeof(int32_t));
    if (!rc) rc = unit_ensure(h, h->d_total, h->total_bytes, (size_t)(n * B) * sizeof(long long));
    if (rc) return rc;
    unsigned long long offender = kNoOffender;
    HIPCHK(h, hipMemcpyAsync(h->d_offender, &offender, sizeof offender, hipMemcpyHostToDevice, h->stream));
    for (int64_t r0 = 0; r0 < n; r0 += kMaxGridZ) {
        const dim3 grid((unsigned)W, (unsigned)div_up(F, kFillFeatures), (unsigned)std::min<int64_t>(kMaxGridZ, n - r0));
        k_spatial_fill<<<grid, 64, 0, h->stream>>>(h->d_stage, N, F, n_pad, W, S1, h->d_states, r0, h->d_img, h->d_masks, h->d_offender);
        HIPCHK(h, hipGetLastError());
    }
    HIPCHK(h, hipMemcpyAsync(&offender, h->d_offender, sizeof offender, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    offender_out = offender;
    if (offender != kNoOffender) return SBE_OK;

    HIPCHK(h, hipMemsetAsync(h->d_cnt, 0, (size_t)(n * E) * sizeof(int32_t), h->stream));
    if (with_cmp) HIPCHK(h, hipMemsetAsync(h->d_cmp, 0, (size_t)(n * E) * sizeof(int32_t), h->stream));
    const int words = std::min(W, kChunk), chunks = W / words;
    const int tile = tile_features(h, S1, words), ftiles = div_up(F, tile);
    const size_t lds = (size_t)tile * S1 * (words | 1) * sizeof(unsigned long long);
    const dim3 per_rep((unsigned)ftiles, (unsigned)div_up(n_pad, kCountBlock), (unsigned)(B * chunks));
    // (a launch stays under kMaxGridBlocks workgroups: as many whole replicates as fit, at least one -- one replicate takes
    // 4096 * 32 * 32 workgroups at the most)
    const int64_t reps = std::max<int64_t>(1, kMaxGridBlocks / ((int64_t)per_rep.x * per_rep.y * per_rep.z));
    rc = unit_timed(h, [&] {
        for (int64_t r0 = 0; r0 < n; r0 += reps) {
            const int64_t n_rep = std::min(reps, n - r0);
            const CountArgs args{h->d_img + r0 * F * n_pad, h->d_masks + r0 * F * S1 * W, h->d_rows, h->d_cnt + r0 * E, with_cmp ? h->d_cmp + r0 * E : nullptr,
                                 N, F, n_pad, W, S1, B, tile, ftiles, chunks};
            const dim3 grid((unsigned)(n_rep * ftiles), per_rep.y, per_rep.z);
            if (with_cmp)
                launch_count<true>(args, words, grid, lds, h->stream);
            else
                launch_count<false>(args, words, grid, lds, h->stream);
            HIPCHK(h, hipGetLastError());
        }
        return SBE_OK;
    });
    if (rc) return rc;
    return unit_for_grid_chunks(n * B, [&](int64_t first, int64_t count) {
        k_spatial_totals<<<(unsigned)count, 256, 0, h->stream>>>(h->d_cnt, F, N, B, first, h->d_total);
        HIPCHK(h, hipGetLastError());
        return SBE_OK;
    });
}

// rows [n] of `width` int32 out of the call's count arrays (pitch E) into a dense host array
int copy_rows(sbe_spatial* h, int32_t* out, const int32_t* d, int64_t width, int64_t n) {
    if (!out || width == 0) return SBE_OK;
    HIPCHK(h, hipMemcpy2DAsync(out, (size_t)width * 4, d, (size_t)h->E() * 4, (size_t)width * 4, (size_t)n, hipMemcpyDeviceToHost, h->stream));
    return SBE_OK;
}

}  // namespace

extern "C" {

int sbe_spatial_abi_version(void) { return SBE_SPATIAL_ABI_VERSION; }

const char* sbe_spatial_last_error(const sbe_spatial* h) { return unit_last_error(h); }

int sbe_spatial_create(sbe_spatial** out, int device) { return unit_create_on_device(out, device, "sbe_spatial_create"); }

int sbe_spatial_destroy(sbe_spatial* h) { return unit_destroy(h, kNullHandle); }

int sbe_spatial_set_tile(sbe_spatial* h, int tile_features) {
    CHECK_HANDLE(h, kNullHandle);
    if (tile_features < 0 || tile_features > SBE_SPATIAL_MAX_TILE)
        return fail(h, SBE_ERR_ARG, "tile_features=%d out of range [0, %d]", tile_features, SBE_SPATIAL_MAX_TILE);
    h->tile = tile_features;
    return SBE_OK;
}

int64_t sbe_spatial_max_replicates(int64_t n_objects, int64_t n_features) {
    return shape_in_limits(n_objects, n_features) ? max_replicates(n_objects, n_features) : 0;
}

int64_t sbe_spatial_replicate_bytes(int64_t n_objects, int64_t n_features, int max_states, int n_bands) {
    if (!shape_in_limits(n_objects, n_features) || max_states < 1 || max_states > SBE_SPATIAL_MAX_STATES || n_bands < 1 || n_bands > SBE_SPATIAL_MAX_BANDS)
        return 0;
    return replicate_bytes(n_objects, n_features, max_states, n_bands);
}

int sbe_spatial_set_data(sbe_spatial* h, const uint8_t* x, int64_t n_objects, int64_t n_features, const int32_t* n_states, const uint8_t* band,
                         int n_bands) {
    CHECK_HANDLE(h, kNullHandle);
    if (!x || !n_states || !band) return fail(h, SBE_ERR_ARG, "null pointer argument: %s", !x ? "x" : !n_states ? "n_states" : "band");
    h->F = 0;                                       // (a refused call leaves the handle without data)
    const int64_t N = n_objects, F = n_features;
    if (N < 1 || N > SBE_SPATIAL_MAX_OBJECTS)
        return fail(h, SBE_ERR_ARG, "n_objects=%lld out of range [1, %d] (the classes are an [N][N] matrix)", (long long)N, SBE_SPATIAL_MAX_OBJECTS);
    if (F < 1 || F > SBE_SPATIAL_MAX_FEATURES) return fail(h, SBE_ERR_ARG, "n_features=%lld out of range [1, %d]", (long long)F, SBE_SPATIAL_MAX_FEATURES);
    int s_max = 1;
    for (int64_t f = 0; f < F; ++f) {
        if (n_states[f] < 1 || n_states[f] > SBE_SPATIAL_MAX_STATES)
            return fail(h, SBE_ERR_ARG, "n_states[%lld]=%d out of range [1, %d] (the state limit of the replicates' source, sbe_ppc.h)", (long long)f,
                         n_states[f], SBE_SPATIAL_MAX_STATES);
        s_max = std::max(s_max, (int)n_states[f]);
    }
    if (n_bands < 1 || n_bands > SBE_SPATIAL_MAX_BANDS) return fail(h, SBE_ERR_ARG, "n_bands=%d out of range [1, %d]", n_bands, SBE_SPATIAL_MAX_BANDS);
    for (int64_t i = 0; i < N; ++i)
        for (int64_t f = 0; f < F; ++f) {
            const uint8_t c = x[i * F + f];
            if (c != SBE_SPATIAL_NA && c >= n_states[f])
                return fail(h, SBE_ERR_DATA, "x[%lld][%lld]=%d is neither below n_states[%lld]=%d nor %d (not observed)", (long long)i, (long long)f, (int)c,
                             (long long)f, n_states[f], SBE_SPATIAL_NA);
        }
    for (int64_t i = 0; i < N; ++i)
        for (int64_t j = 0; j < N; ++j) {
            const uint8_t b = band[i * N + j];
            if (i != j && b != SBE_SPATIAL_NA && b >= n_bands)
                return fail(h, SBE_ERR_DATA, "band[%lld][%lld]=%d is neither below n_bands=%d nor %d (pair not counted)", (long long)i, (long long)j, (int)b,
                             n_bands, SBE_SPATIAL_NA);
        }
    const int B = n_bands, W = padded_words(N), n_pad = 64 * W;
    std::vector<unsigned long long> rows((size_t)B * W * n_pad, 0ull);
    for (int64_t i = 0; i < N; ++i)
        for (int64_t j = 0; j < N; ++j) {
            const uint8_t b = band[i * N + j];
            if (i == j) continue;
            if (b != band[j * N + i])
                return fail(h, SBE_ERR_DATA, "band[%lld][%lld]=%d differs from band[%lld][%lld]=%d: the classes must be symmetric", (long long)i, (long long)j,
                             (int)b, (long long)j, (long long)i, (int)band[j * N + i]);
            if (b != SBE_SPATIAL_NA) rows[((size_t)b * W + (size_t)(j >> 6)) * n_pad + i] |= 1ull << (j & 63);
        }

    HIPCHK(h, hipSetDevice(h->device));
    h->N = N;                                       // (the shape the helpers below read; F stays 0 until the data is in place)
    h->B = B;
    h->S1 = s_max + 1;
    h->W = W;
    h->n_pad = n_pad;
    const int64_t E = (int64_t)B * (F + N);
    int rc = unit_ensure(h, h->d_rows, h->rows_bytes, rows.size() * sizeof(unsigned long long));
    if (!rc) rc = unit_ensure(h, h->d_states, h->states_bytes, (size_t)F * sizeof(int32_t));
    if (!rc) rc = unit_ensure(h, h->d_obs, h->obs_bytes, (size_t)B * 8 + (size_t)E * 4);
    if (!rc) rc = unit_ensure(h, h->d_acc, h->acc_bytes, (size_t)E * 16 + (size_t)(E + B) * 12);
    if (!rc) rc = unit_ensure(h, h->d_stage, h->stage_bytes, (size_t)(N * F));
    if (!rc) rc = unit_ensure(h, h->d_offender, sizeof(unsigned long long));
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(h->d_rows, rows.data(), rows.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_states, n_states, (size_t)F * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_stage, x, (size_t)(N * F), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(h->d_acc, 0, (size_t)E * 16 + (size_t)(E + B) * 12, h->stream));
    h->F = F;                                       // (count_staged reads the whole shape; taken back on failure)
    unsigned long long offender = kNoOffender;
    rc = count_staged(h, 1, true, offender);
    h->F = 0;
    if (rc) return rc;
    if (offender != kNoOffender) return fail(h, SBE_ERR_DATA, "the device refused code %llu of x that the host check had passed", offender);
    h->obs.assign((size_t)E, 0);
    h->obs_cmp.assign((size_t)E, 0);
    h->total_obs.assign((size_t)B, 0);
    HIPCHK(h, hipMemcpyAsync(h->obs.data(), h->d_cnt, (size_t)E * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->obs_cmp.data(), h->d_cmp, (size_t)E * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->total_obs.data(), h->d_total, (size_t)B * 8, hipMemcpyDeviceToHost, h->stream));
    if ((rc = unit_sync_timed(h))) return rc;
    for (int64_t e = 0; e < (int64_t)B * F; ++e) {  // (every pair was counted from both ends)
        h->obs[(size_t)e] /= 2;
        h->obs_cmp[(size_t)e] /= 2;
    }
    HIPCHK(h, hipMemcpyAsync(h->total_obs_d(), h->total_obs.data(), (size_t)B * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync((int32_t*)((long long*)h->d_obs + B), h->obs.data(), (size_t)E * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->F = F;
    h->n_replicates = 0;
    return SBE_OK;
}

int sbe_spatial_add(sbe_spatial* h, int64_t n, const uint8_t* y_rep, int32_t* agree_rep, int32_t* comparable_rep, int32_t* local_rep,
                    int32_t* local_comparable_rep, int64_t* total_rep) {
    CHECK_HANDLE(h, kNullHandle);
    if (h->F == 0) return fail(h, SBE_ERR_STATE, "sbe_spatial_add needs the data of a successful sbe_spatial_set_data");
    if (n < 0) return fail(h, SBE_ERR_ARG, "n=%lld is negative", (long long)n);
    if (n == 0) return SBE_OK;
    if (!y_rep) return fail(h, SBE_ERR_ARG, "null pointer argument: y_rep");
    const int64_t N = h->N, F = h->F, E = h->E(), most = max_replicates(N, F), each = replicate_bytes(N, F, h->S1 - 1, h->B);
    const int B = h->B;
    if (n > most - h->n_replicates)
        return fail(h, SBE_ERR_ARG, "%lld replicates after %lld exceed the %lld that the int64 sums of squares of %lld objects x %lld features hold "
                     "(sbe_spatial_max_replicates)", (long long)n, (long long)h->n_replicates, (long long)most, (long long)N, (long long)F);
    if (n > SBE_SPATIAL_MAX_STAGE_BYTES / each)
        return fail(h, SBE_ERR_ARG, "%lld replicates of %lld bytes each exceed the %lld bytes one call holds on the device (split the block)",
                     (long long)n, (long long)each, (long long)SBE_SPATIAL_MAX_STAGE_BYTES);
    const bool with_cmp = comparable_rep || local_comparable_rep;

    HIPCHK(h, hipSetDevice(h->device));
    int rc = unit_ensure(h, h->d_stage, h->stage_bytes, (size_t)(n * N * F));
    if (rc) return rc;
    // the upload, checked on the device; nothing of the accumulators is touched before the codes have passed
    HIPCHK(h, hipMemcpyAsync(h->d_stage, y_rep, (size_t)(n * N * F), hipMemcpyHostToDevice, h->stream));
    unsigned long long offender = kNoOffender;
    if ((rc = count_staged(h, n, with_cmp, offender))) return rc;
    if (offender != kNoOffender) {
        const int64_t at = (int64_t)offender, f = at % F, i = at / F % N, r = at / (N * F);
        return fail(h, SBE_ERR_DATA, "y_rep[%lld][%lld][%lld]=%d is neither below n_states[%lld] nor %d (not observed)", (long long)r, (long long)i,
                     (long long)f, (int)y_rep[at], (long long)f, SBE_SPATIAL_NA);
    }
    k_spatial_tally<<<(unsigned)div_up(E + B, 256), 256, 0, h->stream>>>(h->d_cnt, with_cmp ? h->d_cmp : nullptr, h->d_total, n, (int)F, (int)N, B, h->obs_d(),
                                                                        h->total_obs_d(), h->counts(), h->sum(), h->sumsq());
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipEventRecord(h->ev[1], h->stream));                    // (the timed region ends behind the tally)
    const int64_t BF = (int64_t)B * F, BN = (int64_t)B * N;
    rc = copy_rows(h, agree_rep, h->d_cnt, BF, n);
    if (!rc) rc = copy_rows(h, local_rep, h->d_cnt + BF, BN, n);
    if (!rc && with_cmp) rc = copy_rows(h, comparable_rep, h->d_cmp, BF, n);
    if (!rc && with_cmp) rc = copy_rows(h, local_comparable_rep, h->d_cmp + BF, BN, n);
    if (!rc && total_rep) rc = unit_copy_back(h, (const long long*)h->d_total, (size_t)(n * B), {(long long*)total_rep});
    if (!rc) rc = unit_sync_timed(h);
    if (rc) return rc;
    h->n_replicates += n;
    return SBE_OK;
}

int sbe_spatial_read(sbe_spatial* h, int32_t* agree_obs, int32_t* comparable_obs, int32_t* local_obs, int32_t* local_comparable_obs,
                     int64_t* total_obs, int32_t* f_greater, int32_t* f_equal, int32_t* f_less, int64_t* f_sum, int64_t* f_sumsq,
                     int32_t* i_greater, int32_t* i_equal, int32_t* i_less, int64_t* i_sum, int64_t* i_sumsq, int32_t* t_greater,
                     int32_t* t_equal, int32_t* t_less, int64_t* n_replicates_out) {
    CHECK_HANDLE(h, kNullHandle);
    if (!agree_obs || !comparable_obs || !local_obs || !local_comparable_obs || !total_obs || !f_greater || !f_equal || !f_less || !f_sum || !f_sumsq ||
        !i_greater || !i_equal || !i_less || !i_sum || !i_sumsq || !t_greater || !t_equal || !t_less || !n_replicates_out)
        return fail(h, SBE_ERR_ARG, "null pointer argument: output");
    if (h->F == 0) return fail(h, SBE_ERR_STATE, "sbe_spatial_read needs the data of a successful sbe_spatial_set_data");
    HIPCHK(h, hipSetDevice(h->device));
    const size_t BF = (size_t)h->B * (size_t)h->F, BN = (size_t)h->B * (size_t)h->N, E = BF + BN, B = (size_t)h->B;
    std::copy_n(h->obs.begin(), BF, agree_obs);
    std::copy_n(h->obs.begin() + BF, BN, local_obs);
    std::copy_n(h->obs_cmp.begin(), BF, comparable_obs);
    std::copy_n(h->obs_cmp.begin() + BF, BN, local_comparable_obs);
    std::copy_n(h->total_obs.begin(), B, total_obs);
    int32_t* const f_counts[3] = {f_greater, f_equal, f_less};
    int32_t* const i_counts[3] = {i_greater, i_equal, i_less};
    int32_t* const t_counts[3] = {t_greater, t_equal, t_less};
    int rc = SBE_OK;
    for (int k = 0; k < 3 && !rc; ++k) {
        const int32_t* d = h->counts() + (size_t)k * (E + B);
        rc = unit_copy_back(h, d, BF, {f_counts[k]});
        if (!rc) rc = unit_copy_back(h, d + BF, BN, {i_counts[k]});
        if (!rc) rc = unit_copy_back(h, d + E, B, {t_counts[k]});
    }
    if (!rc) rc = unit_copy_back(h, (const long long*)h->sum(), BF, {(long long*)f_sum});
    if (!rc) rc = unit_copy_back(h, (const long long*)h->sum() + BF, BN, {(long long*)i_sum});
    if (!rc) rc = unit_copy_back(h, (const long long*)h->sumsq(), BF, {(long long*)f_sumsq});
    if (!rc) rc = unit_copy_back(h, (const long long*)h->sumsq() + BF, BN, {(long long*)i_sumsq});
    if (rc) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    *n_replicates_out = h->n_replicates;
    return SBE_OK;
}

int sbe_spatial_reset(sbe_spatial* h) {
    CHECK_HANDLE(h, kNullHandle);
    if (h->F == 0) return fail(h, SBE_ERR_STATE, "sbe_spatial_reset needs the data of a successful sbe_spatial_set_data");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemsetAsync(h->d_acc, 0, h->acc_size(), h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->n_replicates = 0;
    return SBE_OK;
}

int sbe_spatial_last_kernel_ms(const sbe_spatial* h, float* ms_out) { return unit_last_kernel_ms(h, ms_out, kNullHandle); }

}  // extern "C"
