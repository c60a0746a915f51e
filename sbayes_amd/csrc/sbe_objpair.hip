// sbe_objpair.hip -- the object-pair posterior predictive check (include/sbe_objpair.h): on how many features every pair of
// objects agrees, on the data and on a stream of replicated data sets, and where the observed counts fall among the replicated
// ones.  The contract is tests/_objpair_oracle.py; DESIGN.md section 31 has the layout and the measurements.
//
// With Y the 0/1 matrix of one-hot state rows, [N][E], E = sum of n_states, the agreement counts of a data set are Y Y^T;
// with P the 0/1 matrix of observed cells, [N][F], the comparable counts are P P^T.  Both are computed a 32 x 32 tile per wave,
// for the tile pairs I <= J, with the FP4 contraction of sbe_unit_tiles.hip.h (exact in the f32 accumulator: a count is at most
// F <= 4096).  k_objpair_pack has written the operands, so the contraction is loads and MFMAs only.
//   image: [n][N_pad objects][E_pad / 2 bytes], the object-major image of sbe_consensus.hip: element e = off[f] + y[i][f] (off: the
//   exclusive prefix sum of n_states) is nibble e & 7 of dword e >> 3 of the object's row, 0x2 for the one element of a coded cell;
//   rows are padded to whole rounds of 256 elements, objects to whole tiles, both with zeros.  A lane owns one object
//   (lane & 31) and one half of a step (lane >> 5): 32 elements, one 16-byte load, and both operands come from this one image.
// k_objpair_replicates keeps a tile's agree_obs in registers and walks a chunk of the call's replicates: contract, compare, and
// five running sums per entry, added to the handle's accumulators once per chunk with integer atomics (the replicates are dealt
// over waves in chunks: at N = 1000 there are 528 tile pairs for 1024 SIMDs).  Only the tiles I <= J are accumulated;
// k_objpair_mirror fills the lower triangle from the upper one, so that every atomic instruction covers whole row segments.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "sbe_unit_tiles.hip.h"
#include "../../include/sbe_objpair.h"

namespace {

constexpr unsigned long long kNoOffender = ~0ull;
constexpr int kMaxGridY = 65535;
constexpr int kPackBlock = 256;
constexpr int64_t kTargetWaves = 8 * 1024;           // waves of a replicate launch the chunks aim at: eight per SIMD of an MI355X
constexpr int64_t kMaxChunk = 255;                   // replicates of a chunk: its sums of squares, at most 255 * 2^24, fit 32 bits
static_assert(kRoundElems == SBE_OBJPAIR_ROUND, "the header states the round length");

// ---- pack: y [n][N][F] (staging) -> the operand image [n][N_pad][dwords], and the first code that is neither below its
// feature's state count nor NA, by its index in y (an integer atomic minimum).  A thread owns one (object, dword): the elements
// [8 d, 8 d + 8) of the row, which hold the states of the features first[d] .. while off[f] < 8 d + 8 (a feature of up to 32
// states spans up to five dwords, and every feature is read by the thread of its first one at least).  kPresence: element f is
// the cell's "observed" instead (E' = F; nothing is validated).  blockIdx.x: kPackBlock (object, dword) entries, y + r0: replicate
template <bool kPresence>
__global__ __launch_bounds__(kPackBlock) void k_objpair_pack(const uint8_t* y, int N, int F, int N_pad, int dwords, const int32_t* off, const int32_t* first,
                                                            int64_t r0, uint32_t* img, unsigned long long* offender) {
    const int64_t idx = (int64_t)blockIdx.x * kPackBlock + threadIdx.x;
    if (idx >= (int64_t)N_pad * dwords) return;
    const int64_t r = r0 + blockIdx.y;
    const int i = (int)(idx / dwords), d = (int)(idx - (int64_t)i * dwords), e0 = 8 * d;
    uint32_t bits = 0;
    if (i < N) {
        const int64_t at = (r * N + i) * F;
        if (kPresence) {
            for (int f = e0; f < F && f < e0 + 8; ++f)
                if (y[at + f] != SBE_OBJPAIR_NA) bits |= 2u << (4 * (f - e0));
        } else {
            for (int f = first[d]; f < F && off[f] < e0 + 8; ++f) {
                const int c = y[at + f];
                if (c == SBE_OBJPAIR_NA) continue;
                if (c >= off[f + 1] - off[f]) {
                    atomicMin(offender, (unsigned long long)(at + f));
                    continue;
                }
                const int e = off[f] + c - e0;
                if (e >= 0 && e < 8) bits |= 2u << (4 * e);
            }
        }
    }
    img[(r * N_pad + i) * dwords + d] = bits;
}

// ---- the contraction of one tile: rows the objects of tile I, columns those of tile J, over `rounds` rounds of one data set's image
__device__ inline v16f contract_tile(const uint8_t* img, int64_t row_bytes, int rounds, int64_t I, int64_t J, int lane) {
    // (the image has whole tiles of objects: the rows behind N are zero)
    const uint8_t* a = img + (I * kTile + (lane & 31)) * row_bytes + (kStep / 4) * (lane >> 5);
    const uint8_t* b = img + (J * kTile + (lane & 31)) * row_bytes + (kStep / 4) * (lane >> 5);
    v16f acc = {};
    for (int r = 0; r < rounds; ++r, a += kRoundBytes, b += kRoundBytes) {
        const LaneRound ca = load_round(a), cb = load_round(b);
#pragma unroll
        for (int u = 0; u < kRound; ++u) acc = mfma_fp4(fp4_operand(ca.q[u]), fp4_operand(cb.q[u]), acc);
    }
    return acc;
}

// ---- the counts of one data set (the data: agree from the state image, comparable from the presence image); one wave per tile pair
struct CountArgs {
    const uint8_t* img;       // [N_pad][row_bytes]
    int64_t row_bytes;
    int rounds, N;
    int64_t t0, t_end;        // tile pairs [t0, t_end) of the enumeration t = J (J + 1) / 2 + I, I <= J
    int32_t* counts;          // [N][N]: both triangles, the diagonal 0
};

__global__ __launch_bounds__(64) void k_objpair_counts(const CountArgs g) {
    const int64_t t = g.t0 + blockIdx.x;
    if (t >= g.t_end) return;
    const TilePair pair = tile_pair(t);
    const int64_t I = pair.I, J = pair.J;
    const int lane = threadIdx.x;
    const v16f acc = contract_tile(g.img, g.row_bytes, g.rounds, I, J, lane);
    const int64_t j = J * kTile + (lane & 31), N = g.N;
    if (j >= N) return;
    int32_t* const counts = g.counts;
    for_acc_entries(acc, (int64_t)(lane >> 5), lane & 31, [=](int64_t row, int, float v) {
        const int64_t i = I * kTile + row;
        if (i >= N) return;
        const int32_t c = i == j ? 0 : (int32_t)v;
        counts[i * N + j] = c;
        if (I != J) counts[j * N + i] = c;                   // (a diagonal tile holds both triangles itself)
    });
}

// ---- the replicates: blockIdx.x: tile pair, blockIdx.y: chunk of the call's replicates.  A lane's 16 entries of agree_obs and
// their running sums stay in registers over the chunk; n_less is what is left of the chunk
struct ReplicateArgs {
    const uint8_t* img;       // [n_rep][N_pad][row_bytes]
    int64_t row_bytes, set_bytes;   // of an object's row, of one data set's image
    int rounds, N;
    int64_t n_rep, chunk;     // replicates of the call, replicates per chunk
    int64_t t0, t_end;
    const int32_t* obs;       // agree_obs [N][N]
    int32_t* counts;          // [3][N][N]: n_greater, n_equal, n_less
    unsigned long long* sum;  // [N][N]
    unsigned long long* sumsq;
    int32_t* rep;             // [n_rep][N][N] or null: the replicates' own counts (the tiles I <= J; k_objpair_mirror follows)
};

// kRep: the replicates' own counts are stored as well
template <bool kRep>
__device__ __forceinline__ void replicate_chunk(const ReplicateArgs& g) {
    const int64_t t = g.t0 + blockIdx.x;
    if (t >= g.t_end) return;
    const int64_t r_lo = (int64_t)blockIdx.y * g.chunk, r_hi = min(g.n_rep, r_lo + g.chunk);
    const TilePair pair = tile_pair(t);
    const int64_t I = pair.I, J = pair.J;
    const int lane = threadIdx.x, half = lane >> 5, col = lane & 31;
    const int64_t N = g.N, nn = N * N;
    const int64_t j = J * kTile + col;
    const int rows = (int)min((int64_t)kTile, N - I * kTile);      // rows of the tile that are objects
    const int diagonal = I == J ? col : -1;                        // the row of this lane's entry on the diagonal, if it has one

    // a chunk has at most kMaxChunk = 255 replicates and v <= 2^12: its sum of squares stays below 2^32, and the counts of the
    // replicates above (low half) and at (high half) the observed value share one register.  An entry on the diagonal or behind
    // N is tallied like the others and never written
    int32_t obs[kAccRegs];
    uint32_t tally[kAccRegs], sum[kAccRegs], sumsq[kAccRegs];
    const int32_t* const obs_at = g.obs + (I * kTile) * N + j;
#pragma unroll
    for (int reg = 0; reg < kAccRegs; ++reg) {
        const int row = acc_row(reg, half);
        obs[reg] = row < rows && j < N ? obs_at[(int64_t)row * N] : 0;
        tally[reg] = sum[reg] = sumsq[reg] = 0;
    }
    for (int64_t r = r_lo; r < r_hi; ++r) {
        const v16f acc = contract_tile(g.img + r * g.set_bytes, g.row_bytes, g.rounds, I, J, lane);
        int32_t* const rep_at = kRep ? g.rep + r * nn + (I * kTile) * N + j : nullptr;
        int reg = 0;                                          // (the walk is unrolled: a constant in every copy of the body)
        for_acc_entries(acc, half, col, [&](int row, int, float value) {
            const int32_t v = (int32_t)value;
            tally[reg] += (uint32_t)(v > obs[reg]) + ((uint32_t)(v == obs[reg]) << 16);
            sum[reg] += (uint32_t)v;
            sumsq[reg] += (uint32_t)v * (uint32_t)v;
            if (kRep && row < rows && j < N) rep_at[(int64_t)row * N] = row == diagonal ? 0 : v;
            ++reg;
        });
    }
    if (j >= N) return;
    const int32_t n_chunk = (int32_t)(r_hi - r_lo);
#pragma unroll
    for (int reg = 0; reg < kAccRegs; ++reg) {
        const int row = acc_row(reg, half);
        if (row >= rows || row == diagonal) continue;         // (the diagonal stays 0)
        const int64_t at = (I * kTile + row) * N + j;
        const int32_t greater = (int32_t)(tally[reg] & 0xffffu), equal = (int32_t)(tally[reg] >> 16);
        atomicAdd(g.counts + at, greater);
        atomicAdd(g.counts + nn + at, equal);
        atomicAdd(g.counts + 2 * nn + at, n_chunk - greater - equal);
        atomicAdd(g.sum + at, (unsigned long long)sum[reg]);
        atomicAdd(g.sumsq + at, (unsigned long long)sumsq[reg]);
    }
}

__global__ __launch_bounds__(64) void k_objpair_replicates(const ReplicateArgs g) { replicate_chunk<false>(g); }
__global__ __launch_bounds__(64) void k_objpair_replicates_kept(const ReplicateArgs g) { replicate_chunk<true>(g); }

// ---- the lower triangle from the upper one: m[j][i] = m[i][j] for the tiles I < J of `count` matrices [N][N], a 32 x 32 tile
// through LDS.  blockIdx.x + t0: tile pair, blockIdx.y: matrix
template <class T>
__global__ __launch_bounds__(256) void k_objpair_mirror(T* matrices, int64_t N, int64_t t0) {
    __shared__ T tile[kTile][kTile + 1];
    const TilePair pair = tile_pair(t0 + blockIdx.x);
    if (pair.I == pair.J) return;                             // (uniform for the block)
    T* m = matrices + (int64_t)blockIdx.y * N * N;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
    for (int k = ty; k < kTile; k += 8) {
        const int64_t i = pair.I * kTile + k, j = pair.J * kTile + tx;
        if (i < N && j < N) tile[k][tx] = m[i * N + j];
    }
    __syncthreads();
    for (int k = ty; k < kTile; k += 8) {
        const int64_t j = pair.J * kTile + k, i = pair.I * kTile + tx;
        if (i < N && j < N) m[j * N + i] = tile[tx][k];
    }
}

}  // namespace

struct sbe_objpair : sbe_unit_handle, unit_tile_launches {   // (sbe_unit.hip.h; ev: around the count kernels' launches)
    int32_t* d_off = nullptr;                    // off [F + 1], then first [E_pad / 8]
    size_t off_bytes = 0;
    int32_t* d_obs = nullptr;                    // agree_obs, comparable_obs [N][N]
    size_t obs_bytes = 0;
    void* d_acc = nullptr;                       // sum, sumsq int64 [N][N], then the counts int32 [3][N][N]
    size_t acc_bytes = 0;
    uint8_t* d_stage = nullptr;                  // the data sets of one call as uploaded, [n][N][F]
    size_t stage_bytes = 0;
    uint8_t* d_img = nullptr;                    // ... their operand images [n][N_pad][row_bytes]
    size_t img_bytes = 0;
    int32_t* d_rep = nullptr;                    // ... their own counts [n][N][N] (agree_rep_out)
    size_t rep_bytes = 0;
    unsigned long long* d_offender = nullptr;
    int64_t N = 0, F = 0;                        // shape of the data (F == 0: none yet)
    int64_t E = 0, e_pad = 0, n_pad = 0;
    int64_t n_replicates = 0;
    int64_t tile_pairs = 0, launches = 0;        // of the last set_data or add
    std::vector<void*> buffers() const { return {d_off, d_obs, d_acc, d_stage, d_img, d_rep, d_offender}; }

    size_t nn() const { return (size_t)N * (size_t)N; }
    int64_t row_bytes() const { return e_pad / 2; }
    const int32_t* first() const { return d_off + F + 1; }
    unsigned long long* sum() const { return (unsigned long long*)d_acc; }
    unsigned long long* sumsq() const { return sum() + nn(); }
    int32_t* counts() const { return (int32_t*)(sumsq() + nn()); }
    size_t acc_size() const { return nn() * 28; }
};

namespace {

constexpr char kNullHandle[] = "null handle";

bool shape_in_limits(int64_t N, int64_t F) { return N >= 1 && N <= SBE_OBJPAIR_MAX_OBJECTS && F >= 1 && F <= SBE_OBJPAIR_MAX_FEATURES; }

int64_t replicate_bytes(int64_t N, int64_t F, int64_t E, bool with_agree_rep) {
    return N * F + whole_tiles(N) * (whole_rounds(E) / 2) + (with_agree_rep ? 4 * N * N : 0);
}

// the most replicates one call takes: what fits the staging limit, and one at least
int64_t call_replicates(int64_t each) { return std::max<int64_t>(1, SBE_OBJPAIR_MAX_STAGE_BYTES / each); }

// The n data sets in d_stage [n][N][F] packed into d_img (the handle's shape members and d_off are set; its device is current):
// checked on the way, `offender_out` the first bad code's index or kNoOffender.  kPresence: the presence image of one data set
// at row length `row_bytes` instead.
template <bool kPresence>
int pack_staged(sbe_objpair* h, int64_t n, int64_t row_bytes, unsigned long long& offender_out) {
    const int dwords = (int)(row_bytes / 4);
    unsigned long long offender = kNoOffender;
    HIPCHK(h, hipMemcpyAsync(h->d_offender, &offender, sizeof offender, hipMemcpyHostToDevice, h->stream));
    for (int64_t r0 = 0; r0 < n; r0 += kMaxGridY) {
        const dim3 grid((unsigned)div_up(h->n_pad * dwords, kPackBlock), (unsigned)std::min<int64_t>(kMaxGridY, n - r0));
        k_objpair_pack<kPresence><<<grid, kPackBlock, 0, h->stream>>>(h->d_stage, (int)h->N, (int)h->F, (int)h->n_pad, dwords, h->d_off, h->first(), r0,
                                                                      (uint32_t*)h->d_img, h->d_offender);
        HIPCHK(h, hipGetLastError());
    }
    HIPCHK(h, hipMemcpyAsync(&offender, h->d_offender, sizeof offender, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    offender_out = offender;
    return SBE_OK;
}

// the tile pairs of the image of one data set in d_img into counts [N][N]; `launches` grows by the launches made
int count_image(sbe_objpair* h, int64_t row_bytes, int32_t* counts, int64_t& launches) {
    const int64_t tiles = tiles_of(h->N), tile_pairs = tiles * (tiles + 1) / 2, rounds = row_bytes / kRoundBytes;
    return unit_for_tile_launches(tile_pairs, tiles_per_launch(rounds * kRound, h->launch_tiles), [&](int64_t t0, int64_t t_end) {
        const CountArgs args{h->d_img, row_bytes, (int)rounds, (int)h->N, t0, t_end, counts};
        k_objpair_counts<<<(unsigned)(t_end - t0), 64, 0, h->stream>>>(args);
        HIPCHK(h, hipGetLastError());
        ++launches;
        return SBE_OK;
    });
}

// the lower triangles of `count` matrices [N][N] of T from `first` on
template <class T>
int mirror(sbe_objpair* h, T* first, int64_t count) {
    const int64_t tiles = tiles_of(h->N), tile_pairs = tiles * (tiles + 1) / 2;
    for (int64_t m0 = 0; m0 < count; m0 += kMaxGridY) {
        const dim3 grid((unsigned)tile_pairs, (unsigned)std::min<int64_t>(kMaxGridY, count - m0));
        k_objpair_mirror<T><<<grid, 256, 0, h->stream>>>(first + m0 * (int64_t)h->nn(), h->N, 0);
        HIPCHK(h, hipGetLastError());
    }
    return SBE_OK;
}

}  // namespace

extern "C" {

int sbe_objpair_abi_version(void) { return SBE_OBJPAIR_ABI_VERSION; }

const char* sbe_objpair_last_error(const sbe_objpair* h) { return unit_last_error(h); }

int sbe_objpair_create(sbe_objpair** out, int device) { return unit_create_on_device(out, device, "sbe_objpair_create"); }

int sbe_objpair_destroy(sbe_objpair* h) { return unit_destroy(h, kNullHandle); }

int sbe_objpair_set_launch_tiles(sbe_objpair* h, int64_t tile_pairs) { return unit_set_launch_tiles(h, tile_pairs, kNullHandle); }

int64_t sbe_objpair_max_replicates(int64_t n_objects, int64_t n_features) { return shape_in_limits(n_objects, n_features) ? INT32_MAX : 0; }

int64_t sbe_objpair_replicate_bytes(int64_t n_objects, int64_t n_features, int64_t n_elements, int with_agree_rep) {
    if (!shape_in_limits(n_objects, n_features) || n_elements < n_features || n_elements > SBE_OBJPAIR_MAX_STATES * n_features) return 0;
    return replicate_bytes(n_objects, n_features, n_elements, with_agree_rep != 0);
}

int sbe_objpair_set_data(sbe_objpair* h, const uint8_t* x, int64_t n_objects, int64_t n_features, const int32_t* n_states) {
    CHECK_HANDLE(h, kNullHandle);
    if (!x || !n_states) return fail(h, SBE_ERR_ARG, "null pointer argument: %s", !x ? "x" : "n_states");
    h->F = 0;                                       // (a refused call leaves the handle without data)
    const int64_t N = n_objects, F = n_features;
    if (N < 1 || N > SBE_OBJPAIR_MAX_OBJECTS)
        return fail(h, SBE_ERR_ARG, "n_objects=%lld out of range [1, %d] (the outputs are [N][N] matrices)", (long long)N, SBE_OBJPAIR_MAX_OBJECTS);
    if (F < 1 || F > SBE_OBJPAIR_MAX_FEATURES) return fail(h, SBE_ERR_ARG, "n_features=%lld out of range [1, %d]", (long long)F, SBE_OBJPAIR_MAX_FEATURES);
    std::vector<int32_t> off((size_t)F + 1, 0);
    for (int64_t f = 0; f < F; ++f) {
        if (n_states[f] < 1 || n_states[f] > SBE_OBJPAIR_MAX_STATES)
            return fail(h, SBE_ERR_ARG, "n_states[%lld]=%d out of range [1, %d] (the state limit of the replicates' source, sbe_ppc.h)", (long long)f,
                         n_states[f], SBE_OBJPAIR_MAX_STATES);
        off[(size_t)f + 1] = off[(size_t)f] + n_states[f];
    }
    for (int64_t i = 0; i < N; ++i)
        for (int64_t f = 0; f < F; ++f) {
            const uint8_t c = x[i * F + f];
            if (c != SBE_OBJPAIR_NA && c >= n_states[f])
                return fail(h, SBE_ERR_DATA, "x[%lld][%lld]=%d is neither below n_states[%lld]=%d nor %d (not observed)", (long long)i, (long long)f, (int)c,
                             (long long)f, n_states[f], SBE_OBJPAIR_NA);
        }
    const int64_t E = off[(size_t)F], e_pad = whole_rounds(E), n_pad = whole_tiles(N), presence_bytes = whole_rounds(F) / 2;
    // first[d]: the first feature with a state in or behind dword d (F: none)
    const size_t dwords = (size_t)(e_pad / 8);
    off.resize((size_t)F + 1 + dwords, (int32_t)F);
    for (int64_t f = F - 1; f >= 0; --f)
        for (int64_t d = off[(size_t)f] / 8; d <= (off[(size_t)f + 1] - 1) / 8; ++d) off[(size_t)(F + 1 + d)] = (int32_t)f;

    HIPCHK(h, hipSetDevice(h->device));
    h->N = N;                                       // (the shape the helpers below read; F stays 0 until the data is in place)
    h->E = E;
    h->e_pad = e_pad;
    h->n_pad = n_pad;
    const size_t nn = h->nn();
    int rc = unit_ensure(h, h->d_off, h->off_bytes, off.size() * sizeof(int32_t));
    if (!rc) rc = unit_ensure(h, h->d_obs, h->obs_bytes, 2 * nn * sizeof(int32_t));
    if (!rc) rc = unit_ensure(h, h->d_acc, h->acc_bytes, h->acc_size());
    if (!rc) rc = unit_ensure(h, h->d_stage, h->stage_bytes, (size_t)(N * F));
    if (!rc) rc = unit_ensure(h, h->d_img, h->img_bytes, (size_t)(n_pad * std::max(e_pad / 2, presence_bytes)));
    if (!rc) rc = unit_ensure(h, h->d_offender, sizeof(unsigned long long));
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(h->d_off, off.data(), off.size() * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_stage, x, (size_t)(N * F), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(h->d_acc, 0, h->acc_size(), h->stream));
    h->F = F;                                       // (the helpers read the whole shape; taken back on failure)
    unsigned long long offender = kNoOffender;
    int64_t launches = 0;
    rc = pack_staged<false>(h, 1, e_pad / 2, offender);
    if (!rc && offender != kNoOffender) rc = fail(h, SBE_ERR_DATA, "the device refused code %llu of x that the host check had passed", offender);
    if (!rc) rc = unit_timed(h, [&] {
        if (const int rc_agree = count_image(h, e_pad / 2, h->d_obs, launches)) return rc_agree;
        // (the same stream: the presence image replaces the state image once its tiles are counted)
        unsigned long long none = kNoOffender;
        if (const int rc_pack = pack_staged<true>(h, 1, presence_bytes, none)) return rc_pack;
        return count_image(h, presence_bytes, h->d_obs + nn, launches);
    });
    if (!rc) rc = unit_sync_timed(h);
    h->F = 0;
    if (rc) return rc;
    h->F = F;
    h->n_replicates = 0;
    const int64_t tiles = tiles_of(N);
    h->tile_pairs = tiles * (tiles + 1) / 2;
    h->launches = launches;
    return SBE_OK;
}

int sbe_objpair_add(sbe_objpair* h, int64_t n, const uint8_t* y_rep, int32_t* agree_rep_out) {
    CHECK_HANDLE(h, kNullHandle);
    if (h->F == 0) return fail(h, SBE_ERR_STATE, "sbe_objpair_add needs the data of a successful sbe_objpair_set_data");
    if (n < 0) return fail(h, SBE_ERR_ARG, "n=%lld is negative", (long long)n);
    if (n == 0) return SBE_OK;
    if (!y_rep) return fail(h, SBE_ERR_ARG, "null pointer argument: y_rep");
    const int64_t N = h->N, F = h->F, each = replicate_bytes(N, F, h->E, agree_rep_out != nullptr);
    if (n > (int64_t)INT32_MAX - h->n_replicates)
        return fail(h, SBE_ERR_ARG, "%lld replicates after %lld exceed the %lld that the int32 counts hold (sbe_objpair_max_replicates)", (long long)n,
                     (long long)h->n_replicates, (long long)INT32_MAX);
    if (n > call_replicates(each))
        return fail(h, SBE_ERR_ARG, "%lld replicates of %lld bytes each exceed the %lld bytes one call holds on the device (split the block)",
                     (long long)n, (long long)each, (long long)SBE_OBJPAIR_MAX_STAGE_BYTES);
    const int64_t row_bytes = h->row_bytes(), set_bytes = h->n_pad * row_bytes, rounds = row_bytes / kRoundBytes;
    const int64_t tiles = tiles_of(N), tile_pairs = tiles * (tiles + 1) / 2;
    // the replicates are dealt over waves in chunks of at most kMaxChunk, so that a launch has about kTargetWaves of them
    const int64_t chunks = std::max<int64_t>(div_up(n, kMaxChunk), std::min<int64_t>(n, div_up(kTargetWaves, tile_pairs)));
    const int64_t chunk = (n + chunks - 1) / chunks;
    const int64_t n_chunks = div_up(n, chunk);            // (below 2^16: the staging limit holds n there)
    // (a tile pair walks every replicate of the call within one launch, a block per chunk: the blocks stay within a grid's)
    const int64_t per_launch = std::min(tiles_per_launch(n * rounds * kRound, h->launch_tiles), kMaxGridBlocks / n_chunks);
    const size_t nn = h->nn();

    HIPCHK(h, hipSetDevice(h->device));
    int rc = unit_ensure(h, h->d_stage, h->stage_bytes, (size_t)(n * N * F));
    if (!rc) rc = unit_ensure(h, h->d_img, h->img_bytes, (size_t)(n * set_bytes));
    if (!rc && agree_rep_out) rc = unit_ensure(h, h->d_rep, h->rep_bytes, (size_t)n * nn * sizeof(int32_t));
    if (rc) return rc;
    // the upload, checked on the device while it is packed; nothing of the accumulators is touched before the codes have passed
    HIPCHK(h, hipMemcpyAsync(h->d_stage, y_rep, (size_t)(n * N * F), hipMemcpyHostToDevice, h->stream));
    unsigned long long offender = kNoOffender;
    if ((rc = pack_staged<false>(h, n, row_bytes, offender))) return rc;
    if (offender != kNoOffender) {
        const int64_t at = (int64_t)offender, f = at % F, i = at / F % N, r = at / (N * F);
        return fail(h, SBE_ERR_DATA, "y_rep[%lld][%lld][%lld]=%d is neither below n_states[%lld] nor %d (not observed)", (long long)r, (long long)i,
                     (long long)f, (int)y_rep[at], (long long)f, SBE_OBJPAIR_NA);
    }
    int64_t launches = 0;
    rc = unit_timed(h, [&] {
        return unit_for_tile_launches(tile_pairs, per_launch, [&](int64_t t0, int64_t t_end) {
            const ReplicateArgs args{h->d_img, row_bytes, set_bytes, (int)rounds, (int)N, n, chunk, t0, t_end, h->d_obs, h->counts(), h->sum(), h->sumsq(),
                                     agree_rep_out ? h->d_rep : nullptr};
            const dim3 grid((unsigned)(t_end - t0), (unsigned)n_chunks);
            if (agree_rep_out)
                k_objpair_replicates_kept<<<grid, 64, 0, h->stream>>>(args);
            else
                k_objpair_replicates<<<grid, 64, 0, h->stream>>>(args);
            HIPCHK(h, hipGetLastError());
            ++launches;
            return SBE_OK;
        });
    });
    if (!rc && agree_rep_out) rc = mirror(h, h->d_rep, n);
    if (!rc && agree_rep_out) rc = unit_copy_back(h, (const int32_t*)h->d_rep, (size_t)n * nn, {agree_rep_out});
    if (!rc) rc = unit_sync_timed(h);
    if (rc) return rc;
    h->n_replicates += n;
    h->tile_pairs = tile_pairs;
    h->launches = launches;
    return SBE_OK;
}

int sbe_objpair_read(sbe_objpair* h, int32_t* agree_obs, int32_t* comparable_obs, int32_t* n_greater, int32_t* n_equal, int32_t* n_less,
                     int64_t* sum, int64_t* sumsq, int64_t* n_replicates_out) {
    CHECK_HANDLE(h, kNullHandle);
    if (h->F == 0) return fail(h, SBE_ERR_STATE, "sbe_objpair_read needs the data of a successful sbe_objpair_set_data");
    HIPCHK(h, hipSetDevice(h->device));
    const size_t nn = h->nn();
    // the accumulators hold the tiles I <= J: the lower triangle is filled here (again after every add; it changes nothing above)
    int rc = mirror(h, h->counts(), 3);
    if (!rc) rc = mirror(h, h->sum(), 2);
    int32_t* const outs32[5] = {agree_obs, comparable_obs, n_greater, n_equal, n_less};
    const int32_t* const from32[5] = {h->d_obs, h->d_obs + nn, h->counts(), h->counts() + nn, h->counts() + 2 * nn};
    for (int k = 0; k < 5 && !rc; ++k)
        if (outs32[k]) rc = unit_copy_back(h, from32[k], nn, {outs32[k]});
    if (!rc && sum) rc = unit_copy_back(h, (const long long*)h->sum(), nn, {(long long*)sum});
    if (!rc && sumsq) rc = unit_copy_back(h, (const long long*)h->sumsq(), nn, {(long long*)sumsq});
    if (rc) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (n_replicates_out) *n_replicates_out = h->n_replicates;
    return SBE_OK;
}

int sbe_objpair_reset(sbe_objpair* h) {
    CHECK_HANDLE(h, kNullHandle);
    if (h->F == 0) return fail(h, SBE_ERR_STATE, "sbe_objpair_reset needs the data of a successful sbe_objpair_set_data");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemsetAsync(h->d_acc, 0, h->acc_size(), h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->n_replicates = 0;
    return SBE_OK;
}

int sbe_objpair_last_shape(const sbe_objpair* h, int64_t* e_pad_out, int64_t* tile_pairs_out, int64_t* launches_out) {
    CHECK_HANDLE(h, kNullHandle);
    if (!e_pad_out || !tile_pairs_out || !launches_out) return fail(h, SBE_ERR_ARG, "null pointer argument: output");
    if (h->F == 0) return fail(h, SBE_ERR_STATE, "no successful sbe_objpair_set_data yet");
    *e_pad_out = h->e_pad;
    *tile_pairs_out = h->tile_pairs;
    *launches_out = h->launches;
    return SBE_OK;
}

int sbe_objpair_last_kernel_ms(const sbe_objpair* h, float* ms_out) { return unit_last_kernel_ms(h, ms_out, kNullHandle); }

}  // extern "C"
