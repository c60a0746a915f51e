#pragma once
// sbe_assoc_pair.hip.h -- the arithmetic of one 32 x 32 tile pair of the feature screening, written once for the two units
// that run it (sbe_assoc.hip on the data, sbe_pairppc.hip on the data and on a stream of replicates, and no other file): the
// FP4 operands built in registers from feature-major codes, the contraction over objects, the margins of every sub-table,
// total and dof, the Pearson terms in fp64 and their ordered sum; and on the host the checks of a data set and its feature-major
// image.  tests/_assoc_oracle.py is the numerical contract; DESIGN.md section 13 has the layout.  A wave of 64 lanes is one
// workgroup; everything lives in an unnamed namespace.
//
// With X the one-hot matrix [N][F * S_pad] (S_pad: the next power of two >= the largest state count, so that a 32 x 32
// tile holds (32 / S_pad)^2 whole pairs), all contingency tables at once are X^T X.  For the tile pair I <= J:
//   1. pair_contract: the FP4 contraction over objects of sbe_unit_tiles.hip.h (the counts are exact in the f32 accumulator
//      while N <= 2^24).  A lane owns one one-hot column (feature f, state s) and 32 objects of the step; four byte-parallel
//      operations turn four codes into four "code == s" bits (an NA object, 255, matches no state, and neither does the
//      padding behind N);
//   2. pair_terms: the accumulator tile goes to LDS; margins of every sub-table along both tile axes, then per pair its
//      total, the occupied rows R and columns C, dof = (R-1)(C-1);
//   3. pair_terms: per cell the Pearson term in fp64 (expected r c / n, Yates' correction when dof == 1), into LDS;
//   4. pair_statistic: one lane sums a pair's terms in the fixed order (a major, b minor) -- empty rows and columns add +0.0,
//      which changes no bit of a non-negative sum.
#include <algorithm>
#include <vector>

#include "sbe_unit.hip.h"
#include "sbe_unit_tiles.hip.h"
#include "../../include/sbe_assoc.h"

namespace {

constexpr int kPad = 256;                            // the codes are padded to whole rounds: a lane reads a byte per object
static_assert(kPad == kRoundElems, "a round of codes is a round of the contraction");

// four "code == s" bits of four codes: codes are < 32 or 255, s < 32 (or 0x40 for a column behind the last feature, which
// matches nothing).  Masked to six bits an NA code is 63; the xor is zero exactly for a match; adding 0x7f sets bit 7 of
// every non-zero byte without a carry (63 + 127 < 256)
__device__ inline uint32_t match4(uint32_t codes, uint32_t s4) {
    return ~(((codes & 0x3f3f3f3fu) ^ s4) + 0x7f7f7f7fu) & 0x80808080u;
}

// FP4 operand of one lane: 32 objects (32 codes) against the lane's state; 1.0 = 0x2 in e2m1, so a match sets bit 1 of its
// nibble.  Object 8 d + b of the 32 goes to nibble 2 b (b < 4) or 2 (b - 4) + 1 of dword d
__device__ inline v8i fp4_operand(const uint4 lo, const uint4 hi, uint32_t s4) {
    v8i v = {};
    v[0] = (int)((match4(lo.x, s4) >> 6) | (match4(lo.y, s4) >> 2));
    v[1] = (int)((match4(lo.z, s4) >> 6) | (match4(lo.w, s4) >> 2));
    v[2] = (int)((match4(hi.x, s4) >> 6) | (match4(hi.y, s4) >> 2));
    v[3] = (int)((match4(hi.z, s4) >> 6) | (match4(hi.w, s4) >> 2));
    return v;
}

// the codes of one lane for one round of kRound contraction steps: q[2 u], q[2 u + 1] are its 32 objects of step u.  A round's
// loads are issued together, so their latency is paid once per round
struct LaneCodes {
    uint4 q[2 * kRound];
};

__device__ inline LaneCodes load_codes(const uint8_t* p) {
    LaneCodes c;
#pragma unroll
    for (int u = 0; u < kRound; ++u) {
        c.q[2 * u] = *reinterpret_cast<const uint4*>(p + u * kStep);
        c.q[2 * u + 1] = *reinterpret_cast<const uint4*>(p + u * kStep + 16);
    }
    return c;
}

// ---- the LDS of one wave -------------------------------------------------------------------------------------------------
// pair_lds_bytes(sub): the terms (8 KiB) -- whose first half holds the tile of X^T X until step 3 -- then the margins and the
// per-pair values, sized by the sub-tables per tile edge, so that four waves fit a SIMD from S_pad = 8 on
struct PairLds {
    double (*term)[kTile];
    float (*cnt)[kTile];      // rows = columns of tile I, columns = of tile J
    float* rm;                // [row][q]: sum of the row over the states of column feature q
    float* cm;                // [p][col]: sum of the column over the states of row feature p
    float* pn;                // per sub-table: total
    int* pdof;                //                dof (0: not valid)
};

__device__ inline PairLds pair_lds(double* base, int sub) {
    PairLds l;
    l.term = reinterpret_cast<double(*)[kTile]>(base);
    l.cnt = reinterpret_cast<float(*)[kTile]>(base);
    l.rm = reinterpret_cast<float*>(base + kTile * kTile);
    l.cm = l.rm + kTile * sub;
    l.pn = l.cm + kTile * sub;
    l.pdof = reinterpret_cast<int*>(l.pn + sub * sub);
    return l;
}

SBE_TILE_HD constexpr size_t pair_lds_bytes(int sub) { return (size_t)kTile * kTile * sizeof(double) + (size_t)(2 * kTile * sub + 2 * sub * sub) * 4; }

// ---- 1. the contraction of the tile pair (I, J) over the n_pad objects of xt: feature-major codes [F][n_pad], padded with
// 255 behind N; S_pad = 1 << log_s
__device__ inline v16f pair_contract(const uint8_t* xt, int64_t n_pad, int F, int log_s, int64_t I, int64_t J, int lane) {
    const int S = 1 << log_s, half = lane >> 5;
    auto column = [&](int64_t tile, const uint8_t*& base, uint32_t& s4) {
        const int64_t col = tile * kTile + (lane & 31);
        int64_t f = col >> log_s;
        uint32_t s = (uint32_t)(col & (S - 1));
        if (f >= F) { f = 0; s = 0x40u; }
        base = xt + f * n_pad + 32 * half;
        s4 = s * 0x01010101u;
    };
    const uint8_t *pa, *pb;
    uint32_t sa, sb;
    column(I, pa, sa);
    column(J, pb, sb);
    v16f acc = {};
    for (int64_t n0 = 0; n0 < n_pad; n0 += kPad) {
        const LaneCodes ca = load_codes(pa + n0), cb = load_codes(pb + n0);
#pragma unroll
        for (int u = 0; u < kRound; ++u) {
            const v8i a = fp4_operand(ca.q[2 * u], ca.q[2 * u + 1], sa);
            const v8i b = fp4_operand(cb.q[2 * u], cb.q[2 * u + 1], sb);
            acc = mfma_fp4(a, b, acc);
        }
    }
    return acc;
}

// ---- 2. and 3.: from the accumulator to the Pearson terms in l.term, with l.pn and l.pdof per sub-table.  Every lane of the
// wave calls it; it ends behind a barrier, so the terms can be read at once.  (The caller keeps a barrier between the last
// read of the terms and the next call: the counts go where the terms lie.)
__device__ inline void pair_terms(const PairLds& l, const v16f& acc, int log_s, int lane) {
    const int S = 1 << log_s, sub = kTile >> log_s, half = lane >> 5;      // states per feature (padded), features per tile edge
    for_acc_entries(acc, half, lane & 31, [&](int row, int col, float v) { l.cnt[row][col] = v; });
    __syncthreads();

    // ---- 2. margins along both tile axes, then total, R, C and dof per sub-table
    for (int idx = lane; idx < kTile * sub; idx += 64) {
        const int row = idx / sub, q = idx - row * sub;
        float s = 0.f;
        for (int b = 0; b < S; ++b) s += l.cnt[row][q * S + b];
        l.rm[row * sub + q] = s;
        const int p = idx / kTile, col = idx - p * kTile;
        s = 0.f;
        for (int a = 0; a < S; ++a) s += l.cnt[p * S + a][col];
        l.cm[p * kTile + col] = s;
    }
    __syncthreads();
    for (int idx = lane; idx < sub * sub; idx += 64) {
        const int p = idx / sub, q = idx - p * sub;
        float n = 0.f;
        int R = 0, C = 0;
        for (int a = 0; a < S; ++a) {
            const float r = l.rm[(p * S + a) * sub + q];
            n += r;
            R += r > 0.f;
            C += l.cm[p * kTile + q * S + a] > 0.f;
        }
        l.pn[idx] = n;
        l.pdof[idx] = (R > 1 && C > 1) ? (R - 1) * (C - 1) : 0;
    }
    __syncthreads();

    // ---- 3. the Pearson terms (each lane takes its 16 counts out of the shared buffer before the terms go in)
    float obs[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) obs[k] = l.cnt[2 * k + half][lane & 31];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int row = 2 * k + half, col = lane & 31, p = row >> log_s, q = col >> log_s;
        const float r = l.rm[row * sub + q], c = l.cm[p * kTile + col];
        const int dof = l.pdof[p * sub + q];
        double v = 0.0;
        if (dof > 0 && r > 0.f && c > 0.f) {
            const double o = (double)obs[k];
            const double e = (double)r * (double)c / (double)l.pn[p * sub + q];
            double oc = o;
            if (dof == 1) {                              // Yates: O + sign(E - O) min(0.5, |E - O|)
                const double d = e - o;
                const double sgn = d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0);
                oc = o + fmin(0.5, fabs(d)) * sgn;
            }
            const double diff = oc - e;
            v = diff * diff / e;
        }
        l.term[row][col] = v;
    }
    __syncthreads();
}

// ---- 4. the statistic of sub-table (p, q): its terms summed a major, b minor
__device__ inline double pair_statistic(const PairLds& l, int p, int q, int S) {
    double stat = 0.0;
    for (int a = 0; a < S; ++a)
#pragma unroll 4
        for (int b = 0; b < S; b += 2) {           // (S is even; the reads run ahead, the adds keep their order)
            const double t0 = l.term[p * S + a][q * S + b], t1 = l.term[p * S + a][q * S + b + 1];
            stat += t0;
            stat += t1;
        }
    return stat;
}

// ---- the host side of a data set: what sbe_assoc_compute and sbe_pairppc_set_data check before any device call ---------
// the shape and the state counts against the SBE_ASSOC_MAX_* limits; s_max: the largest state count
template <class H>
int pair_check_shape(H* h, int64_t N, int64_t F, const int32_t* n_states, int& s_max) {
    if (N < 1 || N > SBE_ASSOC_MAX_OBJECTS)
        return fail(h, SBE_ERR_ARG, "n_objects=%lld out of range [1, %d] (2^24: counts are exact in the f32 accumulator up to there)",
                     (long long)N, SBE_ASSOC_MAX_OBJECTS);
    if (F < 1 || F > SBE_ASSOC_MAX_FEATURES)
        return fail(h, SBE_ERR_ARG, "n_features=%lld out of range [1, %d] (the [F][F] outputs take 25 bytes per entry)",
                     (long long)F, SBE_ASSOC_MAX_FEATURES);
    if (N * F > SBE_ASSOC_MAX_CODES)
        return fail(h, SBE_ERR_ARG, "n_objects * n_features = %lld exceeds the limit of %lld (2^31) codes", (long long)(N * F),
                     (long long)SBE_ASSOC_MAX_CODES);
    s_max = 1;
    for (int64_t f = 0; f < F; ++f) {
        if (n_states[f] < 1 || n_states[f] > SBE_ASSOC_MAX_STATES)
            return fail(h, SBE_ERR_ARG, "n_states[%lld]=%d out of range [1, %d] (this unit's limit: a 32 x 32 tile holds whole pairs)",
                         (long long)f, n_states[f], SBE_ASSOC_MAX_STATES);
        s_max = std::max(s_max, (int)n_states[f]);
    }
    return SBE_OK;
}

// the codes x [N][F], checked and turned feature-major into xt [F][n_pad], padded with NA
template <class H>
int pair_feature_major(H* h, const uint8_t* x, int64_t N, int64_t F, const int32_t* n_states, int64_t n_pad, std::vector<uint8_t>& xt) {
    xt.assign((size_t)(F * n_pad), (uint8_t)SBE_ASSOC_NA);
    for (int64_t i0 = 0; i0 < N; i0 += kStep) {        // (blocks of objects: the block's rows stay in cache, the writes are contiguous)
        const int64_t i1 = std::min(N, i0 + kStep);
        for (int64_t f = 0; f < F; ++f) {
            const int32_t ns = n_states[f];
            uint8_t* dst = xt.data() + (size_t)(f * n_pad);
            for (int64_t i = i0; i < i1; ++i) {
                const uint8_t c = x[i * F + f];
                if (c != SBE_ASSOC_NA && c >= ns)
                    return fail(h, SBE_ERR_DATA, "x[%lld][%lld]=%d is neither below n_states[%lld]=%d nor %d (not observed)", (long long)i,
                                 (long long)f, (int)c, (long long)f, ns, SBE_ASSOC_NA);
                dst[i] = c;
            }
        }
    }
    return SBE_OK;
}

// log2 of S_pad: the next power of two >= s_max, at least 2
inline int pair_log_s(int s_max) {
    int log_s = 1;
    while ((1 << log_s) < s_max) ++log_s;
    return log_s;
}

}  // namespace
