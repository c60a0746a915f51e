// sbe_mixture_mfma.hip.h -- pieces of the matrix-pipe kernel of the batched group-tuple form (sbe_mixture_mfma.hip:
// k_mixture_tuple_mfma): fragment types, the block shape, the table-driven log, the tuple metadata, phase 0 of a block (metadata,
// log table and the A fragments -- the indicator image [tid == t] of the block's slots -- into LDS) and the descriptors of the
// shared-operand epilogue.
#pragma once
#include "sbe_mixture.hip.h"

namespace sbe {

typedef int v4i_t __attribute__((ext_vector_type(4)));
typedef int v8i_t __attribute__((ext_vector_type(8)));
typedef float v16f_t __attribute__((ext_vector_type(16)));
typedef __attribute__((address_space(3))) const v4i_t lds_cv4i_t;

constexpr int kMfmaSlots = 16;          // slots per block in the narrow form (<= 8 tuples); wide forms: 4 (<= 32 tuples), 2 (<= 64)
constexpr int kMfmaThreads = kMfmaWaves * kWave;

// Table-driven log for this kernel's epilogue, G chains interleaved: log v = k ln2 + log c_i + log1p(r), r = m / c_i - 1, with
// its own FINER table (kFineLogEntries = 1024 intervals of the mantissa m in [1, 2): {RN(1/c_i) / 2, log c_i}, built by ensure_xt) so
// that |r| <= 2^-11 (2^-10 in interval 0) and the series stops after r^4: first dropped term r^5 / 5 <= 6e-18 per log (2e-16 in
// interval 0).  v_fma_f64 is the dearest instruction of the epilogue (tools/probe/valu_rates.hip: 6.5 cycles against 4.0 for
// 32-bit integer work at two waves per SIMD): against the 128-entry / r^5 form this is one FMA fewer per entry.
// The binary exponent is NOT folded in here: it is returned as an integer and summed exactly, count-weighted, by the caller (one
// v_mad_i32_i24 instead of a conversion and an FMA per entry; k ln2 is applied once per accumulator at the end).  So that the
// two sums never cancel, mantissas from sqrt(2) on (table index >= kFineLogSplit) count as m / 2 with k + 1 -- the exponent comes
// from hi + kFineLogCarry, which carries exactly there, and their table rows hold log(c_i / 2) -- so a probability in [0.707, 1)
// has k = 0 and a small negative mantissa part; the centres of the first and the last interval are 1 and 2 (log exactly 0):
// log 1 = 0 exactly, and for v = 1 - eps the result is log1p(-eps) to 1e-13 relative (a state that every table entry gives
// probability ~1 has a log-likelihood of ~0, which the reference gets to its own rounding: tools/fuzz_gpu.py checks to
// 1e-10 relative + 1e-16 per observation, and caught a first form that summed k ln2 and log m apart without the split:
// 2e-12 off at a log-likelihood of 1e-5).
constexpr int kFineLogSplit = 424;                                        // 1 + 424/1024 = 1.4140625 ~ sqrt(2)
constexpr uint32_t kFineLogCarry = 0x00100000u - ((uint32_t)kFineLogSplit << 10);
// (round 6: the exponent comes back BIASED -- (hi + carry) >> 20, no "- 1023" per entry: the caller takes 1023 x the column's
//  object count off the integer sum once per lane -- and the mantissa's high word is one v_bfi_b32 with the mask in an SGPR and the
//  exponent pattern in a VGPR instead of v_and + v_or with two literals: two vector instructions fewer per table entry.)
constexpr int kFineLogBias = 1023;
template <int G>
__device__ __forceinline__ void tab_log4_n(const double (&v)[G], double (&out)[G], int (&kexp)[G], uint32_t tab, uint32_t one_hi /* 0x3FF00000 in a VGPR */) {
    f64x2_t e[G];
    double m[G], r[G], q[G];
    uint32_t mant_mask = 0x000FFFFFu;
    asm volatile("" : "+s"(mant_mask));                                          // (kept in an SGPR: v_bfi_b32 takes no literal)
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const uint32_t hi = (uint32_t)__double2hiint(v[g]);
        e[g] = *(lds_cf64x2_t*)(uintptr_t)(tab + ((hi >> 6) & 0x3FF0u));        // entry (hi >> 10) & 1023
        uint32_t mh;
        asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(mh) : "s"(mant_mask), "v"(hi), "v"(one_hi));   // (hi & 0xFFFFF) | 0x3FF00000
        m[g] = __hiloint2double((int)mh, __double2loint(v[g]));
        kexp[g] = (int)((hi + kFineLogCarry) >> 20);                              // biased by kFineLogBias
    }
    // log1p(r) to r^4 in s = r / 2 (the table holds 1 / (2 c), so s comes out of the first FMA):
    //     r - r^2/2 + r^3/3 - r^4/4 = s (2 + s (-2 + s (8/3 - 4 s)))
    // Every constant but 8/3 is an inline operand, so the chain is five v_fma_f64 and nothing else (the Horner form in r needs
    // two constants in one instruction: a register move per entry, and a separate r^2 and final add).
#pragma unroll
    for (int g = 0; g < G; ++g) r[g] = fma(m[g], e[g].x, -0.5);               // s
#pragma unroll
    for (int g = 0; g < G; ++g) q[g] = fma(r[g], -4.0, 8.0 / 3.0);
#pragma unroll
    for (int g = 0; g < G; ++g) q[g] = fma(r[g], q[g], -2.0);
#pragma unroll
    for (int g = 0; g < G; ++g) q[g] = fma(r[g], q[g], 2.0);
#pragma unroll
    for (int g = 0; g < G; ++g) out[g] = fma(r[g], q[g], e[g].y);
}

// per (slot of the block, tuple): byte offsets of the tuple's probability rows inside the probs array and of its
// pattern's weight rows inside the wpat array
template <int CT>
struct __attribute__((aligned(CT <= 1 ? 8 : (CT <= 3 ? 16 : 32)))) TupleMeta {
    uint32_t woff;
    uint32_t goff[CT];
};

// Phase 0 of a block (all kMfmaThreads threads call it; the caller's barrier follows): tuple metadata, log table, A fragments.
// `slot_of(sl)`: absolute slot of the block's sl-th slot, or -1; `slot_mine` = slot_of(threadIdx.x % SL), the slot of every
// id unit of this thread (the thread count is a multiple of SL), looked up once by the caller.  LDS: log table at tab_off
// (= 0), A fragments from a_off, metadata at `meta`.
// SL = slots per block (16 / 4 / 2): an M tile's 32 rows are 32 / SL tuples x SL slots, row = (tuple in tile) * SL + slot; the
// block holds TPB = MT * 32 / SL tuples.
// META = false: no per-tuple metadata (the shared-operand epilogue reads its own descriptors: mfma_shared_desc).
template <int MT, int CT, typename SlotOf, int SL = kMfmaSlots, bool META = true>
__device__ __forceinline__ void mfma_phase0(unsigned char* lds_raw, const MfmaMixParams& p, const SlotOf& slot_of, uint32_t tab_off,
                                            uint32_t a_off, TupleMeta<CT>* meta, int KBp, int slot_mine) {
    typedef TupleMeta<CT> Meta;
    constexpr int TPT = 32 / SL, TPB = MT * TPT;                  // tuples per M tile / per block
    static_assert(SL == 16 || SL == 4 || SL == 2, "slots per block");
    static_assert(kMfmaThreads % SL == 0, "a thread's id units all belong to one slot");
    // ---- phase 0: tuple metadata, log table, A fragments ------------------------------------------------------------
    // Offsets of a tuple that is not there (another slot's tuple, the padding tuple of an odd KT, a slot beyond the batch)
    // and of a component the tuple has no group in point at the rows of ONES behind the two arrays: no observation is
    // counted on the former (and log C is an ordinary number), the normalised weight of the latter is exactly 0.
    // Every global load of the phase is ASKED FOR FIRST -- the tuple ids of this thread's first units, its share of the log table,
    // the tuple's pattern and groups (unconditionally: the rows exist for every tuple index) -- and consumed afterwards: one round
    // trip to L2 / HBM instead of three or four dependent ones at the start of every block (round 6).
    auto meta_of = [&](int slot, int t, uint32_t pat, const uint32_t (&g)[CT]) -> Meta {
        Meta md;
        md.woff = p.wpat_ones_off;
#pragma unroll
        for (int c = 0; c < CT; ++c) md.goff[c] = p.probs_ones_off;
        if (slot >= 0 && t < p.KT && pat != 0xFFu) {
            md.woff = (uint32_t)(((int64_t)slot * p.wpat_stride + (int64_t)pat * p.F * CT) * 4);
#pragma unroll
            for (int c = 0; c < CT; ++c)
                if ((int)g[c] < p.Gtot) md.goff[c] = (uint32_t)(((int64_t)slot * p.probs_stride + (int64_t)g[c] * p.FS) * 4);
        }
        return md;
    };
    // one unit = the 32 tuple ids of (slot sl, lane half h of k-block kb: 32 objects) -> the 2 MT indicator pieces (16 bytes =
    // 32 nibbles each).  UB units' ids are asked for together.
    // Up to 8 tuples per block (PERM): an id byte is 0..7 -- the host numbers a slot's tuples densely and the launch's KT is the
    // largest count among its slots (derive_tuples / update_patterns_and_tuples, plan_mixture), so KT <= TPB <= 8 bounds every
    // id of the launch -- and v_perm_b32 with the id word as selector looks four objects up at once in an 8-byte table whose
    // byte t is 0x02 (1.0 in e2m1) and whose other bytes are 0: selector 0..3 takes a byte of the low table word, 4..7 of
    // the high one, 12 the constant 0x00 (13 and above would give 0xFF, 8..11 a replicated sign bit: never ids here).  The
    // filler for objects beyond Np and slots that are not there is therefore 12 in every byte.  Wider blocks compare bytes.
    constexpr bool PERM = TPB <= 8;
    constexpr uint32_t kNoTuple = PERM ? 0x0C0C0C0Cu : 0xFFFFFFFFu;
    const int n_units = SL * KBp * 2;
    constexpr int UB = 2;
    uint32_t d[UB][8];
    auto load_ids = [&](int u0) {
#pragma unroll
        for (int k = 0; k < UB; ++k) {
            const int u = u0 + k * kMfmaThreads;
            const int n0 = (u / SL) * 32;                  // (u / SL) = kb * 2 + h; u % SL = threadIdx.x % SL
            const int slot = u < n_units ? slot_mine : -1;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                d[k][i] = kNoTuple;                                           // matches no tuple
                if (slot >= 0 && n0 + 4 * i + 4 <= p.Np)
                    d[k][i] = *reinterpret_cast<const uint32_t*>(p.tid + (int64_t)slot * p.tid_stride + n0 + 4 * i);
            }
        }
    };
    auto emit = [&](int u0) {
#pragma unroll
        for (int k = 0; k < UB; ++k) {
            const int u = u0 + k * kMfmaThreads;
            if (u >= n_units) break;
            const int sl = u % SL, hk = u / SL;
            const int kb = hk >> 1, h = hk & 1;
#pragma unroll 8
            for (int t = 0; t < TPB; ++t) {
                uint4 o;
                uint32_t* ov = reinterpret_cast<uint32_t*>(&o);
#pragma unroll
                for (int wv = 0; wv < 4; ++wv) {
                    if constexpr (PERM) {
                        const uint64_t lut = 0x02ull << (8 * (t & 7));
                        const uint32_t lo = __builtin_amdgcn_perm((uint32_t)(lut >> 32), (uint32_t)lut, d[k][2 * wv]);
                        const uint32_t hi = __builtin_amdgcn_perm((uint32_t)(lut >> 32), (uint32_t)lut, d[k][2 * wv + 1]);
                        ov[wv] = lo | (hi << 4);                // the same bytes as below
                        continue;
                    }
                    uint32_t eq[2];
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        const uint32_t x = d[k][2 * wv + q] ^ ((uint32_t)t * 0x01010101u);
                        const uint32_t nz = ((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x;      // bit 7 of a byte: byte != 0
                        eq[q] = (~nz >> 7) & 0x01010101u;
                    }
                    ov[wv] = (eq[0] << 1) | (eq[1] << 5);       // 1.0 = 0x2: low nibbles = objects 8 wv + b, high = 8 wv + 4 + b
                }
                // fragment (m = t / TPT, kb): lane = h * 32 + row, row = (t % TPT) * SL + sl
                const uint32_t fl = (uint32_t)(h * 32 + (t % TPT) * SL + sl);
                *reinterpret_cast<uint4*>(lds_raw + a_off + (((uint32_t)(t / TPT) * (uint32_t)KBp + (uint32_t)kb) * 64u + fl) * 16u) = o;
            }
        }
    };
    const int u_first = (int)threadIdx.x;
    load_ids(u_first);
    constexpr int LT = (2 * kFineLogEntries + kMfmaThreads - 1) / kMfmaThreads;
    double lt[LT];
#pragma unroll
    for (int k = 0; k < LT; ++k) {
        const int i = (int)threadIdx.x + k * kMfmaThreads;
        lt[k] = i < 2 * kFineLogEntries ? reinterpret_cast<const double*>(p.logtab)[i] : 0.0;
    }
    const bool has_meta = META && (int)threadIdx.x < SL * TPB;
    const int m_sl = (int)threadIdx.x / TPB, m_t = (int)threadIdx.x % TPB;
    const int m_slot = has_meta ? slot_of(m_sl) : -1;
    uint32_t m_pat = 0xFFu, m_g[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) m_g[c] = 0xFFFFFFFFu;
    if (m_slot >= 0) {                                   // (m_t < TPB <= kMaxTuples: the rows exist whatever KT is)
        m_pat = p.tuple_p[(int64_t)m_slot * p.tuple_p_stride + m_t];
#pragma unroll
        for (int c = 0; c < CT; ++c) m_g[c] = p.tuple_g[(int64_t)m_slot * p.tuple_g_stride + m_t * kMaxComponents + c];
    }
    if (has_meta) meta[m_sl * TPB + m_t] = meta_of(m_slot, m_t, m_pat, m_g);
    (void)meta;
#pragma unroll
    for (int k = 0; k < LT; ++k) {
        const int i = (int)threadIdx.x + k * kMfmaThreads;
        if (i < 2 * kFineLogEntries) reinterpret_cast<double*>(lds_raw + tab_off)[i] = lt[k];
    }
    for (int u0 = u_first; u0 < n_units; u0 += UB * kMfmaThreads) {
        if (u0 != u_first) load_ids(u0);
        emit(u0);
    }
}

// Descriptors of the shared-operand epilogue (k_mixture_tuple_mfma, SHARE: 16 slots, C = 2).  A slot of that form has, over
// its present tuples, ONE component-1 group and at most two weight patterns a, b; a tuple differs from its neighbours only in
// its component-0 group and in which of the two patterns it has.  Per slot sl of the block (thread sl builds it):
//     sdesc[sl]          = {goff1, woff_a, woff_b, bad}                          (byte offsets into probs / wpat)
//     tdesc[sl * MT + m] = {goff0(2m), goff0(2m + 1), sel(2m), sel(2m + 1)}      (one ds_read_b128 per epilogue step)
// sel = 1: the tuple has pattern b.  A tuple that is not there (pattern 0xFF, t >= KT, a slot beyond the batch) has no counts;
// it keeps its component-0 row on the ones row, as in the per-tuple metadata, and selector 0.  bad != 0: the slot does not
// fit the form (the host's per-slot flag was wrong) -- the block then reports NaN for its slots instead of a wrong number.
// The two halves are called apart: the loads (thread sl's slot and its tuples' pattern and groups) leave with phase 0's first
// loads, the descriptors are built after the A image is written -- one round trip to L2 / HBM for the block, not two.
template <int TPB>
struct SharedDescIn {
    int slot;
    uint32_t pat[TPB], g0[TPB], g1[TPB];
};

// `slot`: thread sl's slot of the block, or -1.  The rows exist for every slot and every tuple index below kMaxTuples, so the
// loads carry no condition (a branch per tuple makes each wait for the one before); what is not there is masked afterwards.
template <int MT, int SL>
__device__ __forceinline__ void mfma_shared_desc_load(const MfmaMixParams& p, int slot, SharedDescIn<MT * 32 / SL>& in) {
    constexpr int TPB = MT * 32 / SL;
    static_assert(SL == 16 && TPB <= kMaxTuples, "the shared-operand form has 16 slots of <= 8 tuples");
    if ((int)threadIdx.x >= SL) return;
    in.slot = slot;
    const uint8_t* const tp = p.tuple_p + (int64_t)max(slot, 0) * p.tuple_p_stride;
    const uint16_t* const tg = p.tuple_g + (int64_t)max(slot, 0) * p.tuple_g_stride;
#pragma unroll
    for (int t = 0; t < TPB; ++t) {                       // (asked for together: one round trip)
        in.pat[t] = tp[t];
        in.g0[t] = tg[t * kMaxComponents + 0];
        in.g1[t] = tg[t * kMaxComponents + 1];
    }
}

template <int MT, int SL>
__device__ __forceinline__ void mfma_shared_desc(const MfmaMixParams& p, const SharedDescIn<MT * 32 / SL>& in, uint4* sdesc, uint4* tdesc) {
    constexpr int TPB = MT * 32 / SL;
    if ((int)threadIdx.x >= SL) return;
    const int sl = (int)threadIdx.x, slot = in.slot;
    const uint32_t (&g0)[TPB] = in.g0, (&g1)[TPB] = in.g1;
    uint32_t pat[TPB];
#pragma unroll
    for (int t = 0; t < TPB; ++t) pat[t] = (slot >= 0 && t < p.KT) ? in.pat[t] : 0xFFu;      // (not there: its groups are not looked at)
    auto goff = [&](uint32_t g) -> uint32_t {
        return (int)g < p.Gtot ? (uint32_t)(((int64_t)slot * p.probs_stride + (int64_t)g * p.FS) * 4) : p.probs_ones_off;
    };
    uint32_t goff1 = p.probs_ones_off, wa = p.wpat_ones_off, wb = p.wpat_ones_off, bad = 0u;
    uint32_t go0[TPB], sel[TPB];
    bool any = false;
#pragma unroll
    for (int t = 0; t < TPB; ++t) {
        go0[t] = p.probs_ones_off; sel[t] = 0u;
        if (pat[t] == 0xFFu) continue;
        go0[t] = goff(g0[t]);
        const uint32_t wo = (uint32_t)(((int64_t)slot * p.wpat_stride + (int64_t)pat[t] * p.F * 2) * 4), g1o = goff(g1[t]);
        if (!any) { any = true; goff1 = g1o; wa = wb = wo; }
        if (g1o != goff1) bad = 1u;
        if (wo != wa) {
            if (wb == wa) wb = wo;
            else if (wo != wb) bad = 1u;
            sel[t] = 1u;
        }
    }
    sdesc[sl] = make_uint4(goff1, wa, wb, bad);
#pragma unroll
    for (int m = 0; m < MT; ++m) tdesc[sl * MT + m] = make_uint4(go0[2 * m], go0[2 * m + 1], sel[2 * m], sel[2 * m + 1]);
}

}  // namespace sbe
