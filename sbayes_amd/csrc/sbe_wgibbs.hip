// sbe_wgibbs.hip -- the deterministic part of sBayes' GibbsSampleWeights._propose (sbayes/sampling/operators.py:597-676) on an
// engine slot's resident state: include/sbe_wgibbs.h.  The contract is written out in tests/_wgibbs_oracle.py
// (DESIGN.md section 15).  Two calls, nothing kept between them:
//   sbe_wgibbs_pair_counts   the source counts of the two components over the objects that have both (k_wgibbs_counts)
//   sbe_wgibbs_step          proposed weights, Metropolis log ratio, decision and output row per feature in ONE launch
//                            (k_wgibbs_step)
// Both kernels take k_source_lh_by_feature's shape (sbe_kernels_operators.hip.h): a block is a tile of 16 features x 64
// object lanes, loads are unconditional (indices clamped) and grouped by level so that they are in flight together,
// every lane adds its objects in a fixed order, the 64 lanes of a feature are combined by a fixed tree.  No float
// atomics: results are bit-identical run to run.  Small inputs and results cross PCIe in the engine's host-mapped I/O
// block, completion comes by flag (wait_done), as in the other latency-bound calls of the engine.
#include "sbe_engine_internal.hip.h"   // the engine object: the slot's resident arrays
#include "../../include/sbe_wgibbs.h"

#include <cmath>

namespace {

constexpr int kWgFT = SBE_WGIBBS_FEATURE_TILE, kWgOL = 1024 / kWgFT, kWgPer = 8;
static_assert(kWgOL == kWave, "one wave of object lanes per feature of the tile");
constexpr size_t kWgMaxLds = (size_t)kWgFT * 64 * kMaxComponents * sizeof(double) + (size_t)kWgOL * kWgFT * sizeof(double);   // 72 KB

// ------------------------------------------------------------------------------------------
// counts[f][0 / 1] = #{n : pattern(n) has i1 and i2, x(n, f) not NA, source(n, f) == i1 / i2}
// (np.sum(source[has_both], axis=0)[:, [i1, i2]], operators.py:649-652).  Integer sums: exact in any order.
// ------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(1024) void k_wgibbs_counts(
    const uint8_t* __restrict__ state, const uint8_t* __restrict__ src, const uint8_t* __restrict__ pid,
    const uint32_t* __restrict__ patbits, int P, int i1, int i2, int32_t* __restrict__ out, int N, int F, int Fp, DoneSig done) {
    __shared__ int32_t part[2][kWgOL][kWgFT];              // 8 KB
    const int fl = threadIdx.x & (kWgFT - 1), ol = threadIdx.x / kWgFT;
    const int f = blockIdx.x * kWgFT + fl;
    const int fc = min(f, F - 1);                          // (clamped: every load below is unconditional)
    const uint32_t need = (1u << i1) | (1u << i2);
    int32_t c1 = 0, c2 = 0;
    for (int n0 = 0; n0 < N; n0 += kWgOL * kWgPer) {
        uint8_t x[kWgPer], sc[kWgPer], pp[kWgPer];
        uint32_t bits[kWgPer];
#pragma unroll
        for (int j = 0; j < kWgPer; ++j) {
            const int n = min(n0 + ol + kWgOL * j, N - 1);
            x[j] = state[(int64_t)n * Fp + fc];
            sc[j] = src[(int64_t)n * Fp + fc];
            pp[j] = pid[n];
        }
#pragma unroll
        for (int j = 0; j < kWgPer; ++j) bits[j] = patbits[min((int)pp[j], P - 1)];
#pragma unroll
        for (int j = 0; j < kWgPer; ++j) {
            const int n = n0 + ol + kWgOL * j;
            const bool counted = n < N && x[j] != kNA && (bits[j] & need) == need;
            c1 += (counted && sc[j] == i1) ? 1 : 0;
            c2 += (counted && sc[j] == i2) ? 1 : 0;
        }
    }
    part[0][ol][fl] = c1;
    part[1][ol][fl] = c2;
    __syncthreads();
    for (int half = kWgOL / 2; half > 0; half >>= 1) {
        if (ol < half) { part[0][ol][fl] += part[0][ol + half][fl]; part[1][ol][fl] += part[1][ol + half][fl]; }
        __syncthreads();
    }
    if (ol == 0 && f < F) { out[2 * f] = part[0][0][fl]; out[2 * f + 1] = part[1][0][fl]; }
    signal_done(done);
}

// The proposed row of one feature, float32 as the reference computes it (operators.py:665-672, util.py:1007): wn[c] for
// c < C, and a2_old.  C <= 8: NumPy's sum of a contiguous row is np_sum_regs' order.
__device__ __forceinline__ void wgibbs_propose_row(const float (&w)[kMaxComponents], int C, int i1, int i2, double a2,
                                                   float (&wn)[kMaxComponents], float& a2_old) {
    float w1 = 0.0f, w2 = 0.0f;
#pragma unroll
    for (int c = 0; c < kMaxComponents; ++c) { if (c == i1) w1 = w[c]; if (c == i2) w2 = w[c]; }
    const float w02 = w1 + w2;
    const float n1 = (float)((1.0 - a2) * (double)w02), n2 = (float)(a2 * (double)w02);
    float t[kMaxComponents];
#pragma unroll
    for (int c = 0; c < kMaxComponents; ++c) t[c] = c == i1 ? n1 : (c == i2 ? n2 : (c < C ? w[c] : 0.0f));
    const float tot = np_sum_regs<float, kMaxComponents>(t, C);
#pragma unroll
    for (int c = 0; c < kMaxComponents; ++c) wn[c] = t[c] / tot;
    a2_old = w2 / w02;
}

// coefficient * value with SciPy's xlogy convention: 0 where the coefficient is 0, whatever the value is
__device__ __forceinline__ double coef_log(double coef, double value) { return coef == 0.0 ? 0.0 : coef * value; }

// ------------------------------------------------------------------------------------------
// One launch per step.  Per feature tile:
//   1. thread <-> (pattern, feature of the tile): the old and the new per-pattern normalised weights (normalize_weights,
//      likelihood.py:171-190, float32) and, into LDS, dl[fl][p][c] = log wn_new - log wn_old in float64;
//   2. one sweep over the objects: every lane adds the dl entries of its observations in float64, fixed tree over the lanes;
//   3. one thread per feature: prior and proposal terms, the decision, the output row.
// ------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(1024) void k_wgibbs_step(
    const uint8_t* __restrict__ state, const uint8_t* __restrict__ src, const uint8_t* __restrict__ pid,
    const float* __restrict__ weights /* [F][C] */, const uint32_t* __restrict__ patbits, int P, int i1, int i2,
    const double* __restrict__ a2, const float* __restrict__ u, const double* __restrict__ alpha, const double* __restrict__ beta_ab,
    double prior_temperature, float* __restrict__ weights_out, uint8_t* __restrict__ accept_out, double* __restrict__ log_p_out,
    int N, int F, int C, int Fp, DoneSig done) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* part = reinterpret_cast<double*>(smem);                    // [kWgOL][kWgFT]
    double* dl = part + kWgOL * kWgFT;                                 // [kWgFT][P][C]
    const int f0 = blockIdx.x * kWgFT;
    for (int t = threadIdx.x; t < kWgFT * P; t += 1024) {
        const int tf = t & (kWgFT - 1), p = t / kWgFT;
        const int fc = min(f0 + tf, F - 1);
        const uint32_t bits = patbits[p];
        float w[kMaxComponents], wn[kMaxComponents], mo[kMaxComponents], mn[kMaxComponents], a2_old;
#pragma unroll
        for (int c = 0; c < kMaxComponents; ++c) w[c] = c < C ? weights[(int64_t)fc * C + c] : 0.0f;
        wgibbs_propose_row(w, C, i1, i2, a2[fc], wn, a2_old);
#pragma unroll
        for (int c = 0; c < kMaxComponents; ++c) {
            const bool on = (bits >> c) & 1u;
            mo[c] = c < C ? (on ? w[c] : 0.0f * w[c]) : 0.0f;
            mn[c] = c < C ? (on ? wn[c] : 0.0f * wn[c]) : 0.0f;
        }
        const float to = np_sum_regs<float, kMaxComponents>(mo, C), tn = np_sum_regs<float, kMaxComponents>(mn, C);
#pragma unroll
        for (int c = 0; c < kMaxComponents; ++c)
            if (c < C) dl[((int64_t)tf * P + p) * C + c] = log((double)(mn[c] / tn)) - log((double)(mo[c] / to));
    }
    __syncthreads();
    const int fl = threadIdx.x & (kWgFT - 1), ol = threadIdx.x / kWgFT;
    const int f = f0 + fl;
    const int fc = min(f, F - 1);                          // (clamped: every load below is unconditional)
    const double* dlf = dl + (int64_t)fl * P * C;
    const double nan = __builtin_nan("");
    double acc = 0.0;
    for (int n0 = 0; n0 < N; n0 += kWgOL * kWgPer) {
        uint8_t x[kWgPer], sc[kWgPer], pp[kWgPer];
#pragma unroll
        for (int j = 0; j < kWgPer; ++j) {
            const int n = min(n0 + ol + kWgOL * j, N - 1);
            x[j] = state[(int64_t)n * Fp + fc];
            sc[j] = src[(int64_t)n * Fp + fc];
            pp[j] = pid[n];
        }
#pragma unroll
        for (int j = 0; j < kWgPer; ++j) {
            const int n = n0 + ol + kWgOL * j;
            const double v = dlf[min((int)pp[j], P - 1) * C + min((int)sc[j], C - 1)];
            if (!(n < N) || x[j] == kNA) continue;         // NA (and padding): no term
            acc += sc[j] < C ? v : nan;                    // no source component set: log 0 - log 0
        }
    }
    part[ol * kWgFT + fl] = acc;
    __syncthreads();
    for (int half = kWgOL / 2; half > 0; half >>= 1) {     // fixed tree over the object lanes
        if (ol < half) part[ol * kWgFT + fl] += part[(ol + half) * kWgFT + fl];
        __syncthreads();
    }
    if (ol == 0 && f < F) {
        const double d_lh = part[fl];
        float w[kMaxComponents], wn[kMaxComponents], a2_old;
#pragma unroll
        for (int c = 0; c < kMaxComponents; ++c) w[c] = c < C ? weights[(int64_t)f * C + c] : 0.0f;
        const double a = a2[f];
        wgibbs_propose_row(w, C, i1, i2, a, wn, a2_old);
        double d_prior = 0.0;
#pragma unroll
        for (int c = 0; c < kMaxComponents; ++c)
            if (c < C) d_prior += coef_log(alpha[(int64_t)f * C + c] - 1.0, log((double)wn[c]) - log((double)w[c]));
        const double ao = (double)a2_old;
        const double d_q = coef_log(beta_ab[2 * f] - 1.0, log(ao) - log(a)) + coef_log(beta_ab[2 * f + 1] - 1.0, log1p(-ao) - log1p(-a));
        const double log_p = (d_lh + d_prior + d_q) / prior_temperature;
        const bool accept = (double)u[f] < exp(log_p);     // (a NaN compares false: reject)
#pragma unroll
        for (int c = 0; c < kMaxComponents; ++c)
            if (c < C) weights_out[(int64_t)f * C + c] = accept ? wn[c] : w[c];
        accept_out[f] = accept ? 1 : 0;
        log_p_out[f] = log_p;
    }
    signal_done(done);
}

// what both calls check and prepare: arguments, then the slot's state, then its pattern tables on the device
int wgibbs_ready(sbe_engine* e, int slot, int i1, int i2) {
    if (i1 < 0 || i1 >= e->C || i2 < 0 || i2 >= e->C || i1 == i2)
        return fail(e, SBE_ERR_ARG, "components (%d, %d): two different indices in [0,%d) are needed", i1, i2, e->C);
    Slot& s = e->slots[slot];
    if (!s.groups_set || !s.source_set || !s.weights_set) return fail(e, SBE_ERR_STATE, "slot %d: groups / source / weights not set", slot);
    HIPCHK(e, hipSetDevice(e->device));
    if (s.patterns_dirty) { int rc = upload_patterns_and_weights(e, slot); if (rc) return rc; }
    if (s.patterns.empty() || (int)s.patterns.size() > e->Pmax) return fail(e, SBE_ERR_STATE, "slot %d: no has_components patterns", slot);
    return SBE_OK;
}

}  // namespace

extern "C" {

int sbe_wgibbs_abi_version(void) { return SBE_WGIBBS_ABI_VERSION; }

int sbe_wgibbs_pair_counts(sbe_engine* e, int slot, int i1, int i2, int32_t* counts_out) {
    CHECK_ENGINE(e); CHECK_SLOT(e, slot); CHECK_PTR(e, counts_out);
    int rc = wgibbs_ready(e, slot, i1, i2);
    if (rc) return rc;
    const size_t out_bytes = (size_t)e->F * 2 * sizeof(int32_t);
    rc = ensure_io(e, out_bytes);
    if (rc) return rc;
    const int n_blocks = div_up(e->F, kWgFT);
    const DoneSig done = next_done(e, (unsigned)n_blocks);
    k_wgibbs_counts<<<n_blocks, 1024, 0, e->stream>>>(
        e->d_state, e->d_src + (int64_t)slot * e->N * e->Fp, e->d_pid + (int64_t)slot * e->Np, e->d_patbits + (int64_t)slot * e->Pmax,
        (int)e->slots[slot].patterns.size(), i1, i2, (int32_t*)e->d_io, e->N, e->F, e->Fp, done);
    HIPCHK(e, hipGetLastError());
    rc = wait_done(e, done);
    if (rc) return rc;
    memcpy(counts_out, e->h_io, out_bytes);
    return synced(e);
}

int sbe_wgibbs_step(sbe_engine* e, int slot, int i1, int i2, const double* a2, const float* u, const double* alpha,
                    const double* beta_ab, double prior_temperature, float* weights_out, uint8_t* accept_out, double* log_p_out) {
    CHECK_ENGINE(e); CHECK_SLOT(e, slot); CHECK_PTR(e, a2); CHECK_PTR(e, u); CHECK_PTR(e, alpha); CHECK_PTR(e, beta_ab);
    CHECK_PTR(e, weights_out); CHECK_PTR(e, accept_out);
    if (!(prior_temperature > 0.0) || !std::isfinite(prior_temperature))
        return fail(e, SBE_ERR_ARG, "prior_temperature must be positive and finite");
    int rc = wgibbs_ready(e, slot, i1, i2);
    if (rc) return rc;
    const int F = e->F, C = e->C, P = (int)e->slots[slot].patterns.size();
    // the I/O block: a2 | u | alpha | beta_ab | weights_out | log_p | accept
    const size_t b_a2 = al256((size_t)F * sizeof(double)), b_u = al256((size_t)F * sizeof(float));
    const size_t b_al = al256((size_t)F * C * sizeof(double)), b_ab = al256((size_t)F * 2 * sizeof(double));
    const size_t b_w = al256((size_t)F * C * sizeof(float)), b_lp = al256((size_t)F * sizeof(double));
    const size_t o_u = b_a2, o_al = o_u + b_u, o_ab = o_al + b_al, o_w = o_ab + b_ab, o_lp = o_w + b_w, o_acc = o_lp + b_lp;
    rc = ensure_io(e, o_acc + (size_t)F);
    if (rc) return rc;
    memcpy(e->h_io, a2, (size_t)F * sizeof(double));
    memcpy(e->h_io + o_u, u, (size_t)F * sizeof(float));
    memcpy(e->h_io + o_al, alpha, (size_t)F * C * sizeof(double));
    memcpy(e->h_io + o_ab, beta_ab, (size_t)F * 2 * sizeof(double));
    const size_t lds = (size_t)kWgOL * kWgFT * sizeof(double) + (size_t)kWgFT * P * C * sizeof(double);
    if (lds > kWgMaxLds) return fail(e, SBE_ERR_ARG, "%d patterns x %d components exceed the step kernel's tile", P, C);
    if (lds > ((size_t)32 << 10))
        HIPCHK(e, hipFuncSetAttribute((const void*)k_wgibbs_step, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kWgMaxLds));
    const int n_blocks = div_up(F, kWgFT);
    const DoneSig done = next_done(e, (unsigned)n_blocks);
    k_wgibbs_step<<<n_blocks, 1024, lds, e->stream>>>(
        e->d_state, e->d_src + (int64_t)slot * e->N * e->Fp, e->d_pid + (int64_t)slot * e->Np, e->d_weights + (int64_t)slot * F * C,
        e->d_patbits + (int64_t)slot * e->Pmax, P, i1, i2, (const double*)e->d_io, (const float*)(e->d_io + o_u),
        (const double*)(e->d_io + o_al), (const double*)(e->d_io + o_ab), prior_temperature, (float*)(e->d_io + o_w),
        e->d_io + o_acc, (double*)(e->d_io + o_lp), e->N, F, C, e->Fp, done);
    HIPCHK(e, hipGetLastError());
    rc = wait_done(e, done);
    if (rc) return rc;
    memcpy(weights_out, e->h_io + o_w, (size_t)F * C * sizeof(float));
    memcpy(accept_out, e->h_io + o_acc, (size_t)F);
    if (log_p_out) memcpy(log_p_out, e->h_io + o_lp, (size_t)F * sizeof(double));
    return synced(e);
}

}  // extern "C"
