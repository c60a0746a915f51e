/* sbe_ppc.h -- C ABI of the posterior predictive check on the device: per logged sample one replicated data set drawn from
 * the fitted model, and a deviance discrepancy of the replicate next to the same discrepancy of the data, per feature and per
 * object, with the state counts of the replicate.
 *
 * The posterior predictive unit (sbe_predict.h) puts the fitted model back on the data as probabilities.  This unit asks
 * whether the data look like what the fitted model would produce: a draw y_t[n][f] from the mixture row m_t[n,f,.] of every
 * cell that has a code (the row simulate_features draws from, sbayes/simulation.py:207-255), the discrepancy
 * d = -2 log m_t[.] at the drawn and at the observed state, and its sums.  A posterior predictive p-value is the share of
 * samples whose replicated sum exceeds the observed one (sbayes_amd/ppc.py computes it on the host).  Given the logged effect
 * draws these p-values are conservative: they concentrate around 1/2 more than a uniform variable would, so a small one is
 * stronger evidence than its size says and a moderate one is no proof of fit.
 *
 * The contract (tests/_ppc_oracle.py restates it in fp64; DESIGN.md section 22 states it):
 *   data, a sample:   those of sbe_predict.h, word for word: codes uint8 [N][F], 255 = NA; groups uint8 [C-1][N] with
 *                     n_groups; K clusters; a sample is clusters uint8 [K][N], weights float64 [F][C], tables float64
 *                     [R][F][S].  The limits are SBE_PREDICT_*'s (the bound on the accumulators' bytes included).
 *   draw index:       sample t of a call has the global draw index tau = first_draw + t.
 *   per cell (n, f) with a code x != 255, per sample:
 *     wn, m[s]        exactly sbe_predict.h's operations in its order: the normalising sum over c in order, one division,
 *                     m[s] = sum_c wn_c table_c[s] with c in order, every product rounded, then added; no FMA.
 *     cdf_s           = m[0] + .. + m[s] in index order, float64;  total = cdf_{S-1}.
 *     skipped         if total is not > 0 the cell is skipped for this sample: y = 255, it adds to no sum, n_skipped += 1.
 *     u               uniforms[t][n F + f] if the caller passed uniforms, else philox_uniform(seed, tau, n F + f) (Philox4x32-10,
 *                     counter (i_lo, i_hi, tau_lo, tau_hi), key (seed_lo, seed_hi), 53 bits of the first two words).
 *     v               = u * total, one rounding.
 *     y               = #{s : cdf_s <= v}, clamped to the last state with m[s] > 0.  A state of zero mass is never drawn
 *                     (cdf_s > v >= cdf_{s-1} implies m[s] > 0); the clamp only acts when u * total rounds up to total.
 *     d_obs, d_rep    = -2 log m[x] (+inf where m[x] = 0) and -2 log m[y], float64, the device library's log.
 *   outputs, per sample (every pointer may be NULL):
 *     y_rep uint8 [n][N][F]          NA and skipped cells are 255: the replicate has the data's missingness
 *     dev_feature float64 [n][2][F]  sum over n of d_obs, of d_rep
 *     dev_object float64 [n][2][N]   sum over f of d_obs, of d_rep
 *     count_rep int32 [n][F][S]      the objects that drew state s
 *     n_skipped int64                for the call
 *   sums:             no floating-point atomics.  Every cell writes its two d values (+0.0 for a cell without a code and for a
 *                     skipped one), and two kernels add them in trees that the shape alone fixes.  dev_feature[t][.][f]: 16
 *                     lanes, lane j adds the objects j, j + 16, .. in order onto 0, then the lanes are added in order 0 .. 15
 *                     onto lane 0's sum.  dev_object[t][.][n]: 64 lanes, lane j adds the features j, j + 64, .. in order onto
 *                     0, then the lanes are folded by xor exchanges at distances 32, 16, .. 1.  The observed and the replicated
 *                     sum run over the same cells in the same order: a replicate equal to the data gives equal bits.  The
 *                     bits of every output are a function of the inputs alone: not of the feature tile, not of how the
 *                     samples are split across calls (first_draw continued), not of the call.  count_rep uses integer atomics.
 *   uniforms:         float64 [n][N F], each in [0, 1): the route for a caller's own generator and for range tests.  Every
 *                     entry is validated, whether its cell has a code or not.
 *   validation:       on the device, before anything is written.  SBE_ERR_DATA names the first offender -- by sample, then
 *                     in the order of the list, then by position: the six kinds of sbe_predict.h in its order, then (7) a
 *                     uniform outside [0, 1) or not finite.  A refused call has written none of the outputs.
 * The handle holds the data only; there are no accumulators, so first_draw makes the split explicit.
 *
 * Conventions are those of sbe_engine.h: every function returns SBE_OK (0) or an SBE_ERR_* code with the message in
 * sbe_ppc_last_error(); nothing throws across the boundary; arguments are checked before any device call; calls are
 * synchronous; the caller owns every host buffer.  The symbols are exported by the same library as the engine's.
 */
#ifndef SBE_PPC_H
#define SBE_PPC_H

#include <stdint.h>

#include "sbe_engine.h"
#include "sbe_predict.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sbe_ppc sbe_ppc;

#define SBE_PPC_ABI_VERSION 1

/* limits (SBE_ERR_ARG beyond them): the shape's are SBE_PREDICT_MAX_STATES, _COMPONENTS, _ROWS, _OBJECTS, _FEATURES, _ACC_BYTES */
#define SBE_PPC_MAX_STAGE_BYTES SBE_PREDICT_MAX_STAGE_BYTES   /* what one check call holds on the device: n * sbe_ppc_sample_bytes */
#define SBE_PPC_MAX_TILE SBE_PREDICT_MAX_TILE                 /* features per tile (the test hook)                                */

int sbe_ppc_abi_version(void);
/* the message of the last failed call on `h` (NULL: of the last failed call of this thread) */
const char* sbe_ppc_last_error(const sbe_ppc* h);

int sbe_ppc_create(sbe_ppc** out, int device);
int sbe_ppc_destroy(sbe_ppc* h);
/* device time of the kernels of the last check call (preparation, validation, draws and sums; HIP events), in ms */
int sbe_ppc_last_kernel_ms(const sbe_ppc* h, float* ms_out);

/* Device bytes one sample of a check call takes while the call runs: its cluster rows, weights, tables and cluster ids as in
 * sbe_predict_sample_bytes, the two d values of every cell (16 N F), its sums (16 F + 16 N) and counts (4 F S), and, with the
 * flags, its replicate (N F) and its uniforms (8 N F).  0 for a shape beyond the limits. */
int64_t sbe_ppc_sample_bytes(int64_t n_objects, int64_t n_features, int n_states, int n_components, int n_clusters, int n_rows, int with_y_rep,
                             int with_uniforms);

/* The data, as sbe_predict_set_data takes it.  SBE_ERR_DATA names the first code or group index out of range.  Device
 * memory only grows. */
int sbe_ppc_set_data(sbe_ppc* h, int64_t n_objects, int64_t n_features, int n_states, int n_components, int n_clusters, const uint8_t* codes,
                     const uint8_t* groups, const int* n_groups);
/* n samples with the draw indices first_draw .. first_draw + n - 1: clusters uint8 [n][K][N], weights float64 [n][F][C],
 * tables float64 [n][R][F][S]; uniforms float64 [n][N F] or NULL (then Philox under `seed`).  Outputs, each may be NULL:
 * y_rep uint8 [n][N][F], dev_feature float64 [n][2][F], dev_object float64 [n][2][N], count_rep int32 [n][F][S],
 * *n_skipped_out.  n >= 0, first_draw >= 0 and n * sbe_ppc_sample_bytes(.., y_rep != NULL, uniforms != NULL) <=
 * SBE_PPC_MAX_STAGE_BYTES (SBE_ERR_ARG beyond: split the samples across calls and continue first_draw, no bit depends on the
 * split).  Host blocks move in pieces of at most 64 MiB.  SBE_ERR_STATE before sbe_ppc_set_data.  On SBE_ERR_DATA no output
 * was written. */
int sbe_ppc_check(sbe_ppc* h, int64_t n, int64_t first_draw, uint64_t seed, const uint8_t* clusters, const double* weights, const double* tables,
                  const double* uniforms, uint8_t* y_rep, double* dev_feature, double* dev_object, int32_t* count_rep, int64_t* n_skipped_out);
/* A test hook, as sbe_predict_set_feature_tile: the features of a workgroup's tile; 0: the default, planned from the shape.
 * SBE_ERR_ARG, at the next check, if the tile's slice of a sample's tables does not fit the LDS.  No output depends on it. */
int sbe_ppc_set_feature_tile(sbe_ppc* h, int features);

#ifdef __cplusplus
}
#endif

#endif /* SBE_PPC_H */
