/* sbe_loopred.h -- C ABI of the leave-one-out predictive of every observed cell on the device: had this cell not been observed,
 * what would the fitted model have predicted for it?
 *
 * sbe_predict.h puts the logged samples back on the data, in sample: the cell's own value shaped the draws that predict it.
 * sbe_elpd.h computes, per observed cell, the Pareto-smoothed importance weights that remove that influence, and keeps only
 * their log score.  This unit keeps the weights and runs the samples past them a second time:
 *     p_loo[n][f][s] = sum_t w_t(n, f) m_t[n][f][s]
 * with m_t the mixture row of sbe_predict.h and w_t the normalised PSIS weight of sample t for the cell.
 *
 * The data, a sample's inputs, k_t(n), wn, m and the validation are sbe_predict.h's, word for word: codes, groups, n_groups, K;
 * per sample clusters [K][N], weights [F][C], tables [R][F][S]; the same limits and the same SBE_ERR_DATA order.  The observed
 * cells (codes != 255) are the unit's columns, in n F + f order, M of them.  With T samples in all, three phases
 * (tests/_loopred_oracle.py restates them in fp64; DESIGN.md section 26 states them):
 *   1. rows     sbe_loopred_add, any number of calls: per sample and observed cell lik = float32(m[x]), stored column-major on the
 *               device, sbe_predict.h's lik bit for bit; nothing is copied back.
 *   2. weights  sbe_loopred_weights: per column PSIS over the T rows exactly as sbe_elpd_compute does it (arviz.psislw, reff = 1:
 *               min and check, cutoff, tail sort, _gpdfit, _gpinv, clamp at 0).  With x'_t the smoothed, clamped value of
 *               sample t and A = sum_t exp(x'_t) (a fixed tree), w_t = exp(x'_t) / A in float64, kept per (column, sample).
 *               Tail positions among equal lik follow the oracle's stable argsort: in ascending x the earlier sample first.
 *               Per column: loo_i and k_i (sbe_elpd_compute's bits) and n_eff = 1 / sum_t w_t^2 (a fixed tree).
 *               An observed cell with m[x] == 0, or not finite, in any sample is SBE_ERR_DATA here, naming the first such
 *               (cell, sample): its raw weight would be infinite.
 *   3. accumulate  sbe_loopred_accumulate: the same samples a second time, in the same order; t0 is the index of the call's
 *               first sample and the calls cover 0 .. T in order without gaps (SBE_ERR_STATE otherwise).  Per observed cell
 *               and state p_loo += w_t m_t[s]: the product rounded, then added, in float64, in sample order, a cell's
 *               accumulators held by one thread for the whole call -- sbe_predict.h's rule, so the sums are bit-identical for
 *               every split of the samples and every feature tile.  The samples are validated again, and a sample whose lik
 *               row differs from the stored one is SBE_ERR_DATA, naming the sample (a cheap guard against other samples);
 *               the call then leaves the sums as they were.  NA cells get nothing.
 * Everything is conditional on the logged effect draws, as in sbe_predict.h: leave-one-out removes the cell's influence on
 * the weighting of the samples, not on a draw already made.  This is not the LikelihoodLogger's collapsed form.
 *
 * Conventions are those of sbe_predict.h and sbe_engine.h: every function returns SBE_OK (0) or an SBE_ERR_* code with the
 * message in sbe_loopred_last_error(); nothing throws across the boundary; arguments are checked before any device call; calls
 * are synchronous; the caller owns every host buffer.  The symbols are exported by the same library as the engine's.
 */
#ifndef SBE_LOOPRED_H
#define SBE_LOOPRED_H

#include <stdint.h>

#include "sbe_elpd.h"
#include "sbe_predict.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sbe_loopred sbe_loopred;

#define SBE_LOOPRED_ABI_VERSION 1

/* limits (SBE_ERR_ARG beyond them); the shape's are sbe_predict.h's */
#define SBE_LOOPRED_MAX_SAMPLES SBE_ELPD_MAX_SAMPLES         /* T: the capacity of the store, in samples                        */
#define SBE_LOOPRED_MAX_STORE_BYTES (1ll << 34)              /* the store of rows and weights: M * capacity * (4 + 8) bytes     */
#define SBE_LOOPRED_MAX_STAGE_BYTES SBE_PREDICT_MAX_STAGE_BYTES   /* the samples of one add / accumulate call on the device    */
#define SBE_LOOPRED_MAX_TILE SBE_PREDICT_MAX_TILE

int sbe_loopred_abi_version(void);
/* the message of the last failed call on `h` (NULL: of the last failed call of this thread) */
const char* sbe_loopred_last_error(const sbe_loopred* h);

int sbe_loopred_create(sbe_loopred** out, int device);
int sbe_loopred_destroy(sbe_loopred* h);
/* device time of the kernels of the last add, weights or accumulate call (HIP events), in ms */
int sbe_loopred_last_kernel_ms(const sbe_loopred* h, float* ms_out);

/* Device bytes of the store for n_observed columns and `capacity` samples: float32 rows and float64 weights.  -1 if either
 * is negative or capacity is beyond SBE_LOOPRED_MAX_SAMPLES.  Beyond SBE_LOOPRED_MAX_STORE_BYTES set_data refuses the shape. */
int64_t sbe_loopred_store_bytes(int64_t n_observed, int64_t capacity);
/* Device bytes one sample of an add or accumulate call takes while the call runs: sbe_predict_sample_bytes(.., with_lik = 1).
 * 0 for a shape beyond the limits. */
int64_t sbe_loopred_sample_bytes(int64_t n_objects, int64_t n_features, int n_states, int n_components, int n_clusters, int n_rows);
/* largest T whose column sbe_loopred_weights stages in LDS; longer columns are read from global memory in every pass (the
 * tail's keys carry the sample index here, so this is somewhat below sbe_elpd_lds_max_samples) */
int64_t sbe_loopred_lds_max_samples(void);

/* The data of sbe_predict_set_data and the capacity of the store in samples, 1 .. SBE_LOOPRED_MAX_SAMPLES.  The store is
 * emptied and the sums are zeroed.  Device memory only grows. */
int sbe_loopred_set_data(sbe_loopred* h, int64_t n_objects, int64_t n_features, int n_states, int n_components, int n_clusters,
                         const uint8_t* codes, const uint8_t* groups, const int* n_groups, int64_t capacity);
/* Forget the rows, the weights and the sums, keep the data and the capacity. */
int sbe_loopred_reset(sbe_loopred* h);

/* Phase 1.  n samples as in sbe_predict_accumulate; n * sbe_loopred_sample_bytes <= SBE_LOOPRED_MAX_STAGE_BYTES and the rows
 * stored so far + n <= capacity (SBE_ERR_ARG beyond either).  On SBE_ERR_DATA nothing was stored.  A call after
 * sbe_loopred_weights discards the weights and the sums: phase 2 comes again. */
int sbe_loopred_add(sbe_loopred* h, int64_t n, const uint8_t* clusters, const double* weights, const double* tables);
/* Phase 2.  loo_i, k_i, n_eff: float64 [M] each, in column order.  SBE_ERR_STATE with fewer than SBE_ELPD_MIN_SAMPLES rows.
 * Zeroes the sums: phase 3 starts at t0 = 0. */
int sbe_loopred_weights(sbe_loopred* h, double* loo_i, double* k_i, double* n_eff);
/* Phase 3.  The samples [t0, t0 + n) of phase 1. */
int sbe_loopred_accumulate(sbe_loopred* h, int64_t t0, int64_t n, const uint8_t* clusters, const double* weights, const double* tables);
/* p_loo float64 [N][F][S] (zero at NA cells; may be NULL); *n_samples_out: the samples accumulated since phase 2 (the sums
 * are complete once that is T). */
int sbe_loopred_read(sbe_loopred* h, double* p_loo, int64_t* n_samples_out);

/* Test hooks, not part of what a caller needs.  The features of a workgroup's tile, as sbe_predict_set_feature_tile: the
 * results do not depend on it, bit for bit. */
int sbe_loopred_set_feature_tile(sbe_loopred* h, int features);
/* The store as it stands, column-major and compact: lik float32 [M][T], w float64 [M][T] (either may be NULL; w needs phase 2). */
int sbe_loopred_get_store(sbe_loopred* h, float* lik, double* w);

#ifdef __cplusplus
}
#endif

#endif /* SBE_LOOPRED_H */
