/* sbe_contrib.h -- C ABI of the per-cluster evidence of the logged samples on the device: for every logged sample, every
 * cluster k and every cell that has a code, the log-likelihood ratio of "the object is in cluster k" against "the object is
 * in no cluster", summed per object (affinity) and, over the cluster's members, per feature (gain).
 *
 * The posterior predictive units (sbe_predict.h, sbe_ppc.h) evaluate the mixture row of a cell under the membership the sample
 * logged.  This unit evaluates the counterfactual rows of the same cell: the object placed in cluster k, for every k, and in no
 * cluster at all.  It is the quantity AlterCluster.compute_cluster_posterior evaluates inside the sampler
 * (sbayes/sampling/operators.py), here after the fact on the logged draws, in log space, for all objects, clusters and samples
 * at once; the reference's lh_a<i> columns (sbayes/sampling/loggers.py:140-142, 239-251) are its sum over a cluster's members,
 * which the reference gets by re-running the collapsed likelihood once per cluster.  Labels must be aligned first (sbe_align.h)
 * for means over samples to refer to one cluster, and a member's affinity is optimistic: the cluster's effect draw was fitted
 * with that member's data (the data are used twice, as in sbe_ppc.h).
 *
 * The contract (tests/_contrib_oracle.py restates it in fp64; DESIGN.md section 24 states it):
 *   data, a sample:   those of sbe_predict.h, word for word: codes uint8 [N][F], 255 = NA; groups uint8 [C-1][N] with
 *                     n_groups; K clusters; a sample is clusters uint8 [K][N], weights float64 [F][C], tables float64
 *                     [R][F][S].  The limits are SBE_PREDICT_*'s (the bound on the accumulators' bytes included).
 *   per sample t, per cell (n, f) with a code x != 255, per cluster k < K (the object's own membership is not used here; it
 *   only selects terms of gain_feature):
 *     a_c             = h[n][c] w[f][c] for c >= 1 (the confounders that apply to n);  a_0 = w[f][0].
 *     wsum1, wsum0    = a_0 + a_1 + .. in index order;  a_1 + a_2 + .. in index order.
 *     w1_c, w0_c      = a_c / wsum1 (c >= 0);  a_c / wsum0 (c >= 1).
 *     m0              = sum_{c >= 1} w0_c table_c[row_c(n)][f][x], c in order, every product rounded, then added; no FMA.
 *     m_k             = w1_0 table[k][f][x] + sum_{c >= 1} w1_c table_c[row_c(n)][f][x], the same order, starting from the
 *                       cluster's term.  For a member of k this is sbe_predict.h's m[x], bit for bit; m0 is its m[x] for an
 *                       object in no cluster.
 *     d[t][k][n][f]   = log m_k - log m0, float64, the device library's log; +inf where m0 = 0.
 *     skipped         a cell with wsum0 not > 0 (no confounder applies) is skipped for all k; a (cell, k) with m_k not > 0 is
 *                     skipped.  A skipped entry is +0.0 and adds 1 to n_skipped.  A cell without a code is +0.0 and not counted.
 *   outputs, per sample (every pointer may be NULL):
 *     affinity float64 [n][K][N]      sum over f of d[t][k][n][f], for every object, member or not
 *     gain_feature float64 [n][K][F]  sum over the objects n in cluster k in sample t of d[t][k][n][f]
 *     n_skipped int64                 for the call
 *   sums:             no floating-point atomics.  Every (k, cell) writes its d, and two kernels add them in trees that the shape
 *                     alone fixes, those of sbe_ppc.h.  affinity[t][k][n]: 64 lanes, lane j adds the features j, j + 64, .. in
 *                     order onto 0, then the lanes are folded by xor exchanges at distances 32, 16, .. 1.  gain_feature[t][k][f]:
 *                     16 lanes, lane j adds the objects j, j + 16, .. in order onto 0, a non-member adding +0.0, then the lanes
 *                     are added in order 0 .. 15 onto lane 0's sum.  The bits of every output are a function of the inputs
 *                     alone: not of the feature tile, not of how the samples are split across calls, not of the call.
 *   validation:       on the device, before anything is written: the six kinds of sbe_predict.h in its order, with its
 *                     messages.  A refused call has written none of the outputs.
 * The handle holds the data only; there are no accumulators.
 *
 * Conventions are those of sbe_engine.h: every function returns SBE_OK (0) or an SBE_ERR_* code with the message in
 * sbe_contrib_last_error(); nothing throws across the boundary; arguments are checked before any device call; calls are
 * synchronous; the caller owns every host buffer.  The symbols are exported by the same library as the engine's.
 */
#ifndef SBE_CONTRIB_H
#define SBE_CONTRIB_H

#include <stdint.h>

#include "sbe_engine.h"
#include "sbe_predict.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sbe_contrib sbe_contrib;

#define SBE_CONTRIB_ABI_VERSION 1

/* limits (SBE_ERR_ARG beyond them): the shape's are SBE_PREDICT_MAX_STATES, _COMPONENTS, _ROWS, _OBJECTS, _FEATURES, _ACC_BYTES */
#define SBE_CONTRIB_MAX_STAGE_BYTES SBE_PREDICT_MAX_STAGE_BYTES   /* what one evaluate call holds on the device: n * sbe_contrib_sample_bytes */
#define SBE_CONTRIB_MAX_TILE SBE_PREDICT_MAX_TILE                 /* features per tile (the test hook)                                      */

int sbe_contrib_abi_version(void);
/* the message of the last failed call on `h` (NULL: of the last failed call of this thread) */
const char* sbe_contrib_last_error(const sbe_contrib* h);

int sbe_contrib_create(sbe_contrib** out, int device);
int sbe_contrib_destroy(sbe_contrib* h);
/* device time of the kernels of the last evaluate call (preparation, validation, cells and sums; HIP events), in ms */
int sbe_contrib_last_kernel_ms(const sbe_contrib* h, float* ms_out);

/* Device bytes one sample of an evaluate call takes while the call runs: its cluster rows, weights, tables and cluster ids as
 * in sbe_predict_sample_bytes(.., 0), the d value of every (cluster, cell) (8 K N F) and its sums (8 K (N + F)).  0 for a shape
 * beyond the limits. */
int64_t sbe_contrib_sample_bytes(int64_t n_objects, int64_t n_features, int n_states, int n_components, int n_clusters, int n_rows);

/* The data, as sbe_predict_set_data takes it.  SBE_ERR_DATA names the first code or group index out of range.  Device
 * memory only grows. */
int sbe_contrib_set_data(sbe_contrib* h, int64_t n_objects, int64_t n_features, int n_states, int n_components, int n_clusters, const uint8_t* codes,
                         const uint8_t* groups, const int* n_groups);
/* n samples: clusters uint8 [n][K][N], weights float64 [n][F][C], tables float64 [n][R][F][S].  Outputs, each may be NULL:
 * affinity float64 [n][K][N], gain_feature float64 [n][K][F], *n_skipped_out.  n >= 0 and n * sbe_contrib_sample_bytes(..) <=
 * SBE_CONTRIB_MAX_STAGE_BYTES (SBE_ERR_ARG beyond: split the samples across calls, no bit depends on the split).  Host blocks
 * move in pieces of at most 64 MiB.  SBE_ERR_STATE before sbe_contrib_set_data.  On SBE_ERR_DATA no output was written. */
int sbe_contrib_evaluate(sbe_contrib* h, int64_t n, const uint8_t* clusters, const double* weights, const double* tables, double* affinity,
                         double* gain_feature, int64_t* n_skipped_out);
/* A test hook, as sbe_predict_set_feature_tile: the features of a workgroup's tile; 0: the default, planned from the shape.
 * SBE_ERR_ARG, at the next evaluate, if the tile's slice of a sample's tables does not fit the LDS.  No output depends on it. */
int sbe_contrib_set_feature_tile(sbe_contrib* h, int features);

#ifdef __cplusplus
}
#endif

#endif /* SBE_CONTRIB_H */
