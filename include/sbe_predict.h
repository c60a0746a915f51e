/* sbe_predict.h -- C ABI of the posterior predictive of the logged samples on the device: the per-cell mixture row of every
 * logged draw of the model, summed over the draws, with each component's responsibility for the observed cells and the
 * pointwise likelihood rows.
 *
 * A run's stats file holds one full draw of the mixture model per logged sample (sbayes/sampling/loggers.py:106-130,
 * 157-228): the weights, a Dirichlet draw of every cluster's effect and of every confounder group's effect; the clusters
 * file holds the membership.  This unit puts them back together with the data: the mixture row of a cell is
 * simulate_features' lh_feature (sbayes/simulation.py:238-252).
 *
 * The contract (tests/_predict_oracle.py restates it in fp64; DESIGN.md section 21 states it):
 *   data (set once):  codes uint8 [N][F], the state index of a cell, 255 = NA;  per confounder c = 1 .. C-1 a group index
 *                     uint8 [N], 255 = none, with G_c groups;  K clusters.  A sample's table has R = K + sum_c G_c rows:
 *                     the clusters first, then the confounders' groups in order.
 *   one sample t:     clusters uint8 [K][N] (0 / not 0),  weights float64 [F][C],  tables float64 [R][F][S], zero at
 *                     inapplicable states.
 *   per object:       k_t(n) the one cluster holding n, or none;  h[n][0] = (k_t(n) exists), h[n][c] = (group_c(n) != none);
 *                     wn[n][f][c] = h w[f][c] / sum_c' h w[f][c'], the sum over c' = 0, 1, .. in order (normalize_weights,
 *                     sbayes/model/likelihood.py:171-190, in float64); 0 where that sum is 0 (the reference: NaN).
 *   per cell:         m[n][f][s] = sum_c wn[n][f][c] * table[row_c(n)][f][s], c = 0, 1, .. in order, product rounded,
 *                     then added;  pred_sum[n][f][s] += m[n][f][s];
 *                     observed (x = codes[n][f] != 255) and m[x] > 0:  resp_sum[n][f][c] += wn_c table_c[x] / m[x];
 *                     observed and m[x] == 0:  nothing is added to resp_sum, n_zero += 1;   NA: nothing is added;
 *                     lik[t][n F + f] = float32(m[x]) for an observed cell, 1.0f for an NA cell.
 *   accumulation:     float64; a cell's accumulators add the samples' terms in sample order, one at a time, by one
 *                     thread: no atomics on floating-point values, bit-identical from call to call and however the
 *                     samples are split across sbe_predict_accumulate calls.
 *   validation:       on the device, before anything is accumulated.  SBE_ERR_DATA names the first offender -- by sample,
 *                     then in the order of the list, then by position -- and the accumulators are left untouched:
 *                     (1) an object in two clusters; (2) a weight that is negative or not finite; (3) a weight row whose
 *                     sum over c is further than SBE_PREDICT_SUM_TOL from 1; (4) a table entry that is negative or not
 *                     finite; (5) a table row without a positive entry; (6) a table row whose sum over s is further than
 *                     SBE_PREDICT_SUM_TOL from 1.  Sums run over the entries in index order.
 * This estimator conditions on the logged effect draws; it is not the LikelihoodLogger's collapsed leave-one-out form.
 *
 * Conventions are those of sbe_engine.h: every function returns SBE_OK (0) or an SBE_ERR_* code with the message in
 * sbe_predict_last_error(); nothing throws across the boundary; arguments are checked before any device call; calls are
 * synchronous; the caller owns every host buffer.  The symbols are exported by the same library as the engine's.
 */
#ifndef SBE_PREDICT_H
#define SBE_PREDICT_H

#include <stdint.h>

#include "sbe_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sbe_predict sbe_predict;

#define SBE_PREDICT_ABI_VERSION 1

/* limits (SBE_ERR_ARG beyond them) */
#define SBE_PREDICT_MAX_STATES 32                  /* S                                                                   */
#define SBE_PREDICT_MAX_COMPONENTS 8               /* C: the clusters' component and C - 1 confounders                    */
#define SBE_PREDICT_MAX_ROWS 256                   /* R = K + sum_c G_c: the rows of one sample's table                   */
#define SBE_PREDICT_MAX_OBJECTS (1 << 20)          /* N                                                                   */
#define SBE_PREDICT_MAX_FEATURES (1 << 16)         /* F                                                                   */
#define SBE_PREDICT_MAX_ACC_BYTES (1ll << 32)      /* the accumulators, N F (S + C) 8 bytes                               */
#define SBE_PREDICT_MAX_STAGE_BYTES (1ll << 28)    /* the samples of one accumulate call on the device: n * sbe_predict_sample_bytes */
#define SBE_PREDICT_MAX_TILE 256                   /* features per tile (the test hook)                                   */
#define SBE_PREDICT_SUM_TOL 1e-5                   /* a weight row's or a table row's sum may be this far from 1          */
#define SBE_PREDICT_NA 255                         /* in codes: the cell is missing; in groups: the object is in no group */

int sbe_predict_abi_version(void);
/* the message of the last failed call on `h` (NULL: of the last failed call of this thread) */
const char* sbe_predict_last_error(const sbe_predict* h);

int sbe_predict_create(sbe_predict** out, int device);
int sbe_predict_destroy(sbe_predict* h);
/* device time of the kernels of the last accumulate call (preparation, validation and accumulation; HIP events), in ms */
int sbe_predict_last_kernel_ms(const sbe_predict* h, float* ms_out);

/* Device bytes one sample of an accumulate call takes while the call runs: its cluster rows, weights, tables, cluster ids
 * and, with_lik != 0, its likelihood row.  0 for a shape beyond the limits. */
int64_t sbe_predict_sample_bytes(int64_t n_objects, int64_t n_features, int n_states, int n_components, int n_clusters, int n_rows, int with_lik);

/* The data: N objects, F features, S states, C components, K clusters; codes uint8 [N][F] (a state < S, or 255);
 * groups uint8 [C-1][N] (a group < n_groups[c-1], or 255) and n_groups int [C-1], both may be NULL when C = 1.
 * SBE_ERR_DATA names the first code or group index out of range.  The accumulators are reset.  Device memory only grows. */
int sbe_predict_set_data(sbe_predict* h, int64_t n_objects, int64_t n_features, int n_states, int n_components, int n_clusters,
                         const uint8_t* codes, const uint8_t* groups, const int* n_groups);
/* Zero the accumulators and the counts, keep the data. */
int sbe_predict_reset(sbe_predict* h);
/* n samples: clusters uint8 [n][K][N], weights float64 [n][F][C], tables float64 [n][R][F][S]; lik_out float32 [n][N F] or
 * NULL.  n >= 0 and n * sbe_predict_sample_bytes(.., lik_out != NULL) <= SBE_PREDICT_MAX_STAGE_BYTES (SBE_ERR_ARG beyond:
 * split the samples across calls, the sums do not depend on the split).  Host blocks go up in pieces of at most 64 MiB.
 * SBE_ERR_STATE before sbe_predict_set_data.  On SBE_ERR_DATA nothing was accumulated and lik_out is not written. */
int sbe_predict_accumulate(sbe_predict* h, int64_t n, const uint8_t* clusters, const double* weights, const double* tables, float* lik_out);
/* pred_sum float64 [N][F][S], resp_sum float64 [N][F][C] (either may be NULL); *n_samples_out: the samples accumulated since
 * the last reset; *n_zero_out: the (sample, observed cell) pairs with m[x] == 0 among them. */
int sbe_predict_read(sbe_predict* h, double* pred_sum, double* resp_sum, int64_t* n_samples_out, int64_t* n_zero_out);
/* A test hook, not part of what a caller needs: the features of a workgroup's tile, so that a small case can be made to
 * run several tiles along the features; 0: the default, planned from the shape.  SBE_ERR_ARG, at the next accumulate, if
 * the tile's slice of a sample's tables does not fit the LDS.  The results do not depend on the value, bit for bit. */
int sbe_predict_set_feature_tile(sbe_predict* h, int features);

#ifdef __cplusplus
}
#endif

#endif /* SBE_PREDICT_H */
