/* sbe_compare.h -- C ABI of the on-device comparison of models by their pointwise ELPD values: totals, differences against
 * a reference model with their standard errors, stacking weights and pseudo-BMA+ weights by the Bayesian bootstrap.
 *
 * sBayes chooses the number of clusters by running K = 1..n and comparing ELPD-LOO across the runs (sbayes/tools/elpd.py);
 * sbe_elpd.h produces the pointwise loo_i / waic_i of one run.  This header is the step after it, what arviz.compare does
 * with the pointwise values of several runs:
 *
 *   - a handle owns a STORE of M models, each a float64 vector of N pointwise ELPD values on the log scale (the same
 *     observations in every model), model-major on one device with N padded to whole chunks of SBE_COMPARE_CHUNK;
 *   - totals, differences, stacking and bootstrap read the store.  Every model must have been set since the last reset
 *     (SBE_ERR_STATE otherwise).
 *
 * The contract (tests/_compare_oracle.py restates it in fp64; DESIGN.md section 20 states it):
 *   totals:       elpd[k] = sum_i x[i][k];  se[k] = sqrt(N var_i(x[i][k])), ddof 0.
 *   differences:  d_i = x[i][ref] - x[i][k];  elpd_diff[k] = sum_i d_i;  dse[k] = sqrt(N var_i(d_i)), ddof 0; both exactly
 *                 0 for k = ref.
 *   stacking:     maximise f(w) = mean_i log(sum_k w_k p[i][k]) over the simplex, p[i][k] = exp(x[i][k] - max_k x[i][k]).
 *                 From w = 1/M the update g_k = mean_i(p[i][k] / sum_j w_j p[i][j]), w_k <- w_k g_k / sum_j w_j g_j is
 *                 repeated (the divisor is 1 but for rounding).  gap(w) = max_k g_k - 1 >= f* - f(w).  The call returns the
 *                 last weights whose gap was evaluated, with that gap and the number of updates that led to them; it stops
 *                 when a gap read by the host is <= tol, or with the weights after max_iter updates.  The host reads the
 *                 gap every SBE_COMPARE_CHECK_EVERY evaluations, so the number of updates is not part of the contract.
 *   bootstrap:    for replicate b and observation i, u = the engine's Philox uniform (seed, draw = b, index i),
 *                 e = -log(1 - u);  z[b][k] = N sum_i(e x[i][k]) / sum_i e;  w_b = softmax_k(z[b]);  weights = mean_b w_b;
 *                 se[k] = the standard deviation over b of z[b][k], ddof 0.  (Normalised Exp(1) draws are Dirichlet(1, .., 1).)
 *   Sums: no floating-point atomics, bit-identical from call to call and from card to card; no accumulator adds more than
 *   SBE_COMPARE_RUN terms in sequence, longer sums combine partial sums in a fixed tree.
 *
 * Conventions are those of sbe_engine.h: every function returns SBE_OK (0) or an SBE_ERR_* code with the message in
 * sbe_compare_last_error(); nothing throws across the boundary; arguments are checked before any device call; calls are
 * synchronous; the caller owns every host buffer.  The symbols are exported by the same library as the engine's.
 */
#ifndef SBE_COMPARE_H
#define SBE_COMPARE_H

#include <stdint.h>

#include "sbe_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sbe_compare sbe_compare;

#define SBE_COMPARE_ABI_VERSION 1

/* limits (SBE_ERR_ARG beyond them) */
#define SBE_COMPARE_MAX_MODELS 32                  /* M                                                                   */
#define SBE_COMPARE_MAX_POINTS (1 << 24)           /* N: observations per model                                           */
#define SBE_COMPARE_MAX_REPLICATES (1 << 16)       /* B: bootstrap replicates of one call                                 */
#define SBE_COMPARE_MAX_IMAGE_BYTES (1ll << 32)    /* the two images of a store (x, and p for stacking): 2 M N_pad 8 bytes; 4 GiB, so M = 32 goes with N <= 2^23 */
/* the shape of the sums (not tunable: results do not depend on the card) */
#define SBE_COMPARE_BLOCK 256                      /* threads per workgroup of the totals and stacking kernels            */
#define SBE_COMPARE_CHUNK 4096                     /* observations per workgroup there: 16 terms per thread               */
#define SBE_COMPARE_RUN 1024                       /* the longest run of terms any accumulator adds in sequence           */
#define SBE_COMPARE_BOOT_CHUNK 1024                /* observations a lane of the bootstrap kernel walks for its replicate */
#define SBE_COMPARE_CHECK_EVERY 32                 /* R: stacking evaluations between two reads of the gap by the host    */

int sbe_compare_abi_version(void);
/* the message of the last failed call on `h` (NULL: of the last failed call of this thread) */
const char* sbe_compare_last_error(const sbe_compare* h);

int sbe_compare_create(sbe_compare** out, int device);
int sbe_compare_destroy(sbe_compare* h);
/* device time between the first and the last kernel of the last totals, differences, stacking or bootstrap call (HIP
 * events; for stacking that span holds the host's reads of the gap), in milliseconds */
int sbe_compare_last_kernel_ms(const sbe_compare* h, float* ms_out);

/* Shape the store: n_models models of n_points values, none of them set.  Device memory only grows. */
int sbe_compare_reset(sbe_compare* h, int n_models, int64_t n_points);
/* Model k <- x: float64 [n_points].  The values are checked on the device; SBE_ERR_DATA names the first value that is not
 * finite, and the model is then not set. */
int sbe_compare_set_model(sbe_compare* h, int k, const double* x);

/* elpd, se: float64 [n_models] */
int sbe_compare_totals(sbe_compare* h, double* elpd, double* se);
/* against model `ref`: elpd_diff, dse float64 [n_models] */
int sbe_compare_differences(sbe_compare* h, int ref, double* elpd_diff, double* dse);
/* Stacking weights: weights float64 [n_models]; *gap_out: the gap of those weights; *updates_out: the updates that led to
 * them (<= max_iter).  Converged: *gap_out <= tol.  tol > 0, 1 <= max_iter <= 2^31 - 1. */
int sbe_compare_stacking(sbe_compare* h, double tol, int64_t max_iter, double* weights, double* gap_out, int64_t* updates_out);
/* Pseudo-BMA+ weights over `replicates` Bayesian-bootstrap replicates (alpha = 1): weights, se float64 [n_models]; z_out
 * float64 [replicates][n_models], may be NULL. */
int sbe_compare_bootstrap(sbe_compare* h, uint64_t seed, int64_t replicates, double* weights, double* se, double* z_out);
/* A test hook, not part of what a caller needs: replicates per batch of the bootstrap (a multiple of 64), so that a small
 * case can be made to run several batches; 0: the default, as many as keep the chunk partials of a batch
 * under 512 MiB.  The results do not depend on the value, bit for bit. */
int sbe_compare_set_bootstrap_batch(sbe_compare* h, int64_t replicates);

#ifdef __cplusplus
}
#endif

#endif /* SBE_COMPARE_H */
