/* sbe_summary.h -- C ABI of the on-device posterior summary per column: quantiles, the highest-density interval (HDI),
 * the rank-normalised R-hat and the bulk and tail effective sample sizes of Vehtari et al. 2021, beside what sbe_diag.h
 * gives (mean, sd, ESS, classic R-hat, mcse_mean).
 *
 * A handle owns the same float64 STORE as sbe_diag.h: M chains (runs) of rows [S_r][P], column-major per chain, filled
 * per chain in pieces of any size.  sbe_summary_compute drops the burn-in, cuts and splits as sbe_diag_compute does, and
 * per column, over the N = M * n draws that remain (x + 0.0 on load: a -0 never reaches an output; s: their ascending sort):
 *
 *   quantile(p)  h = (N-1) p; k = floor(h); g = h - k; s[k] + (s[min(k+1, N-1)] - s[k]) g   (in that order, no contraction)
 *   HDI          inc = floor(hdi_prob N) clipped to [1, N-1]; (s[i], s[i+inc]) at the lowest i that minimises the width
 *   ranks        average ranks r (exact half-integers); z(x) = ndtri((r - 0.375) / (N + 0.25))
 *   derived      zb = z(x); zf = z(|x - quantile(0.5)|) (own sort); i05 = [x <= quantile(0.05)], i95 = [x <= quantile(0.95)]
 *                (a column constant within every chain, the chains differing: zb and zf hold 2 r instead of z, integers whose
 *                chain sums are exact, so W = 0 exactly, rhat_rank = +inf and ess_bulk is that of rho = 1)
 *   ess_bulk     ess(zb);  ess_tail = min(ess(i05), ess(i95));  rhat_rank = the larger of rhat(zb), rhat(zf) (a NaN side is
 *                ignored), each by the column kernel of sbe_diag.h under its rule for a constant column
 *
 * A column with a non-finite value (SBE_DIAG_FLAG_NONFINITE) gives NaN everywhere; a constant column
 * (SBE_DIAG_FLAG_CONSTANT) gives its quantiles and HDI, rhat_rank = NaN and ess_bulk = ess_tail = N.  The flag ORs
 * SBE_DIAG_FLAG_TRUNCATED over the five passes of the column kernel.  The numerical contract is written out in
 * tests/_summary_oracle.py and in DESIGN.md section 18.
 *
 * Conventions are those of sbe_engine.h and sbe_diag.h: every function returns SBE_OK (0) or an SBE_ERR_* code with the
 * message in sbe_summary_last_error(); nothing throws across the boundary; arguments are checked before any device call;
 * calls are synchronous; the caller owns every host buffer.  The symbols are exported by the same library as the engine's.
 */
#ifndef SBE_SUMMARY_H
#define SBE_SUMMARY_H

#include <stdint.h>

#include "sbe_diag.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sbe_summary sbe_summary;

#define SBE_SUMMARY_ABI_VERSION 1

/* limits (SBE_ERR_ARG beyond them): those of sbe_diag.h (SBE_DIAG_MAX_CHAINS, SBE_DIAG_MIN_DRAWS, SBE_DIAG_MAX_DRAWS,
 * columns 1 .. INT32_MAX) and */
#define SBE_SUMMARY_MAX_PROBS 8                     /* quantile probabilities per compute call                           */

/* `which` of sbe_summary_derived_column */
#define SBE_SUMMARY_DERIVED_ZB 0                    /* z of the values' ranks (2 r where every chain is constant)         */
#define SBE_SUMMARY_DERIVED_ZF 1                    /* z of the ranks of |x - median|                                     */
#define SBE_SUMMARY_DERIVED_I05 2                   /* [x <= quantile(0.05)] as 0.0 / 1.0                                 */
#define SBE_SUMMARY_DERIVED_I95 3                   /* [x <= quantile(0.95)] as 0.0 / 1.0                                 */
#define SBE_SUMMARY_DERIVED_RANK 4                  /* the average ranks of the values (1 .. N, half-integers)            */

int sbe_summary_abi_version(void);
/* the message of the last failed call on `h` (NULL: of the last failed call of this thread) */
const char* sbe_summary_last_error(const sbe_summary* h);

int sbe_summary_create(sbe_summary** out, int device);
int sbe_summary_destroy(sbe_summary* h);
/* Shape the store: n_chains chains of up to capacity_rows rows of n_columns values, all empty.  Device memory only
 * grows; what the store held is forgotten. */
int sbe_summary_reset(sbe_summary* h, int n_chains, int64_t n_columns, int64_t capacity_rows);
/* append host rows to one chain: float64 [n_rows][n_columns], C order */
int sbe_summary_append_rows(sbe_summary* h, int chain, const double* rows, int64_t n_rows);
/* rows stored for one chain */
int sbe_summary_rows(const sbe_summary* h, int chain, int64_t* n_rows_out);
/* columns per launch of the rank kernel and of the column kernel on the store (0: the default, sized from the scratch
 * budget and from M * n).  Results do not depend on it, bit for bit. */
int sbe_summary_set_launch_columns(sbe_summary* h, int64_t columns);

/* The summary of every column.  burn_rows, split, max_lag: as sbe_diag_compute (max_lag bounds all five passes of the
 * column kernel).  probs: n_probs (0 .. SBE_SUMMARY_MAX_PROBS) probabilities in [0, 1]; hdi_prob in (0, 1).  Outputs,
 * [n_columns] each unless noted: quantiles (float64 [n_probs][n_columns]; may be NULL when n_probs is 0), hdi_lo, hdi_hi,
 * ess_bulk, ess_tail, rhat_rank (float64); mean, sd, ess, rhat, mcse_mean, n_lags, flag: what sbe_diag_compute gives for
 * the same rows, bit for bit, but for the flag's SBE_DIAG_FLAG_TRUNCATED, which is ORed over the five passes. */
int sbe_summary_compute(sbe_summary* h, const int64_t* burn_rows, int split, int64_t max_lag, int n_probs, const double* probs,
                        double hdi_prob, double* quantiles_out, double* hdi_lo_out, double* hdi_hi_out, double* ess_bulk_out,
                        double* ess_tail_out, double* rhat_rank_out, double* mean_out, double* sd_out, double* ess_out,
                        double* rhat_out, double* mcse_mean_out, int32_t* n_lags_out, uint8_t* flag_out);

/* of the last successful compute call: M and n after the split, the path (SBE_DIAG_PATH_*: both kernels change path at
 * sbe_diag_lds_max_draws()), the launches of the rank kernel and the columns of each */
int sbe_summary_last_shape(const sbe_summary* h, int* chains_out, int64_t* draws_out, int* path_out, int64_t* launches_out,
                           int64_t* launch_columns_out);
/* device time of that call's kernels (HIP events), in milliseconds: ms_out[0] the rank kernel, ms_out[1] the five passes
 * of the column kernel (with the kernel that combines them) */
int sbe_summary_last_kernel_ms(const sbe_summary* h, float* ms_out);

/* An inspection call (the tests use it; nothing else needs it): re-runs the rank kernel for one column with the rows and
 * the shape of the last successful compute call and returns one derived column (SBE_SUMMARY_DERIVED_*), float64 [M][n]
 * in the order of the chains after the split.  SBE_ERR_STATE without such a call, or once the store was reset. */
int sbe_summary_derived_column(sbe_summary* h, int64_t column, int which, double* out);

#ifdef __cplusplus
}
#endif

#endif /* SBE_SUMMARY_H */
