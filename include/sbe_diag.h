/* sbe_diag.h -- C ABI of the on-device convergence diagnostics: effective sample size (ESS) and split R-hat per column.
 *
 * The sBayes manual asks for several runs of one model, a check of convergence and of the effective sample size, and a
 * comparison across runs.  A `stats_K*_*.txt` file holds one column per weight and per effect entry -- thousands to
 * hundreds of thousands of them -- and every column is one independent reduction over its samples.  This header is the
 * device form of that step:
 *
 *   - a handle owns a float64 STORE of M chains (runs) of rows [S_r][P], column-major per chain: [chain][P][capacity],
 *     so one column's samples of one chain are contiguous.  Rows are appended per chain, in pieces of any size;
 *   - sbe_diag_compute drops the burn-in of every chain, cuts the chains to the shortest remaining length, splits each
 *     in two halves (optional) and computes per column: mean, sd, ESS (Geyer's initial positive and initial monotone
 *     sequence over the combined autocorrelations), R-hat and the Monte-Carlo standard error of the mean.
 *     The numerical contract is written out in tests/_diag_oracle.py and in DESIGN.md section 16.
 *
 * Conventions are those of sbe_engine.h: every function returns SBE_OK (0) or an SBE_ERR_* code with the message in
 * sbe_diag_last_error(); nothing throws across the boundary; arguments are checked before any device call; calls
 * are synchronous; the caller owns every host buffer.  The symbols are exported by the same library as the engine's.
 */
#ifndef SBE_DIAG_H
#define SBE_DIAG_H

#include <stdint.h>

#include "sbe_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sbe_diag sbe_diag;

#define SBE_DIAG_ABI_VERSION 1

/* limits (SBE_ERR_ARG beyond them) */
#define SBE_DIAG_MAX_CHAINS 64                      /* chains (runs) in the store                                        */
#define SBE_DIAG_MIN_DRAWS 4                        /* n: draws per chain after burn-in, cut and split                   */
#define SBE_DIAG_MAX_DRAWS (1 << 20)                /* M * n: draws per column after split, over all chains              */
/* columns: 1 .. INT32_MAX */

/* per-column flags (bits) */
#define SBE_DIAG_FLAG_CONSTANT 1                    /* max - min < 1e-15: ess = M * n, rhat = NaN, mcse_mean = 0          */
#define SBE_DIAG_FLAG_NONFINITE 2                   /* the column holds a NaN or an infinity: every output is NaN         */
#define SBE_DIAG_FLAG_TRUNCATED 4                   /* the positive sequence was stopped by max_lag                       */

/* the path of the last compute call (sbe_diag_last_shape) */
#define SBE_DIAG_PATH_LDS 0                         /* columns staged in LDS, centred per chain                           */
#define SBE_DIAG_PATH_GLOBAL 1                      /* columns read from the store in every pass                          */

int sbe_diag_abi_version(void);
/* the message of the last failed call on `h` (NULL: of the last failed call of this thread) */
const char* sbe_diag_last_error(const sbe_diag* h);
/* largest M * n (after split) whose columns are staged in LDS; longer columns take the global path.  The arithmetic is
 * the same on both paths. */
int64_t sbe_diag_lds_max_draws(void);

int sbe_diag_create(sbe_diag** out, int device);
int sbe_diag_destroy(sbe_diag* h);
/* Shape the store: n_chains chains of up to capacity_rows rows of n_columns values, all empty.  Device memory only
 * grows; what the store held is forgotten. */
int sbe_diag_reset(sbe_diag* h, int n_chains, int64_t n_columns, int64_t capacity_rows);
/* append host rows to one chain: float64 [n_rows][n_columns], C order */
int sbe_diag_append_rows(sbe_diag* h, int chain, const double* rows, int64_t n_rows);
/* rows stored for one chain */
int sbe_diag_rows(const sbe_diag* h, int chain, int64_t* n_rows_out);
/* columns per launch of the column kernel (0: the default, sized from M * n so that a launch whose columns all run to
 * the n - 3 bound stays short).  Results do not depend on it, bit for bit. */
int sbe_diag_set_launch_columns(sbe_diag* h, int64_t columns);

/* The diagnostics of every column.  burn_rows (int64 [n_chains]): rows dropped from the front of each chain; the chains
 * are then cut at the end to the shortest remaining length, and with split != 0 each becomes two chains of half that
 * length (the middle draw of an odd length is dropped).  max_lag: 0 for none, else the positive sequence stops once its
 * next pair of lags would pass it (flag SBE_DIAG_FLAG_TRUNCATED).  Outputs, [n_columns] each: mean, sd, ess, rhat,
 * mcse_mean (float64), n_lags (int32: the largest lag whose autocovariance the column needed), flag (uint8). */
int sbe_diag_compute(sbe_diag* h, const int64_t* burn_rows, int split, int64_t max_lag, double* mean_out, double* sd_out,
                     double* ess_out, double* rhat_out, double* mcse_mean_out, int32_t* n_lags_out, uint8_t* flag_out);

/* of the last successful compute call: M and n after the split, the path (SBE_DIAG_PATH_*), the launches */
int sbe_diag_last_shape(const sbe_diag* h, int* chains_out, int64_t* draws_out, int* path_out, int64_t* launches_out);
/* device time of the column kernel of that call (HIP events), in milliseconds */
int sbe_diag_last_kernel_ms(const sbe_diag* h, float* ms_out);

#ifdef __cplusplus
}
#endif

#endif /* SBE_DIAG_H */
