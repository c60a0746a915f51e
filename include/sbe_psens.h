/* sbe_psens.h -- C ABI of the on-device power-scaling sensitivity of every logged column (Kallioinen, Paananen, Buerkner &
 * Vehtari 2023): how far the empirical distribution of a column moves when one logged component of the log posterior
 * (the likelihood, the prior or one of its parts) is raised to a power alpha near 1.
 *
 * A handle owns the same float64 STORE as sbe_diag.h: M chains (runs) of rows [S_r][P], column-major per chain, filled per
 * chain in pieces of any size.  There is no split and no cut: burn_rows[r] rows are dropped from the front of chain r and
 * the n_r rows that remain are stacked in chain order, N = sum n_r draws per column (sample index: the place in that
 * stack).  V weight vectors [V][N] live on the device, set in one of two ways:
 *
 *   sbe_psens_weights_from_components   vector 2 g is alpha = 1 / (1 + delta), vector 2 g + 1 is alpha = 1 + delta of component
 *       g; the log ratios (alpha - 1) x[:, component_columns[g]] are taken from the store and smoothed by PSIS exactly as
 *       tests/_elpd_oracle.psis_column(-ratios) does (tail count, strict cutoff, ties in the order of the sample index, gpdfit,
 *       gpinv, truncation at 0, renormalisation by logsumexp), in float64; ess = 1 / sum w^2;
 *   sbe_psens_set_weights               the caller's own non-negative finite weights of positive sum.
 *
 * sbe_psens_compute then gives per (vector v, column), with s the ascending sort of the column (x + 0.0 on load; ties in the
 * order of the sample index), q_i = w[v][sample_i], Q_i = (prefix sum of q)_i / sum q, P_i = (i + 1) / N,
 * M_i = (P_i + Q_i) / 2, b_i = s_(i+1) - s_i for i = 0 .. N - 2:
 *
 *   Pint = sum b_i P_i;  Qint = sum b_i Q_i;  bound = Pint + Qint
 *   pq = max(0, sum b_i P_i (log2 P_i - log2 M_i) + (0.5 / ln 2) (Qint - Pint))        (log2 0 := 0)
 *   qp = max(0, sum b_i Q_i (log2 Q_i - log2 M_i) + (0.5 / ln 2) (Pint - Qint));   js = pq + qp
 *
 * and js_neg, bound_neg: the same of -x (the sort reversed, the prefix sums running from the other end).  The prefix sum has
 * one stated order: thread t of 256 adds its chunk of ceil(N / 256) consecutive sorted draws in sequence, the 256 chunk
 * totals are added in sequence, and Q_i is (the totals before the chunk + the sum within the chunk up to i) / (all totals).
 * Every other sum is a fixed tree over the threads' sequential chunk sums.  wmean = sum q s / sum q and wsd = sqrt(sum q
 * (s - wmean)^2 / sum q) are formed in the same way.  The cumulative Jensen-Shannon distance sqrt(js / bound) and the
 * sensitivity are left to the caller (sbayes_amd/psens.py).  tests/_psens_oracle.py restates all of it in NumPy; DESIGN.md
 * section 28 states it.
 *
 * A column with a non-finite value (SBE_DIAG_FLAG_NONFINITE) gives NaN everywhere; a constant column (SBE_DIAG_FLAG_CONSTANT,
 * max - min < 1e-15) gives js = bound = 0 and its moments.  A vector flagged SBE_PSENS_VFLAG_CONSTANT counts as q = 1: js = 0
 * exactly, bound and the moments those of the unweighted draws.
 *
 * Conventions are those of sbe_engine.h and sbe_diag.h: every function returns SBE_OK (0) or an SBE_ERR_* code with the
 * message in sbe_psens_last_error(); nothing throws across the boundary; arguments are checked before any device call;
 * calls are synchronous; the caller owns every host buffer.  The symbols are exported by the same library as the engine's.
 */
#ifndef SBE_PSENS_H
#define SBE_PSENS_H

#include <stdint.h>

#include "sbe_diag.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sbe_psens sbe_psens;

#define SBE_PSENS_ABI_VERSION 1

/* limits (SBE_ERR_ARG beyond them): those of sbe_diag.h (SBE_DIAG_MAX_CHAINS; SBE_DIAG_MIN_DRAWS per chain after burn-in;
 * SBE_DIAG_MAX_DRAWS for N; columns 1 .. INT32_MAX) and */
#define SBE_PSENS_MAX_COMPONENTS 8                  /* components per sbe_psens_weights_from_components call              */
#define SBE_PSENS_MAX_VECTORS 16                    /* weight vectors on the device                                       */

/* per weight vector */
#define SBE_PSENS_VFLAG_CONSTANT 1                  /* every log ratio equal: uniform weights 1 / N, k = +inf             */
#define SBE_PSENS_VFLAG_UNRELIABLE 2                /* Pareto k > 0.7                                                     */

int sbe_psens_abi_version(void);
/* the message of the last failed call on `h` (NULL: of the last failed call of this thread) */
const char* sbe_psens_last_error(const sbe_psens* h);
/* the largest N whose sort keys (12 bytes per draw) both kernels keep in LDS; longer columns sort in a global scratch */
int64_t sbe_psens_lds_max_draws(void);

int sbe_psens_create(sbe_psens** out, int device);
int sbe_psens_destroy(sbe_psens* h);
/* Shape the store: n_chains chains of up to capacity_rows rows of n_columns values, all empty.  Device memory only
 * grows; what the store held, the weights included, is forgotten. */
int sbe_psens_reset(sbe_psens* h, int n_chains, int64_t n_columns, int64_t capacity_rows);
/* append host rows to one chain: float64 [n_rows][n_columns], C order (the weights are forgotten) */
int sbe_psens_append_rows(sbe_psens* h, int chain, const double* rows, int64_t n_rows);
/* rows stored for one chain */
int sbe_psens_rows(const sbe_psens* h, int chain, int64_t* n_rows_out);
/* columns per launch of the column kernel (0: the default, sized from the scratch budget).  Results do not depend on it,
 * bit for bit. */
int sbe_psens_set_launch_columns(sbe_psens* h, int64_t columns);
/* on != 0: both kernels sort in the global scratch whatever N is (the tests' path switch).  Results do not depend on it,
 * bit for bit. */
int sbe_psens_set_global_path(sbe_psens* h, int on);

/* The 2 n_components PSIS weight vectors of the components' power-scaling (see above); burn_rows [n_chains] fixes the draws
 * for sbe_psens_compute as well.  component_columns [n_components]: columns of the store.  delta > 0.  Outputs, [2
 * n_components] each: pareto_k_out, ess_out (float64), vflag_out (SBE_PSENS_VFLAG_*); weights_out: float64 [2 n_components][N]
 * or NULL.  SBE_ERR_ARG, naming the column, when a component column holds a non-finite value or its ratios overflow. */
int sbe_psens_weights_from_components(sbe_psens* h, const int64_t* burn_rows, int n_components, const int64_t* component_columns,
                                      double delta, double* pareto_k_out, double* ess_out, uint8_t* vflag_out, double* weights_out);
/* The caller's n_vectors (1 .. SBE_PSENS_MAX_VECTORS) weight vectors, float64 [n_vectors][N], N = sum over the chains of
 * (rows - burn_rows): non-negative, finite, of positive sum (checked on the device: SBE_ERR_ARG naming the vector). */
int sbe_psens_set_weights(sbe_psens* h, const int64_t* burn_rows, int n_vectors, const double* weights);

/* The sums of every (vector, column) under the weights last set (SBE_ERR_STATE without any): float64 [V][n_columns] each,
 * and flag_out [n_columns] (SBE_DIAG_FLAG_CONSTANT, SBE_DIAG_FLAG_NONFINITE). */
int sbe_psens_compute(sbe_psens* h, double* js_out, double* bound_out, double* js_neg_out, double* bound_neg_out, double* wmean_out,
                      double* wsd_out, uint8_t* flag_out);

/* of the last successful weights call, and of the last compute call behind it: chains, N, V, the path (SBE_DIAG_PATH_*:
 * both kernels change path at sbe_psens_lds_max_draws()), the launches of the column kernel and the columns of each (0, 0
 * before a compute call) */
int sbe_psens_last_shape(const sbe_psens* h, int* chains_out, int64_t* draws_out, int* vectors_out, int* path_out, int64_t* launches_out,
                         int64_t* launch_columns_out);
/* device time (HIP events), in milliseconds: ms_out[0] the weights kernel of the last weights call, ms_out[1] the column
 * kernel of the last compute call */
int sbe_psens_last_kernel_ms(const sbe_psens* h, float* ms_out);

/* Inspection calls (the tests and tools/psens_speed.py use them; nothing else needs them).  sorted_column: the sorted pairs
 * of one column under the draws of the last weights call, values_out float64 [N] and samples_out int32 [N] (NaN and -1 for
 * a column with a non-finite value).  device_log2: out[i] = the kernels' log2(in[i]), float64 [n], 1 <= n <= 2^24. */
int sbe_psens_sorted_column(sbe_psens* h, int64_t column, double* values_out, int32_t* samples_out);
int sbe_psens_device_log2(sbe_psens* h, int64_t n, const double* in, double* out);

#ifdef __cplusplus
}
#endif

#endif /* SBE_PSENS_H */
