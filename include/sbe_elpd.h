/* sbe_elpd.h -- C ABI of the on-device model comparison over logged observation likelihoods: PSIS-LOO and WAIC.
 *
 * sBayes compares runs of different cluster counts by ELPD-LOO (sbayes/tools/elpd.py:22-61): the LikelihoodLogger rows
 * (sbayes/sampling/loggers.py:354-359, float32 sum_c w * lh_exact per observation) are read back, the NA columns and
 * the burn-in dropped, and arviz.loo run over the log of the matrix.  This header is the device form of that step:
 *
 *   - a STORE owns float32 likelihood rows on one device, column-major [n_columns][capacity] (one observation's samples
 *     are contiguous).  It is filled from host rows (an .h5 / .npy matrix) or straight from an engine slot (the
 *     LikelihoodLogger row, computed and written on the device: only the engine's status word crosses PCIe);
 *   - sbe_elpd_compute runs PSIS-LOO (arviz.loo for one chain: psislw -> _psislw -> _gpdfit -> _gpinv) and the
 *     per-observation terms of WAIC (arviz.waic) over the kept columns and the sample window [burn_rows, n_rows).
 *     The numerical contract is written out in tests/_elpd_oracle.py.
 *
 * Conventions are those of sbe_engine.h: every function returns SBE_OK (0) or an SBE_ERR_* code with the message in
 * sbe_elpd_last_error(); nothing throws across the boundary; arguments are checked before any device call; calls
 * are synchronous; the caller owns every host buffer.  The symbols are exported by the same library as the engine's.
 */
#ifndef SBE_ELPD_H
#define SBE_ELPD_H

#include <stdint.h>

#include "sbe_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sbe_elpd_store sbe_elpd_store;

#define SBE_ELPD_ABI_VERSION 1

/* limits: samples per column in one compute call (S = n_rows - burn_rows) */
#define SBE_ELPD_MIN_SAMPLES 2
#define SBE_ELPD_MAX_SAMPLES (1 << 20)

int sbe_elpd_abi_version(void);
/* the message of the last failed call on `st` (NULL: of the last failed call of this thread) */
const char* sbe_elpd_last_error(const sbe_elpd_store* st);
/* largest S whose column is staged in LDS by sbe_elpd_compute; longer columns take the global-memory selection */
int64_t sbe_elpd_lds_max_samples(void);

int sbe_elpd_create(sbe_elpd_store** out, int device, int64_t n_columns, int64_t capacity);
int sbe_elpd_destroy(sbe_elpd_store* st);
int sbe_elpd_n_rows(const sbe_elpd_store* st, int64_t* n_rows_out);
/* device time of the column kernel of the last successful sbe_elpd_compute (HIP events), in milliseconds */
int sbe_elpd_last_kernel_ms(const sbe_elpd_store* st, float* ms_out);
/* forget every row (the device memory is kept) */
int sbe_elpd_reset(sbe_elpd_store* st);

/* append host rows: float32 [n_rows][n_columns], C order */
int sbe_elpd_append_rows(sbe_elpd_store* st, const float* rows, int64_t n_rows);
/* append the LikelihoodLogger row of an engine slot (loggers.py:354-359): float32(sum_c w * lh_exact), the row
 * sbe_observation_lh_exact returns, flattened over [N][F].  The store must live on the engine's device and have
 * n_columns == N * F.  Errors of the likelihood evaluation are those of sbe_observation_lh_exact. */
int sbe_elpd_append_engine(sbe_elpd_store* st, sbe_engine* e, int slot);
/* copy rows [row0, row0 + n_rows) back: float32 [n_rows][n_columns] */
int sbe_elpd_get_rows(sbe_elpd_store* st, int64_t row0, int64_t n_rows, float* out);

/* PSIS-LOO / WAIC terms per kept column over the rows [burn_rows, n_rows).  Columns are dropped where na_values
 * (uint8 [n_columns], may be NULL) is non-zero; with na_values NULL and na_isclose != 0, where every stored row is
 * isclose(lh, 1) (rtol 1e-5, atol 1e-8: elpd.py:31); with both unset every column is kept.  The four outputs
 * (float64, at least n_columns entries each) are filled for the kept columns in column order: loo_i, Pareto k, lppd_i
 * (logsumexp(ll) - log S), v_i (variance of ll, ddof 0); *n_kept_out receives their number.
 * SBE_ERR_DATA if a kept value in the window is not positive and finite. */
int sbe_elpd_compute(sbe_elpd_store* st, int64_t burn_rows, const uint8_t* na_values, int na_isclose,
                     double* loo_i, double* k_i, double* lppd_i, double* v_i, int64_t* n_kept_out);

#ifdef __cplusplus
}
#endif

#endif /* SBE_ELPD_H */
