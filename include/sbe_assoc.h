/* sbe_assoc.h -- C ABI of the on-device feature screening: the chi-squared test of independence for every pair of features.
 *
 * sBayes treats features as independent given their source, and ships a tool that screens a data set for pairs that
 * are not (sbayes/tools/find_correlated_features.py): for every pair of features the contingency table of the two state
 * columns over the objects where both are observed (pd.crosstab), scipy.stats.chi2_contingency on it, and a report of
 * the pairs whose p-value is below a threshold.  This header is the device form of that loop:
 *
 *   - sbe_assoc_compute takes the state codes (uint8 [N][F], SBE_ASSOC_NA = not observed) and fills, for every pair,
 *     the statistic, the p-value, the degrees of freedom, the table's total and whether the tool would have tested the
 *     pair at all.  All contingency tables at once are X^T X of the one-hot matrix: a 0/1 contraction over objects on
 *     the matrix pipe (FP4 operands, exact counts in the f32 accumulator), with the test itself in the same kernel;
 *   - sbe_assoc_tables returns the observed tables of a list of pairs of the last computed data set (integer counts
 *     on the vector pipe: what the tool plots for the flagged pairs, and an independent check of the counts).
 *     The numerical contract is written out in tests/_assoc_oracle.py.
 *
 * Conventions are those of sbe_engine.h: every function returns SBE_OK (0) or an SBE_ERR_* code with the message in
 * sbe_assoc_last_error(); nothing throws across the boundary; arguments are checked before any device call; calls
 * are synchronous; the caller owns every host buffer.  The symbols are exported by the same library as the engine's.
 */
#ifndef SBE_ASSOC_H
#define SBE_ASSOC_H

#include <stdint.h>

#include "sbe_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sbe_assoc sbe_assoc;

#define SBE_ASSOC_ABI_VERSION 1

#define SBE_ASSOC_NA 255                    /* the code of "not observed" */
/* limits.  Objects: counts are exact in the f32 accumulator up to 2^24.  States: a 32 x 32 accumulator tile holds whole
 * pairs.  Features: the five [F][F] outputs take 25 bytes per entry, 400 MiB at the limit.  Codes: N * F bytes. */
#define SBE_ASSOC_MAX_OBJECTS (1 << 24)
#define SBE_ASSOC_MAX_STATES 32
#define SBE_ASSOC_MAX_FEATURES 4096
#define SBE_ASSOC_MAX_CODES ((int64_t)1 << 31)

int sbe_assoc_abi_version(void);
/* the message of the last failed call on `h` (NULL: of the last failed call of this thread) */
const char* sbe_assoc_last_error(const sbe_assoc* h);

int sbe_assoc_create(sbe_assoc** out, int device);
int sbe_assoc_destroy(sbe_assoc* h);
/* tile pairs per launch of the pair kernel (0: the default, chosen from N so that no launch runs long).  Results do
 * not depend on it, bit for bit. */
int sbe_assoc_set_launch_tiles(sbe_assoc* h, int64_t tile_pairs);

/* The chi-squared test of independence for every pair of the F features.  x: uint8 [N][F], each code below
 * n_states[f] or SBE_ASSOC_NA (else SBE_ERR_DATA); n_states: int32 [F], each in [1, SBE_ASSOC_MAX_STATES].  Outputs,
 * [F][F] each, symmetric: statistic and pvalue (float64), dof and n (int32), valid (uint8).  A pair is valid when both
 * features take more than one state over the objects where both are observed; the others (and the diagonal) hold
 * statistic 0, pvalue NaN, dof 0.  The codes stay on the device for sbe_assoc_tables until the next call. */
int sbe_assoc_compute(sbe_assoc* h, const uint8_t* x, int64_t n_objects, int64_t n_features, const int32_t* n_states,
                      double* statistic, double* pvalue, int32_t* dof, int32_t* n, uint8_t* valid);
/* The observed tables of n_pairs pairs (int32 [n_pairs][2]: i, j) of the data set of the last sbe_assoc_compute:
 * out is int32 [n_pairs][S][S] with S the largest n_states of that call, rows = states of i.  SBE_ERR_STATE before
 * the first compute call. */
int sbe_assoc_tables(sbe_assoc* h, const int32_t* pairs, int64_t n_pairs, int32_t* out);

/* of the last successful sbe_assoc_compute: the padded state count (2 .. 32), the 32 x 32 tile pairs computed and
 * the launches they were split over */
int sbe_assoc_last_shape(const sbe_assoc* h, int32_t* s_pad_out, int64_t* tile_pairs_out, int64_t* launches_out);
/* device time of the pair kernel's launches of the last successful sbe_assoc_compute (HIP events), in milliseconds */
int sbe_assoc_last_kernel_ms(const sbe_assoc* h, float* ms_out);

#ifdef __cplusplus
}
#endif

#endif /* SBE_ASSOC_H */
