/* sbe_pairppc.h -- C ABI of the pairwise posterior predictive check: where the chi-squared statistic of every feature pair on
 * the data falls among the same statistic on data sets replicated from the fitted model.
 *
 * sBayes treats features as independent given their source.  The screening (sbe_assoc.h) tests the raw data, and flags the
 * pairs that depend on each other through a shared family or area -- which is what the model is fitted to explain.  This
 * unit asks what is left: sbe_ppc.h draws one replicated data set per logged sample from the fitted mixture rows, this unit
 * runs the screening's pair kernel over the data and over a stream of such replicates, and keeps per pair how often the
 * replicated statistic was above, at or below the observed one: the posterior predictive p-value of a pairwise discrepancy.
 *
 * Contract (tests/_pairppc_oracle.py restates it):
 *
 *   Data.  x: uint8 [N][F], SBE_PAIRPPC_NA = 255 = not observed; n_states: int32 [F]; the limits are SBE_ASSOC_MAX_*.
 *   sbe_pairppc_set_data validates as sbe_assoc_compute does, computes stat_obs [F][F], dof_obs, n_obs and valid_obs by the
 *   screening's arithmetic and clears the accumulators.
 *
 *   Statistic.  The statistic of a table is the screening's without the p-value (csrc/sbe_assoc_pair.hip.h, written once for
 *   both units): counts from the FP4 contraction on the matrix pipe, margins and totals in float32, dof = (R-1)(C-1) over the
 *   occupied rows and columns, the Pearson terms in fp64 with Yates' correction when dof == 1, summed a major, b minor.  On
 *   the data it equals sbe_assoc_compute's `statistic` bit for bit.
 *
 *   Replicates.  sbe_pairppc_add takes y_rep: uint8 [n][N][F], each code below n_states[f] or 255 -- what sbe_ppc_check
 *   returns, skipped cells included.  The codes are validated on the device before any accumulator changes; SBE_ERR_DATA
 *   names the first offender by replicate, object and feature, and a refused call leaves the accumulators as they were.
 *   For every replicate, in the order given, and every pair i < j with valid_obs:
 *       s = the statistic of the replicate's table of the pair; a table with dof 0 has s = 0 and n_degenerate += 1;
 *       exactly one of n_greater, n_equal, n_less += 1, by comparing the fp64 values s and stat_obs;
 *       sum += s;  sumsq += s * s, the product rounded and then added (no FMA).
 *   Pairs that are not valid on the data, and the diagonal, stay at 0.  stat_rep_out (optional) is float64 [n][F][F],
 *   symmetric, and holds the s values (0 where nothing is accumulated).
 *
 *   Accumulators.  They live on the handle; the sums are sequential in replicate order.  No output bit depends on how the
 *   replicates are split across sbe_pairppc_add calls, on the launch-tile setting, on the form, on stat_rep_out, or on the call.  There are
 *   no floating-point atomics.
 *
 * What the p-value is not: it conditions on the logged effect draws and uses the data twice, so it is conservative (DESIGN.md
 * section 22); the F (F - 1) / 2 pairs are multiple comparisons; and Yates' correction scales the statistic of a dof 1 table
 * differently from a dof > 1 one, which shows where a replicate loses a state the data has.
 *
 * Conventions are those of sbe_engine.h: every function returns SBE_OK (0) or an SBE_ERR_* code with the message in
 * sbe_pairppc_last_error(); nothing throws across the boundary; arguments are checked before any device call; calls are
 * synchronous; the caller owns every host buffer.  The symbols are exported by the same library as the engine's.
 */
#ifndef SBE_PAIRPPC_H
#define SBE_PAIRPPC_H

#include <stdint.h>

#include "sbe_assoc.h"
#include "sbe_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sbe_pairppc sbe_pairppc;

#define SBE_PAIRPPC_ABI_VERSION 1

#define SBE_PAIRPPC_NA 255                              /* the code of "not observed" (SBE_ASSOC_NA) */
#define SBE_PAIRPPC_MAX_STAGE_BYTES (256ll << 20)       /* device bytes of the replicates of one sbe_pairppc_add call */
/* The two forms of the replicate kernel (sbe_pairppc_set_form).  Sequential: one wave per tile pair walks the call's replicates
 * in order.  Spread: the replicates are dealt out over waves, and their statistics wait in a buffer of the handle of
 * SBE_PAIRPPC_HELD_BYTES to be added per pair in replicate order.  The two forms give the same bits. */
#define SBE_PAIRPPC_FORM_AUTO 0
#define SBE_PAIRPPC_FORM_SEQUENTIAL 1
#define SBE_PAIRPPC_FORM_SPREAD 2
/* device bytes the spread form holds beside the replicates of a call (allocated on its first use, not part of
 * sbe_pairppc_replicate_bytes: it does not grow with the replicates) */
#define SBE_PAIRPPC_HELD_BYTES (32ll << 20)

int sbe_pairppc_abi_version(void);
/* the message of the last failed call on `h` (NULL: of the last failed call of this thread) */
const char* sbe_pairppc_last_error(const sbe_pairppc* h);

int sbe_pairppc_create(sbe_pairppc** out, int device);
int sbe_pairppc_destroy(sbe_pairppc* h);
/* tile pairs per launch of the pair kernels (0: the default, chosen from N and the replicates of the call so that no launch
 * runs long).  Results do not depend on it, bit for bit. */
int sbe_pairppc_set_launch_tiles(sbe_pairppc* h, int64_t tile_pairs);

/* The form of the replicate kernel: SBE_PAIRPPC_FORM_AUTO (the default: the unit picks by the tile pairs and the replicates of
 * the call, so that the device is filled), _SEQUENTIAL or _SPREAD.  Results do not depend on it, bit for bit. */
int sbe_pairppc_set_form(sbe_pairppc* h, int form);

/* Device bytes one replicate of an sbe_pairppc_add call takes while the call runs: the upload N F, the feature-major image
 * F n_pad (n_pad: N rounded up to 256) and, with_stat_rep, 8 F F.  0 for a shape beyond the SBE_ASSOC_MAX_* limits.  (Beside
 * them the handle holds 49 F F bytes of statistics and accumulators and, once the spread form has run, SBE_PAIRPPC_HELD_BYTES.) */
int64_t sbe_pairppc_replicate_bytes(int64_t n_objects, int64_t n_features, int with_stat_rep);

/* The data: x uint8 [N][F], n_states int32 [F], checked as sbe_assoc_compute checks them.  Computes the observed statistic
 * and clears the accumulators.  A failed call leaves the handle without data. */
int sbe_pairppc_set_data(sbe_pairppc* h, const uint8_t* x, int64_t n_objects, int64_t n_features, const int32_t* n_states);
/* n >= 0 replicates y_rep uint8 [n][N][F]; stat_rep_out: NULL or float64 [n][F][F].  SBE_ERR_STATE before set_data,
 * SBE_ERR_ARG when n * sbe_pairppc_replicate_bytes exceeds SBE_PAIRPPC_MAX_STAGE_BYTES (the caller splits), SBE_ERR_DATA for a
 * code that is neither below n_states[f] nor 255. */
int sbe_pairppc_add(sbe_pairppc* h, int64_t n, const uint8_t* y_rep, double* stat_rep_out);
/* Copies back, [F][F] each and symmetric: stat_obs (float64), dof_obs, n_obs (int32), valid_obs (uint8), n_greater, n_equal,
 * n_less, n_degenerate (int32), sum, sumsq (float64); and the number of replicates added since the last set_data or reset. */
int sbe_pairppc_read(sbe_pairppc* h, double* stat_obs, int32_t* dof_obs, int32_t* n_obs, uint8_t* valid_obs, int32_t* n_greater,
                     int32_t* n_equal, int32_t* n_less, int32_t* n_degenerate, double* sum, double* sumsq, int64_t* n_replicates_out);
/* clears the accumulators and keeps the data */
int sbe_pairppc_reset(sbe_pairppc* h);

/* of the last successful set_data or add: the padded state count (2 .. 32), the 32 x 32 tile pairs computed and the launches
 * they were split over */
int sbe_pairppc_last_shape(const sbe_pairppc* h, int32_t* s_pad_out, int64_t* tile_pairs_out, int64_t* launches_out);
/* device time of the pair kernel's launches of the last successful set_data or add (HIP events), in milliseconds */
int sbe_pairppc_last_kernel_ms(const sbe_pairppc* h, float* ms_out);

#ifdef __cplusplus
}
#endif

#endif /* SBE_PAIRPPC_H */
