/* sbe_objpair.h -- C ABI of the object-pair posterior predictive check: on how many features every pair of objects shows the
 * same state, on the data and on data sets replicated from the fitted model.
 *
 * sBayes looks for objects that share more features than their confounders explain.  After a fit the most direct question is
 * asked per pair of objects: do these two still agree more often than the fitted model reproduces?  A pair that does is
 * similarity the model has not explained -- a missed contact area, a K that is too small, a missing family.  The other checks
 * aggregate (sbe_ppc.h per feature and per object, sbe_pairppc.h per feature pair, sbe_spatial.h per class of object pairs);
 * this unit keeps the pair itself.  sbe_ppc.h draws one replicated data set per logged sample; this unit counts the agreements
 * of every pair on the data and on a stream of such replicates and keeps per pair how often the replicated count was above, at
 * or below the observed one.
 *
 * Contract (tests/_objpair_oracle.py restates it):
 *
 *   Data.  x: uint8 [N][F], SBE_OBJPAIR_NA = 255 = not observed; n_states: int32 [F], each in [1, SBE_OBJPAIR_MAX_STATES] (the
 *   state limit of sbe_ppc.h, so that every replicate sbe_ppc_check can return is accepted); N <= SBE_OBJPAIR_MAX_OBJECTS,
 *   F <= SBE_OBJPAIR_MAX_FEATURES (the limits of sbe_spatial.h).  The checks and the naming of the first offender are
 *   sbe_pairppc_set_data's.
 *
 *   Statistics of one data set y (the data, or a replicate), exact integers, for i != j:
 *       agree[i][j]      = #{f : y[i][f] and y[j][f] are codes, y[i][f] = y[j][f]}
 *       comparable[i][j] = the same without the equality
 *   Both are symmetric int32 [N][N]; the diagonal is 0 in every output.
 *
 *   sbe_objpair_set_data computes agree_obs and comparable_obs and clears the accumulators.  A failed call leaves the handle
 *   without data.
 *
 *   Replicates.  sbe_objpair_add takes y_rep: uint8 [n][N][F], each code below n_states[f] or 255 -- what sbe_ppc_check
 *   returns, skipped cells included.  The codes are validated on the device before any accumulator changes; SBE_ERR_DATA names
 *   the first offender by replicate, object and feature, and a refused call leaves the accumulators as they were.  For every
 *   replicate and every pair i < j:
 *       exactly one of n_greater, n_equal, n_less (int32) += 1, by comparing the replicate's v = agree[i][j] with agree_obs[i][j];
 *       sum += v and sumsq += v * v (int64);
 *   mirrored to [j][i].  agree_rep_out (optional) is int32 [n][N][N] and holds the replicates' own counts.  A replicate's NA
 *   cells are simply not comparable: the unit does not require the data's NA pattern.
 *
 *   Overflow.  v <= F <= 2^12, so after n replicates sumsq <= n 2^24: the int32 counts bind first.
 *   sbe_objpair_max_replicates is 2^31 - 1, and sbe_objpair_add refuses with SBE_ERR_ARG a call after which the handle would hold
 *   more.
 *
 *   Exactness.  The counts are 0/1 contractions on the matrix pipe, FP4 operands and an f32 accumulator: the contraction axis has
 *   E = sum of n_states <= 131072 elements and a count is at most F <= 4096, both far below 2^24.  No other floating-point number
 *   exists on the device.
 *
 *   Determinism.  The accumulators are added with integer atomics.  No output depends on how the replicates are split over
 *   sbe_objpair_add calls, on sbe_objpair_set_launch_tiles or on whether agree_rep_out is asked for.
 *
 * What the p-value is not: it conditions on the logged effect draws and uses the data twice, so it is conservative (DESIGN.md
 * section 22), and the N (N - 1) / 2 pairs are dependent multiple comparisons (every object is in N - 1 of them).
 *
 * Conventions are those of sbe_engine.h: every function returns SBE_OK (0) or an SBE_ERR_* code with the message in
 * sbe_objpair_last_error(); nothing throws across the boundary; arguments are checked before any device call; calls are
 * synchronous; the caller owns every host buffer.  The symbols are exported by the same library as the engine's.
 */
#ifndef SBE_OBJPAIR_H
#define SBE_OBJPAIR_H

#include <stdint.h>

#include "sbe_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sbe_objpair sbe_objpair;

#define SBE_OBJPAIR_ABI_VERSION 1

#define SBE_OBJPAIR_NA 255                              /* the code of "not observed" */
#define SBE_OBJPAIR_MAX_OBJECTS 4096                    /* N (SBE_SPATIAL_MAX_OBJECTS) */
#define SBE_OBJPAIR_MAX_FEATURES 4096                   /* F (SBE_SPATIAL_MAX_FEATURES) */
#define SBE_OBJPAIR_MAX_STATES 32                       /* S (SBE_PREDICT_MAX_STATES, the limit of sbe_ppc.h) */
#define SBE_OBJPAIR_ROUND 256                           /* the contraction axis is padded to whole rounds of this many elements */
#define SBE_OBJPAIR_MAX_STAGE_BYTES (256ll << 20)       /* device bytes of the replicates of one sbe_objpair_add call */

int sbe_objpair_abi_version(void);
/* the message of the last failed call on `h` (NULL: of the last failed call of this thread) */
const char* sbe_objpair_last_error(const sbe_objpair* h);

int sbe_objpair_create(sbe_objpair** out, int device);
int sbe_objpair_destroy(sbe_objpair* h);
/* tile pairs per launch of the count kernels (0: the default, chosen from E and the replicates of the call so that no launch
 * runs long).  Results do not depend on it. */
int sbe_objpair_set_launch_tiles(sbe_objpair* h, int64_t tile_pairs);

/* the most replicates a handle of this shape accumulates (see Overflow): 2^31 - 1; 0 for a shape beyond the limits */
int64_t sbe_objpair_max_replicates(int64_t n_objects, int64_t n_features);
/* Device bytes one replicate of an sbe_objpair_add call takes while the call runs, for data with E = sum of n_states: the upload
 * N F, the operand image N_pad E_pad / 2 (N_pad: N in whole tiles of 32 objects, E_pad: E in whole rounds, a nibble per element)
 * and, with_agree_rep, 4 N N.  0 for a shape beyond the limits or an E outside [F, 32 F].  (Beside them the handle holds 36 N N
 * bytes of observed counts and accumulators.) */
int64_t sbe_objpair_replicate_bytes(int64_t n_objects, int64_t n_features, int64_t n_elements, int with_agree_rep);

/* The data: x uint8 [N][F], n_states int32 [F].  Computes agree_obs and comparable_obs and clears the accumulators.  A failed
 * call leaves the handle without data. */
int sbe_objpair_set_data(sbe_objpair* h, const uint8_t* x, int64_t n_objects, int64_t n_features, const int32_t* n_states);
/* n >= 0 replicates y_rep uint8 [n][N][F]; agree_rep_out: NULL or int32 [n][N][N].  SBE_ERR_STATE before set_data; SBE_ERR_ARG
 * when the handle would hold more than sbe_objpair_max_replicates, or when n > 1 and n * sbe_objpair_replicate_bytes exceeds
 * SBE_OBJPAIR_MAX_STAGE_BYTES (the caller splits; one replicate alone is always taken: at the largest shape its image is
 * 256 MiB by itself); SBE_ERR_DATA for a code that is neither below n_states[f] nor 255. */
int sbe_objpair_add(sbe_objpair* h, int64_t n, const uint8_t* y_rep, int32_t* agree_rep_out);
/* Copies back, [N][N] each and symmetric with a zero diagonal: agree_obs, comparable_obs, n_greater, n_equal, n_less (int32),
 * sum, sumsq (int64); and the number of replicates added since the last set_data or reset.  Every output pointer may be NULL
 * (not wanted): at N = 4096 the seven arrays take 470 MB. */
int sbe_objpair_read(sbe_objpair* h, int32_t* agree_obs, int32_t* comparable_obs, int32_t* n_greater, int32_t* n_equal, int32_t* n_less,
                     int64_t* sum, int64_t* sumsq, int64_t* n_replicates_out);
/* clears the accumulators and keeps the data */
int sbe_objpair_reset(sbe_objpair* h);

/* of the last successful set_data or add: the padded contraction length E_pad, the 32 x 32 tile pairs computed and the launches
 * they were split over */
int sbe_objpair_last_shape(const sbe_objpair* h, int64_t* e_pad_out, int64_t* tile_pairs_out, int64_t* launches_out);
/* device time of the count kernels' launches (in add: contraction and tally) of the last successful set_data or add (HIP events),
 * in milliseconds */
int sbe_objpair_last_kernel_ms(const sbe_objpair* h, float* ms_out);

#ifdef __cplusplus
}
#endif

#endif /* SBE_OBJPAIR_H */
