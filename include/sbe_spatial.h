/* sbe_spatial.h -- C ABI of the spatial posterior predictive check: how often neighbouring objects show the same state, per
 * class of pairs (a neighbour graph, or classes of distance), on the data and on data sets replicated from the fitted model.
 *
 * sBayes looks for areas of neighbouring objects that share features beyond what the confounders explain.  After a fit the
 * question is whether neighbours still agree more often than the fitted model reproduces: if they do, a contact area has been
 * missed.  The statistic for categorical data is the join count -- the neighbouring pairs in the same state -- and, per class
 * of distance, the correlogram.  The null is the fitted model's own replicates: sbe_ppc.h draws one replicated data set per
 * logged sample, this unit counts the joins of the data and of a stream of such replicates and keeps per (class, feature),
 * per (class, object) and per class how often the replicated count was above, at or below the observed one.
 *
 * Contract (tests/_spatial_oracle.py restates it):
 *
 *   Data.  x: uint8 [N][F], SBE_SPATIAL_NA = 255 = not observed; n_states: int32 [F], each in [1, SBE_SPATIAL_MAX_STATES] (the
 *   state limit of sbe_ppc.h, so that every replicate sbe_ppc_check can return is accepted); N <= SBE_SPATIAL_MAX_OBJECTS,
 *   F <= SBE_SPATIAL_MAX_FEATURES.  The checks and the naming of the first offender are sbe_pairppc_set_data's.
 *
 *   Pair classes.  band: uint8 [N][N]; entry (i, j) is a class b < B or SBE_SPATIAL_NA for "pair not counted";
 *   1 <= B <= SBE_SPATIAL_MAX_BANDS.  The matrix must be symmetric; the diagonal is ignored whatever it holds.  SBE_ERR_DATA
 *   names the first entry off the diagonal (row-major) that is neither below B nor 255, else the first (i, j) with
 *   band[i][j] != band[j][i].  One class over a neighbour graph gives the plain join count, classes of distance over all pairs
 *   the correlogram.  A refused sbe_spatial_set_data leaves the handle without data.
 *
 *   Statistics of one data set y (the data, or a replicate), exact integers:
 *       agree[b][f]            = #{i < j : band[i][j] = b, y[i][f] and y[j][f] are codes, y[i][f] = y[j][f]}
 *       comparable[b][f]       = the same without the equality
 *       local_agree[b][i]      = sum over f of #{j != i : band[i][j] = b, y[i][f] and y[j][f] are codes, y[i][f] = y[j][f]}
 *       local_comparable[b][i] = the same without the equality
 *       total[b]               = sum over f of agree[b][f]                                         (int64)
 *   so that the sum over i of local_agree[b][i] is 2 total[b].
 *
 *   sbe_spatial_set_data computes the five arrays on the data and clears the accumulators.
 *
 *   Replicates.  sbe_spatial_add takes y_rep: uint8 [n][N][F], each code below n_states[f] or 255 -- what sbe_ppc_check
 *   returns, skipped cells included.  The codes are validated on the device before any accumulator changes; SBE_ERR_DATA names
 *   the first offender by replicate, object and feature, and a refused call leaves the accumulators as they were.  For every
 *   replicate and every (b, f), every (b, i) and every b:
 *       exactly one of n_greater, n_equal, n_less += 1, by comparing the replicate's agree, local_agree or total with the
 *       observed one;   sum += v and sumsq += v * v (int64), for agree and local_agree only.
 *   The optional outputs hold the replicates' own arrays.  (The caller keeps total_rep and has the totals' mean and sd from it
 *   exactly: the totals need no sumsq.)
 *
 *   Overflow.  In one replicate agree <= A = N (N - 1) / 2 and local_agree <= L = (N - 1) F, so after n replicates
 *   sumsq <= n max(A, L)^2, which stays below 2^63 for n <= (2^63 - 1) / max(A, L)^2; the three counts are int32, so n <= 2^31 - 1
 *   as well.  sbe_spatial_max_replicates(N, F) is the smaller of the two (2^31 - 1 when max(A, L) = 0, that is N = 1), and
 *   sbe_spatial_add refuses with SBE_ERR_ARG a call after which the handle would hold more.  (sum <= n max(A, L) is then
 *   safe too.)  At N = F = 4096: A = 8386560, L = 16773120, the limit is 32784 replicates; at N = 4096, F = 3
 *   it is 131136.
 *
 *   Determinism.  No floating-point number exists on the device; the counts are added with integer atomics.  No output
 *   depends on how the replicates are split over sbe_spatial_add calls, on sbe_spatial_set_tile or on which optional outputs
 *   are asked for.
 *
 * What the p-value is not: it conditions on the logged effect draws and uses the data twice, so it is conservative (DESIGN.md
 * section 22), and the B F (or B N) entries are multiple comparisons.
 *
 * Conventions are those of sbe_engine.h: every function returns SBE_OK (0) or an SBE_ERR_* code with the message in
 * sbe_spatial_last_error(); nothing throws across the boundary; arguments are checked before any device call; calls are
 * synchronous; the caller owns every host buffer.  The symbols are exported by the same library as the engine's.
 */
#ifndef SBE_SPATIAL_H
#define SBE_SPATIAL_H

#include <stdint.h>

#include "sbe_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sbe_spatial sbe_spatial;

#define SBE_SPATIAL_ABI_VERSION 1

#define SBE_SPATIAL_NA 255                              /* the code of "not observed", and of "pair not counted" in band */
#define SBE_SPATIAL_MAX_OBJECTS 4096                    /* N */
#define SBE_SPATIAL_MAX_FEATURES 4096                   /* F */
#define SBE_SPATIAL_MAX_STATES 32                       /* S (SBE_PREDICT_MAX_STATES, the limit of sbe_ppc.h) */
#define SBE_SPATIAL_MAX_BANDS 8                         /* B */
#define SBE_SPATIAL_MAX_TILE 32                         /* features per tile (the test hook) */
#define SBE_SPATIAL_MAX_STAGE_BYTES (256ll << 20)       /* device bytes of the replicates of one sbe_spatial_add call */

int sbe_spatial_abi_version(void);
/* the message of the last failed call on `h` (NULL: of the last failed call of this thread) */
const char* sbe_spatial_last_error(const sbe_spatial* h);

int sbe_spatial_create(sbe_spatial** out, int device);
int sbe_spatial_destroy(sbe_spatial* h);
/* features per tile of the count kernel (0: the default; at most SBE_SPATIAL_MAX_TILE; a tile whose state masks would not fit
 * the kernel's 64 KiB of LDS is shortened).  Results do not depend on it. */
int sbe_spatial_set_tile(sbe_spatial* h, int tile_features);

/* the most replicates a handle of this shape accumulates (see Overflow); 0 for a shape beyond the limits */
int64_t sbe_spatial_max_replicates(int64_t n_objects, int64_t n_features);
/* Device bytes one replicate of an sbe_spatial_add call takes while the call runs.  With W the 64-bit words of N objects, padded
 * to a power of two up to 16 and to a multiple of 16 beyond: the upload N F, the feature-major image 64 W F, the state masks
 * 8 W F (max_states + 1), two count arrays 4 B (F + N) each and the totals 8 B.  0 for arguments beyond the limits. */
int64_t sbe_spatial_replicate_bytes(int64_t n_objects, int64_t n_features, int max_states, int n_bands);

/* The data and the pair classes: x uint8 [N][F], n_states int32 [F], band uint8 [N][N] with n_bands classes.  Computes the
 * observed arrays and clears the accumulators.  A failed call leaves the handle without data. */
int sbe_spatial_set_data(sbe_spatial* h, const uint8_t* x, int64_t n_objects, int64_t n_features, const int32_t* n_states,
                         const uint8_t* band, int n_bands);
/* n >= 0 replicates y_rep uint8 [n][N][F].  Optional outputs (NULL: not wanted): agree_rep, comparable_rep int32 [n][B][F];
 * local_rep, local_comparable_rep int32 [n][B][N]; total_rep int64 [n][B].  SBE_ERR_STATE before set_data; SBE_ERR_ARG when the
 * handle would hold more than sbe_spatial_max_replicates, or when n * sbe_spatial_replicate_bytes exceeds
 * SBE_SPATIAL_MAX_STAGE_BYTES (the caller splits); SBE_ERR_DATA for a code that is neither below n_states[f] nor 255. */
int sbe_spatial_add(sbe_spatial* h, int64_t n, const uint8_t* y_rep, int32_t* agree_rep, int32_t* comparable_rep, int32_t* local_rep,
                    int32_t* local_comparable_rep, int64_t* total_rep);
/* Copies back the observed arrays: agree_obs, comparable_obs int32 [B][F]; local_obs, local_comparable_obs int32 [B][N];
 * total_obs int64 [B]; the accumulators of agree, [B][F]: n_greater, n_equal, n_less (int32), sum, sumsq (int64); those of
 * local_agree, [B][N], likewise; those of total, [B]: n_greater, n_equal, n_less (int32); and the number of replicates added
 * since the last set_data or reset. */
int sbe_spatial_read(sbe_spatial* h, int32_t* agree_obs, int32_t* comparable_obs, int32_t* local_obs, int32_t* local_comparable_obs,
                     int64_t* total_obs, int32_t* f_greater, int32_t* f_equal, int32_t* f_less, int64_t* f_sum, int64_t* f_sumsq,
                     int32_t* i_greater, int32_t* i_equal, int32_t* i_less, int64_t* i_sum, int64_t* i_sumsq, int32_t* t_greater,
                     int32_t* t_equal, int32_t* t_less, int64_t* n_replicates_out);
/* clears the accumulators and keeps the data */
int sbe_spatial_reset(sbe_spatial* h);

/* device time of the count kernels (and, in add, the totals and the tally) of the last successful set_data or add (HIP events),
 * in milliseconds */
int sbe_spatial_last_kernel_ms(const sbe_spatial* h, float* ms_out);

#ifdef __cplusplus
}
#endif

#endif /* SBE_SPATIAL_H */
