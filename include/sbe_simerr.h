/* sbe_simerr.h -- C ABI of the Monte-Carlo error of the posterior similarity matrix and of run agreement measured in it.
 *
 * sbe_consensus.h counts how often two objects share an area.  This unit says how well those counts are known: every run is
 * cut into batches of b consecutive samples, the co-clustering of every pair of objects is counted per batch, and the spread
 * of the batch counts is the Monte-Carlo error of the pair's similarity (batch means).  Two selections of runs are then
 * compared pair by pair in units of that error.  The per-batch counts are the exact 0/1 contraction of the consensus unit on
 * the matrix pipe, closed at every batch boundary.
 *
 *   - a handle owns a STORE of R runs of cluster samples c[r][s][k][n] in {0,1}.  Rows are appended per run, as uint8
 *     [n][K][N], in pieces of any size, and packed on the device into an object-major FP4 operand image (one nibble per
 *     contraction element, 0x0 or 0x2, one segment per run).  The batch length b >= 1 (samples per batch) is fixed at reset.
 *     Batch q of run r is its samples [q b, (q + 1) b) and starts on a step boundary of the image: a batch occupies
 *     ceil(b K / SBE_SIMERR_STEP) steps of SBE_SIMERR_STEP elements and is zero behind its b K elements.  A trailing
 *     incomplete batch is stored but not used until later appends complete it.  Burn-in is the caller's;
 *   - the handle holds the moments of two SIDES, side 0 and side 1, each a selection of runs.
 *
 * The contract (tests/_simerr_oracle.py restates it in NumPy; DESIGN.md section 30 states it).  Integers are exact.  For a
 * side with nB complete batches in all its selected runs, and every ordered pair (i, j), the diagonal included:
 *   c_q[i][j] = sum_{s in batch q} sum_k c[s][k][i] c[s][k][j]
 *   S1 = sum_q c_q (int32), S2 = sum_q c_q^2 (int64), V = nB S2 - S1^2 (int64, >= 0).
 *   With T = nB b the limit T K <= SBE_SIMERR_MAX_ELEMENTS makes every c_q exact in the f32 accumulator and bounds nB S2
 *   and S1^2 by 2^48.  A side needs nB >= 2 (SBE_ERR_STATE below that).
 *   Derived on the host: P = S1 / (nB b), se^2 = V / (nB^2 (nB - 1) b^2).  When b divides every selected run's length, S1
 *   equals sbe_consensus_similarity's counts for the same runs.
 *   compare (side 0 = a against side 1 = b):  D = S1_a nB_b - S1_b nB_a (int64, exact);
 *       z2 = D^2 / (nB_b^2 V_a / (nB_a - 1) + nB_a^2 V_b / (nB_b - 1)), which is (P_a - P_b)^2 / (se_a^2 + se_b^2) with the
 *       common factors cancelled, in float64 in exactly this order:
 *           d = (double)D;  num = d * d;
 *           qa = ((double)V_a * (double)(nB_b * nB_b)) / (double)(nB_a - 1);
 *           qb = ((double)V_b * (double)(nB_a * nB_a)) / (double)(nB_b - 1);
 *           den = qa + qb;  z2 = den > 0 ? num / den : (D == 0 ? 0 : +inf).
 *       Every operand is an exactly representable integer and no step can be contracted into an FMA.
 *       row_max[i] = max_j z2[i][j]; row_arg[i]: the smallest j that attains it; row_count[i][m]: the number of j with
 *       z2[i][j] > thresholds[m] (strictly), int32 [N][n_thresholds].
 *   No output depends on the tiles per launch or on how the appended rows were cut into pieces.
 *
 * Limits (SBE_ERR_ARG beyond them, checked before any device call): 1 <= K <= SBE_SIMERR_MAX_CLUSTERS; 1 <= N <=
 * SBE_SIMERR_MAX_OBJECTS; at most SBE_SIMERR_MAX_RUNS runs of at most SBE_SIMERR_MAX_ROWS rows; 1 <= batch_rows <=
 * capacity_rows; T K <= SBE_SIMERR_MAX_ELEMENTS for a side; sbe_simerr_image_bytes(...) <= SBE_SIMERR_MAX_IMAGE_BYTES.
 *
 * Conventions are those of sbe_engine.h: every function returns SBE_OK (0) or an SBE_ERR_* code with the message in
 * sbe_simerr_last_error(); nothing throws across the boundary; arguments are checked before any device call; calls are
 * synchronous; the caller owns every host buffer.  The symbols are exported by the same library as the engine's.
 */
#ifndef SBE_SIMERR_H
#define SBE_SIMERR_H

#include <stdint.h>

#include "sbe_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sbe_simerr sbe_simerr;

#define SBE_SIMERR_ABI_VERSION 1

/* limits (SBE_ERR_ARG beyond them) */
#define SBE_SIMERR_MAX_CLUSTERS 8                /* K                                                                 */
#define SBE_SIMERR_MAX_OBJECTS 8192              /* N: a side holds 12 N^2 bytes (int32 S1, int64 S2), 768 MiB here; the handle holds two, and 8 N^2 bytes of z2 when asked */
#define SBE_SIMERR_MAX_RUNS 64                   /* runs in the store                                                 */
#define SBE_SIMERR_MAX_ROWS (1 << 20)            /* S_r: samples per run (and the store's capacity)                   */
#define SBE_SIMERR_MAX_ELEMENTS (1 << 24)        /* T K of a side, T = nB b: every c_q is exact in the f32 accumulator, nB S2 and S1^2 stay below 2^48 */
#define SBE_SIMERR_STEP 64                       /* contraction elements per step of the image: a batch starts on a step boundary */
#define SBE_SIMERR_MAX_THRESHOLDS 4              /* thresholds of one compare                                         */
#define SBE_SIMERR_MAX_IMAGE_BYTES (1ll << 34)   /* operand image of a store: 16 GiB, as the consensus unit's store   */

int sbe_simerr_abi_version(void);
/* the message of the last failed call on `h` (NULL: of the last failed call of this thread) */
const char* sbe_simerr_last_error(const sbe_simerr* h);
/* Device bytes of a store of this shape: 32 ceil(N/32) rows of n_runs segments of ceil(capacity_rows / batch_rows)
 * batches of ceil(batch_rows K / SBE_SIMERR_STEP) steps of SBE_SIMERR_STEP / 2 bytes.  0 for a shape outside the limits
 * above (the byte limit is the caller's to compare).  No device call. */
int64_t sbe_simerr_image_bytes(int n_runs, int n_clusters, int64_t n_objects, int64_t capacity_rows, int64_t batch_rows);

int sbe_simerr_create(sbe_simerr** out, int device);
int sbe_simerr_destroy(sbe_simerr* h);
/* Shape the store: n_runs runs of up to capacity_rows samples of n_clusters x n_objects bits in batches of batch_rows
 * samples, all empty.  Device memory only grows; what the store and the two sides held is forgotten. */
int sbe_simerr_reset(sbe_simerr* h, int n_runs, int n_clusters, int64_t n_objects, int64_t capacity_rows, int64_t batch_rows);
/* append host rows to one run: uint8 [n_rows][K][N] of 0 / 1, C order (SBE_ERR_DATA for any other byte).  Both sides are
 * out of date afterwards.  A call that fails on the device (SBE_ERR_HIP) leaves the store without a shape: reset comes next. */
int sbe_simerr_append_rows(sbe_simerr* h, int run, const uint8_t* rows, int64_t n_rows);
/* rows stored for one run (those of a trailing incomplete batch included) */
int sbe_simerr_rows(const sbe_simerr* h, int run, int64_t* n_rows_out);

/* The moments over the complete batches of the runs r with run_mask[r] != 0 (uint8 [n_runs]) into side 0 or 1, and, unless
 * the pointer is NULL, to the host: s1_out int32 [N][N], s2_out int64 [N][N], n_batches_out the side's nB.  SBE_ERR_STATE
 * for a selection with fewer than two complete batches. */
int sbe_simerr_moments(sbe_simerr* h, const uint8_t* run_mask, int side, int32_t* s1_out, int64_t* s2_out, int64_t* n_batches_out);
/* Side 0 against side 1: thresholds double [n_thresholds], 0 <= n_thresholds <= SBE_SIMERR_MAX_THRESHOLDS (NULL with
 * none); z2_out float64 [N][N] or NULL; row_max float64 [N]; row_arg int32 [N]; row_count int32 [N][n_thresholds] (NULL
 * with no threshold).  SBE_ERR_STATE if either side is empty or was computed before the store last changed. */
int sbe_simerr_compare(sbe_simerr* h, const double* thresholds, int n_thresholds, double* z2_out, double* row_max, int32_t* row_arg,
                       int32_t* row_count);

/* tile pairs per launch of the moments kernel; 0: the default, chosen so that no launch runs long.  The results do not
 * depend on the value, bit for bit. */
int sbe_simerr_set_launch_tiles(sbe_simerr* h, int64_t tile_pairs);
/* device time of the kernels of the last moments or compare call (HIP events), in milliseconds */
int sbe_simerr_last_kernel_ms(const sbe_simerr* h, float* ms_out);

#ifdef __cplusplus
}
#endif

#endif /* SBE_SIMERR_H */
