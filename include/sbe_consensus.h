/* sbe_consensus.h -- C ABI of the on-device posterior similarity of objects and of the consensus clustering read from it.
 *
 * The other post-run units look at a clustering through its labels.  This one is label free: it counts how often two
 * objects share an area (the posterior similarity, or co-clustering, matrix), scores every logged sample against such a
 * matrix (Dahl's least-squares clustering: the sample that minimises Binder's loss) and compares the matrices of two
 * selections of runs.
 *
 *   - a handle owns a STORE of R runs of cluster samples c[r][s][k][n] in {0,1}.  Rows are appended per run, as uint8
 *     [n][K][N], in pieces of any size, and packed on the device into two forms: an object-major FP4 operand image
 *     for the matrix pipe (one nibble per contraction element e = s K + k, 0x0 or 0x2, one segment per run, zero-padded to
 *     whole rounds of SBE_CONSENSUS_ROUND elements) and sample-major bit rows [run][row][K][ceil(N/32)] for the scores;
 *   - the handle holds two matrices, slot 0 and slot 1, each with the T it was computed over.
 *
 * The contract (tests/_consensus_oracle.py restates it in NumPy; DESIGN.md section 19 states it).  All of it in exact
 * integers.  For a selection Sel of runs, T = sum_{r in Sel} S_r:
 *   similarity:  C[i][j] = sum_{r in Sel} sum_s sum_k c[r][s][k][i] c[r][s][k][j], int32 [N][N], symmetric; C[i][i] counts
 *       the rows that hold i (with disjoint areas: the samples that hold i in any area).  With disjoint areas C[i][j] / T is the posterior probability that i and j
 *       share an area; the definition does not need disjointness.
 *   scores:  score[s] = sum_k sum_{i,j} c[s][k][i] c[s][k][j] (T - 2 C[i][j]), int64, for the samples of any stored run
 *       against the matrix (C, T) of a slot.  For disjoint areas T^2 Binder(s) = T score[s] + sum C^2, so the smallest
 *       score is the least-squares sample.  An empty cluster adds 0.
 *   compare (slot 0 = a against slot 1 = b):  d[i][j] = |C_a[i][j] T_b - C_b[i][j] T_a|; row_max[i] = max_j d[i][j],
 *       row_sum[i] = sum_j d[i][j], int64.  d / (T_a T_b) is |P_a - P_b|.  A row sum stays below 2^63 (N 2^24 2^24 = 2^62);
 *       the sum of all rows need not, so it is left to the caller's wider integers.
 *
 * Limits (SBE_ERR_ARG beyond them, checked before any device call): 1 <= K <= SBE_CONSENSUS_MAX_CLUSTERS; 1 <= N <=
 * SBE_CONSENSUS_MAX_OBJECTS; at most SBE_CONSENSUS_MAX_RUNS runs of at most SBE_CONSENSUS_MAX_ROWS rows; T K <=
 * SBE_CONSENSUS_MAX_ELEMENTS for a selection; sbe_consensus_image_bytes(...) <= SBE_CONSENSUS_MAX_IMAGE_BYTES for a store.
 *
 * Conventions are those of sbe_engine.h: every function returns SBE_OK (0) or an SBE_ERR_* code with the message in
 * sbe_consensus_last_error(); nothing throws across the boundary; arguments are checked before any device call; calls are
 * synchronous; the caller owns every host buffer.  The symbols are exported by the same library as the engine's.
 */
#ifndef SBE_CONSENSUS_H
#define SBE_CONSENSUS_H

#include <stdint.h>

#include "sbe_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sbe_consensus sbe_consensus;

#define SBE_CONSENSUS_ABI_VERSION 1

/* limits (SBE_ERR_ARG beyond them) */
#define SBE_CONSENSUS_MAX_CLUSTERS 8                /* K                                                                 */
#define SBE_CONSENSUS_MAX_OBJECTS 16384             /* N: one int32 matrix is then at most 1 GiB (the handle holds two), and an object index of the scores' member list fits 16 bits (32 KiB of LDS) */
#define SBE_CONSENSUS_MAX_RUNS 64                   /* runs in the store                                                 */
#define SBE_CONSENSUS_MAX_ROWS (1 << 20)            /* S_r: samples per run (and the store's capacity)                   */
#define SBE_CONSENSUS_MAX_ELEMENTS (1 << 24)        /* T K of a selection: the counts are exact in the f32 accumulator of the matrix pipe up to 2^24 */
#define SBE_CONSENSUS_ROUND 256                     /* contraction elements per round of the similarity kernel's loop: a run's segment is padded to whole rounds */
#define SBE_CONSENSUS_MAX_IMAGE_BYTES (1ll << 34)   /* operand image plus bit rows of a store: 16 GiB.  With the two matrices (2 GiB) and the staging buffer that is under a tenth of the device's memory, which the store shares with the engine and the other units' handles */

int sbe_consensus_abi_version(void);
/* the message of the last failed call on `h` (NULL: of the last failed call of this thread) */
const char* sbe_consensus_last_error(const sbe_consensus* h);
/* Device bytes of a store of this shape: the operand image, 32 ceil(N/32) rows of n_runs segments of
 * ceil(capacity_rows K / SBE_CONSENSUS_ROUND) SBE_CONSENSUS_ROUND / 2 bytes, plus the bit rows, n_runs capacity_rows K
 * ceil(N/32) words.  0 for a shape outside the limits above (the byte limit is the caller's to compare).  No device call. */
int64_t sbe_consensus_image_bytes(int n_runs, int n_clusters, int64_t n_objects, int64_t capacity_rows);

int sbe_consensus_create(sbe_consensus** out, int device);
int sbe_consensus_destroy(sbe_consensus* h);
/* Shape the store: n_runs runs of up to capacity_rows samples of n_clusters x n_objects bits, all empty.  Device memory
 * only grows; what the store and the two slots held is forgotten. */
int sbe_consensus_reset(sbe_consensus* h, int n_runs, int n_clusters, int64_t n_objects, int64_t capacity_rows);
/* append host rows to one run: uint8 [n_rows][K][N] of 0 / 1, C order (SBE_ERR_DATA for any other byte).  Both slots are
 * out of date afterwards.  A call that fails on the device (SBE_ERR_HIP) leaves the store without a shape: reset comes next. */
int sbe_consensus_append_rows(sbe_consensus* h, int run, const uint8_t* rows, int64_t n_rows);
/* rows stored for one run */
int sbe_consensus_rows(const sbe_consensus* h, int run, int64_t* n_rows_out);

/* The similarity counts over the runs r with run_mask[r] != 0 (uint8 [n_runs]) into slot 0 or 1, and, unless counts_out
 * is NULL, to the host: int32 [N][N].  SBE_ERR_STATE for a selection that holds no rows. */
int sbe_consensus_similarity(sbe_consensus* h, const uint8_t* run_mask, int slot, int32_t* counts_out);
/* The scores of every stored sample of `run` (selected for the slot's matrix or not) against the matrix of `slot`:
 * int64 [rows(run)].  SBE_ERR_STATE if the slot is empty or was computed before the store last changed. */
int sbe_consensus_scores(sbe_consensus* h, int slot, int run, int64_t* score_out);
/* Slot 0 against slot 1: row_max, row_sum int64 [N].  SBE_ERR_STATE if either slot is empty or out of date. */
int sbe_consensus_compare(sbe_consensus* h, int64_t* row_max, int64_t* row_sum);

/* tile pairs per launch of the similarity kernel; 0: the default, chosen so that no launch runs long.  The results do not
 * depend on the value, bit for bit. */
int sbe_consensus_set_launch_tiles(sbe_consensus* h, int64_t tile_pairs);
/* device time of the kernels of the last similarity, scores or compare call (HIP events), in milliseconds */
int sbe_consensus_last_kernel_ms(const sbe_consensus* h, float* ms_out);

#ifdef __cplusplus
}
#endif

#endif /* SBE_CONSENSUS_H */
