/* sbe_align.h -- C ABI of the on-device alignment of cluster labels, within a run and across runs.
 *
 * Cluster labels are arbitrary: area 0 of one sample (or of one run) is in general not area 0 of the next.  The reference
 * matches every logged sample against the running sum of the samples aligned so far (its loggers), re-aligns a finished
 * run from a seed (tools/realign_clusters_within_run.py) and matches two runs by their mean memberships
 * (tools/align_clusters.py).  This header is the device form of the three:
 *
 *   - a handle owns a bit STORE of R runs of cluster samples c[r][s][k][n] in {0,1}: [run][row][K][ceil(N/32)] words.
 *     Rows are appended per run, as uint8 [n][K][N], in pieces of any size, and packed on the device;
 *   - sbe_align_within finds one permutation P_s per sample, sbe_align_counts the membership counts of every run with or
 *     without them, sbe_align_runs one permutation Q_b per run against a pivot run.
 *
 * The contract (tests/_align_oracle.py restates it in NumPy; DESIGN.md section 17 states it).  Assignment rule: for an
 * integer agreement matrix d[K][K] the permutation p maximises sum_i d[i][p[i]], and among the maximisers it is the one
 * whose sequence (p[0], ..., p[K-1]) is lexicographically smallest.  The aligned sample is c[p[i]] at label i.  All
 * arithmetic is exact: int32 sums, int64 agreements.
 *   within (seed_rows = m0):  m = min(m0, S_r), w = max(m, 1); sum[i][n] = sum_{s<m} c[s][i][n]; for s = 0 .. S_r-1:
 *       d[i][j] = sum_n sum[i][n] c[s][j][n], P_s = rule(d), sum[i][n] += w c[s][P_s[i]][n].
 *   counts:  cnt[r][i][n] = sum_{s >= burn_r} c[s][P_s[i]][n]   (P_s the identity when aligned == 0).
 *   runs (pivot a):  d[i][j] = sum_n cnt[a][i][n] cnt[b][j][n], Q_b = rule(d).
 *
 * Limits (SBE_ERR_ARG beyond them, checked before any device call): 1 <= K <= SBE_ALIGN_MAX_CLUSTERS; 1 <= N <=
 * sbe_align_max_objects(K), the largest N whose int32 running sums [K][N] fit the 160 KiB of LDS of a CU next to the
 * kernel's own SBE_ALIGN_STATIC_LDS bytes; at most SBE_ALIGN_MAX_RUNS runs; at most SBE_ALIGN_MAX_ROWS rows per run;
 * seed_rows <= SBE_ALIGN_MAX_SEED_ROWS, so that w S < 2^31.
 *
 * Conventions are those of sbe_engine.h: every function returns SBE_OK (0) or an SBE_ERR_* code with the message in
 * sbe_align_last_error(); nothing throws across the boundary; arguments are checked before any device call; calls are
 * synchronous; the caller owns every host buffer.  The symbols are exported by the same library as the engine's.
 */
#ifndef SBE_ALIGN_H
#define SBE_ALIGN_H

#include <stdint.h>

#include "sbe_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sbe_align sbe_align;

#define SBE_ALIGN_ABI_VERSION 1

/* limits (SBE_ERR_ARG beyond them) */
#define SBE_ALIGN_MAX_CLUSTERS 8                    /* K                                                                 */
#define SBE_ALIGN_MAX_RUNS 64                       /* runs in the store                                                 */
#define SBE_ALIGN_MAX_ROWS (1 << 20)                /* S_r: samples per run (and the store's capacity)                   */
#define SBE_ALIGN_MAX_SEED_ROWS 1024                /* seed_rows of sbe_align_within                                     */
#define SBE_ALIGN_LDS_BYTES (160 * 1024)            /* LDS of a CU                                                       */
#define SBE_ALIGN_STATIC_LDS 4096                   /* kept for the kernel's own LDS (reductions, the permutation, padding of the sums to whole words) */

int sbe_align_abi_version(void);
/* the message of the last failed call on `h` (NULL: of the last failed call of this thread) */
const char* sbe_align_last_error(const sbe_align* h);
/* largest N for K clusters: (SBE_ALIGN_LDS_BYTES - SBE_ALIGN_STATIC_LDS) / (4 K); 0 for K out of range */
int64_t sbe_align_max_objects(int n_clusters);

int sbe_align_create(sbe_align** out, int device);
int sbe_align_destroy(sbe_align* h);
/* Shape the store: n_runs runs of up to capacity_rows samples of n_clusters x n_objects bits, all empty.  Device memory
 * only grows; what the store held, permutations included, is forgotten. */
int sbe_align_reset(sbe_align* h, int n_runs, int n_clusters, int64_t n_objects, int64_t capacity_rows);
/* append host rows to one run: uint8 [n_rows][K][N] of 0 / 1, C order (a byte other than 0 counts as 1).  The
 * permutations of an earlier sbe_align_within are forgotten. */
int sbe_align_append_rows(sbe_align* h, int run, const uint8_t* rows, int64_t n_rows);
/* rows stored for one run */
int sbe_align_rows(const sbe_align* h, int run, int64_t* n_rows_out);

/* One permutation per stored sample of every run.  perm_out: int8 [n_runs][capacity_rows][K]; the rows of run r at and
 * beyond sbe_align_rows(r) are not written.  The handle keeps the permutations for sbe_align_counts and sbe_align_runs
 * until the store changes.  seed_rows 0 is the loggers' rule, 20 that of realign_clusters_within_run. */
int sbe_align_within(sbe_align* h, int seed_rows, int8_t* perm_out);
/* Membership counts int32 [n_runs][K][N] over the rows s >= burn_rows[r] of every run; aligned != 0: through the
 * permutations of the last sbe_align_within (SBE_ERR_STATE if there are none), else as stored. */
int sbe_align_counts(sbe_align* h, int aligned, const int64_t* burn_rows, int32_t* counts_out);
/* One permutation per run against run `pivot`, from the counts above (aligned, burn_rows: as for sbe_align_counts).
 * run_perm_out: int8 [n_runs][K]; agreement_out: int64 [n_runs][K][K], the matrices d the permutations were chosen on. */
int sbe_align_runs(sbe_align* h, int pivot, int aligned, const int64_t* burn_rows, int8_t* run_perm_out, int64_t* agreement_out);

/* device time of the last sbe_align_within's kernel (HIP events), in milliseconds */
int sbe_align_last_kernel_ms(const sbe_align* h, float* ms_out);

#ifdef __cplusplus
}
#endif

#endif /* SBE_ALIGN_H */
