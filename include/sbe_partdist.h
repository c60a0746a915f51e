/* sbe_partdist.h -- C ABI of the pairwise distances between cluster samples on the device.
 *
 * sbe_consensus.h reduces a posterior to one [N][N] matrix before anything is compared.  This unit compares the samples with
 * each other, with no label matching: Binder's distance, the variation of information and what the (adjusted) Rand index
 * needs, for all pairs of samples of a block, their sums per run, and the raw contingency tables of listed pairs.
 *
 *   - a handle owns a STORE of R runs of cluster samples c[r][s][k][n] in {0,1}, as sbe_consensus.h's: rows are appended
 *     per run, as uint8 [n][K][N], in pieces of any size.  The areas of a sample must be DISJOINT (the measures below are
 *     partition measures): an appended call is scanned on the host before its first piece goes to the device, and a byte
 *     other than 0 / 1 or an object in two areas of one sample is SBE_ERR_DATA; the store is then unchanged.
 *   - on the device the rows are held in two forms: a sample-major FP4 operand image for the matrix pipe,
 *     [run][row K_pad + k][N_pad / 2 bytes] (K_pad the power of two >= K, N_pad = N rounded up to SBE_PARTDIST_ROUND; object
 *     i is nibble i & 7 of dword i >> 3, 0x0 or 0x2; the rows k >= K and the objects >= N are zero; a run's rows are
 *     padded to whole tiles of 32), and bit rows [run][row][K][ceil(N/32)], from which the area sizes are counted.
 *
 * A sample is a partition of the N objects into K + 1 blocks: block 0 the objects in no area, blocks 1..K the areas.
 * Samples are ordered by (run, row).
 *
 * The contract (tests/_partdist_oracle.py restates it in NumPy; DESIGN.md section 23 states it).  For samples x and y:
 *   n[k][l] = sum_i x[k][i] y[l][i]; a_k, b_l the area sizes.  The extended table E is (K+1) x (K+1):
 *       E[k][l] = n[k][l] (k, l >= 1), E[k][0] = a_k - sum_l n[k][l], E[0][l] = b_l - sum_k n[k][l],
 *       E[0][0] = N - sum a - sum b + sum n;  the extended sizes a+ = (N - sum a, a_1 .. a_K), b+ likewise.
 *   binder(x,y) = sum_k a_k^2 + sum_l b_l^2 - 2 sum_kl n[k][l]^2, int32, exact, at most 2 N^2 = 2^29: the ordered object
 *       pairs, diagonal included, that share an area in exactly one of the two samples (section 19's delta).  For the
 *       samples of a selection with similarity counts C: sum_t binder(s,t) = score[s] + sum_ij C[i][j].
 *   sumsq(x,y) = sum_kl E[k][l]^2, int32, at most N^2 = 2^28: with the sizes, what the Rand and adjusted Rand index of the
 *       (K+1)-block partitions need.
 *   vi(x,y) = max(0, ((h_x + h_y) - 2 j) / N), float64, in nats, with x the EARLIER of the two samples in (run, row) order
 *       (so vi(y,x) = vi(x,y)), h_x = sum_{k=0..K} L[a+_k], h_y = sum_{l=0..K} L[b+_l], j = sum_{k=0..K} sum_{l=0..K}
 *       L[E[k][l]], k major and l minor.  Every sum runs left to right from 0.0 in float64, without contraction.  L is the
 *       caller's table, float64 [N+1], L[0] = 0 and L[m] = m log m, handed over at reset: the device never takes a log,
 *       so device and oracle agree bit for bit given the table.  On the diagonal, and for two samples with the same
 *       blocks in the same label order, the value is exactly 0.0.
 *   sums: for every sample s of the selected runs and every selected run r', binder_sum[s][r'] = sum_{t in r'} binder(s,t),
 *       int64, exact; vi_sum[s][r'] float64 in one fixed tree: 64 lanes, lane j adds t = j, j + 64, .. of run r' onto 0.0,
 *       then xor exchanges at distances 32 .. 1.  The tree does not depend on tile geometry or launch chunking.
 *   tables: n[k][l] of listed pairs, int32 [K][K], from the bit rows by AND and population count on the vector pipe: what
 *       a user inspects for a pair, and an independent check of the matrix pipe's counts.
 *
 * Limits (SBE_ERR_ARG beyond them, checked before any device call): 1 <= K <= SBE_PARTDIST_MAX_CLUSTERS; 1 <= N <=
 * SBE_PARTDIST_MAX_OBJECTS; at most SBE_PARTDIST_MAX_RUNS runs of at most SBE_PARTDIST_MAX_ROWS rows;
 * sbe_partdist_image_bytes(...) <= SBE_PARTDIST_MAX_IMAGE_BYTES; a block of at most SBE_PARTDIST_MAX_BLOCK entries; a
 * selection of at most SBE_PARTDIST_MAX_SUM_ROWS samples for the sums; at most SBE_PARTDIST_MAX_PAIRS listed pairs.
 *
 * Conventions are those of sbe_engine.h: every function returns SBE_OK (0) or an SBE_ERR_* code with the message in
 * sbe_partdist_last_error(); nothing throws across the boundary; arguments are checked before any device call; calls are
 * synchronous; the caller owns every host buffer.  The symbols are exported by the same library as the engine's.
 */
#ifndef SBE_PARTDIST_H
#define SBE_PARTDIST_H

#include <stdint.h>

#include "sbe_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sbe_partdist sbe_partdist;

#define SBE_PARTDIST_ABI_VERSION 1

/* limits (SBE_ERR_ARG beyond them) */
#define SBE_PARTDIST_MAX_CLUSTERS 8                /* K                                                                  */
#define SBE_PARTDIST_MAX_OBJECTS 16384             /* N: binder <= 2 N^2 = 2^29 and sumsq <= N^2 = 2^28 fit an int32, a count <= N is exact in the f32 accumulator */
#define SBE_PARTDIST_MAX_RUNS 64                   /* runs in the store                                                  */
#define SBE_PARTDIST_MAX_ROWS (1 << 20)            /* S_r: samples per run (and the store's capacity)                    */
#define SBE_PARTDIST_ROUND 256                     /* objects per round of the tile kernel's loop: a row of the image is padded to whole rounds */
#define SBE_PARTDIST_MAX_IMAGE_BYTES (1ll << 34)   /* operand image plus bit rows of a store: 16 GiB                     */
#define SBE_PARTDIST_MAX_BLOCK (1 << 28)           /* n_rows n_cols of one block call                                    */
#define SBE_PARTDIST_MAX_SUM_ROWS (1 << 16)        /* samples of a selection for the sums: 2^32 pairs, a call stays in seconds */
#define SBE_PARTDIST_MAX_PAIRS (1 << 24)           /* listed pairs of one tables call                                    */

int sbe_partdist_abi_version(void);
/* the message of the last failed call on `h` (NULL: of the last failed call of this thread) */
const char* sbe_partdist_last_error(const sbe_partdist* h);
/* Device bytes of a store of this shape: the operand image, n_runs runs of capacity_rows K_pad rows (rounded up to 32) of
 * N_pad / 2 bytes, plus the bit rows, n_runs capacity_rows K ceil(N/32) words.  0 for a shape outside the limits above
 * (the byte limit is the caller's to compare).  No device call. */
int64_t sbe_partdist_image_bytes(int n_runs, int n_clusters, int64_t n_objects, int64_t capacity_rows);

int sbe_partdist_create(sbe_partdist** out, int device);
int sbe_partdist_destroy(sbe_partdist* h);
/* Shape the store: n_runs runs of up to capacity_rows samples of n_clusters x n_objects bits, all empty.  xlogx: float64
 * [n_objects + 1], the table L of the contract (copied to the device).  Device memory only grows; what the store held is
 * forgotten. */
int sbe_partdist_reset(sbe_partdist* h, int n_runs, int n_clusters, int64_t n_objects, int64_t capacity_rows, const double* xlogx);
/* append host rows to one run: uint8 [n_rows][K][N] of 0 / 1, C order, disjoint areas per sample (SBE_ERR_DATA otherwise,
 * and the store is unchanged).  A call that fails on the device (SBE_ERR_HIP) leaves the store without a shape: reset comes next. */
int sbe_partdist_append_rows(sbe_partdist* h, int run, const uint8_t* rows, int64_t n_rows);
/* rows stored for one run */
int sbe_partdist_rows(const sbe_partdist* h, int run, int64_t* n_rows_out);

/* the area sizes of every stored sample of `run`, counted from the bit rows when the rows were appended: int32 [rows(run)][K] */
int sbe_partdist_sizes(sbe_partdist* h, int run, int32_t* sizes_out);
/* The measures of the samples [row_first, row_first + n_rows) of row_run against [col_first, col_first + n_cols) of col_run:
 * dense [n_rows][n_cols] each.  Any output may be NULL, at least one must not be. */
int sbe_partdist_block(sbe_partdist* h, int row_run, int64_t row_first, int64_t n_rows, int col_run, int64_t col_first, int64_t n_cols,
                       int32_t* binder_out, double* vi_out, int32_t* sumsq_out);
/* The sums over the runs r with run_mask[r] != 0 (uint8 [n_runs]): [T_sel][R_sel], the samples in (run, row) order and the
 * runs in run order; R_sel counts every selected run, T_sel the rows they hold.  Either output may be NULL, not both.
 * SBE_ERR_STATE for a selection that holds no rows. */
int sbe_partdist_sums(sbe_partdist* h, const uint8_t* run_mask, int64_t* binder_sum_out, double* vi_sum_out);
/* The raw tables of listed pairs: pairs int64 [n_pairs][4] (run, row, run, row), tables_out int32 [n_pairs][K][K], the
 * first sample's areas along the rows. */
int sbe_partdist_tables(sbe_partdist* h, const int64_t* pairs, int64_t n_pairs, int32_t* tables_out);

/* tiles per launch of the tile kernel; 0: the default, chosen so that no launch runs long.  The results do not depend on
 * the value, bit for bit. */
int sbe_partdist_set_launch_tiles(sbe_partdist* h, int64_t tile_pairs);
/* device time of the kernels of the last block, sums or tables call (HIP events), in milliseconds */
int sbe_partdist_last_kernel_ms(const sbe_partdist* h, float* ms_out);

#ifdef __cplusplus
}
#endif

#endif /* SBE_PARTDIST_H */
