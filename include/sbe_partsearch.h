/* sbe_partsearch.h -- C ABI of the search for the partition that minimises the expected VI or Binder loss, on the device.
 *
 * sbe_partdist.h's medoid and sbe_consensus.h's least-squares estimate can only return one of the logged samples.  This
 * unit searches over partitions: greedy single-object reallocation sweeps that minimise the Monte-Carlo expected loss,
 * from many starts (the sweetening phase of Dahl, Johnson and Mueller 2022; the greedy search of Wade and Ghahramani 2018),
 * and it evaluates listed candidates against every stored sample (the credible ball around an estimate).
 *
 *   - a handle owns a STORE of T cluster samples c[t][k][n] in {0,1} with DISJOINT areas, as sbe_partdist.h's: rows are
 *     appended as uint8 [n][K][N], in pieces of any size; an appended call is scanned on the host before its first piece
 *     goes to the device, and a byte other than 0 / 1 or an object in two areas of one sample is SBE_ERR_DATA; the store
 *     is then unchanged.  The store has no runs: the samples of several runs are appended one after the other.
 *   - on the device the store is the labels, object-major: lab[N][capacity] uint8, y[t][i] = 0 for an object in no area
 *     and k + 1 for area k.  A thread per sample reads one object's labels coalesced.
 *
 * The contract (tests/_partsearch_oracle.py restates it in NumPy, in the kernel's order; DESIGN.md section 27 states it).
 * B = K + 1.  A candidate c is uint8 [N] with labels in 0..K; blocks may be empty.  For a candidate and sample t,
 * E_t[q][l] counts the objects with c = q and y[t] = l: the extended table of sbe_partdist.h with the candidate along the
 * rows; a_q are the candidate's extended sizes and b_t[l] the sample's.  L is the caller's table, float64 [N+1], L[0] = 0
 * and L[m] = m log m, handed over at reset; dL[m] = L[m+1] - L[m] is one float64 subtraction, formed on the device.
 *   vi(c,t)     = max(0, ((h_c + h_t) - 2 j_t) / N), h_c = sum_q L[a_q], h_t = sum_l L[b_t[l]], j_t = sum_q sum_l
 *                 L[E_t[q][l]] (q major); every sum runs left to right from 0.0 in float64, without contraction.
 *   binder(c,t) = sum_{q>=1} a_q^2 + sum_{l>=1} b_l^2 - 2 sum_{q,l>=1} E_t[q][l]^2, int32.
 *                 Both equal sbe_partdist_block's values bit for bit, with the candidate stored as run 0 and the samples
 *                 as run 1.
 *   sums        binder_sum = sum_t binder(c,t), int64, exact; vi_sum = sum_t vi(c,t) in one fixed tree: 256 threads,
 *                 thread j adds t = j, j + 256, .. onto 0.0, the 64 lanes of a wave are exchanged by xor at distances
 *                 32 .. 1, then the four waves are added in index order.
 *   object step for object i with label p: remove i (a_p -= 1, E_t[p][y[t][i]] -= 1 for all t), score every q in 0..K,
 *                 VI:     g(q) = T dL[a_q] - 2 S_q, S_q the sum over t of dL[E_t[q][y[t][i]]] in the tree above; T dL is
 *                         one product, 2 S_q is exact, then one subtraction;
 *                 Binder: g(0) = 0, g(q) = T (2 a_q + 1) - 2 sum_{t: y >= 1} (2 E_t[q][y] + 1) for q >= 1, int64, exact;
 *                 choose the smallest g (among equal values p if it is one of them, else the smallest q); put i there.
 *   search of one start: the tables are built once from init[N]; sweeps visit the objects in order[N] (a permutation);
 *                 the search stops after a sweep without a move, or after max_sweeps.  Starts are independent, and no
 *                 output bit depends on how the starts are split over calls, how the rows were appended in pieces or any
 *                 launch setting.  There are no floating-point atomics.
 *
 * On the device a start is one workgroup of 256 threads, persistent over all sweeps, one launch per call.  Its tables
 * live in global scratch, E[start][B][B][T_pad] uint16 (a count is at most N <= 16384), sample-minor, T_pad = T rounded up
 * to SBE_PARTSEARCH_THREADS; a thread owns the samples t = j, j + 256, .. and nobody else touches their columns.  The
 * candidate lives in LDS; its sizes live in registers (every thread holds the same).  The ORDER IS READ FROM GLOBAL MEMORY,
 * one step ahead: no workgroup takes more than 16 KiB of LDS for N objects, and the read is off the step's path.
 *
 * Limits (SBE_ERR_ARG beyond them, checked before any device call): 1 <= K <= SBE_PARTSEARCH_MAX_CLUSTERS; 1 <= N <=
 * SBE_PARTSEARCH_MAX_OBJECTS; a capacity of at most SBE_PARTSEARCH_MAX_ROWS samples; 1 <= max_sweeps <=
 * SBE_PARTSEARCH_MAX_SWEEPS; sbe_partsearch_scratch_bytes(K, T, starts) <= SBE_PARTSEARCH_MAX_SCRATCH_BYTES for the starts
 * of one search call and the candidates of one evaluate call (the caller splits them over calls).
 *
 * Conventions are those of sbe_engine.h: every function returns SBE_OK (0) or an SBE_ERR_* code with the message in
 * sbe_partsearch_last_error(); nothing throws across the boundary; arguments are checked before any device call; calls
 * are synchronous; the caller owns every host buffer.  The symbols are exported by the same library as the engine's.
 */
#ifndef SBE_PARTSEARCH_H
#define SBE_PARTSEARCH_H

#include <stdint.h>

#include "sbe_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sbe_partsearch sbe_partsearch;

#define SBE_PARTSEARCH_ABI_VERSION 1

/* limits (SBE_ERR_ARG beyond them) */
#define SBE_PARTSEARCH_MAX_CLUSTERS 8                /* K: sbe_partdist.h's                                                */
#define SBE_PARTSEARCH_MAX_OBJECTS 16384             /* N: sbe_partdist.h's; a count fits a uint16, binder an int32         */
#define SBE_PARTSEARCH_MAX_ROWS (1 << 16)            /* T and the store's capacity: SBE_PARTDIST_MAX_SUM_ROWS              */
#define SBE_PARTSEARCH_MAX_SWEEPS 1024               /* max_sweeps of one search                                           */
#define SBE_PARTSEARCH_THREADS 256                   /* threads of a start's workgroup: the tree of the sums               */
#define SBE_PARTSEARCH_MAX_SCRATCH_BYTES (1ll << 30) /* the tables of one call's starts or candidates: 1 GiB               */

/* losses */
#define SBE_PARTSEARCH_LOSS_VI 0
#define SBE_PARTSEARCH_LOSS_BINDER 1

int sbe_partsearch_abi_version(void);
/* the message of the last failed call on `h` (NULL: of the last failed call of this thread) */
const char* sbe_partsearch_last_error(const sbe_partsearch* h);
/* Device bytes of the tables of `n_starts` starts (or candidates) against n_samples samples: n_starts (K+1)^2 T_pad
 * uint16.  0 for a shape outside the limits above (the byte limit is the caller's to compare).  No device call. */
int64_t sbe_partsearch_scratch_bytes(int n_clusters, int64_t n_samples, int64_t n_starts);

int sbe_partsearch_create(sbe_partsearch** out, int device);
int sbe_partsearch_destroy(sbe_partsearch* h);
/* Shape the store: up to capacity_rows samples of n_clusters x n_objects bits, empty.  xlogx: float64 [n_objects + 1], the
 * table L of the contract (copied to the device, where dL is formed).  Device memory only grows; what the store held is
 * forgotten. */
int sbe_partsearch_reset(sbe_partsearch* h, int n_clusters, int64_t n_objects, int64_t capacity_rows, const double* xlogx);
/* append host rows: uint8 [n_rows][K][N] of 0 / 1, C order, disjoint areas per sample (SBE_ERR_DATA otherwise, with the
 * sample and the object in the message, and the store is unchanged).  A call that fails on the device (SBE_ERR_HIP) leaves
 * the store without a shape: reset comes next. */
int sbe_partsearch_append_rows(sbe_partsearch* h, const uint8_t* rows, int64_t n_rows);
/* samples stored */
int sbe_partsearch_rows(const sbe_partsearch* h, int64_t* n_rows_out);

/* n_starts searches against the T stored samples.  loss: SBE_PARTSEARCH_LOSS_*.  init: uint8 [n_starts][N], labels in 0..K;
 * order: int32 [n_starts][N], a permutation of 0..N-1 per start (SBE_ERR_DATA otherwise, naming the start and the entry;
 * nothing has run then).  Outputs per start: labels_out uint8 [n_starts][N]; sweeps_out int32, the sweeps made; moves_out
 * int64, the objects moved; converged_out uint8, 1 if the last sweep moved nothing; binder_sum_out int64 and vi_sum_out
 * float64, the sums of the final labels (both, whatever the loss); trace_out, which may be NULL: float64
 * [n_starts][max_sweeps], the sum of `loss` after each sweep, NaN behind the last.  SBE_ERR_STATE before reset or with no rows. */
int sbe_partsearch_search(sbe_partsearch* h, int loss, int64_t n_starts, const uint8_t* init, const int32_t* order, int max_sweeps,
                          uint8_t* labels_out, int32_t* sweeps_out, int64_t* moves_out, uint8_t* converged_out, int64_t* binder_sum_out,
                          double* vi_sum_out, double* trace_out);
/* n candidates against the T stored samples: labels uint8 [n][N] in 0..K (SBE_ERR_DATA otherwise); vi_out float64 [n][T],
 * binder_out int32 [n][T], vi_sum_out float64 [n], binder_sum_out int64 [n].  Any output may be NULL, at least one must
 * not be.  It is what a search ends with.  SBE_ERR_STATE before reset or with no rows. */
int sbe_partsearch_evaluate(sbe_partsearch* h, int64_t n, const uint8_t* labels, double* vi_out, int32_t* binder_out, double* vi_sum_out,
                            int64_t* binder_sum_out);

/* device time of the kernel of the last search or evaluate call (HIP events), in milliseconds */
int sbe_partsearch_last_kernel_ms(const sbe_partsearch* h, float* ms_out);

#ifdef __cplusplus
}
#endif

#endif /* SBE_PARTSEARCH_H */
