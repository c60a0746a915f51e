/* sbe_objloo.h -- C ABI of the leave-one-object-out ELPD with the cluster membership integrated out, on the device: had this
 * object (a language, a site) not been documented at all, how well would the fitted model have predicted it, and what would
 * it have predicted for each of its cells?
 *
 * sbe_elpd.h and sbe_loopred.h score one observed cell at a time, and every score is conditional on the object's logged
 * membership z_n, a per-object latent variable fitted to the very cells being scored.  For comparing numbers of clusters the
 * unit of a latent-variable model is the object with its local latent integrated out (Merkle, Furr & Rabe-Hesketh 2019; the
 * integrated importance sampling of Vehtari et al. 2016).  This unit forms, per logged sample t and object n,
 *     L[t][n]   = log sum_j prior_j exp(H[t][n][j]),     H[t][n][j] = sum_f log m_j[n][f][x]
 * over the hypotheses j = 0 ("in no cluster") and j = 1 .. K ("in cluster j - 1"), with sbe_contrib.h's counterfactual rows
 * m0 and m_k, runs PSIS over the T values of an object, keeps the weights and runs the samples past them a second time:
 *     p_loo[n][f][s] = sum_t w_t(n) sum_j prior_j m_j[n][f][s]
 * for every cell of the object, with a code or without one.  Everything is conditional on the logged effect draws, as in
 * sbe_predict.h.
 *
 * The data and a sample are sbe_predict.h's word for word, with its limits, its six validation kinds and their order: codes
 * uint8 [N][F] (255 = NA), groups uint8 [C-1][N] with n_groups, K clusters; per sample clusters uint8 [K][N], weights float64
 * [F][C], tables float64 [R][F][S].  Each sample additionally carries
 *     prior float64 [N][K+1]   the conditional prior probability of "no cluster" (index 0) and of clusters 1 .. K for every
 *                              object.  NULL means 1.0 / (K + 1) everywhere.  Entries must be finite and >= 0 and a row must
 *                              sum (in index order) to within SBE_PREDICT_SUM_TOL of 1; a bad row is a seventh validation kind,
 *                              "prior row", checked on the device after the six, naming the (sample, object).  A zero entry
 *                              excludes that hypothesis.
 * With T samples in all, three phases (tests/_objloo_oracle.py restates them in fp64 in this order):
 *   1. rows     sbe_objloo_add, any number of calls; on SBE_ERR_DATA nothing is stored.  Per sample t, object n, hypothesis j:
 *                 m_0 is sbe_contrib.h's m0 and m_{k+1} its m_k, the same operations in the same order, bit for bit (a_c, wsum1,
 *                 wsum0, w1_c, w0_c; where wsum0 is not > 0 every w0_c is 0, where wsum1 is not > 0 every w1_c is 0).
 *                 H[t][n][j] = sum over the cells f with a code x of log m_j[n][f][x], the device library's float64 log, in
 *                 sbe_ppc.h's per-object tree: 64 lanes, lane i adds the features i, i + 64, .. in order onto 0 (a cell without
 *                 a code adds +0.0), then the lanes are folded by xor exchanges at distances 32, 16, .. 1.  Every bit is
 *                 therefore independent of the feature tile and of how the samples are split over calls.  log 0 = -inf: a
 *                 hypothesis with an observed cell whose m is not > 0 is -inf as a whole.
 *                 An observed cell to which no confounder applies (wsum0 not > 0) is SBE_ERR_DATA, naming the cell and the sample.
 *                 Cnd[t][n] = H[t][n][z], z = 1 + the logged cluster of n in t, 0 if none.
 *                 a_j = log(prior_j) + H[t][n][j];  mx = max_j a_j (fmax in index order);
 *                 L[t][n] = mx + log(sum_j exp(a_j - mx)), the sum in index order onto 0.
 *                 Cnd or L not finite is SBE_ERR_DATA, naming the first (object, sample).
 *                 H, a, Cnd and L stay on the device, column-major (an object's samples contiguous); nothing is copied back.
 *   2. weights  sbe_objloo_weights.  Per object PSIS over the T values of L, and again over Cnd, exactly as
 *                 tests/_elpd_oracle.psis_column(ll) does for a float64 ll: the ratios are -ll, reff = 1, the maximum subtracted,
 *                 the cutoff floored at log DBL_MIN, the tail strictly above the cutoff in (value, sample) order (a stable
 *                 argsort), _gpdfit and _gpinv for more than four tail values, truncation at 0, lw = x' - logsumexp(x').
 *                 Per object: loo_i = logsumexp(lw + ll), k_i, n_eff_i = 1 / sum_t w_t^2 with w_t = exp(lw_t), and
 *                 lppd_i = logsumexp(ll) - log T for the marginal column; loo_cond_i, k_cond_i, lppd_cond_i for the conditional
 *                 one.  The marginal w[n][t] are kept on the device.  In the same pass
 *                 membership[n][j] = (1 / T) sum_t exp(a_j[t] - L[t]): the Rao-Blackwellised membership probabilities.
 *                 Every sum is a fixed tree: thread i of 256 adds the samples i, i + 256, .. in order onto 0, the 64 lanes of a
 *                 wave are folded by xor exchanges at distances 32 .. 1, the four waves are added in order.  No output depends
 *                 on the store's capacity or on how the store was filled.  Fewer than SBE_ELPD_MIN_SAMPLES rows: SBE_ERR_STATE.
 *   3. accumulate  sbe_objloo_accumulate(t0, n, .. the same samples and priors ..); t0 is the index of the call's first sample
 *                 and the calls cover 0 .. T in order without gaps (SBE_ERR_STATE otherwise).  For every cell of every object,
 *                 with a code or without one, and every state s:
 *                     mz = sum_j prior_j m_j[n][f][s], j in index order onto 0, every product rounded, then added; no FMA
 *                     p_loo[n][f][s] += w_t(n) mz, the product rounded, then added, in float64, in sample order.
 *                 A cell's accumulators are held by one thread for the whole call (sbe_predict.h's rule), so the sums are
 *                 bit-identical for every split of the samples and every feature tile.  The call's H and a are recomputed with
 *                 phase 1's code and compared with the store bit for bit; a sample that differs is SBE_ERR_DATA, naming the
 *                 sample, and the sums are left as they were.
 * Pareto k is an output and has to be read: with few samples many objects have k > 0.7, and their weights are unreliable.
 * `prior` must be the model's conditional prior of the membership (uniform under a uniform area prior).  Labels must be
 * aligned (sbe_align.h) for membership's columns 1 .. K to mean one cluster each.
 *
 * Conventions are those of sbe_loopred.h and sbe_engine.h: every function returns SBE_OK (0) or an SBE_ERR_* code with the
 * message in sbe_objloo_last_error(); nothing throws across the boundary; arguments are checked before any device call; calls
 * are synchronous; the caller owns every host buffer.  The symbols are exported by the same library as the engine's.
 */
#ifndef SBE_OBJLOO_H
#define SBE_OBJLOO_H

#include <stdint.h>

#include "sbe_elpd.h"
#include "sbe_predict.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sbe_objloo sbe_objloo;

#define SBE_OBJLOO_ABI_VERSION 1

/* limits (SBE_ERR_ARG beyond them); the shape's are sbe_predict.h's */
#define SBE_OBJLOO_MAX_SAMPLES SBE_ELPD_MAX_SAMPLES          /* T: the capacity of the store, in samples                        */
#define SBE_OBJLOO_MAX_STORE_BYTES (1ll << 34)               /* the store: N * capacity * 8 * (2 (K + 1) + 3) bytes             */
#define SBE_OBJLOO_MAX_STAGE_BYTES SBE_PREDICT_MAX_STAGE_BYTES    /* the samples of one add / accumulate call on the device    */
#define SBE_OBJLOO_MAX_TILE SBE_PREDICT_MAX_TILE

int sbe_objloo_abi_version(void);
/* the message of the last failed call on `h` (NULL: of the last failed call of this thread) */
const char* sbe_objloo_last_error(const sbe_objloo* h);

int sbe_objloo_create(sbe_objloo** out, int device);
int sbe_objloo_destroy(sbe_objloo* h);
/* device time of the kernels of the last add, weights or accumulate call (HIP events), in ms */
int sbe_objloo_last_kernel_ms(const sbe_objloo* h, float* ms_out);

/* Device bytes of the store for n_objects objects, n_clusters clusters and `capacity` samples: float64 H and a per hypothesis,
 * L, Cnd and w.  -1 if an argument is negative, n_clusters is 0 or capacity is beyond SBE_OBJLOO_MAX_SAMPLES.  Beyond
 * SBE_OBJLOO_MAX_STORE_BYTES set_data refuses the shape. */
int64_t sbe_objloo_store_bytes(int64_t n_objects, int n_clusters, int64_t capacity);
/* Device bytes one sample of an add or accumulate call takes while the call runs: sbe_predict_sample_bytes(.., 0), the log of
 * every (hypothesis, cell) (8 (K + 1) N F), its sums (8 (K + 1) N) and the prior (8 (K + 1) N).  0 for a shape beyond the limits. */
int64_t sbe_objloo_sample_bytes(int64_t n_objects, int64_t n_features, int n_states, int n_components, int n_clusters, int n_rows);
/* largest T whose sort keys (value, sample) and tail sbe_objloo_weights holds in LDS; longer columns are sorted in a slice
 * of global memory per workgroup (the same code, the same comparisons) */
int64_t sbe_objloo_lds_max_samples(void);

/* The data of sbe_predict_set_data and the capacity of the store in samples, 1 .. SBE_OBJLOO_MAX_SAMPLES.  The store is
 * emptied and the sums are zeroed.  Device memory only grows. */
int sbe_objloo_set_data(sbe_objloo* h, int64_t n_objects, int64_t n_features, int n_states, int n_components, int n_clusters,
                        const uint8_t* codes, const uint8_t* groups, const int* n_groups, int64_t capacity);
/* Forget the rows, the weights and the sums, keep the data and the capacity. */
int sbe_objloo_reset(sbe_objloo* h);

/* Phase 1.  n samples as in sbe_predict_accumulate and prior float64 [n][N][K+1] or NULL; n * sbe_objloo_sample_bytes <=
 * SBE_OBJLOO_MAX_STAGE_BYTES and the rows stored so far + n <= capacity (SBE_ERR_ARG beyond either).  On SBE_ERR_DATA nothing
 * was stored.  A call after sbe_objloo_weights discards the weights and the sums: phase 2 comes again. */
int sbe_objloo_add(sbe_objloo* h, int64_t n, const uint8_t* clusters, const double* weights, const double* tables, const double* prior);
/* Phase 2.  float64 [N] each: loo_i, k_i, n_eff_i, lppd_i (marginal), loo_cond_i, k_cond_i, lppd_cond_i (conditional on the
 * logged membership); membership float64 [N][K+1].  SBE_ERR_STATE with fewer than SBE_ELPD_MIN_SAMPLES rows.  Zeroes the sums:
 * phase 3 starts at t0 = 0. */
int sbe_objloo_weights(sbe_objloo* h, double* loo_i, double* k_i, double* n_eff_i, double* lppd_i, double* loo_cond_i, double* k_cond_i,
                       double* lppd_cond_i, double* membership);
/* Phase 3.  The samples [t0, t0 + n) of phase 1, with their priors. */
int sbe_objloo_accumulate(sbe_objloo* h, int64_t t0, int64_t n, const uint8_t* clusters, const double* weights, const double* tables,
                          const double* prior);
/* p_loo float64 [N][F][S] (may be NULL); *n_samples_out: the samples accumulated since phase 2 (the sums are complete once
 * that is T). */
int sbe_objloo_read(sbe_objloo* h, double* p_loo, int64_t* n_samples_out);

/* Test hooks, not part of what a caller needs.  The features of a workgroup's tile, as sbe_predict_set_feature_tile: the
 * results do not depend on it, bit for bit. */
int sbe_objloo_set_feature_tile(sbe_objloo* h, int features);
/* The store as it stands, column-major and compact: H float64 [N][K+1][T], L, Cnd and w float64 [N][T] (each may be NULL; w
 * needs phase 2). */
int sbe_objloo_get_store(sbe_objloo* h, double* H, double* L, double* Cnd, double* w);

#ifdef __cplusplus
}
#endif

#endif /* SBE_OBJLOO_H */
