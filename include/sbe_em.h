/* sbe_em.h -- C ABI of the on-device EM cluster initializer.
 *
 * sBayes starts every chain with SbayesInitializer.generate_sample, which runs generate_clusters_em
 * (sbayes/sampling/initializers.py:93-169) once per attempt: n_em_steps (default 50) steps of a soft assignment z [G][N]
 * of the N objects to the G = K + sum(confounder groups) groups.  This header is the device form of those steps; the
 * draws (total_size, the uniforms of z0) and the discretization stay on the host, in the reference's own methods.
 *
 * One EM step, all in fp64 on the device (the contract is written out in tests/_em_oracle.py):
 *   counts[g,f,s] = sum_n z[g,n] [x_nf = s]                   (NA observations contribute nothing; ascending n)
 *   p[g,f,s]      = (counts + 0.5 applicable[f,s]) / sum_s (counts + 0.5 applicable[f,s])
 *   logp[g,f,s]   = log p;   logp[g,f,S] = log sum_s p        (the NA column)
 *   ll[g,n]       = sum_f logp[g,f,x_nf]                      (ascending f)
 *   with a cost matrix:  zp = softmax(N z[:K], over n);  geo[k,n] = -(sum_m zp[k,m] cost[m,n]) / scale / 2;
 *                        geo[g >= K, n] = logsumexp(geo[:K]) - log(K N);   else geo = 0
 *   z[:,n]        = softmax over g of (available ? geo + ll / T_i : -inf)
 * Every sum runs in a fixed order (no float atomics): results are bit-identical run to run and for any split of the
 * steps into calls.  T_i comes from the caller (the reference's own double).
 *
 * Conventions are those of sbe_engine.h: every function returns SBE_OK (0) or an SBE_ERR_* code with the message in
 * sbe_em_last_error(); nothing throws across the boundary; arguments are checked before any device call; calls are
 * synchronous; the caller owns every host buffer.  The symbols are exported by the same library as the engine's.
 */
#ifndef SBE_EM_H
#define SBE_EM_H

#include <stdint.h>

#include "sbe_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sbe_em sbe_em;

#define SBE_EM_ABI_VERSION 1

/* limits (SBE_ERR_ARG beyond them) */
#define SBE_EM_MAX_STATES 254                       /* S: the NA index S must fit a uint8, as in the engine            */
#define SBE_EM_MAX_GROUPS 1024                      /* G = K + sum of confounder groups                                */
#define SBE_EM_MAX_OBJECTS (1 << 20)                /* N                                                               */
#define SBE_EM_MAX_FEATURES (1 << 16)               /* F                                                               */
#define SBE_EM_MAX_COST_BYTES ((int64_t)8 << 30)    /* the cost matrix: N * N * 8 bytes (N <= 32768)                   */
#define SBE_EM_MAX_STEPS (1 << 20)                  /* steps in one sbe_em_run call                                    */

int sbe_em_abi_version(void);
/* the message of the last failed call on `h` (NULL: of the last failed call of this thread) */
const char* sbe_em_last_error(const sbe_em* h);

/* A handle on `device` holding the data of one initializer:
 *   state_idx        uint8 [N][F]: the observed state of object n, feature f; S for a missing observation (NA);
 *   applicable       uint8 [F][S]: non-zero where state s applies to feature f (data.features.states);
 *   groups_available uint8 [G][N]: non-zero where object n may belong to group g; rows [0, K) are the clusters.
 * SBE_ERR_DATA if a state index exceeds S, a feature has no applicable state, or an object has no available group. */
int sbe_em_create(sbe_em** out, int device, int64_t n_objects, int64_t n_features, int64_t n_states, const uint8_t* state_idx,
                  const uint8_t* applicable, int64_t n_groups, int64_t n_clusters, const uint8_t* groups_available);
int sbe_em_destroy(sbe_em* h);
/* Turn the cost-based geo prior on: cost float64 [N][N] (C order), scale > 0 and finite.  cost == NULL turns it off.
 * SBE_ERR_DATA if a cost is not finite. */
int sbe_em_set_geo_cost(sbe_em* h, const double* cost, double scale);
/* n_steps EM steps from z_in (float64 [G][N]) with the temperatures T_i (float64 [n_steps], finite and > 0); z after the
 * last step into z_out (float64 [G][N]; may equal z_in).  n_steps == 0 copies z_in.  SBE_ERR_DATA if a column of z_in
 * holds a non-finite value or sums to 0, or if a step produced a non-finite z. */
int sbe_em_run(sbe_em* h, const double* z_in, int64_t n_steps, const double* temperatures, double* z_out);
/* device time of the steps of the last successful sbe_em_run (HIP events around them), in milliseconds */
int sbe_em_last_kernel_ms(const sbe_em* h, float* ms_out);

#ifdef __cplusplus
}
#endif

#endif /* SBE_EM_H */
