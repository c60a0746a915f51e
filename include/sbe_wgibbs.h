/* sbe_wgibbs.h -- C ABI of the on-device step of the Gibbs weights operator.
 *
 * sBayes' GibbsSampleWeights._propose (sbayes/sampling/operators.py:597-676) picks two mixture components i1, i2, draws a new
 * split a2 of their joint weight per feature from a beta distribution built on source counts, and accepts or rejects
 * the new weight row of every feature on its own.  Everything of that step that draws no random number runs here, on
 * the resident state of an engine slot (group ids, source, weights):
 *
 *   sbe_wgibbs_pair_counts   per feature, the objects whose has_components pattern has both components and whose
 *                            source is i1 (column 0) / i2 (column 1); NA observations count for neither.  Exact.
 *   sbe_wgibbs_step          w02 = w[i1] + w[i2] (float32); w_new[i1] = float32((1 - a2) w02), w_new[i2] = float32(a2 w02);
 *                            the row divided by its float32 sum in NumPy's order; a2_old = w[i2] / w02 (float32).  Then, in
 *                            float64 and without any lgamma (ln B(alpha) and betaln are the same on both sides):
 *                              d_lh    = sum over the non-NA observations of log wn_new - log wn_old at the observation's
 *                                        pattern and source component (float32 per-pattern normalised weights; no source
 *                                        component: log 0 on both sides)
 *                              d_prior = sum_c (alpha - 1) (log w_new - log w), a term with alpha == 1 being 0
 *                              d_q     = (A - 1) (log a2_old - log a2) + (B - 1) (log1p(-a2_old) - log1p(-a2)), a term
 *                                        whose coefficient is 0 being 0
 *                              log_p   = (d_lh + d_prior + d_q) / prior_temperature
 *                            accept = (double)u < exp(log_p) (a NaN rejects); weights_out = accept ? w_new : w.
 * The contract is written out in tests/_wgibbs_oracle.py.  Every sum is taken in a fixed order and
 * there are no float atomics: results are bit-identical run to run.  The slot itself is left untouched, and nothing is
 * kept between the two calls.
 *
 * Conventions are those of sbe_engine.h: every function returns SBE_OK (0) or an SBE_ERR_* code with the message in
 * sbe_last_error(e); nothing throws across the boundary; arguments are checked before any device call; calls are
 * synchronous; the caller owns every host buffer.  The symbols are exported by the same library as the engine's.
 */
#ifndef SBE_WGIBBS_H
#define SBE_WGIBBS_H

#include <stdint.h>

#include "sbe_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SBE_WGIBBS_ABI_VERSION 1

/* features of one workgroup of both kernels (x 64 object lanes) */
#define SBE_WGIBBS_FEATURE_TILE 16

int sbe_wgibbs_abi_version(void);

/* SBE_ERR_ARG unless 0 <= i1, i2 < C and i1 != i2; SBE_ERR_STATE unless the slot's groups, source and weights are set. */
int sbe_wgibbs_pair_counts(sbe_engine* e, int slot, int i1, int i2, int32_t* counts_out /* [F][2] */);

/* a2 float64 [F], u float32 [F], alpha float64 [F][C] (the Dirichlet concentration of the weights prior), beta_ab
 * float64 [F][2] (A, B of the beta proposal).  prior_temperature positive and finite (SBE_ERR_ARG otherwise).
 * weights_out float32 [F][C], accept_out uint8 [F], log_p_out float64 [F] (may be NULL). */
int sbe_wgibbs_step(sbe_engine* e, int slot, int i1, int i2, const double* a2, const float* u, const double* alpha /* [F][C] */,
                    const double* beta_ab /* [F][2] */, double prior_temperature, float* weights_out /* [F][C] */,
                    uint8_t* accept_out /* [F] */, double* log_p_out /* [F], may be NULL */);

#ifdef __cplusplus
}
#endif

#endif /* SBE_WGIBBS_H */
