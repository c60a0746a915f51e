/* sbe_geo.h -- C ABI of the on-device cost-based geo prior (the MST skeleton of a cluster).
 *
 * sBayes' geographic prior with `geo: {type: cost_based}` (sbayes/model/prior.py, GeoPrior) takes, per cluster, the cost
 * sub-matrix of its members, the edges of a skeleton over them (a minimum spanning tree, or the complete graph), an
 * aggregate of the edge costs (mean, sum, max) and a probability function of the aggregate (exponential, sigmoid).
 * GeoPrior.get_costs_per_object gives, for every object, the change of that log-probability if the object joined the
 * cluster.  This header is the device form of both; the contract is written out in tests/_geo_oracle.py (DESIGN.md
 * section 14).
 *
 *   members        i_0 < ... < i_{m-1}: the objects where the mask is non-zero (m == 0: SBE_ERR_DATA)
 *   MST skeleton   the multiset of edge weights of a minimum spanning tree of the complete graph on the members, edge
 *                  {a, b} weighing min(cost[a][b], cost[b][a]) (SciPy treats both entries as candidates of one undirected
 *                  edge), with the zero-weight edges dropped: n_edges of them, their sum (added in the order Prim's
 *                  algorithm from i_0 takes them, ties to the lowest member) and their max.  No edge left (m == 1, or
 *                  all weights zero): n_edges 0, sum 0, max 0.  mean = sum / max(n_edges, 1): over the non-zero edges,
 *                  as the reference takes it, not over m - 1
 *   complete       all m * m entries of the sub-matrix, diagonal and both triangles: n_edges = m * m, sum, max
 *   probability    exponential: -x / scale;  sigmoid: log_expit(-(x - x0) / s) - log_expit(x0 / s) with
 *                  log_expit(t) = t - log1p(exp(t)) for t < 0, -log1p(exp(-t)) otherwise.  (With a SciPy whose version
 *                  string compares below '1.8.0' -- 1.15 does -- the reference runs log(expit(t)) instead, which is
 *                  -inf below t = -745; the device form is the stable one the reference intends.)
 *   per object     ctc[n] = min over members of cost[member][n];  before = the aggregate of the MST skeleton (whatever
 *                  skeleton the prior is configured with, as in the reference);  after = (ctc + m before) / (1 + m)
 *                  (mean), ctc + before (sum), max(ctc, before) (max);  out[n] = f(after[n]) - f(before)
 * All in fp64, no float atomics, every sum in a fixed order: results are bit-identical run to run, for any position of a
 * mask in the batch and for any launch chunking.
 *
 * Conventions are those of sbe_engine.h: every function returns SBE_OK (0) or an SBE_ERR_* code with the message in
 * sbe_geo_last_error(); nothing throws across the boundary; arguments are checked before any device call; calls are
 * synchronous; the caller owns every host buffer.  The symbols are exported by the same library as the engine's.
 */
#ifndef SBE_GEO_H
#define SBE_GEO_H

#include <stdint.h>

#include "sbe_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sbe_geo sbe_geo;

#define SBE_GEO_ABI_VERSION 1

/* limits (SBE_ERR_ARG beyond them) */
#define SBE_GEO_MAX_OBJECTS 32768                   /* N: the cost matrix takes N * N * 8 bytes, 8 GiB at the limit      */
#define SBE_GEO_MAX_MASKS (1 << 20)                 /* masks in one call                                                 */
#define SBE_GEO_MAX_LAUNCH_MASKS (1 << 16)          /* masks in one launch (sbe_geo_set_launch_masks)                    */
/* a mask of up to this many members has its m x m sub-matrix staged in LDS (128 KiB at the limit); a larger one reads one
 * cost row per step of Prim's algorithm from memory.  The arithmetic is the same on both paths. */
#define SBE_GEO_LDS_MEMBERS 128

#define SBE_GEO_SKELETON_MST 0
#define SBE_GEO_SKELETON_COMPLETE 1
#define SBE_GEO_AGG_MEAN 0
#define SBE_GEO_AGG_SUM 1
#define SBE_GEO_AGG_MAX 2
#define SBE_GEO_PROB_EXPONENTIAL 0
#define SBE_GEO_PROB_SIGMOID 1

int sbe_geo_abi_version(void);
/* the message of the last failed call on `h` (NULL: of the last failed call of this thread) */
const char* sbe_geo_last_error(const sbe_geo* h);

int sbe_geo_create(sbe_geo** out, int device);
int sbe_geo_destroy(sbe_geo* h);
/* masks per launch of the skeleton kernel (0: the default, chosen from N so that the scratch memory of a launch stays
 * bounded).  Results do not depend on it, bit for bit. */
int sbe_geo_set_launch_masks(sbe_geo* h, int64_t masks);
/* The cost matrix, float64 [N][N] (C order), copied to the device where it stays until the next call.  SBE_ERR_DATA if a
 * cost is not finite (the handle then holds no matrix). */
int sbe_geo_set_cost(sbe_geo* h, const double* cost, int64_t n_objects);

/* The skeleton of every mask (uint8 [n_masks][N], non-zero = member): m (int32), n_edges (int64), sum and max (float64),
 * [n_masks] each.  SBE_ERR_STATE before sbe_geo_set_cost; SBE_ERR_DATA for a mask without a member. */
int sbe_geo_skeleton(sbe_geo* h, const uint8_t* masks, int64_t n_masks, int skeleton, int32_t* m_out, int64_t* n_edges_out,
                     double* sum_out, double* max_out);
/* The log prior of every mask: the probability function of the aggregate of its skeleton, float64 [n_masks].  scale > 0
 * and finite; inflection_point finite (read by the sigmoid only). */
int sbe_geo_prior(sbe_geo* h, const uint8_t* masks, int64_t n_masks, int skeleton, int aggregation, int probability_function,
                  double scale, double inflection_point, double* out);
/* The change of the log prior of one mask (uint8 [N]) per object that would join it: out float64 [N]; ctc_out (may be
 * NULL) float64 [N], the cost of every object to the cluster. */
int sbe_geo_costs_per_object(sbe_geo* h, const uint8_t* mask, int aggregation, int probability_function, double scale,
                             double inflection_point, double* ctc_out, double* out);

/* log_expit(t) as the device evaluates it inside the sigmoid, for n values (float64 [n], n <= SBE_GEO_MAX_MASKS): what the
 * tests measure the device's exp / log1p with. */
int sbe_geo_log_expit(sbe_geo* h, const double* t, int64_t n, double* out);

/* of the last successful skeleton / prior / costs_per_object call: the launches of the skeleton kernel and how many of
 * the masks took the LDS path */
int sbe_geo_last_shape(const sbe_geo* h, int64_t* launches_out, int64_t* lds_masks_out);
/* device time of the kernels of that call (HIP events), in milliseconds */
int sbe_geo_last_kernel_ms(const sbe_geo* h, float* ms_out);

#ifdef __cplusplus
}
#endif

#endif /* SBE_GEO_H */
