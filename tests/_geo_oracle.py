"""NumPy fp64 restatement of the cost-based geo prior of sBayes (sbayes/model/prior.py: GeoPrior.__call__,
GeoPrior.get_costs_per_object, compute_mst_distances): the checker of sbayes_amd.geo.  tests/golden/geo_prior.npz holds
what the reference itself returned.

Numerical contract (sbayes_amd.geo and the kernels of csrc/sbe_geo.hip implement the same):

* a cluster is a mask over N objects, its members in ascending order i_0 < ... < i_{m-1}; m = 0 is an error;
* MST skeleton: the multiset of edge weights of a minimum spanning tree of the complete graph on the members, an edge
  {a, b} weighing min(cost[a, b], cost[b, a]) (SciPy takes both stored entries as candidates of one undirected edge),
  zero-weight edges dropped (SciPy eliminates them from its result).  The multiset does not depend on how ties are
  broken.  `prim` takes the edges in the order of Prim's algorithm from i_0, ties to the lowest member, and adds the
  non-zero ones in that order: n_edges, sum, max.  No non-zero edge (m = 1, all costs zero): the edge set is {0}, that is
  n_edges 0, sum 0, max 0.  mean = sum / max(n_edges, 1): over the non-zero edges, as the reference takes it;
* complete-graph skeleton: all m * m entries of the sub-matrix (diagonal, both triangles): n_edges = m * m, sum, max;
* probability function: exponential -x / scale; sigmoid log_expit(-(x - x0) / s) - log_expit(x0 / s) with the stable
  log_expit(t) = t - log1p(exp(t)) for t < 0, -log1p(exp(-t)) otherwise.  The reference picks scipy.special.log_expit by
  the string comparison scipy.__version__ >= '1.8.0' -- false for SciPy 1.15 -- and then runs log(expit(t)), which is -inf
  below t = -745 and carries the rounding of expit(t) near 1; the two forms agree to that rounding above t = -700;
* costs_per_object: ctc[n] = min over members of cost[member, n] (exact); before = the aggregate of the MST skeleton,
  whatever skeleton is configured; after = (ctc + m before) / (1 + m) (mean), ctc + before (sum), max(ctc, before) (max);
  the result is f(after) - f(before) for all N objects.

Error bounds the tests use (derived, not tuned), u = 2^-53:
* m, n_edges, max, ctc: exact;
* sum: a sum of n non-negative terms in any order lies within (n - 1) u of the exact sum, relatively: `sum_bound`;
* aggregate: the sum's bound, one more rounding for the mean's division: `aggregate_bound`;
* exponential: the aggregate's bound and one more rounding for -x / scale;
* sigmoid (`sigmoid_bound`, absolute): the argument t = -(x - x0) / s carries dx / s from the aggregate plus two roundings
  (the difference and the quotient), |dt| <= |x| rel / s + 2 u |t|; d log_expit / dt = expit(-t) <= 1; each of the two
  terms and their difference is rounded once: expit(-t) |dt| + u (|L1| + |L2| + |L1 - L2|).  Against the recorded reference
  (log(expit(t)) form) each term also carries expit's own rounding, u in absolute terms: + 2 u.  Whoever evaluates exp
  and log1p adds their error per term: `libm` (relative to |L1| + |L2|) is that allowance -- HOST_LIBM for the C library
  under NumPy and SciPy (glibc documents 1 ulp = 2 u for exp and for log1p; with the final rounding 5 u per side, 8 u
  for an oracle-against-SciPy comparison), and for the device four times the largest error measured over a fixed grid
  (profiles/geo/log_expit_error.json, written by tests/test_gpu_geo.py's measurement);
* costs_per_object: `before` carries the aggregate's bound, `after` the same or less (ctc is exact; mean: three more
  roundings; sum: one), and the result is the difference of two values of f: the sum of their two bounds plus one
  rounding of the difference."""
from __future__ import annotations

import numpy as np

U = 2.0 ** -53
HOST_LIBM = 8 * U
SKELETONS = ("mst", "complete_graph")
AGGREGATIONS = ("mean", "sum", "max")
PROBABILITY_FUNCTIONS = ("exponential", "sigmoid")


def euclidean_cost(xy):
    """float64 [N, N]: the Euclidean distances of points [N, 2], sqrt(dx dx + dy dy) (two terms: no summation order)."""
    xy = np.asarray(xy, dtype=np.float64)
    dx, dy = xy[:, None, 0] - xy[None, :, 0], xy[:, None, 1] - xy[None, :, 1]
    return np.sqrt(dx * dx + dy * dy)


def members(mask):
    idx = np.flatnonzero(np.asarray(mask))
    if idx.size == 0:
        raise ValueError("the mask has no member")
    return idx


def edge_weights(cost, idx):
    """[m, m]: the weight of the undirected edge between two members."""
    sub = np.asarray(cost, dtype=np.float64)[np.ix_(idx, idx)]
    return np.minimum(sub, sub.T)


def prim(w):
    """The m - 1 edge weights of a minimum spanning tree of the complete graph with weights w [m, m], in the order Prim's
    algorithm from vertex 0 takes them (ties to the lowest vertex)."""
    m = w.shape[0]
    key = w[0].copy()
    in_tree = np.zeros(m, dtype=bool)
    in_tree[0] = True
    out = np.empty(max(m - 1, 0), dtype=np.float64)
    for step in range(m - 1):
        k = np.where(in_tree, np.inf, key)
        u = int(np.argmin(k))                    # (the first of equal keys)
        out[step] = k[u]
        in_tree[u] = True
        key = np.minimum(key, w[u])
    return out


def skeleton(cost, mask, skeleton="mst"):
    """dict(m, n_edges, sum, max, mean) of one mask."""
    idx = members(mask)
    m = idx.size
    if skeleton == "complete_graph":
        sub = np.asarray(cost, dtype=np.float64)[np.ix_(idx, idx)]
        n_edges, total, largest = m * m, float(np.sum(sub)), float(np.max(sub))
    elif skeleton == "mst":
        edges = prim(edge_weights(cost, idx))
        edges = edges[edges != 0]
        n_edges, total, largest = edges.size, 0.0, 0.0
        for e in edges:                          # in Prim's order
            total += float(e)
        if n_edges:
            largest = float(edges.max())
    else:
        raise ValueError(f"skeleton {skeleton!r} is not covered")
    return dict(m=m, n_edges=n_edges, sum=total, max=largest, mean=total / max(n_edges, 1))


def log_expit(t):
    t = np.asarray(t, dtype=np.float64)
    with np.errstate(over="ignore"):
        return np.where(t < 0, t - np.log1p(np.exp(np.minimum(t, 0))), -np.log1p(np.exp(-np.maximum(t, 0))))


def log_expit_grid():
    """The fixed grid of arguments over which the device's log_expit is measured against scipy.special.log_expit: evenly
    from -2000 to 700 (beyond, exp(-t) is subnormal), densely around 0, and the places where the forms change."""
    return np.concatenate([np.linspace(-2000.0, 700.0, 27001), np.linspace(-40.0, 40.0, 16001), np.linspace(-1.0, 1.0, 8001),
                           [-745.2, -744.0, -709.9, -700.0, -36.8, -1e-8, -1e-300, 0.0, 1e-300, 1e-8, 36.8, 37.5, 699.9]])


def probability(x, probability_function, scale, inflection_point=None):
    x = np.asarray(x, dtype=np.float64)
    if probability_function == "exponential":
        return -x / scale
    if probability_function == "sigmoid":
        return log_expit(-(x - inflection_point) / scale) - log_expit(inflection_point / scale)
    raise ValueError(f"probability function {probability_function!r} is not covered")


def geo_prior(cost, masks, scale, aggregation="mean", probability_function="exponential", inflection_point=None, skeleton_type="mst"):
    """float64 [B]: the log prior of every mask of [B, N]."""
    agg = [skeleton(cost, mk, skeleton_type)[aggregation] for mk in np.asarray(masks).reshape(-1, np.shape(masks)[-1])]
    return probability(np.array(agg), probability_function, scale, inflection_point).reshape(np.shape(masks)[:-1])


def costs_per_object(cost, mask, scale, aggregation="mean", probability_function="exponential", inflection_point=None):
    """(result [N], ctc [N])."""
    cost = np.asarray(cost, dtype=np.float64)
    idx = members(mask)
    m = idx.size
    ctc = cost[idx].min(axis=0)
    before = skeleton(cost, mask, "mst")[aggregation]
    if aggregation == "mean":
        after = (ctc + m * before) / (1 + m)
    elif aggregation == "sum":
        after = ctc + before
    else:
        after = np.maximum(ctc, before)
    f = lambda x: probability(x, probability_function, scale, inflection_point)      # noqa: E731
    return f(after) - f(before), ctc


# ---- the host expression: SciPy's own MST, as the reference calls it ---------------------------------------------------
def scipy_mst_edges(sub):
    """The non-zero edge weights of SciPy's minimum spanning tree of a dense sub-matrix (inf = no edge); zeros(1) when
    none is left or there is a single member."""
    from scipy.sparse.csgraph import csgraph_from_dense, minimum_spanning_tree
    if sub.shape[0] <= 1:
        return np.zeros(1)
    tree = minimum_spanning_tree(csgraph_from_dense(sub, null_value=np.inf))
    if tree.nnz == 0:
        return np.zeros(1)
    return np.asarray(tree.tocsr()[tree.nonzero()]).ravel()


_NP_AGG = {"mean": np.mean, "sum": np.sum, "max": np.max}


def scipy_geo_prior(cost, masks, scale, aggregation="mean", probability_function="exponential", inflection_point=None,
                    skeleton_type="mst"):
    out = []
    for mk in np.asarray(masks).reshape(-1, np.shape(masks)[-1]):
        sub = cost[mk][:, mk]
        edges = scipy_mst_edges(sub) if skeleton_type == "mst" else sub
        out.append(_NP_AGG[aggregation](edges))
    return probability(np.array(out), probability_function, scale, inflection_point).reshape(np.shape(masks)[:-1])


def scipy_costs_per_object(cost, mask, scale, aggregation="mean", probability_function="exponential", inflection_point=None):
    m = np.count_nonzero(mask)
    ctc = np.min(cost[mask], axis=0)
    before = _NP_AGG[aggregation](scipy_mst_edges(cost[mask][:, mask]))
    after = {"mean": lambda: (ctc + m * before) / (1 + m), "sum": lambda: ctc + before, "max": lambda: np.maximum(ctc, before)}[aggregation]()
    f = lambda x: probability(x, probability_function, scale, inflection_point)      # noqa: E731
    return f(after) - f(before)


# ---- bounds (module docstring) -------------------------------------------------------------------------------------------
def sum_bound(n_edges):
    """Relative bound between two sums of the same n non-negative terms."""
    return np.maximum(np.asarray(n_edges, dtype=np.float64) - 1, 0) * U


def aggregate_bound(aggregation, n_edges):
    if aggregation == "max":
        return np.zeros(np.shape(n_edges))
    return sum_bound(n_edges) + (U if aggregation == "mean" else 0.0)


def expit(t):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(t, dtype=np.float64)))


def probability_bound(x, x_rel, probability_function, scale, inflection_point=None, libm=0.0, reference_form=False):
    """Absolute bound on f(x) where x carries the relative bound x_rel."""
    x = np.asarray(x, dtype=np.float64)
    if probability_function == "exponential":
        return (x_rel + U) * np.abs(x / scale)
    t = -(x - inflection_point) / scale
    dt = np.abs(x) * x_rel / scale + 2 * U * np.abs(t)
    l1, l2 = log_expit(t), log_expit(inflection_point / scale)
    terms = np.abs(l1) + np.abs(l2)
    return expit(-t) * dt + U * (terms + np.abs(l1 - l2)) + libm * terms + (2 * U if reference_form else 0.0)


def costs_per_object_bound(ctc, m, before, n_edges, aggregation, probability_function, scale, inflection_point=None, libm=0.0,
                           reference_form=False):
    """Absolute bound on f(after) - f(before), per object."""
    rel_before = aggregate_bound(aggregation, n_edges)
    if aggregation == "mean":
        after = (ctc + m * before) / (1 + m)
        rel_after = rel_before + 3 * U
    elif aggregation == "sum":
        after = ctc + before
        rel_after = rel_before + U
    else:
        after = np.maximum(ctc, before)
        rel_after = rel_before
    kw = dict(libm=libm, reference_form=reference_form)
    fa = probability(after, probability_function, scale, inflection_point)
    fb = probability(before, probability_function, scale, inflection_point)
    return (probability_bound(after, rel_after, probability_function, scale, inflection_point, **kw)
            + probability_bound(before, rel_before, probability_function, scale, inflection_point, **kw) + U * np.abs(fa - fb))
