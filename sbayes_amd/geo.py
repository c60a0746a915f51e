"""The cost-based geo prior on the device: the MST skeleton of a cluster (include/sbe_geo.h).

With `geo: {type: cost_based}` sBayes' GeoPrior (sbayes/model/prior.py) takes, per cluster, the cost sub-matrix of its
members through `scipy.sparse.csgraph.minimum_spanning_tree`, aggregates the tree's edges and applies a probability
function: once per changed cluster in `GeoPrior.__call__`, and once per AlterCluster / AlterClusterWide proposal in
`GeoPrior.get_costs_per_object`.  This module runs both on the GPU, one workgroup per cluster mask:

    h = handle_for(device); h.set_cost(cost)                       # float64 [N, N], resident until replaced
    h.skeleton_costs(masks, skeleton="mst")                        # SkeletonCosts: m, n_edges, sum, max, mean per mask
    geo_prior(masks, scale=..., aggregation="mean", probability_function="exponential", inflection_point=None,
              skeleton="mst")                                      # float64, shaped like masks without its last axis
    costs_per_object(mask, scale=..., aggregation=..., probability_function=..., inflection_point=...)   # float64 [N]
    patch.install(geo_prior=True)                                  # swaps both methods of the reference's GeoPrior

Covered: type cost_based with skeleton mst or complete_graph, aggregation mean / sum / max, probability function
exponential / sigmoid.  Not covered (the patched methods run the reference's own body): simulated, and the skeletons
delaunay and diameter.

Numerical contract (tests/_geo_oracle.py restates it in NumPy).  The MST skeleton is the multiset
of edge weights of a minimum spanning tree over the members, an edge weighing min(cost[a, b], cost[b, a]), zero-weight
edges dropped, as SciPy returns it; the mean is over the non-zero edges, not over m - 1; no non-zero edge (m = 1, all
costs zero) is the edge set {0}.  The complete graph takes all m * m entries.  Sums run in a fixed order in fp64, so
results are bit-identical run to run, for any batch position and any launch chunking.  The sigmoid uses the stable
log_expit (t - log1p(exp(t)) below 0, -log1p(exp(-t)) from 0 on).  The reference picks scipy.special.log_expit by the
string comparison scipy.__version__ >= '1.8.0', which is false for SciPy 1.15, and then runs log(expit(t)): -inf below
t = -745.  The device form is the stable one the reference intends; the two agree to rounding above t = -700.
Limits: N <= 32768, 2^20 masks per call, an empty mask and a non-finite cost are errors.

`HOST_BELOW_MEMBERS`: under patch.install(geo_prior=True) a cluster with fewer members than this stays on the
reference's host path.  It is 0: tools/geo_speed.py on an MI355X (profiles/geo/geo_speed.json) found the device form
faster than the host expression at every size measured, the smallest (N, m) = (100, 20) included.

Handles follow the package's process model (sbayes_amd/_proc.py): one per device, created lazily in the process that
uses it, never pickled, forgotten (not destroyed) in a fork()ed child, where every further call raises."""
from __future__ import annotations

import ctypes as ct
from dataclasses import dataclass

import numpy as np

from . import _handle
from ._handle import _ptr, c_handle_p

ABI_VERSION = 1                          # SBE_GEO_ABI_VERSION of include/sbe_geo.h
MAX_OBJECTS = 32768                      # SBE_GEO_MAX_OBJECTS
MAX_MASKS = 1 << 20                      # SBE_GEO_MAX_MASKS
MAX_LAUNCH_MASKS = 1 << 16               # SBE_GEO_MAX_LAUNCH_MASKS
LDS_MEMBERS = 128                        # SBE_GEO_LDS_MEMBERS
SKELETONS = {"mst": 0, "complete_graph": 1}
AGGREGATIONS = {"mean": 0, "sum": 1, "max": 2}
PROBABILITY_FUNCTIONS = {"exponential": 0, "sigmoid": 1}
HOST_BELOW_MEMBERS = 0                   # (module docstring)

# name -> (restype, argtypes); mirrors include/sbe_geo.h one to one (the engine's own table, _lib.PROTOTYPES, is not extended)
PROTOTYPES = {
    **_handle.unit_prototypes("sbe_geo"),
    "sbe_geo_create": (ct.c_int, [ct.POINTER(c_handle_p), ct.c_int]),
    "sbe_geo_set_launch_masks": (ct.c_int, [c_handle_p, ct.c_int64]),
    "sbe_geo_set_cost": (ct.c_int, [c_handle_p, ct.c_void_p, ct.c_int64]),
    "sbe_geo_skeleton": (ct.c_int, [c_handle_p, ct.c_void_p, ct.c_int64, ct.c_int, ct.c_void_p, ct.c_void_p, ct.c_void_p,
                                    ct.c_void_p]),
    "sbe_geo_prior": (ct.c_int, [c_handle_p, ct.c_void_p, ct.c_int64, ct.c_int, ct.c_int, ct.c_int, ct.c_double, ct.c_double,
                                 ct.c_void_p]),
    "sbe_geo_costs_per_object": (ct.c_int, [c_handle_p, ct.c_void_p, ct.c_int, ct.c_int, ct.c_double, ct.c_double, ct.c_void_p,
                                            ct.c_void_p]),
    "sbe_geo_log_expit": (ct.c_int, [c_handle_p, ct.c_void_p, ct.c_int64, ct.c_void_p]),
    "sbe_geo_last_shape": (ct.c_int, [c_handle_p, ct.POINTER(ct.c_int64), ct.POINTER(ct.c_int64)]),
}


def load():
    """The engine library with the prototypes of include/sbe_geo.h attached."""
    return _handle.bind("sbe_geo", PROTOTYPES, ABI_VERSION)


@dataclass
class SkeletonCosts:
    """Per mask: the member count, the number of non-zero skeleton edges (m * m entries for the complete graph), their
    sum, max and mean (sum / max(n_edges, 1))."""
    m: np.ndarray
    n_edges: np.ndarray
    sum: np.ndarray
    max: np.ndarray
    mean: np.ndarray

    def aggregate(self, aggregation):
        return {"mean": self.mean, "sum": self.sum, "max": self.max}[_choice(aggregation, AGGREGATIONS, "aggregation")[0]]


# ---- validation (host side, before any library call) -----------------------------------------------------------
def _choice(value, table, what):
    name = str(getattr(value, "value", value))            # (the reference's string enums pass as they are)
    if name not in table:
        raise ValueError(f"{what} must be one of {sorted(table)}, got {value!r}")
    return name, table[name]


def _check_cost(cost):
    c = np.asarray(cost)
    if c.ndim != 2 or c.shape[0] != c.shape[1] or c.shape[0] < 1:
        raise ValueError(f"cost must be a square [N, N] matrix, got shape {c.shape}")
    if c.shape[0] > MAX_OBJECTS:
        raise ValueError(f"{c.shape[0]} objects; the cost matrix is limited to {MAX_OBJECTS} (8 GiB)")
    return np.ascontiguousarray(c, dtype=np.float64)


def _check_masks(masks, n):
    a = np.asarray(masks)
    if a.dtype != np.bool_ and not np.issubdtype(a.dtype, np.integer):
        raise TypeError(f"masks must be bool (or integer, non-zero = member), got {a.dtype}")
    if a.ndim < 1 or a.shape[-1] != n:
        raise ValueError(f"masks must end in N = {n} objects, got shape {a.shape}")
    flat = np.ascontiguousarray(a.reshape(-1, n) != 0).view(np.uint8)
    if flat.shape[0] > MAX_MASKS:
        raise ValueError(f"{flat.shape[0]} masks; one call takes at most {MAX_MASKS} (2^20)")
    empty = np.flatnonzero(~flat.any(axis=1))
    if empty.size:
        raise ValueError(f"mask {int(empty[0])} has no member")
    return flat, a.shape[:-1]


def _check_function(scale, probability_function, inflection_point):
    name, pf = _choice(probability_function, PROBABILITY_FUNCTIONS, "probability_function")
    if not (np.isfinite(scale) and scale > 0):
        raise ValueError(f"scale={scale} must be positive and finite")
    if name == "sigmoid":
        if inflection_point is None or not np.isfinite(inflection_point):
            raise ValueError(f"the sigmoid needs a finite inflection_point, got {inflection_point!r}")
        return pf, float(scale), float(inflection_point)
    return pf, float(scale), 0.0


class GeoHandle(_handle.UnitHandle):
    """Owner of one sbe_geo handle: a stream, the cost matrix and the scratch of the last call on one device.
    last_kernel_ms(): the kernels of the last call."""
    _prefix, _noun = "sbe_geo", "a geo-prior handle"

    def __init__(self, device=0):
        self.n_objects = 0
        self.cost_key = None
        self._create_on(load, device)

    def set_launch_masks(self, masks):
        """Masks per launch of the skeleton kernel (0: the default).  Results do not depend on it."""
        self._check(self._lib.sbe_geo_set_launch_masks(self._h, int(masks)))

    def set_cost(self, cost, key=None):
        """The cost matrix (float64 [N, N]) goes to the device and stays.  `key`: an identity under which the upload is
        skipped when the same matrix is set again."""
        if key is not None and key == self.cost_key and self.n_objects:
            return
        c = _check_cost(cost)
        self.n_objects, self.cost_key = 0, None
        self._check(self._lib.sbe_geo_set_cost(self._h, _ptr(c), c.shape[0]))
        self.n_objects, self.cost_key = c.shape[0], key

    def _need_cost(self):
        if not self.n_objects:
            self._check(self._lib.sbe_geo_prior(self._h, None, 0, 0, 0, 0, 1.0, 0.0, None))     # (SBE_ERR_STATE, in its words)

    def skeleton_costs(self, masks, skeleton="mst") -> SkeletonCosts:
        """m, n_edges, sum, max, mean of the skeleton of every mask ([..., N]); the outputs take the leading shape."""
        self._need_cost()
        sk = _choice(skeleton, SKELETONS, "skeleton")[1]
        flat, shape = _check_masks(masks, self.n_objects)
        b = flat.shape[0]
        m, ne = np.empty(b, dtype=np.int32), np.empty(b, dtype=np.int64)
        total, largest = np.empty(b, dtype=np.float64), np.empty(b, dtype=np.float64)
        self._check(self._lib.sbe_geo_skeleton(self._h, _ptr(flat), b, sk, _ptr(m), _ptr(ne), _ptr(total), _ptr(largest)))
        mean = total / np.maximum(ne, 1)
        return SkeletonCosts(*(a.reshape(shape) for a in (m, ne, total, largest, mean)))

    def prior(self, masks, scale, aggregation="mean", probability_function="exponential", inflection_point=None, skeleton="mst"):
        """float64, shaped like masks without its last axis: the log prior of every mask."""
        self._need_cost()
        sk = _choice(skeleton, SKELETONS, "skeleton")[1]
        agg = _choice(aggregation, AGGREGATIONS, "aggregation")[1]
        pf, scale, x0 = _check_function(scale, probability_function, inflection_point)
        flat, shape = _check_masks(masks, self.n_objects)
        out = np.empty(flat.shape[0], dtype=np.float64)
        self._check(self._lib.sbe_geo_prior(self._h, _ptr(flat), flat.shape[0], sk, agg, pf, scale, x0, _ptr(out)))
        return out.reshape(shape)

    def costs_per_object(self, mask, scale, aggregation="mean", probability_function="exponential", inflection_point=None,
                         with_cost_to_cluster=False):
        """float64 [N]: the change of the log prior of `mask` per object that would join it (with_cost_to_cluster: and the
        cost of every object to the cluster, min over the members' rows)."""
        self._need_cost()
        agg = _choice(aggregation, AGGREGATIONS, "aggregation")[1]
        pf, scale, x0 = _check_function(scale, probability_function, inflection_point)
        a = np.asarray(mask)
        if a.ndim != 1:
            raise ValueError(f"costs_per_object takes one mask [N], got shape {a.shape}")
        flat, _shape = _check_masks(a, self.n_objects)
        ctc, out = np.empty(self.n_objects, dtype=np.float64), np.empty(self.n_objects, dtype=np.float64)
        self._check(self._lib.sbe_geo_costs_per_object(self._h, _ptr(flat), agg, pf, scale, x0, _ptr(ctc), _ptr(out)))
        return (out, ctc) if with_cost_to_cluster else out

    def log_expit(self, t):
        """log_expit(t) as the device evaluates it inside the sigmoid (float64, any shape)."""
        a = np.ascontiguousarray(t, dtype=np.float64)
        flat = a.reshape(-1)
        out = np.empty_like(flat)
        self._check(self._lib.sbe_geo_log_expit(self._h, _ptr(flat), flat.size, _ptr(out)))
        return out.reshape(a.shape)

    def last_shape(self):
        """(launches of the skeleton kernel, masks that took the LDS path) of the last call."""
        launches, lds_masks = ct.c_int64(0), ct.c_int64(0)
        self._check(self._lib.sbe_geo_last_shape(self._h, ct.byref(launches), ct.byref(lds_masks)))
        return launches.value, lds_masks.value


_HANDLES = _handle.device_cache()          # device -> GeoHandle


def release_all():
    _handle.release_cached(_HANDLES)


def handle_for(device=0) -> GeoHandle:
    """The process's handle on `device`, created on first use."""
    return _handle.cached_handle(_HANDLES, GeoHandle, device)


# ---- plain functions over the handle of a device (its cost matrix set by handle_for(device).set_cost) ------------------
def geo_prior(masks, *, scale, aggregation="mean", probability_function="exponential", inflection_point=None, skeleton="mst",
              device=0):
    """The log geo prior of every cluster mask: [B, N] -> [B], [n_samples, K, N] -> [n_samples, K], in one call."""
    return handle_for(device).prior(masks, scale, aggregation, probability_function, inflection_point, skeleton)


def costs_per_object(mask, *, scale, aggregation="mean", probability_function="exponential", inflection_point=None, device=0):
    """GeoPrior.get_costs_per_object for one cluster mask [N]: float64 [N]."""
    return handle_for(device).costs_per_object(mask, scale, aggregation, probability_function, inflection_point)


# ---- the device forms of the reference's two methods (patch.install(geo_prior=True)) ----------------------------------
def covered(prior, for_call=True):
    """Does the device form cover this GeoPrior?  cost_based, a covered aggregation and probability function, and -- for
    __call__, which alone follows the configured skeleton -- skeleton mst or complete_graph."""
    try:
        if str(getattr(prior.prior_type, "value", prior.prior_type)) != "cost_based" or prior.cost_matrix is None:
            return False
        if str(getattr(prior.aggregation_policy, "value", prior.aggregation_policy)) not in AGGREGATIONS:
            return False
        pf = str(getattr(prior.probability_function, "value", prior.probability_function))
        if pf not in PROBABILITY_FUNCTIONS or (pf == "sigmoid" and prior.inflection_point is None):
            return False
        skeleton = prior.config.skeleton
        return not for_call or str(getattr(skeleton, "value", skeleton)) in SKELETONS
    except AttributeError:
        return False


def _handle_of(prior, make=None):
    from .registry import default_device
    h = (make or handle_for)(default_device())
    cost = prior.cost_matrix
    h.set_cost(cost, key=(id(cost), np.shape(cost)))
    return h


def geo_prior_call(prior, sample, caching=True, make=None):
    """Device form of GeoPrior.__call__ (prior.py:769-805) for a covered prior: the changed clusters go to the device in
    one call and their values into the reference's own cache node."""
    cache = sample.cache.geo_prior
    if caching and not cache.is_outdated():
        return cache.value.sum()
    h = _handle_of(prior, make)
    with cache.edit() as geo_priors:
        changed = [int(i) for i in cache.what_changed("clusters", caching=caching)]
        if changed:
            masks = np.asarray(sample.clusters.value)[changed]
            geo_priors[changed] = h.prior(masks, prior.scale, prior.aggregation_policy, prior.probability_function,
                                          prior.inflection_point, prior.config.skeleton)
    return cache.value.sum()


def get_costs_per_object(prior, sample, i_cluster, make=None):
    """Device form of GeoPrior.get_costs_per_object (prior.py:824-852) for a covered prior."""
    h = _handle_of(prior, make)
    return h.costs_per_object(np.asarray(sample.clusters.value)[i_cluster], prior.scale, prior.aggregation_policy,
                              prior.probability_function, prior.inflection_point)
