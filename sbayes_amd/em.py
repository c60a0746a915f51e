"""The EM cluster initializer on the device (include/sbe_em.h).

sBayes starts every chain with SbayesInitializer.generate_sample, which runs generate_clusters_em
(sbayes/sampling/initializers.py:93-169) once per attempt: 50 dense EM steps over groups x objects x features x states.
This module runs those steps on the GPU:

    z = run_em(features, applicable, groups_available, n_clusters, z0, temperatures(50))   # plain arrays
    generate_clusters_em(initializer)            # the device form of the method (patch.install(em_init=True) swaps it in)

Numerical contract (tests/_em_oracle.py restates it): every step in fp64 on the device with every sum
in a fixed order, so results are bit-identical run to run and for any split of the steps into calls; T_i is the
reference's own double, computed here; z is rounded to the reference's dtype (float32, float64 with the cost-based geo
prior) before the reference's own discretize_fuzzy_cluster_2 sees it.  The reference carries float32, so the initial
clusters can differ from an unpatched run's on objects near a tie in that discretization.

Handles follow the package's process model (sbayes_amd/_proc.py): created lazily in the process that uses them, on the
device of that process's engine (registry.default_device), never pickled, forgotten (not destroyed) in a fork()ed child.
The handle of an initializer's data is cached per data object: a chain initializes the same data 10 x 10 times."""
from __future__ import annotations

import ctypes as ct
import weakref

import numpy as np

from . import _handle, _proc
from ._handle import _ptr, c_handle_p

ABI_VERSION = 1                          # SBE_EM_ABI_VERSION of include/sbe_em.h
MAX_STATES = 254                         # SBE_EM_MAX_STATES
MAX_GROUPS = 1024                        # SBE_EM_MAX_GROUPS
MAX_OBJECTS = 1 << 20                    # SBE_EM_MAX_OBJECTS
MAX_FEATURES = 1 << 16                   # SBE_EM_MAX_FEATURES
MAX_COST_BYTES = 8 << 30                 # SBE_EM_MAX_COST_BYTES
LOG_EVERY = 5                            # the reference logs the discretized z after every 5th step (i_step % 5 == 0)

# name -> (restype, argtypes); mirrors include/sbe_em.h one to one (the engine's own table, _lib.PROTOTYPES, is not extended)
PROTOTYPES = {
    **_handle.unit_prototypes("sbe_em"),
    "sbe_em_create": (ct.c_int, [ct.POINTER(c_handle_p), ct.c_int, ct.c_int64, ct.c_int64, ct.c_int64, ct.c_void_p, ct.c_void_p,
                                 ct.c_int64, ct.c_int64, ct.c_void_p]),
    "sbe_em_set_geo_cost": (ct.c_int, [c_handle_p, ct.c_void_p, ct.c_double]),
    "sbe_em_run": (ct.c_int, [c_handle_p, ct.c_void_p, ct.c_int64, ct.c_void_p, ct.c_void_p]),
}


def load():
    """The engine library with the prototypes of include/sbe_em.h attached."""
    return _handle.bind("sbe_em", PROTOTYPES, ABI_VERSION)


def temperatures(n_em_steps: int) -> np.ndarray:
    """T_i = (n_em_steps / (1 + i)) ** 3 for i < n_em_steps: the reference's own Python doubles."""
    return np.array([(n_em_steps / (1 + i)) ** 3 for i in range(n_em_steps)], dtype=np.float64)


def state_index(features, na_values=None) -> np.ndarray:
    """uint8 [N, F] state index of a one-hot bool block [N, F, S]; S for a missing observation (the engine's convention).
    Raises ValueError for a row that is neither one-hot nor (where na_values marks it, or has no state set) empty."""
    f = np.asarray(features)
    if f.ndim != 3 or f.dtype != np.bool_:
        raise TypeError(f"features must be a bool [N, F, S] block, got {f.dtype} of shape {f.shape}")
    n_set = f.sum(axis=2)
    na = n_set == 0 if na_values is None else np.asarray(na_values, dtype=bool)
    if na.shape != n_set.shape:
        raise ValueError(f"na_values has shape {na.shape}, the features {n_set.shape}")
    if np.any(n_set[~na] != 1) or np.any(n_set[na] != 0):
        raise ValueError("features must be one-hot where observed and all False where missing")
    x = np.argmax(f, axis=2).astype(np.uint8)
    x[na] = f.shape[2]
    return x


class EmHandle(_handle.UnitHandle):
    """Owner of one sbe_em: the data of one initializer resident on one device.  last_kernel_ms(): the steps of the last run."""
    _prefix, _noun = "sbe_em", "an EM handle"

    def __init__(self, x, applicable, groups_available, n_clusters, device=None):
        x, applicable, groups_available = _check_data(x, applicable, groups_available, n_clusters)
        self.n_objects, self.n_features = x.shape
        self.n_states = applicable.shape[1]
        self.n_groups, self.n_clusters = groups_available.shape[0], int(n_clusters)
        self.geo_key = None
        xa, aa, ga = x, applicable.view(np.uint8), groups_available.view(np.uint8)
        self._create_on(load, device, self.n_objects, self.n_features, self.n_states, _ptr(xa), _ptr(aa), self.n_groups,
                        self.n_clusters, _ptr(ga))

    def set_geo_cost(self, cost, scale, key=None):
        """Cost-based geo prior on (cost float64 [N, N]) or off (cost None).  `key`: an identity under which the upload
        is skipped when the same matrix is set again."""
        if cost is None:
            self._check(self._lib.sbe_em_set_geo_cost(self._h, None, 0.0))
            self.geo_key = None
            return
        if key is not None and key == self.geo_key:
            return
        c = _check_cost(cost, scale, self.n_objects)
        self._check(self._lib.sbe_em_set_geo_cost(self._h, _ptr(c), float(scale)))
        self.geo_key = key

    def run(self, z, temps):
        """z after len(temps) steps from z (float64 [G, N]); temps: float64 [n_steps]."""
        z_in = _check_z(z, self.n_groups, self.n_objects)
        t = np.ascontiguousarray(temps, dtype=np.float64)
        if t.ndim != 1:
            raise ValueError(f"temperatures must be one-dimensional, got shape {t.shape}")
        if t.size and not (np.all(np.isfinite(t)) and np.all(t > 0)):
            raise ValueError("temperatures must be positive and finite")
        out = np.empty_like(z_in)
        self._check(self._lib.sbe_em_run(self._h, _ptr(z_in), t.size, _ptr(t), _ptr(out)))
        return out


# ---- validation (host side, before any library call) -----------------------------------------------------------
def _check_data(x, applicable, groups_available, n_clusters):
    x = np.asarray(x)
    if x.ndim != 2 or x.dtype != np.uint8:
        raise TypeError(f"state index must be uint8 [N, F], got {x.dtype} of shape {x.shape}")
    app = np.asarray(applicable)
    ga = np.asarray(groups_available)
    if app.dtype != np.bool_ or ga.dtype != np.bool_:
        raise TypeError("applicable and groups_available must be bool arrays")
    n, f = x.shape
    if not 1 <= n <= MAX_OBJECTS or not 1 <= f <= MAX_FEATURES:
        raise ValueError(f"N={n}, F={f} out of range (1 <= N <= {MAX_OBJECTS}, 1 <= F <= {MAX_FEATURES})")
    if app.ndim != 2 or app.shape[0] != f or not 1 <= app.shape[1] <= MAX_STATES:
        raise ValueError(f"applicable must be [F={f}, S] with 1 <= S <= {MAX_STATES}, got shape {app.shape}")
    if ga.ndim != 2 or ga.shape[1] != n or not 1 <= ga.shape[0] <= MAX_GROUPS:
        raise ValueError(f"groups_available must be [G, N={n}] with 1 <= G <= {MAX_GROUPS}, got shape {ga.shape}")
    if not 1 <= int(n_clusters) <= ga.shape[0]:
        raise ValueError(f"n_clusters={n_clusters} out of range [1, G={ga.shape[0]}]")
    return np.ascontiguousarray(x), np.ascontiguousarray(app), np.ascontiguousarray(ga)


def _check_cost(cost, scale, n):
    c = np.asarray(cost)
    if c.shape != (n, n):
        raise ValueError(f"cost must be [N, N] = [{n}, {n}], got shape {c.shape}")
    if n * n * 8 > MAX_COST_BYTES:
        raise ValueError(f"the cost matrix of N={n} objects exceeds {MAX_COST_BYTES} bytes (N <= 32768)")
    if not (np.isfinite(scale) and scale > 0):
        raise ValueError(f"scale={scale} must be positive and finite")
    return np.ascontiguousarray(c, dtype=np.float64)


def _check_z(z, g, n):
    a = np.asarray(z)
    if a.shape != (g, n):
        raise ValueError(f"z must be [G, N] = [{g}, {n}], got shape {a.shape}")
    return np.ascontiguousarray(a, dtype=np.float64)


# ---- a plain function over arrays --------------------------------------------------------------------------------
def run_em(features, applicable, groups_available, n_clusters, z0, temps, cost=None, scale=None, na_values=None, device=None):
    """z (float64 [G, N]) after len(temps) EM steps from z0 on the device.  features: bool [N, F, S] (one-hot; all False
    where missing); applicable: bool [F, S]; groups_available: bool [G, N], rows [0, n_clusters) the clusters; cost,
    scale: the cost-based geo prior (float64 [N, N], > 0) or None."""
    x = state_index(features, na_values)
    h = EmHandle(x, np.asarray(applicable, dtype=bool), np.asarray(groups_available, dtype=bool), n_clusters, device=device)
    try:
        if cost is not None:
            h.set_geo_cost(cost, scale)
        return h.run(z0, temps)
    finally:
        h.close()


# ---- the handle cache (per data object) and the device form of generate_clusters_em -----------------------------------
_HANDLES: dict = {}          # id(data) -> (weakref to data, n_clusters, EmHandle); per process, emptied in a fork()ed child


@_proc.on_fork_clear
def _forget_inherited():
    _HANDLES.clear()


def release_all():
    for _ref, _k, h in list(_HANDLES.values()):
        h.close()
    _HANDLES.clear()


def _groups_available(data, n_clusters, n_objects):
    rows = [np.ones((n_clusters, n_objects), dtype=bool)]
    for conf in data.confounders.values():
        rows.append(np.asarray(conf.group_assignment, dtype=bool))
    return np.concatenate(rows, axis=0)


def handle_for(data, n_clusters, make=None) -> EmHandle:
    """The EM handle of `data` (the reference's Data) with n_clusters clusters, created on first use (by `make`, default
    EmHandle)."""
    entry = _HANDLES.get(id(data))
    if entry is not None and entry[0]() is data and entry[1] == n_clusters and getattr(entry[2], "_h", True):
        return entry[2]
    if entry is not None:
        entry[2].close()
    feats = data.features
    x = state_index(feats.values, feats.na_values)
    avail = _groups_available(data, n_clusters, x.shape[0])
    h = (make or EmHandle)(x, np.asarray(feats.states, dtype=bool), avail, n_clusters)
    try:
        ref = weakref.ref(data)
    except TypeError:                         # (a data object without weak references is held by the cache)
        ref = lambda: data                    # noqa: E731
    _HANDLES[id(data)] = (ref, n_clusters, h)
    return h


def generate_clusters_em(self, make=None):
    """Device form of SbayesInitializer.generate_clusters_em (initializers.py:93-169).  The reference's own calls in its
    order -- self.sample_n_objects_in_all_clusters, np.random.random((G, N)) through its normalize, and
    self.discretize_fuzzy_cluster_2 -- so the global np.random stream after the call is the unpatched one's; the steps run
    on the device, z is read back only at the end (and after every 5th step when init_cluster_logger is set)."""
    import sbayes.sampling.initializers as ref_init
    features = self.data.features.values
    n_objects = features.shape[0]
    n_clusters = self.model.n_clusters
    total_size = self.sample_n_objects_in_all_clusters(
        mid=n_clusters * self.initial_size,
        lower_bound=n_clusters * self.model.min_size,
        upper_bound=min(n_objects, n_clusters * self.model.max_size),
    )
    h = handle_for(self.data, n_clusters, make)
    avail = _groups_available(self.data, n_clusters, n_objects)
    z = ref_init.normalize(np.random.random((avail.shape[0], n_objects)) * avail, axis=0)
    geo_prior = self.model.prior.geo_prior
    consider_geo_prior = geo_prior.prior_type is geo_prior.PriorTypes.COST_BASED
    if consider_geo_prior:
        cost = geo_prior.cost_matrix
        h.set_geo_cost(cost, geo_prior.scale, key=(id(cost), float(geo_prior.scale)))
    else:
        h.set_geo_cost(None, 0.0)
    dtype = np.float64 if consider_geo_prior else z.dtype        # the dtype of the reference's z after its loop
    temps = temperatures(self.n_em_steps)
    if self.n_em_steps == 0:
        return self.discretize_fuzzy_cluster_2(z, total_size=total_size)
    logger = self.init_cluster_logger
    if logger is None:
        z = h.run(z, temps)
    else:
        # chunks ending at the logged steps 0, 5, 10, ...: [0], [1, 5], [6, 10], ..., then the rest
        ends = list(range(0, self.n_em_steps, LOG_EVERY)) + [self.n_em_steps - 1]
        start = 0
        for end in ends:
            if end < start:
                continue
            z = h.run(z, temps[start:end + 1])
            start = end + 1
            if end % LOG_EVERY == 0:
                clusters = self.discretize_fuzzy_cluster_2(z.astype(dtype), total_size=total_size)
                logger.write_sample(sample=ref_init.DummySample(clusters))
    return self.discretize_fuzzy_cluster_2(z.astype(dtype), total_size=total_size)
