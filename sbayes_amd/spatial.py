"""Spatial posterior predictive check on the device (include/sbe_spatial.h): do neighbouring objects agree more often than the
fitted model reproduces?

sBayes is a spatial model: it looks for areas of neighbouring objects that share features beyond what the confounders explain.
The other checks of a fitted run (ppc, pairppc, loopred, psens) do not look at geography.  This one counts, per class of pairs --
the edges of a neighbour graph, or classes of distance -- the pairs that show the same state (the join count; per distance class
the correlogram), on the data and on the replicated data sets of the posterior predictive check (sbayes_amd/ppc.py, one per
logged sample, with the data's missingness), and keeps where the observed counts fall among the replicated ones:

    band, n_bands = bands_from_costs(costs, knn=6)             # or edges=[...], n_bands=8; bands_from_adjacency(adj)
    res = spatial_check(codes, groups, clusters, weights, tables, band, burnin=0.1, seed=0)
    res.p_value("feature") [B,F]   (n_greater + n_equal / 2) / T of agree[b, f]; "object": [B,N] of local_agree; "total": [B]
    res.mean(kind), res.sd(kind), res.z(kind), res.share_obs() = agree / comparable
    res.table(names), res.object_table(names), res.worst(5), res.write_tables(features_tsv, objects_tsv)
    h = SpatialHandle(); h.set_data(codes, n_states, band, n_bands); h.add(y_rep); h.result()        # h.set_tile, h.reset
    python -m sbayes_amd.spatial FEATURES FEATURE_STATES STATS CLUSTERS --confounders universal family --knn 6

A small p says that the pairs of the class agree more often in the data than in what the fitted model produces: a contact area
has been missed (K too small, or the geo prior too strict), and the objects with a small p in the objects' table are where to
look.

What the p-value is not.  It conditions on the logged effect draws and uses the data twice, so it is CONSERVATIVE (DESIGN.md
section 22): under a true model it concentrates around 1/2.  The B F entries (B N for the objects) are multiple comparisons, and no
correction is applied.

Numerical contract (tests/_spatial_oracle.py restates it): every quantity is an integer and equals the
oracle's.  No output depends on how the replicates are split across add() calls, on the tile or on the optional outputs.  One
call holds at most 256 MiB on the device and add() splits longer blocks.  Replicates are validated on the device before anything
changes (EngineError, code SBE_ERR_DATA = 4, naming the first offender).

There is no CPU fallback: without the library or a GPU the functions raise.  Handles follow the package's process model
(sbayes_amd/_proc.py): never pickled, forgotten (not destroyed) in a fork()ed child."""
from __future__ import annotations

import ctypes as ct
from dataclasses import dataclass
from pathlib import Path

import numpy as np

from . import _handle, _samples, assoc, ppc, predict         # noqa: F401 (ppc: the handle of the replicates, made by _samples)
from ._handle import _ptr, c_handle_p

ABI_VERSION = 1                              # SBE_SPATIAL_ABI_VERSION of include/sbe_spatial.h
NA = 255                                     # SBE_SPATIAL_NA
MAX_OBJECTS, MAX_FEATURES = 4096, 4096       # SBE_SPATIAL_MAX_OBJECTS, _FEATURES
MAX_STATES = predict.MAX_STATES              # SBE_SPATIAL_MAX_STATES: every replicate of the posterior predictive check is accepted
MAX_BANDS = 8                                # SBE_SPATIAL_MAX_BANDS
MAX_TILE = 32                                # SBE_SPATIAL_MAX_TILE
MAX_STAGE_BYTES = predict.MAX_STAGE_BYTES    # SBE_SPATIAL_MAX_STAGE_BYTES
CHUNK = 16                                   # 64-bit words of an object's bit row that a lane holds at most

# name -> (restype, argtypes); mirrors include/sbe_spatial.h one to one
PROTOTYPES = {
    **_handle.unit_prototypes("sbe_spatial"),
    "sbe_spatial_create": (ct.c_int, [ct.POINTER(c_handle_p), ct.c_int]),
    "sbe_spatial_set_tile": (ct.c_int, [c_handle_p, ct.c_int]),
    "sbe_spatial_max_replicates": (ct.c_int64, [ct.c_int64, ct.c_int64]),
    "sbe_spatial_replicate_bytes": (ct.c_int64, [ct.c_int64, ct.c_int64, ct.c_int, ct.c_int]),
    "sbe_spatial_set_data": (ct.c_int, [c_handle_p, ct.c_void_p, ct.c_int64, ct.c_int64, ct.c_void_p, ct.c_void_p, ct.c_int]),
    "sbe_spatial_add": (ct.c_int, [c_handle_p, ct.c_int64] + [ct.c_void_p] * 6),
    "sbe_spatial_read": (ct.c_int, [c_handle_p] + [ct.c_void_p] * 18 + [ct.POINTER(ct.c_int64)]),
    "sbe_spatial_reset": (ct.c_int, [c_handle_p]),
}

KINDS = {"feature": ("f", "agree_obs"), "object": ("i", "local_agree_obs"), "total": ("t", "total_obs")}
REP_OUTPUTS = ("agree_rep", "comparable_rep", "local_agree_rep", "local_comparable_rep")


def load():
    """The engine library with the prototypes of include/sbe_spatial.h attached."""
    return _handle.bind("sbe_spatial", PROTOTYPES, ABI_VERSION)


def _in_limits(n, f):
    return 1 <= n <= MAX_OBJECTS and 1 <= f <= MAX_FEATURES


def padded_words(n_objects) -> int:
    """The 64-bit words of n_objects, padded: a power of two up to CHUNK, a multiple of CHUNK beyond."""
    w = -(-int(n_objects) // 64)
    return 1 << (w - 1).bit_length() if w <= CHUNK else -(-w // CHUNK) * CHUNK


def max_replicates(n_objects, n_features) -> int:
    """The replicates a handle of this shape accumulates (sbe_spatial_max_replicates): below it no int64 sum of squares and no
    int32 count overflows; 0 beyond the limits."""
    n, f = int(n_objects), int(n_features)
    if not _in_limits(n, f):
        return 0
    most = max(n * (n - 1) // 2, (n - 1) * f)
    return 2 ** 31 - 1 if most == 0 else min(2 ** 31 - 1, (2 ** 63 - 1) // (most * most))


def replicate_bytes(n_objects, n_features, max_states, n_bands) -> int:
    """Device bytes one replicate of an add call takes while the call runs (sbe_spatial_replicate_bytes); 0 beyond the limits."""
    n, f, s, b = int(n_objects), int(n_features), int(max_states), int(n_bands)
    if not (_in_limits(n, f) and 1 <= s <= MAX_STATES and 1 <= b <= MAX_BANDS):
        return 0
    w = padded_words(n)
    return n * f + 64 * w * f + 8 * w * f * (s + 1) + 8 * b * (f + n) + 8 * b


# ---- the classes of pairs ------------------------------------------------------------------------------------------------
def _square(a, what):
    a = np.asarray(a)
    if a.ndim != 2 or a.shape[0] != a.shape[1] or a.shape[0] < 1:
        raise ValueError(f"{what} must be a square matrix, got shape {a.shape}")
    return a


def bands_from_adjacency(adj):
    """(band uint8 [N, N], 1): class 0 on the edges of a boolean or scipy-sparse adjacency matrix (the reference's
    Data.network.adj_mat), 255 elsewhere and on the diagonal.  An asymmetric matrix is refused."""
    if hasattr(adj, "toarray"):
        adj = adj.toarray()
    a = _square(adj, "the adjacency").astype(bool)
    if not np.array_equal(a, a.T):
        i, j = np.argwhere(a != a.T)[0]
        raise ValueError(f"the adjacency is not symmetric: entry ({i}, {j}) differs from ({j}, {i})")
    band = np.where(a, 0, NA).astype(np.uint8)
    np.fill_diagonal(band, NA)
    return band, 1


def bands_from_costs(costs, edges=None, n_bands=None, knn=None):
    """(band uint8 [N, N], B) from a symmetric cost (distance) matrix; exactly one of
      edges    increasing bounds e_0 < ... < e_{B-1}: class b holds the pairs with cost in (e_{b-1}, e_b], class 0 those up to e_0,
               pairs beyond e_{B-1} are not counted;
      n_bands  B classes with quantile bounds: edge b is the (b + 1) / B quantile of the costs of the pairs i < j;
      knn      one class: i and j are joined if either is among the other's k nearest (the union, hence symmetric; ties by index).
    The diagonal is never counted.  An asymmetric matrix is refused."""
    c = _square(costs, "the costs").astype(np.float64)
    n = c.shape[0]
    if not np.array_equal(c, c.T):
        i, j = np.argwhere(c != c.T)[0]
        raise ValueError(f"the costs are not symmetric: entry ({i}, {j}) = {float(c[i, j])!r} differs from ({j}, {i}) = {float(c[j, i])!r}")
    if sum(v is not None for v in (edges, n_bands, knn)) != 1:
        raise ValueError("give exactly one of edges, n_bands and knn")
    if knn is not None:
        k = int(knn)
        if not 1 <= k:
            raise ValueError(f"knn={knn} must be at least 1")
        away = c.copy()
        np.fill_diagonal(away, np.inf)
        near = np.argsort(away, axis=1, kind="stable")[:, :min(k, n - 1)]
        adj = np.zeros((n, n), dtype=bool)
        adj[np.repeat(np.arange(n), near.shape[1]), near.ravel()] = True
        return bands_from_adjacency(adj | adj.T)
    if n_bands is not None:
        b = int(n_bands)
        if not 1 <= b <= MAX_BANDS:
            raise ValueError(f"n_bands={n_bands} out of range [1, {MAX_BANDS}]")
        upper = c[np.triu_indices(n, 1)]
        edges = np.quantile(upper, (np.arange(b) + 1.0) / b) if upper.size else np.arange(b, dtype=np.float64)
        edges = np.maximum.accumulate(edges)
    edges = np.asarray(edges, dtype=np.float64)
    if edges.ndim != 1 or not 1 <= edges.size <= MAX_BANDS:
        raise ValueError(f"edges must be 1 .. {MAX_BANDS} bounds, got shape {edges.shape}")
    if n_bands is None and np.any(np.diff(edges) <= 0):
        raise ValueError("edges must increase")
    cls = np.searchsorted(edges, c, side="left")                    # cost in (e_{b-1}, e_b] -> b
    band = np.where(cls < edges.size, cls, NA).astype(np.uint8)
    np.fill_diagonal(band, NA)
    return band, int(edges.size)


def _check_band(band, n_bands, n):
    band = np.asarray(band)
    if band.dtype != np.uint8:
        raise TypeError(f"band must be uint8 classes [N, N] (255 = pair not counted), got {band.dtype}")
    if band.shape != (n, n):
        raise ValueError(f"band must be [{n}, {n}], got shape {band.shape}")
    b = int(n_bands)
    if not 1 <= b <= MAX_BANDS:
        raise ValueError(f"n_bands={n_bands} out of range [1, {MAX_BANDS}]")
    return np.ascontiguousarray(band), b


# ---- the result ------------------------------------------------------------------------------------------------------------
@dataclass
class SpatialResult:
    """B classes, F features, N objects, T replicates.  agree_obs, comparable_obs [B, F], local_agree_obs, local_comparable_obs
    [B, N] (int32) and total_obs [B] (int64): the data's counts.  f_*: the accumulators of agree [B, F], i_*: of local_agree
    [B, N]: greater, equal, less (int32), sum, sumsq (int64); t_greater, t_equal, t_less [B]: of total.  total_rep int64 [T, B];
    agree_rep, comparable_rep [T, B, F] and local_agree_rep, local_comparable_rep [T, B, N]: None unless kept."""
    agree_obs: np.ndarray
    comparable_obs: np.ndarray
    local_agree_obs: np.ndarray
    local_comparable_obs: np.ndarray
    total_obs: np.ndarray
    f_greater: np.ndarray
    f_equal: np.ndarray
    f_less: np.ndarray
    f_sum: np.ndarray
    f_sumsq: np.ndarray
    i_greater: np.ndarray
    i_equal: np.ndarray
    i_less: np.ndarray
    i_sum: np.ndarray
    i_sumsq: np.ndarray
    t_greater: np.ndarray
    t_equal: np.ndarray
    t_less: np.ndarray
    n_replicates: int
    total_rep: np.ndarray = None
    agree_rep: np.ndarray | None = None
    comparable_rep: np.ndarray | None = None
    local_agree_rep: np.ndarray | None = None
    local_comparable_rep: np.ndarray | None = None
    kernel_ms: float = 0.0
    ppc: object = None                       # the PpcResult of the same replicates (spatial_check)

    def _kind(self, kind):
        if kind not in KINDS:
            raise ValueError(f"kind={kind!r} is none of {sorted(KINDS)}")
        return KINDS[kind]

    def observed(self, kind="feature"):
        return getattr(self, self._kind(kind)[1])

    def p_value(self, kind="feature"):
        """The upper-tail p-value (n_greater + n_equal / 2) / T, ties counting half as in ppc: small where the data agree more
        often than the replicates."""
        k = self._kind(kind)[0]
        with np.errstate(invalid="ignore", divide="ignore"):
            return (getattr(self, k + "_greater") + 0.5 * getattr(self, k + "_equal")) / self.n_replicates

    def mean(self, kind="feature"):
        """Of the replicated counts (the totals': exactly, from total_rep)."""
        with np.errstate(invalid="ignore", divide="ignore"):
            if kind == "total":
                return self.total_rep.sum(axis=0) / self.n_replicates
            return getattr(self, self._kind(kind)[0] + "_sum") / self.n_replicates

    def sd(self, kind="feature"):
        """The standard deviation of the replicated counts (divisor T), from the exact integer sums: T sumsq - sum^2 in Python
        integers, so nothing cancels."""
        k = self._kind(kind)[0]
        t = self.n_replicates
        if kind == "total":
            s1 = self.total_rep.astype(object).sum(axis=0) if t else np.zeros(self.total_obs.shape, dtype=object)
            s2 = (self.total_rep.astype(object) ** 2).sum(axis=0) if t else s1
        else:
            s1, s2 = getattr(self, k + "_sum").astype(object), getattr(self, k + "_sumsq").astype(object)
        if t == 0:
            return np.full(np.shape(s1), np.nan)
        var = np.asarray(t * s2 - s1 * s1, dtype=object)
        return np.sqrt(var.astype(np.float64)) / t

    def z(self, kind="feature"):
        """(observed - mean) / sd; NaN where sd is 0."""
        sd = self.sd(kind)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(sd > 0, (self.observed(kind) - self.mean(kind)) / sd, np.nan)

    def share_obs(self):
        """agree_obs / comparable_obs [B, F]: the share of the comparable pairs of a class that agree; NaN without such pairs."""
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(self.comparable_obs > 0, self.agree_obs / self.comparable_obs, np.nan)

    def _rows(self, kind, names, comparable):
        obs, p, mean, sd, z = self.observed(kind), self.p_value(kind), self.mean(kind), self.sd(kind), self.z(kind)
        count = obs.shape[1]
        prefix = "F" if kind == "feature" else "O"
        names = list(names) if names is not None else [f"{prefix}{i + 1}" for i in range(count)]
        if len(names) != count:
            raise ValueError(f"{len(names)} names for {count} {kind}s")
        rows = []
        for b in range(obs.shape[0]):
            for k in range(count):
                share = float(obs[b, k]) / float(comparable[b, k]) if comparable[b, k] > 0 else float("nan")
                rows.append([b, str(names[k]), int(obs[b, k]), int(comparable[b, k]), share, float(p[b, k]), float(mean[b, k]), float(sd[b, k]),
                             float(z[b, k])])
        rows.sort(key=lambda r: (r[5] if r[5] == r[5] else np.inf, -r[8] if r[8] == r[8] else np.inf))
        return rows

    def table(self, names=None):
        """(header, rows) per (class, feature), sorted by the p-value, then by -z (NaN last)."""
        return (["band", "feature", "agree", "comparable", "share", "p_predictive", "mean_replicated", "sd_replicated", "z"],
                self._rows("feature", names, self.comparable_obs))

    def object_table(self, names=None):
        """(header, rows) per (class, object): the object's agreeing and comparable neighbour cells over all features."""
        return (["band", "object", "agree", "comparable", "share", "p_predictive", "mean_replicated", "sd_replicated", "z"],
                self._rows("object", names, self.local_comparable_obs))

    def worst(self, k=5, names=None):
        """The first k rows of table(names)."""
        return self.table(names)[1][:k]

    def write_tables(self, features_path=None, objects_path=None, feature_names=None, object_names=None):
        for path, make, names in ((features_path, self.table, feature_names), (objects_path, self.object_table, object_names)):
            if path is None:
                continue
            _samples.write_tsv(path, *make(names))


class SpatialHandle(_handle.UnitHandle):
    """Owner of one sbe_spatial handle: the data, the classes' bit rows, the observed counts and the accumulators on one device.
    add() feeds replicates; result() reads back.  last_kernel_ms(): the unit's kernels of the last library call."""
    _prefix, _noun = "sbe_spatial", "a spatial check handle"

    def __init__(self, device=None):
        self.shape = None                                    # (N, F, B) once the data is set
        self.n_states = None
        self._kept = []
        self.kernel_ms = 0.0
        self._create_on(load, device)

    def set_data(self, codes, n_states, band, n_bands):
        """codes uint8 [N, F] (255 = NA) or one-hot bool [N, F, S]; n_states: states per feature (None: one more than the largest
        code that occurs); band uint8 [N, N] with n_bands classes (bands_from_costs, bands_from_adjacency).  Computes the observed
        counts and clears the accumulators."""
        x, ns = assoc._check_inputs(codes, n_states)
        n, f = x.shape
        if n > MAX_OBJECTS:
            raise ValueError(f"{n} objects; the classes are an [N, N] matrix, limited to {MAX_OBJECTS} objects")
        band, b = _check_band(band, n_bands, n)
        self.shape = None
        self._check(self._lib.sbe_spatial_set_data(self._h, _ptr(x), n, f, _ptr(ns), _ptr(band), b))
        self.shape, self.n_states = (n, f, b), ns
        self._kept, self.kernel_ms = [], self.last_kernel_ms()

    def _with_data(self):
        if self.shape is None:
            raise ValueError("no data yet (set_data)")
        return self.shape

    def reset(self):
        """Clear the accumulators, keep the data."""
        self._with_data()
        self._check(self._lib.sbe_spatial_reset(self._h))
        self._kept, self.kernel_ms = [], 0.0

    def set_tile(self, tile_features):
        """Features per tile of the count kernel (0: the default).  Results do not depend on it."""
        self._check(self._lib.sbe_spatial_set_tile(self._h, int(tile_features)))

    def max_replicates(self) -> int:
        """The replicates the handle accumulates before a sum of squares could overflow."""
        n, f, _b = self._with_data()
        return max_replicates(n, f)

    def call_replicates(self) -> int:
        """The replicates one library call holds on the device."""
        n, f, b = self._with_data()
        return MAX_STAGE_BYTES // replicate_bytes(n, f, int(self.n_states.max()), b)

    def add(self, y_rep, keep=()):
        """Replicates uint8 [n, N, F], each code below n_states[f] or 255.  keep: names among REP_OUTPUTS (or True for all) whose
        per-replicate arrays are kept for result(); total_rep always is.  Blocks beyond call_replicates() go in several library
        calls; each call validates its replicates before it changes anything, so an EngineError leaves the replicates of the
        calls before it added."""
        n_obj, f, b = self._with_data()
        y = _samples.check_replicates(y_rep, n_obj, f)
        keep = REP_OUTPUTS if keep is True else tuple(keep)
        if set(keep) - set(REP_OUTPUTS):
            raise ValueError(f"keep={keep!r}: the per-replicate outputs are {REP_OUTPUTS}")
        step = self.call_replicates()
        y = np.ascontiguousarray(y)
        self.kernel_ms = 0.0
        for r0 in range(0, y.shape[0], step):
            block = y[r0:r0 + step]
            k = block.shape[0]
            agree = np.empty((k, b, f), dtype=np.int32) if "agree_rep" in keep else None
            comparable = np.empty((k, b, f), dtype=np.int32) if "comparable_rep" in keep else None
            local = np.empty((k, b, n_obj), dtype=np.int32) if "local_agree_rep" in keep else None
            local_comparable = np.empty((k, b, n_obj), dtype=np.int32) if "local_comparable_rep" in keep else None
            total = np.empty((k, b), dtype=np.int64)
            self._check(self._lib.sbe_spatial_add(self._h, k, _ptr(block), _ptr(agree) if agree is not None else None,
                                                  _ptr(comparable) if comparable is not None else None, _ptr(local) if local is not None else None,
                                                  _ptr(local_comparable) if local_comparable is not None else None, _ptr(total)))
            self.kernel_ms += self.last_kernel_ms()
            self._kept.append(dict(total_rep=total, agree_rep=agree, comparable_rep=comparable, local_agree_rep=local, local_comparable_rep=local_comparable))

    def result(self) -> SpatialResult:
        n, f, b = self._with_data()
        agree_obs, comparable_obs, f_greater, f_equal, f_less = (np.empty((b, f), dtype=np.int32) for _ in range(5))
        local_obs, local_comparable_obs, i_greater, i_equal, i_less = (np.empty((b, n), dtype=np.int32) for _ in range(5))
        f_sum, f_sumsq = (np.empty((b, f), dtype=np.int64) for _ in range(2))
        i_sum, i_sumsq = (np.empty((b, n), dtype=np.int64) for _ in range(2))
        total_obs = np.empty(b, dtype=np.int64)
        t_greater, t_equal, t_less = (np.empty(b, dtype=np.int32) for _ in range(3))
        count = ct.c_int64(0)
        self._check(self._lib.sbe_spatial_read(self._h, _ptr(agree_obs), _ptr(comparable_obs), _ptr(local_obs), _ptr(local_comparable_obs), _ptr(total_obs),
                                               _ptr(f_greater), _ptr(f_equal), _ptr(f_less), _ptr(f_sum), _ptr(f_sumsq), _ptr(i_greater), _ptr(i_equal),
                                               _ptr(i_less), _ptr(i_sum), _ptr(i_sumsq), _ptr(t_greater), _ptr(t_equal), _ptr(t_less), ct.byref(count)))
        kept = {}
        for name in ("total_rep",) + REP_OUTPUTS:
            parts = [k[name] for k in self._kept]
            kept[name] = np.concatenate(parts) if parts and all(p is not None for p in parts) else None
        if kept["total_rep"] is None:
            kept["total_rep"] = np.zeros((0, b), dtype=np.int64)
        return SpatialResult(agree_obs, comparable_obs, local_obs, local_comparable_obs, total_obs, f_greater, f_equal, f_less, f_sum, f_sumsq,
                             i_greater, i_equal, i_less, i_sum, i_sumsq, t_greater, t_equal, t_less, count.value, kernel_ms=self.kernel_ms, **kept)


def spatial_check(codes, groups, clusters, weights, tables, band, n_bands=None, n_states=None, burnin=0.1, seed=0, n_groups=None, uniforms=None,
                  keep=(), device=None) -> SpatialResult:
    """The spatial check of T logged samples after burn-in: the samples, seed and draw indices are posterior_predictive_check's
    (sbayes_amd/ppc.py), so the p-values belong to the same replicates as its per-feature ones (res.ppc holds that result,
    without y_rep).  band: uint8 [N, N] with n_bands classes (None: one more than the largest class that occurs).  n_states:
    states per feature (default: the tables' S for every feature -- a replicate may draw a state the data never shows).  The
    replicates pass through host memory, block by block."""
    groups, n_groups, clusters, weights, tables, uniforms = _samples.after_burnin(groups, clusters, weights, tables, burnin, n_groups, uniforms)
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    band = np.asarray(band)
    if n_bands is None:
        counted = band[band != NA] if band.dtype == np.uint8 else np.zeros(0, dtype=np.uint8)
        n_bands = int(counted.max()) + 1 if counted.size else 1
    band, n_bands = _check_band(band, n_bands, codes.shape[0] if codes.ndim == 2 else 0)
    if n_states is None:
        n_states = np.full(codes.shape[1] if codes.ndim == 2 else 0, tables.shape[3], dtype=np.int32)

    def fill(h):
        h.set_data(codes, n_states, band, n_bands)
        return h.call_replicates(), lambda y: h.add(y, keep=keep)
    return _samples.check_with_replicates(SpatialHandle, fill, codes, groups, n_groups, clusters, weights, tables, seed, uniforms, device)


# ---- files -----------------------------------------------------------------------------------------------------------------
def read_costs(path, object_ids):
    """float64 [N, N]: a square CSV of costs with the objects' ids in its first column and its header (the reference's
    read_costs_from_csv), its rows and columns put in the order of object_ids."""
    import pandas as pd
    frame = pd.read_csv(path, dtype=str, index_col=0)
    frame.index = [str(v).strip() for v in frame.index]
    frame.columns = [str(v).strip() for v in frame.columns]
    ids = [str(v).strip() for v in object_ids]
    missing = [v for v in ids if v not in frame.index or v not in frame.columns]
    if missing:
        raise ValueError(f"the costs file has no row or no column for object {missing[0]!r}")
    return np.ascontiguousarray(frame.loc[ids, ids].to_numpy(dtype=np.float64))


def read_objects(features_csv):
    """(ids, xy float64 [N, 2]) of the features file's id, x, y columns."""
    import pandas as pd
    raw = pd.read_csv(features_csv, dtype=str, keep_default_na=False)
    for col in ("id", "x", "y"):
        if col not in raw.columns:
            raise ValueError(f"the features file has no column {col!r}")
    return [v.strip() for v in raw["id"]], np.stack([raw["x"].astype(np.float64).to_numpy(), raw["y"].astype(np.float64).to_numpy()], axis=1)


def plane_distances(xy):
    """Euclidean distances [N, N] of points in the plane, exactly symmetric."""
    d = np.asarray(xy, dtype=np.float64)
    diff = d[:, None, :] - d[None, :, :]
    return np.sqrt((diff * diff).sum(axis=2))


def parser():
    ap = _samples.run_parser("python -m sbayes_amd.spatial",
                             "Agreement of neighbouring objects of an sBayes run checked against the fitted model: the join counts "
                             "of the data per class of pairs among the same counts on one replicated data set per logged sample "
                             "(conservative: given the logged effect draws; no correction for the many comparisons)", seed=True)
    ap.add_argument("--costs", type=Path, default=None, help="a square CSV of costs between the objects, ids in the first column and the header; "
                                                             "without it plane distances are taken from the x, y columns of the features file")
    how = ap.add_mutually_exclusive_group()
    how.add_argument("--edges", type=float, nargs="+", default=None, help="increasing cost bounds: class b holds the pairs in (edge b-1, edge b]")
    how.add_argument("--bands", type=int, default=None, help="this many classes with quantile bounds over all pairs (the correlogram)")
    how.add_argument("--knn", type=int, default=None, help="one class over the symmetrised k-nearest-neighbour graph (default: --knn 6)")
    ap.add_argument("--out-features", type=Path, default=Path("spatial_features.tsv"), help="the table per class and feature")
    ap.add_argument("--out-objects", type=Path, default=Path("spatial_objects.tsv"), help="the table per class and object")
    return ap


def bands_of_args(args, ids, xy):
    """(band, B) of the command line's choice of costs and classes."""
    costs = read_costs(args.costs, ids) if args.costs is not None else plane_distances(xy)
    if args.edges is not None:
        return bands_from_costs(costs, edges=args.edges)
    if args.bands is not None:
        return bands_from_costs(costs, n_bands=args.bands)
    return bands_from_costs(costs, knn=args.knn if args.knn is not None else 6)


def main(argv=None):
    args = parser().parse_args(argv)
    data, clusters, weights, tables, n_groups = _samples.read_run(args)
    ids, xy = read_objects(args.features)
    band, n_bands = bands_of_args(args, ids, xy)
    n_states = np.array([max(1, len(s)) for s in data["state_names"]], dtype=np.int32)
    res = spatial_check(data["codes"], data["groups"], clusters, weights, tables, band, n_bands, n_states=n_states, burnin=args.burnin, seed=args.seed,
                        n_groups=n_groups, device=args.device)
    entries = n_bands * len(data["feature_names"])
    print(f"{res.n_replicates} replicates, {n_bands} classes of pairs, {len(data['feature_names'])} features "
          f"(the p-values are conservative: given the logged effect draws; {entries} comparisons, uncorrected)")
    p_total, z_total = res.p_value("total"), res.z("total")
    for b in range(n_bands):
        print(f"  class {b}: {int(res.total_obs[b])} agreeing pairs and features, replicated {res.mean('total')[b]:.1f} +- {res.sd('total')[b]:.1f}, "
              f"p {p_total[b]:.4f}, z {z_total[b]:.3f}")
    print("the five (class, feature) entries with the smallest predictive p:")
    for b, name, agree, comparable, share, p, mean, sd, z in res.worst(5, data["feature_names"]):
        print(f"  class {b}\t{name}\tagree {agree} of {comparable} ({share:.3f})\tp predictive {p:.4f}\treplicated {mean:.2f} +- {sd:.2f}\tz {z:.3f}")
    res.write_tables(args.out_features, args.out_objects, data["feature_names"], ids)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
