"""What the units that replay a run's logged samples share on the host side (predict, ppc, contribution, loopred, and pairppc,
spatial and objpair, which consume ppc's replicates): the limits and checks of the data of include/sbe_predict.h, the handle that holds
the data and sends blocks of samples, the opening of the one-call functions, the driver of a replicate consumer, the table
writer and the command lines' common arguments.  The C side's counterpart is the sample store of csrc/sbe_predict_row.hip.h;
DESIGN.md section 7 describes both."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

from . import _handle
from ._handle import _ptr

MAX_STATES = 32                          # SBE_PREDICT_MAX_STATES
MAX_COMPONENTS = 8                       # SBE_PREDICT_MAX_COMPONENTS
MAX_ROWS = 256                           # SBE_PREDICT_MAX_ROWS
MAX_OBJECTS = 1 << 20                    # SBE_PREDICT_MAX_OBJECTS
MAX_FEATURES = 1 << 16                   # SBE_PREDICT_MAX_FEATURES
MAX_ACC_BYTES = 1 << 32                  # SBE_PREDICT_MAX_ACC_BYTES
MAX_STAGE_BYTES = 1 << 28                # SBE_PREDICT_MAX_STAGE_BYTES
MAX_TILE = 256                           # SBE_PREDICT_MAX_TILE
SUM_TOL = 1e-5                           # SBE_PREDICT_SUM_TOL
NA = 255                                 # SBE_PREDICT_NA


# ---- validation (host side, before any library call) -----------------------------------------------------------
def _check_shape(N, F, S, C, K, n_groups):
    """R of a shape within the limits."""
    if not 1 <= N <= MAX_OBJECTS:
        raise ValueError(f"{N} objects; the unit takes 1 .. {MAX_OBJECTS} (2^20)")
    if not 1 <= F <= MAX_FEATURES:
        raise ValueError(f"{F} features; the unit takes 1 .. {MAX_FEATURES} (2^16)")
    if not 1 <= S <= MAX_STATES:
        raise ValueError(f"{S} states; the unit takes 1 .. {MAX_STATES}")
    if not 1 <= C <= MAX_COMPONENTS:
        raise ValueError(f"{C} components; the unit takes 1 .. {MAX_COMPONENTS}")
    if len(n_groups) != C - 1:
        raise ValueError(f"{len(n_groups)} group counts for {C - 1} confounders")
    if K < 1 or any(g < 1 for g in n_groups):
        raise ValueError(f"{K} clusters and group counts {list(n_groups)}: every component needs at least one row")
    R = K + sum(n_groups)
    if R > MAX_ROWS:
        raise ValueError(f"{K} clusters and the confounders' groups make {R} table rows, the limit is {MAX_ROWS}")
    if N * F * (S + C) * 8 > MAX_ACC_BYTES:
        raise ValueError(f"the accumulators of {N} objects x {F} features take {N * F * (S + C) * 8} bytes on the device, the limit is {MAX_ACC_BYTES}")
    return R


def _check_burnin(burnin, n):
    burnin = float(burnin)
    if not 0.0 <= burnin < 1.0:
        raise ValueError(f"burnin={burnin} must lie in [0, 1)")
    return int(burnin * n)


def group_index(assignment):
    """uint8 [N] group index (255 = none) of a bool [G, N] group assignment, the form the reference's Confounder holds."""
    a = np.asarray(assignment, dtype=bool)
    if a.ndim != 2 or a.shape[0] > NA:
        raise ValueError(f"a group assignment is bool [G, N] with G <= {NA}, got shape {a.shape}")
    if (a.sum(axis=0) > 1).any():
        raise ValueError(f"object {int(np.flatnonzero(a.sum(axis=0) > 1)[0])} is in two groups of one confounder")
    return np.where(a.any(axis=0), a.argmax(axis=0), NA).astype(np.uint8)


def codes_of(features):
    """uint8 [N, F] state index (255 = NA) of one-hot bool [N, F, S] features, the form the reference's Features holds."""
    a = np.asarray(features, dtype=bool)
    if a.ndim != 3 or a.shape[2] > MAX_STATES:
        raise ValueError(f"one-hot features are bool [N, F, S] with S <= {MAX_STATES}, got shape {a.shape}")
    return np.where(a.any(axis=2), a.argmax(axis=2), NA).astype(np.uint8)


def check_replicates(y_rep, n_objects, n_features):
    """uint8 [n, N, F] of a consumer's replicates; one replicate [N, F] counts as a block of one."""
    y = np.asarray(y_rep)
    if y.dtype != np.uint8:
        raise TypeError(f"replicates must be uint8 codes, got {y.dtype}")
    if y.ndim == 2:
        y = y[None]
    if y.ndim != 3 or y.shape[1:] != (n_objects, n_features):
        raise ValueError(f"replicates must be [n, {n_objects}, {n_features}], got shape {y.shape}")
    return y


# ---- the handle --------------------------------------------------------------------------------------------------
class SampleHandle(_handle.UnitHandle):
    """Owner of a unit handle that holds the data of include/sbe_predict.h and takes blocks of samples.  The unit's module
    has MAX_STAGE_BYTES and sample_bytes(N, F, S, C, K, R, *flags); the class has max_samples(*flags) and, where it keeps
    rows of its own, _clear()."""

    shape = None                                             # (N, F, S, C, K, R) once the data is set
    _codes = None

    def __init__(self, device=None):
        self._clear()
        self._create_on(sys.modules[type(self).__module__].load, device)

    def _clear(self):
        pass

    def set_data(self, codes, groups, n_groups, n_states, n_clusters):
        """codes uint8 [N,F] (255 = NA); groups uint8 [C-1,N] (255 = none) with n_groups[c] groups each.  Resets the sums and
        forgets the rows."""
        self._set_data(codes, groups, n_groups, n_states, n_clusters)

    def _set_data(self, codes, groups, n_groups, n_states, n_clusters, more=lambda codes: ()):
        """more(codes): the unit's own checks; returns what <prefix>_set_data takes behind n_groups."""
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        if codes.ndim != 2:
            raise ValueError(f"codes must be [N, F], got shape {codes.shape}")
        N, F = codes.shape
        n_groups = [int(g) for g in n_groups]
        C = len(n_groups) + 1
        groups = np.ascontiguousarray(groups, dtype=np.uint8).reshape(C - 1, -1) if C > 1 else np.zeros((0, N), dtype=np.uint8)
        if groups.shape != (C - 1, N):
            raise ValueError(f"groups must be [{C - 1}, {N}], got shape {groups.shape}")
        S, K = int(n_states), int(n_clusters)
        R = _check_shape(N, F, S, C, K, n_groups)
        extra = more(codes)
        counts = np.ascontiguousarray(n_groups, dtype=np.intc)
        self.shape = None
        self._check(self._fn("set_data")(self._h, N, F, S, C, K, _ptr(codes), _ptr(groups) if C > 1 else None,
                                         _ptr(counts) if C > 1 else None, *extra))
        self.shape, self._codes = (N, F, S, C, K, R), codes
        self._clear()

    def _with_data(self):
        if self.shape is None:
            raise ValueError("no data yet (set_data)")
        return self.shape

    def set_feature_tile(self, features):
        """Features per workgroup tile (0: the default); no result depends on it."""
        self._check(self._fn("set_feature_tile")(self._h, int(features)))

    def _blocks(self, clusters, weights, tables, *flags):
        """T and [(t0, clusters, weights, tables)], one entry per library call of at most max_samples(*flags) samples: the
        checked, contiguous block of samples in consecutive slices."""
        N, F, S, C, K, R = self._with_data()
        clusters = np.ascontiguousarray(clusters, dtype=np.uint8)
        weights = np.ascontiguousarray(weights, dtype=np.float64)
        tables = np.ascontiguousarray(tables, dtype=np.float64)
        T = clusters.shape[0]
        if clusters.shape != (T, K, N) or weights.shape != (T, F, C) or tables.shape != (T, R, F, S):
            raise ValueError(f"{T} samples take clusters {(T, K, N)}, weights {(T, F, C)} and tables {(T, R, F, S)}; got {clusters.shape}, "
                             f"{weights.shape}, {tables.shape}")
        step = self.max_samples(*flags)
        if step < 1:
            unit = sys.modules[type(self).__module__]
            raise ValueError(f"one sample takes {unit.sample_bytes(N, F, S, C, K, R, *flags)} bytes on the device, a call holds {unit.MAX_STAGE_BYTES}")
        return T, [(t0, clusters[t0:t0 + step], weights[t0:t0 + step], tables[t0:t0 + step]) for t0 in range(0, T, step)]


# ---- the one-call functions ----------------------------------------------------------------------------------------
def after_burnin(groups, clusters, weights, tables, burnin, n_groups, uniforms=None):
    """The opening of a one-call function: (groups uint8 [C-1,N], n_groups, clusters, weights, tables, uniforms), the last four
    after burn-in.  groups: group indices (with n_groups) or a list of bool [G_c,N] assignments; uniforms: None or one row per
    sample before burn-in."""
    clusters, weights, tables = np.asarray(clusters), np.asarray(weights), np.asarray(tables)
    if tables.ndim != 4 or clusters.ndim != 3:
        raise ValueError(f"clusters must be [T, K, N] and tables [T, R, F, S], got shapes {clusters.shape} and {tables.shape}")
    if n_groups is None:
        n_groups = [np.asarray(g).shape[0] for g in groups]
        groups = np.stack([group_index(g) for g in groups]) if len(n_groups) else np.zeros((0, clusters.shape[2]), dtype=np.uint8)
    burn = _check_burnin(burnin, clusters.shape[0])
    if uniforms is not None:
        uniforms = np.asarray(uniforms)
        if uniforms.shape[0] != clusters.shape[0]:
            raise ValueError(f"{uniforms.shape[0]} rows of uniforms for {clusters.shape[0]} samples")
        uniforms = uniforms[burn:]
    return groups, n_groups, clusters[burn:], weights[burn:], tables[burn:], uniforms


def check_with_replicates(consumer, fill, codes, groups, n_groups, clusters, weights, tables, seed, uniforms, device):
    """The driver of a unit that consumes the replicates of the posterior predictive check, block by block through host memory:
    a ppc handle with the data, a `consumer` handle on the same device, fill(handle) -- it sets the consumer's data and returns
    (the replicates one of its calls takes, its add(y_rep)) -- then check, drain, add per block.  Returns the consumer's
    result() with the check's as .ppc and the consumer's kernel time."""
    from . import ppc
    hp = ppc.PpcHandle(device)
    try:
        hp.set_data(codes, groups, n_groups, tables.shape[3], clusters.shape[1])
        h = consumer(hp.device)
        try:
            limit, add = fill(h)
            step = max(1, min(hp.max_samples(True, uniforms is not None), limit))
            kernel_ms = 0.0
            for t0 in range(0, clusters.shape[0], step):
                hp.check(clusters[t0:t0 + step], weights[t0:t0 + step], tables[t0:t0 + step], seed=seed,
                         uniforms=uniforms[t0:t0 + step] if uniforms is not None else None, replicates=True)
                for y in hp.drain_replicates():
                    add(y)
                    kernel_ms += h.kernel_ms
            res = h.result()
            res.kernel_ms, res.ppc = kernel_ms, hp.result()
            return res
        finally:
            h.close()
    finally:
        hp.close()


# ---- files -------------------------------------------------------------------------------------------------------
def write_tsv(path, header, rows):
    """A tab-separated table: strings as they are, integers in full, floats with ten significant digits."""
    with open(path, "w") as f:
        f.write("\t".join(header) + "\n")
        for row in rows:
            f.write("\t".join(v if isinstance(v, str) else (str(v) if isinstance(v, int) else f"{v:.10g}") for v in row) + "\n")


def run_parser(prog, description, seed=False):
    """The parser of a command line over a run's files: the four files, --confounders, --burnin, --seed where the program
    draws replicates, and --device.  The program adds its own options."""
    import argparse
    ap = argparse.ArgumentParser(prog=prog, description=description)
    ap.add_argument("features", type=Path, help="the features.csv of the run")
    ap.add_argument("feature_states", type=Path, help="the feature_states.csv of the run")
    ap.add_argument("stats", type=Path, help="stats_K*_*.txt")
    ap.add_argument("clusters", type=Path, help="clusters_K*_*.txt")
    ap.add_argument("--confounders", nargs="*", default=[], help="the model's confounders, in its order")
    ap.add_argument("--burnin", type=float, default=0.1, help="fraction of the samples discarded as burn-in")
    if seed:
        ap.add_argument("--seed", type=int, default=0, help="seed of the replicates' uniforms")
    ap.add_argument("--device", type=int, default=None)
    return ap


def read_run(args):
    """(data, clusters uint8 [T,K,N], weights [T,F,C], tables [T,R,F,S], n_groups) of the files run_parser's arguments name;
    data: predict.read_data's dict."""
    from . import predict
    data = predict.read_data(args.features, args.feature_states, args.confounders)
    weights, tables = predict.read_parameters(args.stats, data["feature_names"], data["state_names"], data["confounders"])
    clusters = predict.read_cluster_samples(args.clusters)
    if clusters.shape[0] != weights.shape[0]:
        raise SystemExit(f"{weights.shape[0]} stats rows, {clusters.shape[0]} cluster samples")
    return data, clusters, weights, tables, [len(g) for g in data["confounders"].values()]
