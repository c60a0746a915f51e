"""Screening of all feature pairs for dependence on the device: the chi-squared test of independence (include/sbe_assoc.h).

The mixture model treats features as independent given their source, and sBayes ships a tool to check a data set for
pairs that are not (sbayes/tools/find_correlated_features.py): per pair of features `pd.crosstab` over the objects
where both are observed, `scipy.stats.chi2_contingency` on the table, and a report of the pairs whose p-value is
below a threshold.  This module runs that loop for all pairs at once on the GPU:

    res = feature_association(features, n_states=None, device=0)   # codes [N, F] uint8 (255 = NA) or one-hot bool [N, F, S]
    res.statistic, res.pvalue, res.dof, res.n, res.valid           # [F, F], symmetric; the diagonal is not a pair
    res.correlated(p_threshold=1e-4)    # [(pvalue, i, j)] sorted by p-value, as the tool sorts its corr_features
    res.table(i, j)                     # observed, expected, deviation: what the tool plots for a flagged pair

    python -m sbayes_amd.assoc --input features.csv [-p 1e-4]      # the tool's report (the PDF plots are not made)

Numerical contract (tests/_assoc_oracle.py restates it in NumPy): a pair is valid when both features take more than
one state over the objects where both are observed (the tool skips the others); dof = (R-1)(C-1) over the occupied
rows and columns; expected counts r c / n in fp64; Yates' correction at dof 1 (SciPy's default); Pearson's statistic
summed in a fixed order; p-value Q(dof/2, statistic/2) in fp64 on the device.  Invalid pairs and the diagonal hold
statistic 0, p-value NaN, dof 0.  Limits: at most 2^24 objects, 32 states per feature, 4096 features, 2^31 codes
(SBE_ERR_ARG beyond, with the limit named).

Handles follow the package's process model (sbayes_amd/_proc.py): one per device, created lazily in the process that
uses it, never pickled, forgotten (not destroyed) in a fork()ed child, where every further call raises."""
from __future__ import annotations

import ctypes as ct
from dataclasses import dataclass, field

import numpy as np

from . import _handle
from ._handle import _ptr, c_handle_p

ABI_VERSION = 1                          # SBE_ASSOC_ABI_VERSION of include/sbe_assoc.h
NA = 255                                 # SBE_ASSOC_NA
MAX_OBJECTS = 1 << 24                    # SBE_ASSOC_MAX_OBJECTS
MAX_STATES = 32                          # SBE_ASSOC_MAX_STATES
MAX_FEATURES = 4096                      # SBE_ASSOC_MAX_FEATURES
MAX_CODES = 1 << 31                      # SBE_ASSOC_MAX_CODES
METADATA_COLUMNS = ("id", "name", "family", "x", "y")

# name -> (restype, argtypes); mirrors include/sbe_assoc.h one to one (the engine's own table, _lib.PROTOTYPES, covers
# the three engine headers and is not extended)
PROTOTYPES = {
    **_handle.unit_prototypes("sbe_assoc"),
    "sbe_assoc_create": (ct.c_int, [ct.POINTER(c_handle_p), ct.c_int]),
    "sbe_assoc_set_launch_tiles": (ct.c_int, [c_handle_p, ct.c_int64]),
    "sbe_assoc_compute": (ct.c_int, [c_handle_p, ct.c_void_p, ct.c_int64, ct.c_int64, ct.c_void_p, ct.c_void_p, ct.c_void_p,
                                     ct.c_void_p, ct.c_void_p, ct.c_void_p]),
    "sbe_assoc_tables": (ct.c_int, [c_handle_p, ct.c_void_p, ct.c_int64, ct.c_void_p]),
    "sbe_assoc_last_shape": (ct.c_int, [c_handle_p, ct.POINTER(ct.c_int32), ct.POINTER(ct.c_int64), ct.POINTER(ct.c_int64)]),
}


def load():
    """The engine library with the prototypes of include/sbe_assoc.h attached."""
    return _handle.bind("sbe_assoc", PROTOTYPES, ABI_VERSION)


class AssocHandle(_handle.UnitHandle):
    """Owner of one sbe_assoc handle: a stream and the device buffers of the last data set on one device.
    last_kernel_ms(): the pair kernel's launches of the last compute call."""
    _prefix, _noun = "sbe_assoc", "an association handle"

    def __init__(self, device=0):
        self._data = None                  # the codes the device holds (AssociationResult.tables)
        self._create_on(load, device)

    def set_launch_tiles(self, tile_pairs):
        """Tile pairs per launch of the pair kernel (0: the default).  Results do not depend on it."""
        self._check(self._lib.sbe_assoc_set_launch_tiles(self._h, int(tile_pairs)))

    def compute(self, x, n_states):
        """(statistic, pvalue, dof, n, valid), [F, F] each; x: uint8 [N, F], n_states: int32 [F] (validated by the caller)."""
        n, f = x.shape
        statistic, pvalue = np.empty((f, f), dtype=np.float64), np.empty((f, f), dtype=np.float64)
        dof, cnt = np.empty((f, f), dtype=np.int32), np.empty((f, f), dtype=np.int32)
        valid = np.empty((f, f), dtype=np.uint8)
        self._check(self._lib.sbe_assoc_compute(self._h, _ptr(x), n, f, _ptr(n_states), _ptr(statistic), _ptr(pvalue),
                                                _ptr(dof), _ptr(cnt), _ptr(valid)))
        return statistic, pvalue, dof, cnt, valid.view(np.bool_)

    def tables(self, pairs, n_states_max):
        """int32 [n_pairs, S, S]: the observed tables of `pairs` ([n_pairs, 2]) of the last computed data set."""
        pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        out = np.empty((pairs.shape[0], n_states_max, n_states_max), dtype=np.int32)
        self._check(self._lib.sbe_assoc_tables(self._h, _ptr(pairs), pairs.shape[0], _ptr(out)))
        return out

    def last_shape(self):
        """(S_pad, tile pairs, launches) of the last compute call."""
        s_pad, tiles, launches = ct.c_int32(0), ct.c_int64(0), ct.c_int64(0)
        self._check(self._lib.sbe_assoc_last_shape(self._h, ct.byref(s_pad), ct.byref(tiles), ct.byref(launches)))
        return s_pad.value, tiles.value, launches.value


_HANDLES = _handle.device_cache()          # device -> AssocHandle


def release_all():
    _handle.release_cached(_HANDLES)


def handle_for(device=0) -> AssocHandle:
    """The process's handle on `device`, created on first use."""
    return _handle.cached_handle(_HANDLES, AssocHandle, device)


# ---- validation and conversion (host side, before any library call) ------------------------------------------------
def state_codes(features):
    """uint8 [N, F] codes of the reference's one-hot boolean [N, F, S] (`Features.values`): an all-False row is NA."""
    a = np.asarray(features)
    if a.dtype != np.bool_ or a.ndim != 3:
        raise TypeError(f"one-hot features must be bool [N, F, S], got {a.dtype} with {a.ndim} dimensions")
    if a.shape[2] > MAX_STATES:
        raise ValueError(f"{a.shape[2]} states per feature; the screening handles at most {MAX_STATES}")
    per_row = a.sum(axis=2)
    if np.any(per_row > 1):
        raise ValueError("one-hot features hold more than one state in a row")
    return np.where(per_row == 0, NA, a.argmax(axis=2)).astype(np.uint8)


def _check_inputs(features, n_states):
    a = np.asarray(features)
    if a.dtype == np.bool_:
        if n_states is None and a.ndim == 3 and a.shape[2] >= 1:
            n_states = np.full(a.shape[1], a.shape[2], dtype=np.int32)   # (states that never occur change nothing)
        a = state_codes(a)
    if a.dtype != np.uint8:
        raise TypeError(f"features must be uint8 codes [N, F] (255 = not observed) or one-hot bool [N, F, S], got {a.dtype}")
    if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"codes must be [n_objects, n_features] with both positive, got shape {a.shape}")
    n, f = a.shape
    if n > MAX_OBJECTS:
        raise ValueError(f"{n} objects; counts are exact on the matrix pipe up to {MAX_OBJECTS} (2^24)")
    if f > MAX_FEATURES:
        raise ValueError(f"{f} features; the [F, F] outputs are limited to {MAX_FEATURES} features")
    if n * f > MAX_CODES:
        raise ValueError(f"{n} x {f} codes exceed the limit of {MAX_CODES} (2^31)")
    x = np.ascontiguousarray(a)
    if n_states is None:
        observed = np.where(x == NA, 0, x.astype(np.int64) + 1)
        ns = np.maximum(1, observed.max(axis=0))
    else:
        ns = np.asarray(n_states)
        if ns.shape != (f,) or not np.issubdtype(ns.dtype, np.integer):
            raise ValueError(f"n_states must be {f} integers, got shape {ns.shape} of {ns.dtype}")
    if np.any(ns < 1) or np.any(ns > MAX_STATES):
        raise ValueError(f"n_states must lie in [1, {MAX_STATES}] (this unit's limit), got {int(ns.min())} .. {int(ns.max())}")
    ns = np.ascontiguousarray(ns, dtype=np.int32)
    bad = (x != NA) & (x >= ns[None, :].astype(np.int64))
    if np.any(bad):
        i, j = np.argwhere(bad)[0]
        raise ValueError(f"features[{i}, {j}] = {int(x[i, j])} is neither below n_states[{j}] = {int(ns[j])} nor {NA} (not observed)")
    return x, ns


@dataclass
class AssociationResult:
    """Per pair of features, [F, F] and symmetric: Pearson's chi-squared statistic, its p-value, the degrees of freedom,
    the number of objects where both are observed and whether the pair could be tested at all."""
    statistic: np.ndarray
    pvalue: np.ndarray
    dof: np.ndarray
    n: np.ndarray
    valid: np.ndarray
    n_states: np.ndarray
    names: list = None
    _handle: AssocHandle = field(default=None, repr=False)
    _codes: np.ndarray = field(default=None, repr=False)

    def correlated(self, p_threshold=1e-4):
        """[(pvalue, i, j)], i < j, of the valid pairs with pvalue < p_threshold, sorted as the tool sorts them."""
        i, j = np.nonzero(np.triu(self.valid, 1) & (np.nan_to_num(self.pvalue, nan=np.inf) < p_threshold))
        return sorted((float(self.pvalue[a, b]), int(a), int(b)) for a, b in zip(i, j))

    def tables(self, pairs):
        """int32 [n_pairs, S, S]: the observed tables of the pairs (table kernel), rows = states of the first feature."""
        h = self._handle
        if h is None or not h._h:
            raise RuntimeError("the handle of this result was closed")
        if h._data is not self._codes:                     # another data set went through the handle since
            h.compute(self._codes, self.n_states)
            h._data = self._codes
        return h.tables(pairs, int(self.n_states.max()))

    def table(self, i, j):
        """(observed, expected, deviation) of the pair over its occupied rows and columns, as the tool plots them:
        observed int32 [R, C], expected = r c / n, deviation = observed - expected."""
        full = self.tables([(i, j)])[0]
        obs = full[np.ix_(full.sum(axis=1) > 0, full.sum(axis=0) > 0)]
        if obs.size == 0:
            return obs, obs.astype(np.float64), obs.astype(np.float64)
        expected = np.outer(obs.sum(axis=1).astype(np.float64), obs.sum(axis=0).astype(np.float64)) / float(obs.sum())
        return obs, expected, obs - expected


def feature_association(features, n_states=None, device=0, names=None) -> AssociationResult:
    """The chi-squared test of independence for every pair of features, on the device.  `features`: uint8 codes [N, F]
    with 255 = not observed, or the reference's one-hot bool [N, F, S] (`Features.values`); `n_states`: states per
    feature (default: one more than the largest code that occurs)."""
    x, ns = _check_inputs(features, n_states)
    h = handle_for(device)
    statistic, pvalue, dof, n, valid = h.compute(x, ns)
    h._data = x
    return AssociationResult(statistic, pvalue, dof, n, valid, ns, list(names) if names is not None else None, h, x)


# ---- the tool's command line ---------------------------------------------------------------------------------------
def frame_codes(frame):
    """(codes uint8 [N, F], n_states int32 [F], feature names, state names per feature) of a data frame of state strings:
    the states of a feature are numbered in sorted order, missing cells are NA."""
    import pandas as pd
    names = [str(c) for c in frame.columns]
    codes = np.full(frame.shape, NA, dtype=np.uint8)
    states = []
    for k, col in enumerate(frame.columns):
        values = frame[col]
        seen = sorted(values.dropna().unique())
        if len(seen) > MAX_STATES:
            raise ValueError(f"feature {col!r} has {len(seen)} states; the screening handles at most {MAX_STATES}")
        lookup = {s: c for c, s in enumerate(seen)}
        codes[:, k] = [NA if pd.isna(v) else lookup[v] for v in values]
        states.append(seen)
    return codes, np.array([max(1, len(s)) for s in states], dtype=np.int32), names, states


def read_features_csv(path):
    """The feature columns of an sBayes features.csv as a frame of state strings (pandas, imported only here): the five
    metadata columns are required and dropped, cells are stripped, blank cells are missing.  The reference also folds
    cell strings to ASCII through `unidecode`; that package is not a dependency here, so non-ASCII state names stay as
    they are (distinct strings stay distinct states either way unless two differ only by their accents)."""
    import pandas as pd
    data = pd.read_csv(path, dtype=str, keep_default_na=False)
    for column in METADATA_COLUMNS:
        if column not in data.columns:
            raise ValueError(f"Required column '{column}' missing in data file.")
    frame = data.drop(columns=list(METADATA_COLUMNS))
    frame = frame.apply(lambda col: col.str.strip())
    return frame.mask(frame == "")


def main(argv=None):
    import argparse
    parser = argparse.ArgumentParser(description="Find features with significant correlation in a data set (on the GPU).")
    parser.add_argument("--input", required=True, help="The input CSV file")
    parser.add_argument("-p", "--pThreshold", type=float, default=0.0001, help="The significance level (p-value threshold)")
    parser.add_argument("--device", type=int, default=0)
    args = parser.parse_args(argv)
    frame = read_features_csv(args.input)
    print(frame.shape)
    codes, n_states, names, _states = frame_codes(frame)
    res = feature_association(codes, n_states, device=args.device, names=names)
    for i in range(len(names)):                              # the tool's order: combinations(columns, 2)
        for j in range(i + 1, len(names)):
            if res.valid[i, j] and res.pvalue[i, j] < args.pThreshold:
                print(f"Correlation between [{names[i]}] and [{names[j]}].")
                print(f"Chi-squared test statistic = {res.statistic[i, j]}")
                print(f"Chi-squared test p-value = {res.pvalue[i, j]}")
                print()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
