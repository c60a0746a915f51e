"""How much of a result is the priors: the power-scaling sensitivity of every logged column on the device
(include/sbe_psens.h; Kallioinen, Paananen, Buerkner & Vehtari 2023, Stat. Comput.; the recipe of `priorsense` and `arviz.psens`).

Every row of a `stats_K*.txt` file carries `likelihood`, `prior` and the prior's parts `cluster_size_prior`, `geo_prior`,
`source_prior` and `weights_prior`.  Raising one of them to a power alpha near 1 reweights the logged draws by
exp((alpha - 1) log p_component); the weights are smoothed by PSIS, and for every column the weighted and the unweighted
empirical cdf are compared by the cumulative Jensen-Shannon (CJS) distance.  One number per (component, column) comes out,
without a second run of the sampler, and because the parts are logged apart it is attributed to each prior on its own:

    res = powerscale_sensitivity([run0, run1], names=names, burnin=0.1)     # each run: float [S_r, P]
    res.sensitivity, res.pareto_k; res.diagnosis(); res.worst(20); res.table()
    h = PsensHandle(); h.reset(2, P, capacity=1000); h.append(0, rows); h.append(1, rows)
    h.weights_from_components([2, 3], delta=0.01, burnin=0.1); sums = h.compute()
    h.set_weights(w, burnin=0.1); sums = h.compute()    # any weights: summaries under reweighting
    python -m sbayes_amd.psens stats_K3_0.txt stats_K3_1.txt --clusters clusters_K3_0.txt clusters_K3_1.txt -o sensitivity.tsv

Numerical contract (tests/_psens_oracle.py restates it in NumPy; DESIGN.md section 28 states it): per chain the first
int(burnin * S_r) rows are dropped and the rest of all chains are stacked in chain order, N draws; there is no cut and no
split.  Component g gives two weight vectors, alpha = 1 / (1 + delta) and alpha = 1 + delta: PSIS of the log ratios
(alpha - 1) x[:, component], as tests/_elpd_oracle.psis_column has it, in float64.  Per (vector, column), with s the stable
ascending sort of the column, q the weights in that order, Q the normalised prefix sums of q in the one stated order of the
header, P_i = (i + 1) / N, M = (P + Q) / 2 and b_i = s_(i+1) - s_i: js = max(0, sum b P (log2 P - log2 M) + (Qint - Pint) /
(2 ln 2)) + max(0, sum b Q (log2 Q - log2 M) + (Pint - Qint) / (2 ln 2)) and bound = Pint + Qint, and the same of -x.  Formed
here, on the host: d = sqrt(js / bound) (0 where bound is 0), cjs = max(d, d of -x), and sensitivity[g] = (cjs[2 g] +
cjs[2 g + 1]) / (2 log2(1 + delta)).  A constant column gets flag 1 and distance 0, a column with a non-finite value flag 2 and
NaN; a component whose ratios are all equal gives uniform weights, vector flag 1 and distance exactly 0.

Caveats.  The formula follows the published definition; no `arviz` or `priorsense` value was available to compare with, so
agreement is claimed for the formula only.  The logged effect columns (areal, family, universal effects) were drawn at log
time from the conditionals of the UNSCALED model, so their sensitivity shows only what passes through the clusters, the
source and the weights.  Everything is conditional on PSIS being reliable: pareto_k is reported per vector, and k > 0.7
(vector flag 2) means the numbers of that component are not to be trusted.

There is no CPU fallback: without the library or a GPU the functions raise.  Handles follow the package's process model
(sbayes_amd/_proc.py): never pickled, forgotten (not destroyed) in a fork()ed child."""
from __future__ import annotations

import ctypes as ct
import math
from dataclasses import dataclass

import numpy as np

from . import _handle, diag
from ._handle import _ptr, c_handle_p
from ._samples import write_tsv
from .diag import FLAG_CONSTANT, FLAG_NONFINITE, MAX_CHAINS, MAX_COLUMNS, MAX_DRAWS, MIN_DRAWS, PATHS  # noqa: F401

ABI_VERSION = 1                          # SBE_PSENS_ABI_VERSION of include/sbe_psens.h
MAX_COMPONENTS = 8                       # SBE_PSENS_MAX_COMPONENTS
MAX_VECTORS = 16                         # SBE_PSENS_MAX_VECTORS
VFLAG_CONSTANT, VFLAG_UNRELIABLE = 1, 2  # SBE_PSENS_VFLAG_*
DEFAULT_COMPONENTS = ("likelihood", "prior", "cluster_size_prior", "geo_prior", "source_prior", "weights_prior")
DEFAULT_DELTA = 0.01
DEFAULT_THRESHOLD = 0.05

# name -> (restype, argtypes); mirrors include/sbe_psens.h one to one
PROTOTYPES = {
    **_handle.store_prototypes("sbe_psens", [ct.c_int64, ct.c_int64]),      # (last_kernel_ms fills float [2]: weights kernel, column kernel)
    "sbe_psens_lds_max_draws": (ct.c_int64, []),
    "sbe_psens_set_launch_columns": (ct.c_int, [c_handle_p, ct.c_int64]),
    "sbe_psens_set_global_path": (ct.c_int, [c_handle_p, ct.c_int]),
    "sbe_psens_weights_from_components": (ct.c_int, [c_handle_p, ct.c_void_p, ct.c_int, ct.c_void_p, ct.c_double] + [ct.c_void_p] * 4),
    "sbe_psens_set_weights": (ct.c_int, [c_handle_p, ct.c_void_p, ct.c_int, ct.c_void_p]),
    "sbe_psens_compute": (ct.c_int, [c_handle_p] + [ct.c_void_p] * 7),
    "sbe_psens_last_shape": (ct.c_int, [c_handle_p, ct.POINTER(ct.c_int), ct.POINTER(ct.c_int64), ct.POINTER(ct.c_int), ct.POINTER(ct.c_int),
                                        ct.POINTER(ct.c_int64), ct.POINTER(ct.c_int64)]),
    "sbe_psens_sorted_column": (ct.c_int, [c_handle_p, ct.c_int64, ct.c_void_p, ct.c_void_p]),
    "sbe_psens_device_log2": (ct.c_int, [c_handle_p, ct.c_int64, ct.c_void_p, ct.c_void_p]),
}


def load():
    """The engine library with the prototypes of include/sbe_psens.h attached."""
    return _handle.bind("sbe_psens", PROTOTYPES, ABI_VERSION)


def lds_max_draws() -> int:
    """Largest N whose sort keys (12 bytes per draw) the kernels keep in LDS; longer columns sort in a global scratch."""
    return int(load().sbe_psens_lds_max_draws())


# ---- the host's part of the contract ---------------------------------------------------------------------------------
def distance(js, bound):
    """sqrt(js / bound), and 0 where bound is 0 (NaN stays NaN)."""
    js, bound = np.asarray(js, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.sqrt(js / bound)
    return np.where(bound == 0.0, 0.0, d)


def cjs_distance(js, bound, js_neg, bound_neg):
    """The CJS distance made symmetric as the published recipe does: the larger of the distances of x and of -x."""
    return np.maximum(distance(js, bound), distance(js_neg, bound_neg))


def sensitivity_of(cjs, delta):
    """float64 [G, P] of cjs [2 G, P]: the two directions' distances averaged and divided by log2(1 + delta)."""
    cjs = np.asarray(cjs, dtype=np.float64)
    return (cjs[0::2] + cjs[1::2]) / (2.0 * math.log2(1.0 + float(delta)))


@dataclass
class PsensSums:
    """What sbe_psens_compute returns, float64 [V, P] each, and flag uint8 [P] (1 constant, 2 non-finite)."""
    js: np.ndarray
    bound: np.ndarray
    js_neg: np.ndarray
    bound_neg: np.ndarray
    wmean: np.ndarray
    wsd: np.ndarray
    flag: np.ndarray

    def cjs(self):
        return cjs_distance(self.js, self.bound, self.js_neg, self.bound_neg)


@dataclass
class PsensResult:
    """sensitivity: float64 [G, P], one row per component; cjs, wmean, wsd: float64 [2 G, P] (row 2 g: alpha = 1 / (1 + delta),
    row 2 g + 1: alpha = 1 + delta); pareto_k, ess: float64 [2 G]; vflag: uint8 [2 G] (1: equal ratios, uniform weights; 2:
    k > 0.7); flag: uint8 [P] (1 constant, 2 non-finite); components: their names; component_columns: their columns."""
    sensitivity: np.ndarray
    cjs: np.ndarray
    wmean: np.ndarray
    wsd: np.ndarray
    pareto_k: np.ndarray
    ess: np.ndarray
    vflag: np.ndarray
    flag: np.ndarray
    components: list
    component_columns: list
    delta: float
    names: list
    n_chains: int
    n_draws: int
    path: str = "lds"
    weights_ms: float = 0.0
    column_ms: float = 0.0

    def _row(self, component):
        return self.components.index(component) if component in self.components else None

    def diagnosis(self, threshold=DEFAULT_THRESHOLD):
        """Per column, by the paper's rule on the `prior` and `likelihood` components: "prior-data conflict" where both
        sensitivities exceed the threshold, "strong prior / weak likelihood" where the prior's does and the likelihood's
        does not, "-" otherwise (and everywhere when either component was not among those asked for)."""
        prior, lik = self._row("prior"), self._row("likelihood")
        if prior is None or lik is None:
            return ["-"] * len(self.names)
        threshold = float(threshold)
        p, lk = self.sensitivity[prior] > threshold, self.sensitivity[lik] > threshold
        return ["prior-data conflict" if a and b else "strong prior / weak likelihood" if a else "-" for a, b in zip(p, lk)]

    def header(self):
        return ["column"] + list(self.components) + ["diagnosis", "flag"]

    def table(self, threshold=DEFAULT_THRESHOLD):
        """One row per column, in the order of header(): the name, the sensitivity per component, the diagnosis, the flag."""
        diagnosis = self.diagnosis(threshold)
        return [[name] + [float(v) for v in self.sensitivity[:, i]] + [diagnosis[i], int(self.flag[i])] for i, name in enumerate(self.names)]

    def worst(self, n=20):
        """The n columns of largest sensitivity to any component, largest first (NaN last): [(name, component, sensitivity)]."""
        with np.errstate(invalid="ignore"):
            top = np.where(np.isnan(self.sensitivity), -np.inf, self.sensitivity)
        which = top.argmax(axis=0)
        order = np.argsort(-top.max(axis=0), kind="stable")
        return [(self.names[i], self.components[which[i]], float(self.sensitivity[which[i], i])) for i in order[:max(int(n), 0)]]


# ---- validation (host side, before any library call) -----------------------------------------------------------
def _plan(rows_per_chain, burnin):
    """(burn rows per chain, N) for chains of these lengths; burnin: a share in [0, 1) or the rows to drop per chain."""
    m = len(rows_per_chain)
    if not 1 <= m <= MAX_CHAINS:
        raise ValueError(f"{m} chains; the sensitivity takes 1 .. {MAX_CHAINS}")
    if np.ndim(burnin) == 0:
        burnin = float(burnin)
        if not 0.0 <= burnin < 1.0:
            raise ValueError(f"burnin={burnin} must lie in [0, 1)")
        burn = [int(burnin * int(s)) for s in rows_per_chain]              # Results.drop_burnin
    else:
        burn = [int(b) for b in burnin]
        if len(burn) != m:
            raise ValueError(f"{len(burn)} burn-in row counts for {m} chains")
    left = [int(s) - b for s, b in zip(rows_per_chain, burn)]
    for c, (b, n) in enumerate(zip(burn, left)):
        if b < 0:
            raise ValueError(f"burn-in rows of chain {c} are negative: {b}")
        if n < MIN_DRAWS:
            raise ValueError(f"chain {c} has {n} draws after burn-in; at least {MIN_DRAWS} are needed")
    if sum(left) > MAX_DRAWS:
        raise ValueError(f"{sum(left)} draws per column after burn-in exceed {MAX_DRAWS} (2^20)")
    return burn, sum(left)


def _check_delta(delta):
    delta = float(delta)
    if not (delta > 0.0 and math.isfinite(delta)):
        raise ValueError(f"delta={delta} must be positive and finite")
    return delta


def _check_components(components, names, n_columns):
    """(names of the components, their columns): names are looked up in `names`, indices taken as they are."""
    if components is None:
        components = [c for c in DEFAULT_COMPONENTS if names is not None and c in names]
        if not components:
            raise ValueError(f"none of the default components {list(DEFAULT_COMPONENTS)} is among the column names; name the components")
    components = list(components)
    if not 1 <= len(components) <= MAX_COMPONENTS:
        raise ValueError(f"{len(components)} components; a call takes 1 .. {MAX_COMPONENTS}")
    labels, columns = [], []
    for c in components:
        if isinstance(c, str):
            if names is None or c not in names:
                raise ValueError(f"component {c!r} is not among the column names")
            col = list(names).index(c)
        else:
            col = int(c)
            if not 0 <= col < n_columns:
                raise ValueError(f"component column {col} out of range [0, {n_columns})")
        labels.append(str(names[col]) if names is not None else f"c{col}")
        columns.append(col)
    return labels, columns


def _check_weights(weights, n_draws):
    w = np.asarray(weights)
    if w.dtype.kind not in "fiub":
        raise TypeError(f"weights must be numeric, got {w.dtype}")
    if w.ndim == 1:
        w = w.reshape(1, -1)
    if w.ndim != 2 or not 1 <= w.shape[0] <= MAX_VECTORS or w.shape[1] != n_draws:
        raise ValueError(f"weights must be [V, {n_draws}] with V in 1 .. {MAX_VECTORS} (one row per vector, one entry per draw after burn-in), "
                         f"got shape {w.shape}")
    w = np.ascontiguousarray(w, dtype=np.float64)
    if not np.all(np.isfinite(w)) or np.any(w < 0.0):
        raise ValueError("weights must be non-negative and finite")
    if np.any(w.sum(axis=1) <= 0.0):
        raise ValueError("every weight vector must have a positive sum")
    return w


class PsensHandle(diag.ColumnStoreHandle):
    """Owner of one sbe_psens handle: the float64 store of several chains on one device and up to 16 weight vectors over its
    draws.  last_kernel_ms(): the weights kernel and the column kernel of the last calls, added."""
    _prefix, _noun, _takes = "sbe_psens", "a sensitivity handle", "the sensitivity takes"
    _load = staticmethod(load)

    def _planned(self, burnin):
        if not self.n_chains:
            raise ValueError("the store has no shape yet (reset)")
        return _plan([self.rows(c) for c in range(self.n_chains)], burnin)

    def set_global_path(self, on):
        """Sort in the global scratch whatever N is (the tests' path switch).  Results do not depend on it."""
        self._check(self._lib.sbe_psens_set_global_path(self._h, int(bool(on))))

    def weights_from_components(self, columns, delta=DEFAULT_DELTA, burnin=0.1, weights=False):
        """The PSIS weights of the components' power-scaling (columns: indices into the store): (pareto_k, ess float64
        [2 G], vflag uint8 [2 G]) and, with weights=True, the weights float64 [2 G, N] behind them."""
        delta = _check_delta(delta)
        _labels, columns = _check_components(columns, None, self.n_columns)
        burn, n = self._planned(burnin)
        v = 2 * len(columns)
        burn_rows, cols = np.asarray(burn, dtype=np.int64), np.asarray(columns, dtype=np.int64)
        k, ess, vflag = np.empty(v, dtype=np.float64), np.empty(v, dtype=np.float64), np.empty(v, dtype=np.uint8)
        w = np.empty((v, n), dtype=np.float64) if weights else None
        self._check(self._lib.sbe_psens_weights_from_components(self._h, _ptr(burn_rows), len(columns), _ptr(cols), delta, _ptr(k), _ptr(ess),
                                                                _ptr(vflag), _ptr(w) if weights else None))
        return (k, ess, vflag, w) if weights else (k, ess, vflag)

    def set_weights(self, weights, burnin=0.1):
        """The caller's own weights: float [V, N] (or [N]), non-negative, finite, of positive sum per vector."""
        burn, n = self._planned(burnin)
        w = _check_weights(weights, n)
        burn_rows = np.asarray(burn, dtype=np.int64)
        self._check(self._lib.sbe_psens_set_weights(self._h, _ptr(burn_rows), w.shape[0], _ptr(w)))

    def last_shape(self):
        """(chains, N, V, path, launches of the column kernel, columns of each) of the last weights and compute calls."""
        m, n, v, path, launches, cols = ct.c_int(0), ct.c_int64(0), ct.c_int(0), ct.c_int(0), ct.c_int64(0), ct.c_int64(0)
        self._check(self._lib.sbe_psens_last_shape(self._h, ct.byref(m), ct.byref(n), ct.byref(v), ct.byref(path), ct.byref(launches), ct.byref(cols)))
        return m.value, n.value, v.value, PATHS[path.value], launches.value, cols.value

    def last_kernel_times(self):
        """(weights kernel ms, column kernel ms) of the last weights and compute calls (HIP events)."""
        ms = (ct.c_float * 2)()
        self._check(self._lib.sbe_psens_last_kernel_ms(self._h, ms))
        return float(ms[0]), float(ms[1])

    def last_kernel_ms(self) -> float:
        return sum(self.last_kernel_times())

    def compute(self) -> PsensSums:
        """The sums of every (vector, column) under the weights last set."""
        _m, _n, v, _path, _launches, _cols = self.last_shape()
        p = self.n_columns
        js, bound, js_neg, bound_neg, wmean, wsd = (np.empty((v, p), dtype=np.float64) for _ in range(6))
        flag = np.empty(p, dtype=np.uint8)
        self._check(self._lib.sbe_psens_compute(self._h, _ptr(js), _ptr(bound), _ptr(js_neg), _ptr(bound_neg), _ptr(wmean), _ptr(wsd), _ptr(flag)))
        return PsensSums(js, bound, js_neg, bound_neg, wmean, wsd, flag)

    def sorted_column(self, column):
        """An inspection call: (values float64 [N], samples int32 [N]) of one column's sort under the draws of the last
        weights call."""
        column = int(column)
        if not 0 <= column < self.n_columns:
            raise ValueError(f"column {column} out of range [0, {self.n_columns})")
        _m, n, _v, _path, _launches, _cols = self.last_shape()
        values, samples = np.empty(n, dtype=np.float64), np.empty(n, dtype=np.int32)
        self._check(self._lib.sbe_psens_sorted_column(self._h, column, _ptr(values), _ptr(samples)))
        return values, samples

    def device_log2(self, values):
        """An inspection call: the kernels' float64 log2 of every value."""
        x = np.ascontiguousarray(values, dtype=np.float64).ravel()
        if not 1 <= x.size <= 1 << 24:
            raise ValueError(f"{x.size} values; a call takes 1 .. 2^24")
        out = np.empty_like(x)
        self._check(self._lib.sbe_psens_device_log2(self._h, x.size, _ptr(x), _ptr(out)))
        return out


def powerscale_sensitivity(chains, components=None, delta=DEFAULT_DELTA, burnin=0.1, names=None, device=None) -> PsensResult:
    """The sensitivity of every column of several runs to the power-scaling of logged components.  chains: a float array
    [M, S, P] or a list of [S_r, P] arrays (runs may differ in length: all their draws after burn-in are used).  components:
    names (looked up in `names`) or column indices; default: those of likelihood, prior, cluster_size_prior, geo_prior,
    source_prior and weights_prior that `names` holds."""
    chains, lengths, p = diag._check_chains(chains)
    delta = _check_delta(delta)
    given = None if names is None else [str(v) for v in names]
    names = diag._check_names(names, p)
    labels, columns = _check_components(components, given, p)
    _plan(lengths, burnin)                                                  # (refuses before the device is touched)
    blocks = [diag._check_rows(c) for c in chains]
    h = PsensHandle.filled(device, (len(blocks), p, max(lengths)), blocks)
    try:
        k, ess, vflag = h.weights_from_components(columns, delta=delta, burnin=burnin)
        sums = h.compute()
        m, n, _v, path, _launches, _cols = h.last_shape()
        weights_ms, column_ms = h.last_kernel_times()
    finally:
        h.close()
    cjs = sums.cjs()
    return PsensResult(sensitivity_of(cjs, delta), cjs, sums.wmean, sums.wsd, k, ess, vflag, sums.flag, labels, columns, delta, names, m, n, path,
                       weights_ms, column_ms)


def write_table(path, res: PsensResult, threshold=DEFAULT_THRESHOLD):
    write_tsv(path, res.header(), res.table(threshold))


def _load_aligned_runs(stats_paths, cluster_paths, device):
    """diag._load_runs with the cluster labels of all runs brought to those of the first: the per-cluster stats columns and the
    indicator columns move together (sbayes_amd.align)."""
    if not cluster_paths:
        return diag._load_runs(stats_paths, cluster_paths)
    from . import align
    names, runs = diag._load_runs(stats_paths, cluster_paths)
    samples = [align.read_clusters(p) for p in cluster_paths]
    n_indicators = samples[0].shape[1] * samples[0].shape[2]
    perms = align.align_runs(samples, device=device).total_perms
    n_stats = len(names) - n_indicators
    out = []
    for run, sample, perm in zip(runs, samples, perms):
        _names, stats = align.permute_stats(names[:n_stats], run[:, :n_stats], perm)
        out.append(np.concatenate([stats, align.apply(sample, perm).reshape(sample.shape[0], -1).astype(np.float64)], axis=1))
    return names, out


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m sbayes_amd.psens",
                                 description="power-scaling sensitivity of every column of several sBayes runs to the logged prior and likelihood parts")
    ap.add_argument("stats", nargs="+", help="stats_K*_*.txt files, one per run")
    ap.add_argument("--clusters", nargs="*", default=[], help="clusters_K*_*.txt files, one per run, in the same order")
    ap.add_argument("--components", nargs="*", default=None, help=f"column names (default: those of {', '.join(DEFAULT_COMPONENTS)} present)")
    ap.add_argument("--delta", type=float, default=DEFAULT_DELTA)
    ap.add_argument("--burnin", type=float, default=0.1)
    ap.add_argument("--threshold", type=float, default=DEFAULT_THRESHOLD)
    ap.add_argument("--top", type=int, default=20, help="print the most sensitive columns")
    ap.add_argument("-o", "--out", default=None, help="write the full table (tab-separated) here")
    ap.add_argument("--device", type=int, default=None)
    args = ap.parse_args(argv)
    names, runs = _load_aligned_runs(args.stats, args.clusters, args.device)
    res = powerscale_sensitivity(runs, components=args.components, delta=args.delta, burnin=args.burnin, names=names, device=args.device)
    print(f"{len(res.names)} columns, {res.n_chains} runs, {res.n_draws} draws ({res.path} path, weights kernel {res.weights_ms:.3f} ms, "
          f"column kernel {res.column_ms:.3f} ms)")
    print(f"{'component':24s} {'alpha':>10s} {'pareto_k':>10s} {'ess':>10s} flag")
    for g, name in enumerate(res.components):
        for d, alpha in enumerate((1.0 / (1.0 + res.delta), 1.0 + res.delta)):
            v = 2 * g + d
            print(f"{name:24s} {alpha:10.6f} {res.pareto_k[v]:10.3f} {res.ess[v]:10.1f} {int(res.vflag[v])}")
    if np.any(res.vflag & VFLAG_UNRELIABLE):
        print("pareto_k > 0.7 for some component: its sensitivities are not to be trusted")
    diagnosis = res.diagnosis(args.threshold)
    print(f"prior-data conflict: {diagnosis.count('prior-data conflict')} columns; strong prior / weak likelihood: "
          f"{diagnosis.count('strong prior / weak likelihood')} columns (threshold {args.threshold:g})")
    print(f"{'column':40s} {'component':24s} {'sensitivity':>12s}")
    for name, component, value in res.worst(args.top):
        print(f"{name:40s} {component:24s} {value:12.5f}")
    if args.out:
        write_table(args.out, res, args.threshold)
        print(f"wrote {args.out}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
