"""Convergence diagnostics on the device: effective sample size and split R-hat per column (include/sbe_diag.h).

The sBayes manual asks for several runs of one model, a check of their convergence and effective sample size (ESS), and a
comparison of the estimates across runs.  A `stats_K*_*.txt` file has one column per weight and per effect entry, and
the cluster samples add K * N indicator columns: far more than an interactive tool opens.  This module does the step on
the GPU, one workgroup per column:

    res = convergence([run0, run1, run2], burnin=0.1)    # each run: float [S_r, P]
    res.summary(); res.worst(20)
    h = DiagHandle(); h.reset(2, P, capacity=1000)        # for callers who append rows as they are logged
    h.append(0, rows); h.append(1, rows); h.compute(burnin=0.1)
    names, rows = read_stats("stats_K3_0.txt"); cnames, crows = read_clusters("clusters_K3_0.txt")
    python -m sbayes_amd.diag stats_K3_0.txt stats_K3_1.txt --clusters clusters_K3_0.txt clusters_K3_1.txt --out diag.tsv

Numerical contract (tests/_diag_oracle.py restates it in NumPy; DESIGN.md section 16 states it): per chain the first
int(burnin * S_r) rows are dropped, the chains are cut at the end to the shortest remaining length, and with split=True
every chain of n draws becomes the two chains x[:n // 2] and x[-(n // 2):].  Per column: the biased autocovariances
averaged over the chains, R-hat = sqrt(var_plus / mean_var), the autocorrelations 1 - (mean_var - G(t)) / var_plus cut by
Geyer's initial positive sequence and smoothed by the initial monotone sequence, tau floored at 1 / log10(M n),
ess = M n / tau, mcse_mean = sd / sqrt(ess).  A constant column (max - min < 1e-15) gets flag 1, ess = M n, rhat = NaN,
mcse_mean = 0; a column with a non-finite value gets flag 2 and NaN everywhere; neither fails the call.  Limits: at most
64 chains, at least 4 draws per chain and at most 2^20 draws per column after the split.

There is no CPU fallback: without the library or a GPU the functions raise.  Handles follow the package's process model
(sbayes_amd/_proc.py): never pickled, forgotten (not destroyed) in a fork()ed child."""
from __future__ import annotations

import ctypes as ct
import warnings
from dataclasses import dataclass, field
from pathlib import Path

import numpy as np

from . import _handle
from ._handle import _ptr, c_handle_p

ABI_VERSION = 1                          # SBE_DIAG_ABI_VERSION of include/sbe_diag.h
MAX_CHAINS = 64                          # SBE_DIAG_MAX_CHAINS
MIN_DRAWS = 4                            # SBE_DIAG_MIN_DRAWS (n after the split)
MAX_DRAWS = 1 << 20                      # SBE_DIAG_MAX_DRAWS (M * n after the split)
MAX_COLUMNS = 2 ** 31 - 1                # the int32 of the ABI
FLAG_CONSTANT, FLAG_NONFINITE, FLAG_TRUNCATED = 1, 2, 4
PATHS = {0: "lds", 1: "global"}          # SBE_DIAG_PATH_*

# name -> (restype, argtypes); mirrors include/sbe_diag.h one to one (the engine's own table, _lib.PROTOTYPES, is not extended)
PROTOTYPES = {
    **_handle.store_prototypes("sbe_diag", [ct.c_int64, ct.c_int64]),
    "sbe_diag_lds_max_draws": (ct.c_int64, []),
    "sbe_diag_set_launch_columns": (ct.c_int, [c_handle_p, ct.c_int64]),
    "sbe_diag_compute": (ct.c_int, [c_handle_p, ct.c_void_p, ct.c_int, ct.c_int64, ct.c_void_p, ct.c_void_p, ct.c_void_p,
                                    ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_void_p]),
    "sbe_diag_last_shape": (ct.c_int, [c_handle_p, ct.POINTER(ct.c_int), ct.POINTER(ct.c_int64), ct.POINTER(ct.c_int),
                                       ct.POINTER(ct.c_int64)]),
}

INDEX_COLUMNS = ("Sample", "sample_id")  # columns of a stats file that count samples or name the run: no parameters


def load():
    """The engine library with the prototypes of include/sbe_diag.h attached."""
    return _handle.bind("sbe_diag", PROTOTYPES, ABI_VERSION)


def lds_max_draws() -> int:
    """Largest M * n (after the split) whose columns the kernel stages in LDS; longer columns take the global path."""
    return int(load().sbe_diag_lds_max_draws())


@dataclass
class DiagResult:
    """Per column: mean, sd (ddof 1, over all draws), ess, rhat, mcse_mean (float64), n_lags (int32: the largest lag whose
    autocovariance the column needed), flag (uint8: 1 constant, 2 non-finite, 4 truncated by max_lag).  n_chains and
    n_draws are M and n after the split; cut[r] rows were dropped from the end of run r to reach a common length."""
    mean: np.ndarray
    sd: np.ndarray
    ess: np.ndarray
    rhat: np.ndarray
    mcse_mean: np.ndarray
    n_lags: np.ndarray
    flag: np.ndarray
    names: list
    n_chains: int
    n_draws: int
    cut: tuple = ()
    path: str = "lds"
    launches: int = 1
    kernel_ms: float = 0.0
    _order: np.ndarray = field(default=None, repr=False)

    def worst(self, k=20):
        """The k columns of lowest ESS, lowest first (non-finite columns last): [(name, ess, rhat, mcse_mean, flag)]."""
        if self._order is None:
            self._order = np.argsort(self.ess, kind="stable")              # (NaN sorts last)
        return [(self.names[i], float(self.ess[i]), float(self.rhat[i]), float(self.mcse_mean[i]), int(self.flag[i]))
                for i in self._order[:max(int(k), 0)]]

    def summary(self, rhat_threshold=1.01, ess_threshold=200.0):
        """Counts of columns with rhat above and ess below the thresholds, and the minimum, median and maximum ESS over
        the columns that vary (constant and non-finite columns are counted on their own)."""
        varying = (self.flag & (FLAG_CONSTANT | FLAG_NONFINITE)) == 0
        ess = self.ess[varying]
        some = ess.size > 0
        return {"n_columns": int(self.ess.size), "n_chains": self.n_chains, "n_draws": self.n_draws,
                "n_constant": int(np.count_nonzero(self.flag & FLAG_CONSTANT)),
                "n_nonfinite": int(np.count_nonzero(self.flag & FLAG_NONFINITE)),
                "n_truncated": int(np.count_nonzero(self.flag & FLAG_TRUNCATED)),
                "n_rhat_above": int(np.count_nonzero(self.rhat[varying] > rhat_threshold)),
                "n_ess_below": int(np.count_nonzero(ess < ess_threshold)),
                "rhat_threshold": float(rhat_threshold), "ess_threshold": float(ess_threshold),
                "ess_min": float(ess.min()) if some else float("nan"),
                "ess_median": float(np.median(ess)) if some else float("nan"),
                "ess_max": float(ess.max()) if some else float("nan")}


# ---- validation (host side, before any library call) -----------------------------------------------------------
def _plan(rows_per_chain, burnin, split):
    """(burn rows per chain, rows cut from the end per chain, M, n) for chains of these lengths."""
    burnin = float(burnin)
    if not 0.0 <= burnin < 1.0:
        raise ValueError(f"burnin={burnin} must lie in [0, 1)")
    m = len(rows_per_chain)
    if not 1 <= m <= MAX_CHAINS:
        raise ValueError(f"{m} chains; the diagnostics take 1 .. {MAX_CHAINS}")
    burn = [int(burnin * int(s)) for s in rows_per_chain]                  # Results.drop_burnin
    left = [int(s) - b for s, b in zip(rows_per_chain, burn)]
    common = min(left)
    n = common // 2 if split else common
    m_split = 2 * m if split else m
    if n < MIN_DRAWS:
        raise ValueError(f"{n} draws per chain after burn-in{' and split' if split else ''}; at least {MIN_DRAWS} are needed")
    if m_split * n > MAX_DRAWS:
        raise ValueError(f"{m_split} chains x {n} draws after burn-in{' and split' if split else ''} exceed {MAX_DRAWS} (2^20) "
                         "draws per column")
    return burn, tuple(v - common for v in left), m_split, n


def _check_max_lag(max_lag):
    max_lag = int(max_lag)
    if not 0 <= max_lag < 2 ** 31:
        raise ValueError(f"max_lag={max_lag} must lie in [0, 2^31) (0: none)")
    return max_lag


def _check_rows(rows, n_columns=None):
    a = np.asarray(rows)
    if a.dtype.kind not in "fiub":
        raise TypeError(f"rows must be numeric, got {a.dtype}")
    if a.ndim == 1 and n_columns is not None:
        a = a.reshape(1, -1)
    if a.ndim != 2 or a.shape[1] < 1:
        raise ValueError(f"rows must be [n_samples, n_columns] with at least one column, got shape {a.shape}")
    if n_columns is not None and a.shape[1] != n_columns:
        raise ValueError(f"rows have {a.shape[1]} columns, the store has {n_columns}")
    return np.ascontiguousarray(a, dtype=np.float64)


def _check_chains(chains):
    if isinstance(chains, np.ndarray):
        if chains.ndim != 3:
            raise ValueError(f"chains must be [M, S, P] or a list of [S_r, P] arrays, got shape {chains.shape}")
        chains = list(chains)
    chains = list(chains)
    if not 1 <= len(chains) <= MAX_CHAINS:
        raise ValueError(f"{len(chains)} chains; the diagnostics take 1 .. {MAX_CHAINS}")
    shapes = [np.shape(c) for c in chains]
    if any(len(s) != 2 for s in shapes):
        raise ValueError(f"every chain must be [S_r, P], got shapes {shapes}")
    if len({s[1] for s in shapes}) != 1:
        raise ValueError(f"the chains have unequal column counts: {[s[1] for s in shapes]}")
    if not 1 <= shapes[0][1] <= MAX_COLUMNS:
        raise ValueError(f"{shapes[0][1]} columns; the diagnostics take 1 .. {MAX_COLUMNS}")
    return chains, [s[0] for s in shapes], shapes[0][1]


def _check_names(names, p):
    if names is None:
        return [f"c{i}" for i in range(p)]
    names = [str(v) for v in names]
    if len(names) != p:
        raise ValueError(f"{len(names)} names for {p} columns")
    return names


_warned_cut = False


def _warn_cut(cut):
    global _warned_cut
    if any(cut) and not _warned_cut:
        _warned_cut = True
        warnings.warn(f"the chains differ in length after burn-in; rows cut from the end per chain: {list(cut)} "
                      "(reported as DiagResult.cut; this warning is given once)", stacklevel=3)


class ColumnStoreHandle(_handle.RowStoreHandle):
    """Owner of a handle with the float64 store of several chains on one device (DiagHandle, SummaryHandle), for callers
    who append rows as they are logged.  A subclass says who takes the chains in the messages (_takes) and gives its
    module's load()."""
    _lane, _takes = "chain", "the diagnostics take"
    _load = staticmethod(load)

    def __init__(self, device=None):
        self.n_chains = self.n_columns = self.capacity = 0
        self._create_on(self._load, device)

    def reset(self, n_chains, n_columns, capacity):
        """Shape the store: n_chains empty chains of up to `capacity` rows of n_columns values."""
        n_chains, n_columns, capacity = int(n_chains), int(n_columns), int(capacity)
        if not 1 <= n_chains <= MAX_CHAINS:
            raise ValueError(f"{n_chains} chains; {self._takes} 1 .. {MAX_CHAINS}")
        if not 1 <= n_columns <= MAX_COLUMNS:
            raise ValueError(f"{n_columns} columns; {self._takes} 1 .. {MAX_COLUMNS}")
        if capacity < 1:
            raise ValueError(f"capacity={capacity} must be positive")
        self.n_chains = self.n_columns = self.capacity = 0
        self._check(self._fn("reset")(self._h, n_chains, n_columns, capacity))
        self.n_chains, self.n_columns, self.capacity = n_chains, n_columns, capacity

    def _lane_count(self):
        return self.n_chains

    def append(self, chain, rows):
        """Append rows ([n, n_columns], or one row [n_columns]) to a chain."""
        chain = self._check_lane(chain)
        block = _check_rows(rows, self.n_columns)
        self._check(self._append_rows(chain, block))

    def set_launch_columns(self, columns):
        """Columns per launch of the handle's first kernel (0: the default): the column kernel of the diagnostics, the rank
        kernel of the summary (whose default comes from the scratch budget).  Results do not depend on it."""
        self._check(self._fn("set_launch_columns")(self._h, int(columns)))


class DiagHandle(ColumnStoreHandle):
    """Owner of one sbe_diag handle: the float64 store of several chains on one device, for callers who append rows as
    they are logged.  last_kernel_ms(): the column kernel of the last compute call."""
    _prefix, _noun = "sbe_diag", "a diagnostics handle"

    def last_shape(self):
        """(M, n, path, launches) of the last compute call."""
        m, n, path, launches = ct.c_int(0), ct.c_int64(0), ct.c_int(0), ct.c_int64(0)
        self._check(self._lib.sbe_diag_last_shape(self._h, ct.byref(m), ct.byref(n), ct.byref(path), ct.byref(launches)))
        return m.value, n.value, PATHS[path.value], launches.value

    def compute(self, burnin=0.1, split=True, max_lag=0, names=None) -> DiagResult:
        if not self.n_chains:
            raise ValueError("the store has no shape yet (reset)")
        max_lag = _check_max_lag(max_lag)
        names = _check_names(names, self.n_columns)
        burn, cut, _m, _n = _plan([self.rows(c) for c in range(self.n_chains)], burnin, split)
        _warn_cut(cut)
        p = self.n_columns
        burn_rows = np.asarray(burn, dtype=np.int64)
        mean, sd, ess, rhat, mcse = (np.empty(p, dtype=np.float64) for _ in range(5))
        n_lags, flag = np.empty(p, dtype=np.int32), np.empty(p, dtype=np.uint8)
        self._check(self._lib.sbe_diag_compute(self._h, _ptr(burn_rows), int(bool(split)), max_lag, _ptr(mean), _ptr(sd), _ptr(ess),
                                               _ptr(rhat), _ptr(mcse), _ptr(n_lags), _ptr(flag)))
        m, n, path, launches = self.last_shape()
        return DiagResult(mean, sd, ess, rhat, mcse, n_lags, flag, names, m, n, cut, path, launches, self.last_kernel_ms())


def convergence(chains, burnin=0.1, split=True, max_lag=0, names=None, device=None) -> DiagResult:
    """ESS, split R-hat, mean, sd and mcse_mean of every column of several runs.  chains: a float array [M, S, P] or a list
    of [S_r, P] arrays (runs may differ in length: they are cut to the shortest after burn-in, with a warning)."""
    chains, lengths, p = _check_chains(chains)
    max_lag = _check_max_lag(max_lag)
    names = _check_names(names, p)
    _plan(lengths, burnin, split)                                          # (refuses before the device is touched)
    blocks = [_check_rows(c) for c in chains]
    h = DiagHandle.filled(device, (len(blocks), p, max(lengths)), blocks)
    try:
        return h.compute(burnin=burnin, split=split, max_lag=max_lag, names=names)
    finally:
        h.close()


# ---- the reference's files ------------------------------------------------------------------------------------
def read_stats(path):
    """(names, rows float64 [S, P]) of a tab-separated stats file with a header line, as Results.read_stats reads it:
    the numeric columns only, in file order."""
    path = Path(path)
    with open(path, "r") as f:
        header = f.readline().rstrip("\n").split("\t")
    try:
        rows = np.loadtxt(path, delimiter="\t", skiprows=1, dtype=np.float64, ndmin=2)
        if rows.shape[1] != len(header):
            raise ValueError(f"{path}: {len(header)} column names, {rows.shape[1]} values per line")
        return header, rows
    except ValueError:
        pass
    with open(path, "r") as f:                                             # some column is not numeric: column by column
        cells = [line.rstrip("\n").split("\t") for line in f.readlines()[1:] if line.strip()]
    if any(len(c) != len(header) for c in cells):
        raise ValueError(f"{path}: a line does not have the header's {len(header)} columns")
    names, cols = [], []
    for j, name in enumerate(header):
        try:
            cols.append(np.array([float(c[j]) for c in cells], dtype=np.float64))
            names.append(name)
        except ValueError:
            continue
    return names, (np.stack(cols, axis=1) if cols else np.empty((len(cells), 0)))


def read_clusters(path):
    """(names, rows float64 [S, K * N]) of a clusters file: one line per sample of K tab-separated strings of N
    characters 0 / 1 (ClustersLogger), as indicator columns named a{k}_{object index}."""
    rows, shape = [], None
    with open(path, "r") as f:
        for line in f:
            line = line.strip()
            if not line:
                continue
            parts = line.split("\t")
            if shape is None:
                shape = (len(parts), len(parts[0]))
            if len(parts) != shape[0] or any(len(s) != shape[1] for s in parts):
                raise ValueError(f"{path}: a line does not hold {shape[0]} clusters of {shape[1]} objects")
            bits = np.frombuffer("".join(parts).encode("ascii"), dtype=np.uint8) - ord("0")
            if bits.max(initial=0) > 1:
                raise ValueError(f"{path}: a cluster string holds a character other than 0 and 1")
            rows.append(bits)
    if shape is None:
        raise ValueError(f"{path}: no cluster samples")
    names = [f"a{k}_{i}" for k in range(shape[0]) for i in range(shape[1])]
    return names, np.stack(rows).astype(np.float64)


def _load_runs(stats_paths, cluster_paths):
    """The columns common to all stats files (in the first file's order, without the sample counters), with the
    indicator columns of the runs' cluster files behind them."""
    tables = [read_stats(p) for p in stats_paths]
    common = [n for n in tables[0][0] if n not in INDEX_COLUMNS and all(n in t[0] for t in tables[1:])]
    if not common:
        raise ValueError("the stats files have no parameter column in common")
    runs = []
    for names, rows in tables:
        index = {n: j for j, n in enumerate(names)}
        runs.append(rows[:, [index[n] for n in common]])
    names = list(common)
    if cluster_paths:
        if len(cluster_paths) != len(stats_paths):
            raise ValueError(f"{len(cluster_paths)} cluster files for {len(stats_paths)} stats files")
        clusters = [read_clusters(p) for p in cluster_paths]
        if len({tuple(c[0]) for c in clusters}) != 1:
            raise ValueError("the cluster files differ in the number of clusters or objects")
        for r, (_cn, crows) in enumerate(clusters):
            if crows.shape[0] != runs[r].shape[0]:
                raise ValueError(f"run {r}: {runs[r].shape[0]} stats rows, {crows.shape[0]} cluster samples")
            runs[r] = np.concatenate([runs[r], crows], axis=1)
        names += clusters[0][0]
    return names, runs


def write_table(path, res: DiagResult):
    with open(path, "w") as f:
        f.write("column\tmean\tsd\tess\trhat\tmcse_mean\tn_lags\tflag\n")
        for i, name in enumerate(res.names):
            f.write(f"{name}\t{res.mean[i]:.10g}\t{res.sd[i]:.10g}\t{res.ess[i]:.10g}\t{res.rhat[i]:.10g}\t{res.mcse_mean[i]:.10g}\t"
                    f"{int(res.n_lags[i])}\t{int(res.flag[i])}\n")


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m sbayes_amd.diag", description="ESS and split R-hat of every column of several sBayes runs")
    ap.add_argument("stats", nargs="+", help="stats_K*_*.txt files, one per run")
    ap.add_argument("--clusters", nargs="*", default=[], help="clusters_K*_*.txt files, one per run, in the same order")
    ap.add_argument("--burnin", type=float, default=0.1)
    ap.add_argument("--no-split", action="store_true")
    ap.add_argument("--max-lag", type=int, default=0)
    ap.add_argument("--top", type=int, default=20)
    ap.add_argument("--out", default=None, help="write the full table (tab-separated) here")
    ap.add_argument("--device", type=int, default=None)
    args = ap.parse_args(argv)
    names, runs = _load_runs(args.stats, args.clusters)
    res = convergence(runs, burnin=args.burnin, split=not args.no_split, max_lag=args.max_lag, names=names, device=args.device)
    s = res.summary()
    print(f"{s['n_columns']} columns, {len(runs)} runs -> {s['n_chains']} chains x {s['n_draws']} draws "
          f"({res.path} path, kernel {res.kernel_ms:.3f} ms)")
    if any(res.cut):
        print(f"rows cut from the end per run: {list(res.cut)}")
    print(f"constant {s['n_constant']}, non-finite {s['n_nonfinite']}, truncated {s['n_truncated']}")
    print(f"rhat > {s['rhat_threshold']:g}: {s['n_rhat_above']} columns; ess < {s['ess_threshold']:g}: {s['n_ess_below']} columns")
    print(f"ess min {s['ess_min']:.1f}  median {s['ess_median']:.1f}  max {s['ess_max']:.1f}")
    print(f"{'column':40s} {'ess':>10s} {'rhat':>8s} {'mcse_mean':>12s} flag")
    for name, ess, rhat, mcse, flag in res.worst(args.top):
        print(f"{name:40s} {ess:10.1f} {rhat:8.4f} {mcse:12.4g} {flag}")
    if args.out:
        write_table(args.out, res)
        print(f"wrote {args.out}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
