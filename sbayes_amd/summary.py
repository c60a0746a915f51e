"""The posterior summary table on the device: quantiles, the highest-density interval (HDI), the rank-normalised R-hat and the
bulk and tail effective sample sizes per column, beside the diagnostics of sbayes_amd.diag (include/sbe_summary.h).

The figures people report for weights and effects -- the `arviz.summary` set -- need every column sorted: a stats file has
thousands to hundreds of thousands of columns, and the rank-normalised figures of Vehtari et al. 2021 catch what the
classic R-hat misses (heavy-tailed columns, chains that agree in location but not in scale, 0/1 indicators).  One workgroup
per column sorts, ranks and normalises; the column kernel of the diagnostics then runs on the derived columns:

    res = summarize([run0, run1, run2], burnin=0.1)      # each run: float [S_r, P]
    res.quantiles, res.hdi_lo, res.hdi_hi, res.ess_bulk, res.ess_tail, res.rhat_rank; res.table()
    h = SummaryHandle(); h.reset(2, P, capacity=1000)     # for callers who append rows as they are logged
    h.append(0, rows); h.append(1, rows); h.compute(burnin=0.1)
    python -m sbayes_amd.summary stats_K3_0.txt stats_K3_1.txt --clusters clusters_K3_0.txt clusters_K3_1.txt --out summary.tsv

Numerical contract (tests/_summary_oracle.py restates it in NumPy; DESIGN.md section 18 states it): burn-in, cut and split
as in sbayes_amd.diag; over the N = M n draws of a column that remain (x + 0.0, so a -0 never reaches an output; s their
ascending sort): the quantile at p is s[k] + (s[min(k + 1, N - 1)] - s[k]) g with h = (N - 1) p, k = floor(h), g = h - k;
the HDI is (s[i], s[i + inc]) at the lowest i of least width, inc = floor(hdi_prob N) clipped to [1, N - 1]; ranks are
average ranks and z = ndtri((r - 0.375) / (N + 0.25)); ess_bulk = ess(z(x)), ess_tail = min over the indicators
[x <= q(0.05)] and [x <= q(0.95)] of their ess, rhat_rank = the larger of rhat(z(x)) and rhat(z(|x - q(0.5)|)).  mean, sd,
ess, rhat, mcse_mean and n_lags are those of diag.convergence, bit for bit.  A column with a non-finite value gets flag 2
and NaN everywhere; a constant column flag 1, its quantiles and HDI, rhat_rank = NaN and ess_bulk = ess_tail = N.  A column
constant within every chain while the chains differ (W = 0) is ranked without the normalisation (its derived z columns hold
2 r, exact integers): rhat_rank = +inf, exactly, as rhat is.  Limits:
those of the diagnostics, and at most 8 probabilities.

There is no CPU fallback: without the library or a GPU the functions raise.  Handles follow the package's process model
(sbayes_amd/_proc.py): never pickled, forgotten (not destroyed) in a fork()ed child."""
from __future__ import annotations

import ctypes as ct
from dataclasses import dataclass

import numpy as np

from . import _handle, diag
from ._handle import _ptr, c_handle_p
from ._samples import write_tsv
from .diag import (FLAG_CONSTANT, FLAG_NONFINITE, FLAG_TRUNCATED, MAX_CHAINS, MAX_COLUMNS, MAX_DRAWS, MIN_DRAWS, PATHS,  # noqa: F401
                   read_clusters, read_stats)

ABI_VERSION = 1                          # SBE_SUMMARY_ABI_VERSION of include/sbe_summary.h
MAX_PROBS = 8                            # SBE_SUMMARY_MAX_PROBS
DERIVED = {"zb": 0, "zf": 1, "i05": 2, "i95": 3, "rank": 4}      # SBE_SUMMARY_DERIVED_*
DEFAULT_PROBS = (0.05, 0.5, 0.95)
DEFAULT_HDI_PROB = 0.94

# name -> (restype, argtypes); mirrors include/sbe_summary.h one to one
PROTOTYPES = {
    **_handle.store_prototypes("sbe_summary", [ct.c_int64, ct.c_int64]),    # (last_kernel_ms fills float [2]: rank kernel, column passes)
    "sbe_summary_set_launch_columns": (ct.c_int, [c_handle_p, ct.c_int64]),
    "sbe_summary_compute": (ct.c_int, [c_handle_p, ct.c_void_p, ct.c_int, ct.c_int64, ct.c_int, ct.c_void_p, ct.c_double] + [ct.c_void_p] * 13),
    "sbe_summary_last_shape": (ct.c_int, [c_handle_p, ct.POINTER(ct.c_int), ct.POINTER(ct.c_int64), ct.POINTER(ct.c_int),
                                          ct.POINTER(ct.c_int64), ct.POINTER(ct.c_int64)]),
    "sbe_summary_derived_column": (ct.c_int, [c_handle_p, ct.c_int64, ct.c_int, ct.c_void_p]),
}


def load():
    """The engine library with the prototypes of include/sbe_summary.h attached."""
    return _handle.bind("sbe_summary", PROTOTYPES, ABI_VERSION)


lds_max_draws = diag.lds_max_draws       # both kernels change path there


@dataclass
class SummaryResult:
    """Per column: quantiles (float64 [len(probs), P]), hdi_lo, hdi_hi, ess_bulk, ess_tail, rhat_rank, and what
    diag.DiagResult holds: mean, sd, ess, rhat, mcse_mean (float64), n_lags (int32), flag (uint8: 1 constant, 2 non-finite,
    4 truncated by max_lag in any of the five passes).  n_chains and n_draws are M and n after the split; cut[r] rows were
    dropped from the end of run r.  rank_ms and column_ms: device time of the rank kernel and of the column passes."""
    probs: tuple
    hdi_prob: float
    quantiles: np.ndarray
    hdi_lo: np.ndarray
    hdi_hi: np.ndarray
    ess_bulk: np.ndarray
    ess_tail: np.ndarray
    rhat_rank: np.ndarray
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
    launch_columns: int = 0
    rank_ms: float = 0.0
    column_ms: float = 0.0

    def header(self):
        return (["column", "mean", "sd", f"hdi_{_pct(0.5 - self.hdi_prob / 2)}", f"hdi_{_pct(0.5 + self.hdi_prob / 2)}"]
                + [f"q{_pct(p)}" for p in self.probs] + ["mcse_mean", "ess", "ess_bulk", "ess_tail", "rhat", "rhat_rank", "n_lags", "flag"])

    def table(self):
        """One row per column, in the order of header(): the name, then floats, then n_lags and flag as ints."""
        rows = []
        for i, name in enumerate(self.names):
            rows.append([name, float(self.mean[i]), float(self.sd[i]), float(self.hdi_lo[i]), float(self.hdi_hi[i])]
                        + [float(q) for q in self.quantiles[:, i]]
                        + [float(self.mcse_mean[i]), float(self.ess[i]), float(self.ess_bulk[i]), float(self.ess_tail[i]),
                           float(self.rhat[i]), float(self.rhat_rank[i]), int(self.n_lags[i]), int(self.flag[i])])
        return rows


def _pct(p):
    return f"{100.0 * p:.10g}%"


# ---- validation (host side, before any library call) -----------------------------------------------------------
def _check_probs(probs):
    probs = tuple(float(p) for p in probs)
    if len(probs) > MAX_PROBS:
        raise ValueError(f"{len(probs)} probabilities; a call takes at most {MAX_PROBS}")
    for p in probs:
        if not 0.0 <= p <= 1.0:
            raise ValueError(f"probability {p} must lie in [0, 1]")
    return probs


def _check_hdi_prob(hdi_prob):
    hdi_prob = float(hdi_prob)
    if not 0.0 < hdi_prob < 1.0:
        raise ValueError(f"hdi_prob={hdi_prob} must lie in (0, 1)")
    return hdi_prob


class SummaryHandle(diag.ColumnStoreHandle):
    """Owner of one sbe_summary handle: the float64 store of several chains on one device, for callers who append rows as
    they are logged.  last_kernel_ms(): the rank kernel and the column passes of the last compute call, added."""
    _prefix, _noun, _takes = "sbe_summary", "a summary handle", "the summary takes"
    _load = staticmethod(load)

    def last_shape(self):
        """(M, n, path, launches of the rank kernel, columns of each) of the last compute call."""
        m, n, path, launches, cols = ct.c_int(0), ct.c_int64(0), ct.c_int(0), ct.c_int64(0), ct.c_int64(0)
        self._check(self._lib.sbe_summary_last_shape(self._h, ct.byref(m), ct.byref(n), ct.byref(path), ct.byref(launches), ct.byref(cols)))
        return m.value, n.value, PATHS[path.value], launches.value, cols.value

    def last_kernel_times(self):
        """(rank kernel ms, column passes ms) of the last compute call (HIP events)."""
        ms = (ct.c_float * 2)()
        self._check(self._lib.sbe_summary_last_kernel_ms(self._h, ms))
        return float(ms[0]), float(ms[1])

    def last_kernel_ms(self) -> float:
        return sum(self.last_kernel_times())

    def compute(self, burnin=0.1, split=True, max_lag=0, probs=DEFAULT_PROBS, hdi_prob=DEFAULT_HDI_PROB, names=None) -> SummaryResult:
        if not self.n_chains:
            raise ValueError("the store has no shape yet (reset)")
        max_lag = diag._check_max_lag(max_lag)
        probs, hdi_prob = _check_probs(probs), _check_hdi_prob(hdi_prob)
        names = diag._check_names(names, self.n_columns)
        burn, cut, _m, _n = diag._plan([self.rows(c) for c in range(self.n_chains)], burnin, split)
        diag._warn_cut(cut)
        p = self.n_columns
        burn_rows = np.asarray(burn, dtype=np.int64)
        prob_arr = np.asarray(probs, dtype=np.float64).reshape(len(probs))
        quantiles = np.empty((len(probs), p), dtype=np.float64)
        hdi_lo, hdi_hi, ess_bulk, ess_tail, rhat_rank = (np.empty(p, dtype=np.float64) for _ in range(5))
        mean, sd, ess, rhat, mcse = (np.empty(p, dtype=np.float64) for _ in range(5))
        n_lags, flag = np.empty(p, dtype=np.int32), np.empty(p, dtype=np.uint8)
        self._check(self._lib.sbe_summary_compute(self._h, _ptr(burn_rows), int(bool(split)), max_lag, len(probs), _ptr(prob_arr), hdi_prob,
                                                  _ptr(quantiles), _ptr(hdi_lo), _ptr(hdi_hi), _ptr(ess_bulk), _ptr(ess_tail), _ptr(rhat_rank),
                                                  _ptr(mean), _ptr(sd), _ptr(ess), _ptr(rhat), _ptr(mcse), _ptr(n_lags), _ptr(flag)))
        m, n, path, launches, cols = self.last_shape()
        rank_ms, column_ms = self.last_kernel_times()
        return SummaryResult(probs, hdi_prob, quantiles, hdi_lo, hdi_hi, ess_bulk, ess_tail, rhat_rank, mean, sd, ess, rhat, mcse, n_lags,
                             flag, names, m, n, cut, path, launches, cols, rank_ms, column_ms)

    def derived_column(self, column, which):
        """An inspection call: one derived column of the last compute call ("zb", "zf", "i05", "i95" or "rank"), float64
        [M, n] in the order of the chains after the split.  Re-runs the rank kernel for that column."""
        if which not in DERIVED:
            raise ValueError(f"which={which!r} must be one of {sorted(DERIVED)}")
        column = int(column)
        if not 0 <= column < self.n_columns:
            raise ValueError(f"column {column} out of range [0, {self.n_columns})")
        m, n, _path, _launches, _cols = self.last_shape()
        out = np.empty((m, n), dtype=np.float64)
        self._check(self._lib.sbe_summary_derived_column(self._h, column, DERIVED[which], _ptr(out)))
        return out


def summarize(chains, burnin=0.1, split=True, max_lag=0, probs=DEFAULT_PROBS, hdi_prob=DEFAULT_HDI_PROB, names=None,
              device=None) -> SummaryResult:
    """The summary of every column of several runs.  chains: a float array [M, S, P] or a list of [S_r, P] arrays (runs may
    differ in length: they are cut to the shortest after burn-in, with a warning)."""
    chains, lengths, p = diag._check_chains(chains)
    max_lag = diag._check_max_lag(max_lag)
    probs, hdi_prob = _check_probs(probs), _check_hdi_prob(hdi_prob)
    names = diag._check_names(names, p)
    diag._plan(lengths, burnin, split)                                     # (refuses before the device is touched)
    blocks = [diag._check_rows(c) for c in chains]
    h = SummaryHandle.filled(device, (len(blocks), p, max(lengths)), blocks)
    try:
        return h.compute(burnin=burnin, split=split, max_lag=max_lag, probs=probs, hdi_prob=hdi_prob, names=names)
    finally:
        h.close()


def write_table(path, res: SummaryResult):
    write_tsv(path, res.header(), res.table())


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m sbayes_amd.summary",
                                 description="quantiles, HDI, rank R-hat, bulk and tail ESS of every column of several sBayes runs")
    ap.add_argument("stats", nargs="+", help="stats_K*_*.txt files, one per run")
    ap.add_argument("--clusters", nargs="*", default=[], help="clusters_K*_*.txt files, one per run, in the same order")
    ap.add_argument("--burnin", type=float, default=0.1)
    ap.add_argument("--no-split", action="store_true")
    ap.add_argument("--max-lag", type=int, default=0)
    ap.add_argument("--probs", type=float, nargs="*", default=list(DEFAULT_PROBS))
    ap.add_argument("--hdi-prob", type=float, default=DEFAULT_HDI_PROB)
    ap.add_argument("--top", type=int, default=20, help="print the columns of lowest bulk ESS")
    ap.add_argument("--out", default=None, help="write the full table (tab-separated) here")
    ap.add_argument("--device", type=int, default=None)
    args = ap.parse_args(argv)
    names, runs = diag._load_runs(args.stats, args.clusters)
    res = summarize(runs, burnin=args.burnin, split=not args.no_split, max_lag=args.max_lag, probs=args.probs, hdi_prob=args.hdi_prob,
                    names=names, device=args.device)
    print(f"{len(res.names)} columns, {len(runs)} runs -> {res.n_chains} chains x {res.n_draws} draws "
          f"({res.path} path, rank kernel {res.rank_ms:.3f} ms, column passes {res.column_ms:.3f} ms)")
    if any(res.cut):
        print(f"rows cut from the end per run: {list(res.cut)}")
    print(f"constant {int(np.count_nonzero(res.flag & FLAG_CONSTANT))}, non-finite {int(np.count_nonzero(res.flag & FLAG_NONFINITE))}, "
          f"truncated {int(np.count_nonzero(res.flag & FLAG_TRUNCATED))}")
    print(f"{'column':40s} {'ess_bulk':>10s} {'ess_tail':>10s} {'rhat_rank':>10s} flag")
    order = np.argsort(res.ess_bulk, kind="stable")                        # (NaN sorts last)
    for i in order[:max(args.top, 0)]:
        print(f"{res.names[i]:40s} {res.ess_bulk[i]:10.1f} {res.ess_tail[i]:10.1f} {res.rhat_rank[i]:10.4f} {int(res.flag[i])}")
    if args.out:
        write_table(args.out, res)
        print(f"wrote {args.out}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
