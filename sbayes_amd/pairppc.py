"""Pairwise feature dependence checked against the fitted model's replicates, on the device (include/sbe_pairppc.h).

sBayes treats features as independent given their source.  The screening (sbayes_amd/assoc.py) tests that on the raw data, and
flags the pairs that depend on each other because they share a family or an area -- which is what the model is fitted to
explain.  This module asks which pairs are still dependent after clusters and confounders have been accounted for: it takes the
replicated data sets of the posterior predictive check (sbayes_amd/ppc.py, one per logged sample, with the data's missingness),
runs the screening's chi-squared statistic of every pair on the data and on every replicate, and keeps per pair where the
observed statistic falls among the replicated ones:

    res = pairwise_check(codes, groups, clusters, weights, tables, burnin=0.1, seed=0)
    res.p_value() [F,F]   (n_greater + n_equal / 2) / T: the share of replicates whose statistic exceeds the observed one
    res.mean(), res.sd(), res.z()     of the replicated statistic, and (stat_obs - mean) / sd (NaN where sd is 0)
    res.flagged(0.05), res.worst(5), res.table(names), res.write_table(path)
    h = PairHandle(); h.set_data(codes, n_states); h.add(y_rep); h.add(more); h.result()    # h.set_form, h.set_launch_tiles
    python -m sbayes_amd.pairppc FEATURES FEATURE_STATES STATS CLUSTERS --confounders universal family --out pairs.tsv

A small p says that the pair is more dependent in the data than in what the fitted model produces: evidence the model counts
twice.  Read it next to the raw screen's p-value (the command line writes both): a pair that the raw screen flags and this one
does not is dependence the model explains.

What the p-value is not.  It conditions on the logged effect draws and uses the data twice, so it is CONSERVATIVE (DESIGN.md
section 22): under a true model it concentrates around 1/2, and a small one is stronger evidence than its size says.  The
F (F - 1) / 2 pairs are multiple comparisons, and no correction is applied.  Yates' correction (applied at dof 1 only) scales
the statistic of a dof 1 table differently from a dof > 1 one; where a replicate loses a state that the data has, its statistic
is on the other scale (n_degenerate counts the replicates whose table had no degrees of freedom at all; their statistic is 0).

Numerical contract (tests/_pairppc_oracle.py restates it): the statistic is the screening's, bit for bit on
the data; per replicate, in order, and per pair valid on the data exactly one of n_greater, n_equal, n_less grows by comparing the
fp64 values, sum += s and sumsq += s * s (rounded, then added).  No output bit depends on how the replicates are split across
add() calls, on the launch tiles or on the kernel form.  One call holds at most 256 MiB on the device and add() splits longer blocks.  Replicates
are validated on the device before anything changes (EngineError, code SBE_ERR_DATA = 4, naming the first offender).

There is no CPU fallback: without the library or a GPU the functions raise.  Handles follow the package's process model
(sbayes_amd/_proc.py): never pickled, forgotten (not destroyed) in a fork()ed child."""
from __future__ import annotations

import ctypes as ct
from dataclasses import dataclass
from pathlib import Path

import numpy as np

from . import _handle, _samples, assoc, ppc, predict         # noqa: F401 (ppc: the handle of the replicates, made by _samples)
from ._handle import _ptr, c_handle_p

ABI_VERSION = 1                              # SBE_PAIRPPC_ABI_VERSION of include/sbe_pairppc.h
NA = assoc.NA                                # SBE_PAIRPPC_NA
MAX_STAGE_BYTES = predict.MAX_STAGE_BYTES    # SBE_PAIRPPC_MAX_STAGE_BYTES
ROUND = 256                                  # objects the feature-major image is padded to
FORMS = {"auto": 0, "sequential": 1, "spread": 2}     # SBE_PAIRPPC_FORM_*
HELD_BYTES = 32 << 20                        # SBE_PAIRPPC_HELD_BYTES: what the spread form holds on the device beside a call's replicates

# name -> (restype, argtypes); mirrors include/sbe_pairppc.h one to one
PROTOTYPES = {
    **_handle.unit_prototypes("sbe_pairppc"),
    "sbe_pairppc_create": (ct.c_int, [ct.POINTER(c_handle_p), ct.c_int]),
    "sbe_pairppc_set_launch_tiles": (ct.c_int, [c_handle_p, ct.c_int64]),
    "sbe_pairppc_set_form": (ct.c_int, [c_handle_p, ct.c_int]),
    "sbe_pairppc_replicate_bytes": (ct.c_int64, [ct.c_int64, ct.c_int64, ct.c_int]),
    "sbe_pairppc_set_data": (ct.c_int, [c_handle_p, ct.c_void_p, ct.c_int64, ct.c_int64, ct.c_void_p]),
    "sbe_pairppc_add": (ct.c_int, [c_handle_p, ct.c_int64, ct.c_void_p, ct.c_void_p]),
    "sbe_pairppc_read": (ct.c_int, [c_handle_p] + [ct.c_void_p] * 10 + [ct.POINTER(ct.c_int64)]),
    "sbe_pairppc_reset": (ct.c_int, [c_handle_p]),
    "sbe_pairppc_last_shape": (ct.c_int, [c_handle_p, ct.POINTER(ct.c_int32), ct.POINTER(ct.c_int64), ct.POINTER(ct.c_int64)]),
}


def load():
    """The engine library with the prototypes of include/sbe_pairppc.h attached."""
    return _handle.bind("sbe_pairppc", PROTOTYPES, ABI_VERSION)


def replicate_bytes(n_objects, n_features, with_stat_rep=False) -> int:
    """Device bytes one replicate of an add call takes while the call runs (sbe_pairppc_replicate_bytes); 0 beyond the limits."""
    n, f = int(n_objects), int(n_features)
    if not (1 <= n <= assoc.MAX_OBJECTS and 1 <= f <= assoc.MAX_FEATURES and n * f <= assoc.MAX_CODES):
        return 0
    return n * f + f * (-(-n // ROUND) * ROUND) + (8 * f * f if with_stat_rep else 0)


@dataclass
class PairResult:
    """[F, F] each and symmetric; pairs that are not valid on the data, and the diagonal, hold 0 everywhere.  stat_obs, dof_obs,
    n_obs, valid_obs: the screening's statistic, dof, total and validity of the data; n_greater, n_equal, n_less: the replicates
    whose statistic was above, at, below stat_obs; n_degenerate: those whose table had dof 0 (statistic 0); sum, sumsq: of the
    replicated statistics; n_replicates: T; stat_rep: float64 [T, F, F] or None."""
    stat_obs: np.ndarray
    dof_obs: np.ndarray
    n_obs: np.ndarray
    valid_obs: np.ndarray
    n_greater: np.ndarray
    n_equal: np.ndarray
    n_less: np.ndarray
    n_degenerate: np.ndarray
    sum: np.ndarray
    sumsq: np.ndarray
    n_replicates: int
    n_states: np.ndarray = None
    stat_rep: np.ndarray | None = None
    kernel_ms: float = 0.0
    ppc: object = None                       # the PpcResult of the same replicates (pairwise_check)
    raw_pvalue: np.ndarray | None = None     # the raw screen's p-value of the data (the command line fills it)

    def _pairs(self, value):
        return np.where(self.valid_obs, value, np.nan)

    def p_value(self):
        """ppc.p_value's rule per pair: (n_greater + n_equal / 2) / T; NaN for pairs that are not valid on the data."""
        with np.errstate(invalid="ignore", divide="ignore"):
            return self._pairs((self.n_greater + 0.5 * self.n_equal) / self.n_replicates)

    def mean(self):
        with np.errstate(invalid="ignore", divide="ignore"):
            return self._pairs(self.sum / self.n_replicates)

    def sd(self):
        """The standard deviation of the replicated statistic (divisor T)."""
        with np.errstate(invalid="ignore", divide="ignore"):
            m = self.sum / self.n_replicates
            return self._pairs(np.sqrt(np.maximum(self.sumsq / self.n_replicates - m * m, 0.0)))

    def z(self):
        """(stat_obs - mean) / sd; NaN where sd is 0."""
        sd = self.sd()
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(sd > 0, (self.stat_obs - self.mean()) / sd, np.nan)

    def flagged(self, p_threshold=0.05):
        """[(p, i, j)], i < j, of the valid pairs with p_value() < p_threshold, sorted."""
        p = self.p_value()
        i, j = np.nonzero(np.triu(self.valid_obs, 1) & (np.nan_to_num(p, nan=np.inf) < p_threshold))
        return sorted((float(p[a, b]), int(a), int(b)) for a, b in zip(i, j))

    def table(self, names=None):
        """(header, rows) of the pairs i < j that are valid on the data, sorted by the predictive p, then by -z (NaN last)."""
        f = self.stat_obs.shape[0]
        names = list(names) if names is not None else [f"F{i + 1}" for i in range(f)]
        if len(names) != f:
            raise ValueError(f"{len(names)} names for {f} features")
        p, mean, sd, z = self.p_value(), self.mean(), self.sd(), self.z()
        rows = []
        for i, j in zip(*np.nonzero(np.triu(self.valid_obs, 1))):
            raw = float(self.raw_pvalue[i, j]) if self.raw_pvalue is not None else float("nan")
            rows.append([str(names[i]), str(names[j]), int(self.n_obs[i, j]), int(self.dof_obs[i, j]), float(self.stat_obs[i, j]), raw,
                         float(p[i, j]), float(mean[i, j]), float(sd[i, j]), float(z[i, j])])
        rows.sort(key=lambda r: (r[6], -r[9] if r[9] == r[9] else np.inf))
        return ["feature_1", "feature_2", "n", "dof", "statistic", "p_raw", "p_predictive", "mean_replicated", "sd_replicated", "z"], rows

    def worst(self, k=5, names=None):
        """The first k rows of table(names)."""
        return self.table(names)[1][:k]

    def write_table(self, path, names=None):
        _samples.write_tsv(path, *self.table(names))


class PairHandle(_handle.UnitHandle):
    """Owner of one sbe_pairppc handle: the data, its observed statistic and the accumulators on one device.  add() feeds
    replicates; result() reads the accumulators back.  last_kernel_ms(): the pair kernel's launches of the last library call."""
    _prefix, _noun = "sbe_pairppc", "a pairwise check handle"

    def __init__(self, device=None):
        self.shape = None                                    # (N, F) once the data is set
        self.n_states = None
        self._stat_rep = []
        self.kernel_ms = 0.0
        self._create_on(load, device)

    def set_data(self, codes, n_states=None):
        """codes uint8 [N, F] (255 = NA) or one-hot bool [N, F, S]; n_states: states per feature (default: one more than the largest
        code that occurs).  Computes the observed statistic and clears the accumulators."""
        x, ns = assoc._check_inputs(codes, n_states)
        n, f = x.shape
        self.shape = None
        self._check(self._lib.sbe_pairppc_set_data(self._h, _ptr(x), n, f, _ptr(ns)))
        self.shape, self.n_states = (n, f), ns
        self._stat_rep, self.kernel_ms = [], self.last_kernel_ms()

    def _with_data(self):
        if self.shape is None:
            raise ValueError("no data yet (set_data)")
        return self.shape

    def reset(self):
        """Clear the accumulators, keep the data."""
        self._with_data()
        self._check(self._lib.sbe_pairppc_reset(self._h))
        self._stat_rep, self.kernel_ms = [], 0.0

    def set_launch_tiles(self, tile_pairs):
        """Tile pairs per launch of the pair kernels (0: the default).  Results do not depend on it."""
        self._check(self._lib.sbe_pairppc_set_launch_tiles(self._h, int(tile_pairs)))

    def set_form(self, form):
        """The form of the replicate kernel: "auto" (the default: picked so that the device is filled), "sequential" (a wave per
        tile pair walks the replicates) or "spread" (the replicates dealt out over waves, HELD_BYTES more on the device).
        Results do not depend on it."""
        if form not in FORMS:
            raise ValueError(f"form={form!r} is none of {sorted(FORMS)}")
        self._check(self._lib.sbe_pairppc_set_form(self._h, FORMS[form]))

    def max_replicates(self, stat_rep=False) -> int:
        """The replicates one library call holds."""
        n, f = self._with_data()
        return MAX_STAGE_BYTES // replicate_bytes(n, f, stat_rep)

    def last_shape(self):
        """(S_pad, tile pairs, launches) of the last set_data or add call of the library."""
        s_pad, tiles, launches = ct.c_int32(0), ct.c_int64(0), ct.c_int64(0)
        self._check(self._lib.sbe_pairppc_last_shape(self._h, ct.byref(s_pad), ct.byref(tiles), ct.byref(launches)))
        return s_pad.value, tiles.value, launches.value

    def add(self, y_rep, stat_rep=False):
        """Replicates uint8 [n, N, F], each code below n_states[f] or 255.  stat_rep: keep (and return) the statistics
        float64 [n, F, F].  Blocks beyond max_replicates() go in several library calls; each call validates its replicates before
        it changes anything, so an EngineError leaves the replicates of the calls before it added."""
        n_obj, f = self._with_data()
        y = _samples.check_replicates(y_rep, n_obj, f)
        step = self.max_replicates(stat_rep)
        if step < 1:
            raise ValueError(f"one replicate takes {replicate_bytes(n_obj, f, stat_rep)} bytes on the device, a call holds {MAX_STAGE_BYTES}")
        y = np.ascontiguousarray(y)
        self.kernel_ms = 0.0
        kept = []
        for r0 in range(0, y.shape[0], step):
            block = y[r0:r0 + step]
            out = np.empty((block.shape[0], f, f), dtype=np.float64) if stat_rep else None
            self._check(self._lib.sbe_pairppc_add(self._h, block.shape[0], _ptr(block), _ptr(out) if stat_rep else None))
            self.kernel_ms += self.last_kernel_ms()
            if stat_rep:
                kept.append(out)
        self._stat_rep.append(np.concatenate(kept) if kept else None)
        return self._stat_rep[-1]

    def result(self) -> PairResult:
        _n, f = self._with_data()
        stat, s1, s2 = (np.empty((f, f), dtype=np.float64) for _ in range(3))
        dof, n, gt, eq, lt, deg = (np.empty((f, f), dtype=np.int32) for _ in range(6))
        valid = np.empty((f, f), dtype=np.uint8)
        count = ct.c_int64(0)
        self._check(self._lib.sbe_pairppc_read(self._h, _ptr(stat), _ptr(dof), _ptr(n), _ptr(valid), _ptr(gt), _ptr(eq), _ptr(lt), _ptr(deg),
                                               _ptr(s1), _ptr(s2), ct.byref(count)))
        kept = self._stat_rep
        return PairResult(stat, dof, n, valid.view(np.bool_), gt, eq, lt, deg, s1, s2, count.value, self.n_states,
                          np.concatenate(kept) if kept and all(k is not None for k in kept) else None, self.kernel_ms)


def pairwise_check(codes, groups, clusters, weights, tables, n_states=None, burnin=0.1, seed=0, n_groups=None, uniforms=None,
                   device=None) -> PairResult:
    """The pairwise check of T logged samples after burn-in: the samples, seed and draw indices are posterior_predictive_check's
    (sbayes_amd/ppc.py), so the pairwise p-values belong to the same replicates as its per-feature ones (res.ppc holds that
    result, without y_rep).  n_states: states per feature (default: the tables' S for every feature -- a replicate may draw a state
    the data never shows).  The replicates pass through host memory, block by block."""
    groups, n_groups, clusters, weights, tables, uniforms = _samples.after_burnin(groups, clusters, weights, tables, burnin, n_groups, uniforms)
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    if n_states is None:
        n_states = np.full(codes.shape[1] if codes.ndim == 2 else 0, tables.shape[3], dtype=np.int32)

    def fill(h):
        h.set_data(codes, n_states)
        return h.max_replicates(), h.add
    return _samples.check_with_replicates(PairHandle, fill, codes, groups, n_groups, clusters, weights, tables, seed, uniforms, device)


def main(argv=None):
    ap = _samples.run_parser("python -m sbayes_amd.pairppc",
                             "Pairwise dependence of an sBayes run's features checked against the fitted model: the chi-squared "
                             "statistic of every pair on the data among the same statistic on one replicated data set per logged "
                             "sample (conservative: given the logged effect draws; no correction for the many pairs)", seed=True)
    ap.add_argument("--out", type=Path, default=Path("pairs.tsv"), help="the table of the pairs (default: pairs.tsv)")
    ap.add_argument("-p", "--pThreshold", type=float, default=0.05, help="the predictive p below which a pair is counted as flagged")
    args = ap.parse_args(argv)
    data, clusters, weights, tables, n_groups = _samples.read_run(args)
    n_states = np.array([max(1, len(s)) for s in data["state_names"]], dtype=np.int32)
    res = pairwise_check(data["codes"], data["groups"], clusters, weights, tables, n_states=n_states, burnin=args.burnin, seed=args.seed,
                         n_groups=n_groups, device=args.device)
    res.raw_pvalue = assoc.feature_association(data["codes"], n_states, device=args.device if args.device is not None else 0).pvalue
    pairs = int(np.triu(res.valid_obs, 1).sum())
    print(f"{res.n_replicates} replicates, {pairs} pairs valid on the data, {len(res.flagged(args.pThreshold))} with predictive p < {args.pThreshold:g} "
          f"(conservative: given the logged effect draws; {pairs} comparisons, uncorrected)")
    print("the five pairs with the smallest predictive p:")
    for a, b, _n, dof, stat, raw, p, mean, sd, z in res.worst(5, data["feature_names"]):
        print(f"  {a}\t{b}\tdof {dof}\tstatistic {stat:.4f}\tp raw {raw:.4g}\tp predictive {p:.4f}\treplicated {mean:.4f} +- {sd:.4f}\tz {z:.3f}")
    res.write_table(args.out, data["feature_names"])
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
