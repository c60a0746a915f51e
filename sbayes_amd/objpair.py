"""Every pair of objects checked against the fitted model's replicates, on the device (include/sbe_objpair.h): do these two objects
agree on more features than the fitted model reproduces?

sBayes exists to find objects that share more features than their confounders explain.  The other checks of a fitted run
aggregate: ppc per feature and per object, pairppc per pair of features, spatial per class of object pairs.  This one keeps the
pair of objects itself.  It counts, for every pair, the features on which both are observed and show the same state, on the data
and on the replicated data sets of the posterior predictive check (sbayes_amd/ppc.py, one per logged sample), and keeps per
pair where the observed count falls among the replicated ones:

    res = object_pair_check(codes, groups, clusters, weights, tables, burnin=0.1, seed=0)
    res.observed, res.comparable [N,N]     the features on which a pair agrees, and on which both are observed
    res.p_value() [N,N]   (n_greater + n_equal / 2) / T: the share of replicates in which the pair agrees more often than in the data
    res.mean(), res.sd(), res.z(), res.excess() = observed - mean
    res.flagged(0.05), res.worst(5, names), res.object_table(names), res.write_tables(pairs_tsv, objects_tsv)
    h = ObjPairHandle(); h.set_data(codes, n_states); h.add(y_rep); h.add(more); h.result()      # h.set_launch_tiles, h.reset
    python -m sbayes_amd.objpair FEATURES FEATURE_STATES STATS CLUSTERS --confounders universal family

A small p says that the two objects agree more often in the data than in what the fitted model produces: similarity it has not
explained -- a missed contact area, a K that is too small, a missing family.  The objects' table says where such pairs gather.

What the p-value is not.  It conditions on the logged effect draws and uses the data twice, so it is CONSERVATIVE (DESIGN.md
section 22): under a true model it concentrates around 1/2, and a small one is stronger evidence than its size says.  The
N (N - 1) / 2 pairs are multiple comparisons and they are DEPENDENT -- every object is in N - 1 of them -- and no correction is
applied.

Numerical contract (tests/_objpair_oracle.py restates it): every quantity is an integer and equals the
checker's.  No output depends on how the replicates are split across add() calls, on the launch tiles or on agree_rep.  One
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

ABI_VERSION = 1                              # SBE_OBJPAIR_ABI_VERSION of include/sbe_objpair.h
NA = 255                                     # SBE_OBJPAIR_NA
MAX_OBJECTS, MAX_FEATURES = 4096, 4096       # SBE_OBJPAIR_MAX_OBJECTS, _FEATURES
MAX_STATES = predict.MAX_STATES              # SBE_OBJPAIR_MAX_STATES: every replicate of the posterior predictive check is accepted
MAX_STAGE_BYTES = predict.MAX_STAGE_BYTES    # SBE_OBJPAIR_MAX_STAGE_BYTES
ROUND, TILE = 256, 32                        # SBE_OBJPAIR_ROUND; the objects of a tile

# name -> (restype, argtypes); mirrors include/sbe_objpair.h one to one
PROTOTYPES = {
    **_handle.unit_prototypes("sbe_objpair"),
    "sbe_objpair_create": (ct.c_int, [ct.POINTER(c_handle_p), ct.c_int]),
    "sbe_objpair_set_launch_tiles": (ct.c_int, [c_handle_p, ct.c_int64]),
    "sbe_objpair_max_replicates": (ct.c_int64, [ct.c_int64, ct.c_int64]),
    "sbe_objpair_replicate_bytes": (ct.c_int64, [ct.c_int64, ct.c_int64, ct.c_int64, ct.c_int]),
    "sbe_objpair_set_data": (ct.c_int, [c_handle_p, ct.c_void_p, ct.c_int64, ct.c_int64, ct.c_void_p]),
    "sbe_objpair_add": (ct.c_int, [c_handle_p, ct.c_int64, ct.c_void_p, ct.c_void_p]),
    "sbe_objpair_read": (ct.c_int, [c_handle_p] + [ct.c_void_p] * 7 + [ct.POINTER(ct.c_int64)]),
    "sbe_objpair_reset": (ct.c_int, [c_handle_p]),
    "sbe_objpair_last_shape": (ct.c_int, [c_handle_p, ct.POINTER(ct.c_int64), ct.POINTER(ct.c_int64), ct.POINTER(ct.c_int64)]),
}


def load():
    """The engine library with the prototypes of include/sbe_objpair.h attached."""
    return _handle.bind("sbe_objpair", PROTOTYPES, ABI_VERSION)


def _in_limits(n, f):
    return 1 <= n <= MAX_OBJECTS and 1 <= f <= MAX_FEATURES


def max_replicates(n_objects, n_features) -> int:
    """The replicates a handle of this shape accumulates (sbe_objpair_max_replicates): the int32 counts hold 2^31 - 1; 0 beyond the
    limits."""
    return 2 ** 31 - 1 if _in_limits(int(n_objects), int(n_features)) else 0


def replicate_bytes(n_objects, n_features, n_elements, with_agree_rep=False) -> int:
    """Device bytes one replicate of an add call takes while the call runs (sbe_objpair_replicate_bytes), n_elements the sum of
    the state counts; 0 beyond the limits."""
    n, f, e = int(n_objects), int(n_features), int(n_elements)
    if not (_in_limits(n, f) and f <= e <= MAX_STATES * f):
        return 0
    return n * f + (-(-n // TILE) * TILE) * (-(-e // ROUND) * ROUND) // 2 + (4 * n * n if with_agree_rep else 0)


def _names(names, n):
    names = [str(v) for v in names] if names is not None else [f"O{i + 1}" for i in range(n)]
    if len(names) != n:
        raise ValueError(f"{len(names)} names for {n} objects")
    return names


@dataclass
class ObjPairResult:
    """[N, N] each, symmetric, the diagonal 0.  observed, comparable (int32): the features on which a pair agrees in the data, and
    on which both objects are observed; n_greater, n_equal, n_less (int32): the replicates in which the pair agreed on more, as
    many, fewer features than in the data; sum, sumsq (int64): of the replicated counts; n_replicates: T; agree_rep: int32
    [T, N, N] or None."""
    observed: np.ndarray
    comparable: np.ndarray
    n_greater: np.ndarray
    n_equal: np.ndarray
    n_less: np.ndarray
    sum: np.ndarray
    sumsq: np.ndarray
    n_replicates: int
    n_states: np.ndarray = None
    agree_rep: np.ndarray | None = None
    kernel_ms: float = 0.0
    ppc: object = None                       # the PpcResult of the same replicates (object_pair_check)

    def _off_diagonal(self, value):
        return np.where(np.eye(self.observed.shape[0], dtype=bool), np.nan, value)

    def p_value(self):
        """The upper-tail p-value (n_greater + n_equal / 2) / T, ties counting half as in ppc: small where the pair agrees more
        often in the data than in the replicates.  NaN on the diagonal."""
        with np.errstate(invalid="ignore", divide="ignore"):
            return self._off_diagonal((self.n_greater + 0.5 * self.n_equal) / self.n_replicates)

    def mean(self):
        """Of the replicated counts."""
        with np.errstate(invalid="ignore", divide="ignore"):
            return self.sum / self.n_replicates

    def sd(self):
        """The standard deviation of the replicated counts (divisor T), from the exact integer sums, so nothing cancels: T sumsq - sum^2
        in int64 below 2^19 replicates (sumsq <= T 2^24, so T sumsq < 2^62), in Python integers beyond."""
        t = self.n_replicates
        if t == 0:
            return np.full(self.sum.shape, np.nan)
        if t < 2 ** 19:                                          # t * sumsq <= t^2 2^24 < 2^62
            var = t * self.sumsq - self.sum * self.sum
        else:
            var = np.asarray(t * self.sumsq.astype(object) - self.sum.astype(object) ** 2, dtype=object)
        return np.sqrt(var.astype(np.float64)) / t

    def excess(self):
        """observed - mean: the features a pair shares beyond what the fitted model reproduces."""
        return self.observed - self.mean()

    def z(self):
        """(observed - mean) / sd; NaN where sd is 0."""
        sd = self.sd()
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(sd > 0, self.excess() / sd, np.nan)

    def flagged(self, p_threshold=0.05):
        """[(p, i, j)], i < j, of the pairs with p_value() < p_threshold, sorted."""
        p = self.p_value()
        i, j = np.nonzero(np.triu(np.nan_to_num(p, nan=np.inf) < p_threshold, 1))
        return sorted((float(p[a, b]), int(a), int(b)) for a, b in zip(i, j))

    HEADER = ["object_1", "object_2", "agree", "comparable", "share", "p_predictive", "mean_replicated", "sd_replicated", "excess", "z"]

    def _rows(self, pairs, names):
        names = _names(names, self.observed.shape[0])
        p, mean, sd, z = self.p_value(), self.mean(), self.sd(), self.z()
        rows = []
        for i, j in pairs:
            cmp = int(self.comparable[i, j])
            rows.append([names[i], names[j], int(self.observed[i, j]), cmp, int(self.observed[i, j]) / cmp if cmp else float("nan"), float(p[i, j]),
                         float(mean[i, j]), float(sd[i, j]), float(self.observed[i, j] - mean[i, j]), float(z[i, j])])
        rows.sort(key=lambda r: (r[5] if r[5] == r[5] else np.inf, -r[8] if r[8] == r[8] else np.inf))
        return rows

    def worst(self, k=5, names=None):
        """The k pairs i < j with the smallest p-value, then the largest excess: rows of HEADER.  Only the k are formatted (the
        N (N - 1) / 2 pairs are never all written out)."""
        n = self.observed.shape[0]
        iu, ju = np.triu_indices(n, 1)
        k = min(int(k), iu.size)
        if k <= 0:
            return []
        p = np.nan_to_num(self.p_value()[iu, ju], nan=np.inf)
        order = np.lexsort((-self.excess()[iu, ju], p))[:k]
        return self._rows([(int(iu[q]), int(ju[q])) for q in order], names)

    def pair_table(self, names=None, p_threshold=0.05, top=None):
        """(header, rows): the `top` worst pairs, or (top None) the pairs flagged at p_threshold."""
        if top is not None:
            return self.HEADER, self.worst(top, names)
        return self.HEADER, self._rows([(i, j) for _p, i, j in self.flagged(p_threshold)], names)

    def object_table(self, names=None, p_threshold=0.05):
        """(header, rows) per object: the partners with which it is flagged at p_threshold, its largest excess and that partner,
        and the sum of its excesses over all partners; sorted by the flagged partners, then by the sum."""
        n = self.observed.shape[0]
        names = _names(names, n)
        with np.errstate(invalid="ignore"):
            hit = np.nan_to_num(self.p_value(), nan=np.inf) < p_threshold
        excess = self._off_diagonal(self.excess())
        rows = []
        for i in range(n):
            if n > 1 and self.n_replicates:
                best = int(np.nanargmax(excess[i]))
                rows.append([names[i], int(hit[i].sum()), float(excess[i, best]), names[best], float(np.nansum(excess[i]))])
            else:
                rows.append([names[i], 0, float("nan"), "", float("nan")])
        rows.sort(key=lambda r: (-r[1], -r[4] if r[4] == r[4] else np.inf))
        return ["object", "n_flagged", "max_excess", "max_excess_partner", "sum_excess"], rows

    def write_tables(self, pairs_path=None, objects_path=None, names=None, p_threshold=0.05, top=None):
        if pairs_path is not None:
            _samples.write_tsv(pairs_path, *self.pair_table(names, p_threshold, top))
        if objects_path is not None:
            _samples.write_tsv(objects_path, *self.object_table(names, p_threshold))


class ObjPairHandle(_handle.UnitHandle):
    """Owner of one sbe_objpair handle: the data, its observed counts and the accumulators on one device.  add() feeds replicates;
    result() reads the accumulators back.  last_kernel_ms(): the count kernels' launches of the last library call."""
    _prefix, _noun = "sbe_objpair", "an object-pair check handle"

    def __init__(self, device=None):
        self.shape = None                                    # (N, F, E) once the data is set
        self.n_states = None
        self._agree_rep = []
        self.kernel_ms = 0.0
        self._create_on(load, device)

    def set_data(self, codes, n_states=None):
        """codes uint8 [N, F] (255 = NA) or one-hot bool [N, F, S]; n_states: states per feature (default: one more than the largest
        code that occurs).  Computes the observed counts and clears the accumulators."""
        x, ns = assoc._check_inputs(codes, n_states)
        n, f = x.shape
        if n > MAX_OBJECTS:
            raise ValueError(f"{n} objects; the outputs are [N, N] matrices, limited to {MAX_OBJECTS} objects")
        if f > MAX_FEATURES:
            raise ValueError(f"{f} features; the unit takes 1 .. {MAX_FEATURES}")
        self.shape = None
        self._check(self._lib.sbe_objpair_set_data(self._h, _ptr(x), n, f, _ptr(ns)))
        self.shape, self.n_states = (n, f, int(ns.sum())), ns
        self._agree_rep, self.kernel_ms = [], self.last_kernel_ms()

    def _with_data(self):
        if self.shape is None:
            raise ValueError("no data yet (set_data)")
        return self.shape

    def reset(self):
        """Clear the accumulators, keep the data."""
        self._with_data()
        self._check(self._lib.sbe_objpair_reset(self._h))
        self._agree_rep, self.kernel_ms = [], 0.0

    def set_launch_tiles(self, tile_pairs):
        """Tile pairs per launch of the count kernels (0: the default).  Results do not depend on it."""
        self._check(self._lib.sbe_objpair_set_launch_tiles(self._h, int(tile_pairs)))

    def max_replicates(self, agree_rep=False) -> int:
        """The replicates one library call holds (one at least)."""
        n, f, e = self._with_data()
        return max(1, MAX_STAGE_BYTES // replicate_bytes(n, f, e, agree_rep))

    def last_shape(self):
        """(E_pad, tile pairs, launches) of the last set_data or add call of the library."""
        e_pad, tiles, launches = ct.c_int64(0), ct.c_int64(0), ct.c_int64(0)
        self._check(self._lib.sbe_objpair_last_shape(self._h, ct.byref(e_pad), ct.byref(tiles), ct.byref(launches)))
        return e_pad.value, tiles.value, launches.value

    def add(self, y_rep, agree_rep=False):
        """Replicates uint8 [n, N, F], each code below n_states[f] or 255.  agree_rep: keep (and return) the replicates' own counts
        int32 [n, N, N].  Blocks beyond max_replicates() go in several library calls; each call validates its replicates before
        it changes anything, so an EngineError leaves the replicates of the calls before it added."""
        n_obj, f, _e = self._with_data()
        y = _samples.check_replicates(y_rep, n_obj, f)
        step = self.max_replicates(agree_rep)
        y = np.ascontiguousarray(y)
        self.kernel_ms = 0.0
        kept = []
        for r0 in range(0, y.shape[0], step):
            block = y[r0:r0 + step]
            out = np.empty((block.shape[0], n_obj, n_obj), dtype=np.int32) if agree_rep else None
            self._check(self._lib.sbe_objpair_add(self._h, block.shape[0], _ptr(block), _ptr(out) if agree_rep else None))
            self.kernel_ms += self.last_kernel_ms()
            if agree_rep:
                kept.append(out)
        if y.shape[0]:
            self._agree_rep.append(np.concatenate(kept) if kept else None)
        return self._agree_rep[-1] if y.shape[0] else None

    def result(self) -> ObjPairResult:
        n, _f, _e = self._with_data()
        obs, cmp, gt, eq, lt = (np.empty((n, n), dtype=np.int32) for _ in range(5))
        s1, s2 = (np.empty((n, n), dtype=np.int64) for _ in range(2))
        count = ct.c_int64(0)
        self._check(self._lib.sbe_objpair_read(self._h, _ptr(obs), _ptr(cmp), _ptr(gt), _ptr(eq), _ptr(lt), _ptr(s1), _ptr(s2), ct.byref(count)))
        kept = self._agree_rep
        return ObjPairResult(obs, cmp, gt, eq, lt, s1, s2, count.value, self.n_states,
                             np.concatenate(kept) if kept and all(k is not None for k in kept) else None, self.kernel_ms)


def object_pair_check(codes, groups, clusters, weights, tables, n_states=None, burnin=0.1, seed=0, n_groups=None, uniforms=None,
                      device=None) -> ObjPairResult:
    """The object-pair check of T logged samples after burn-in: the samples, seed and draw indices are posterior_predictive_check's
    (sbayes_amd/ppc.py), as pairwise_check's and spatial_check's are, so the four checks describe the same replicates (res.ppc holds
    that result, without y_rep).  n_states: states per feature (default: the tables' S for every feature -- a replicate may draw a
    state the data never shows).  The replicates pass through host memory, block by block.

    The p-values are conditional on the logged effect draws and use the data twice, so they are conservative (DESIGN.md section
    22), and the N (N - 1) / 2 pairs are dependent multiple comparisons: no correction is applied."""
    groups, n_groups, clusters, weights, tables, uniforms = _samples.after_burnin(groups, clusters, weights, tables, burnin, n_groups, uniforms)
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    if n_states is None:
        n_states = np.full(codes.shape[1] if codes.ndim == 2 else 0, tables.shape[3], dtype=np.int32)

    def fill(h):
        h.set_data(codes, n_states)
        return h.max_replicates(), h.add
    return _samples.check_with_replicates(ObjPairHandle, fill, codes, groups, n_groups, clusters, weights, tables, seed, uniforms, device)


def read_object_ids(features_csv):
    """The `id` column of the features file, or None if it has none (the objects are then numbered)."""
    import pandas as pd
    raw = pd.read_csv(features_csv, dtype=str, keep_default_na=False, usecols=lambda c: c == "id")
    return [v.strip() for v in raw["id"]] if "id" in raw.columns else None


def parser():
    ap = _samples.run_parser("python -m sbayes_amd.objpair",
                             "Agreement of every pair of objects of an sBayes run checked against the fitted model: the features on "
                             "which a pair shows the same state among the same count on one replicated data set per logged sample "
                             "(conservative: given the logged effect draws; the pairs are dependent comparisons, uncorrected)", seed=True)
    ap.add_argument("--out-pairs", type=Path, default=Path("object_pairs.tsv"), help="the table of the flagged pairs, or of the --top worst")
    ap.add_argument("--out-objects", type=Path, default=Path("object_pair_summary.tsv"), help="the table per object")
    ap.add_argument("-p", "--pThreshold", type=float, default=0.05, help="the predictive p below which a pair is flagged")
    ap.add_argument("--top", type=int, default=None, help="write this many pairs with the smallest predictive p instead of the flagged ones")
    return ap


def main(argv=None):
    args = parser().parse_args(argv)
    data, clusters, weights, tables, n_groups = _samples.read_run(args)
    n_states = np.array([max(1, len(s)) for s in data["state_names"]], dtype=np.int32)
    res = object_pair_check(data["codes"], data["groups"], clusters, weights, tables, n_states=n_states, burnin=args.burnin, seed=args.seed,
                            n_groups=n_groups, device=args.device)
    names = read_object_ids(args.features)
    n = res.observed.shape[0]
    pairs = n * (n - 1) // 2
    print(f"{res.n_replicates} replicates, {pairs} pairs of objects, {len(res.flagged(args.pThreshold))} with predictive p < {args.pThreshold:g} "
          f"(conservative: given the logged effect draws; {pairs} dependent comparisons, uncorrected)")
    print("the five pairs with the smallest predictive p:")
    for a, b, agree, cmp, _share, p, mean, sd, excess, z in res.worst(5, names):
        print(f"  {a}\t{b}\tagree {agree} of {cmp}\tp predictive {p:.4f}\treplicated {mean:.2f} +- {sd:.2f}\texcess {excess:.2f}\tz {z:.3f}")
    res.write_tables(args.out_pairs, args.out_objects, names, args.pThreshold, args.top)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
