"""Leave-one-out predictive of every observed cell on the device (include/sbe_loopred.h): had this cell not been observed, what
would the fitted model have predicted for it, and would it have been right?

predict.posterior_predictive's probabilities are in-sample: the cell's own value shaped the cluster's and the family's effect
draw that predicts it.  elpd.psis_loo computes the smoothed importance weights that remove that influence and keeps only their
log score.  This module keeps the weights and runs the logged samples past them a second time:

    p_loo[n, f, s] = sum_t w_t(n, f) m_t[n, f, s]

with m_t the mixture row of sample t (predict's) and w_t the normalised PSIS weight of sample t for the cell (elpd's).

    res = loo_predictive(codes, groups, clusters, weights, tables, burnin=0.1)
    res.probs [N,F,S]            the leave-one-out predictive of every observed cell (NaN at NA cells)
    res.loo_i, res.k, res.n_eff  [N,F]: log p_loo[x], the Pareto shape and the effective sample size 1 / sum_t w_t^2
    res.p_obs, res.predicted     the probability of the observed state; the arg-max state (lowest on ties, -1 at NA cells)
    res.accuracy(by=None | "feature" | "object"), res.brier(by=...), res.log_score(by=...)
    res.calibration(bins=10)     per bin of predicted probability: (cell, state) pairs, mean prediction, observed frequency
    res.optimism(predict_result) in-sample minus leave-one-out accuracy and log score
    res.n_bad_k(0.7), res.table()
    h = LooPredHandle(); h.set_data(..., capacity=T); h.add(...); h.weights(); h.accumulate(...); h.result()
    python -m sbayes_amd.loopred FEATURES FEATURE_STATES STATS CLUSTERS --confounders universal family --out DIR

As in predict, everything is CONDITIONAL ON THE LOGGED EFFECT DRAWS: leave-one-out removes the cell's influence on the weighting
of the samples, not on a draw already made.  This is the estimator here; it is not the LikelihoodLogger's collapsed form, which
integrates the effects out.  Cells with k > 0.7 are counted and flagged, not refitted: their weights are unreliable.

Numerical contract (tests/_loopred_oracle.py restates it in fp64; DESIGN.md section 26 states it): the rows are predict's lik
bit for bit, loo_i and k are elpd's bits on those rows, w_t = exp(x'_t) / sum_t exp(x'_t) in float64 with the tail's positions
among equal values in sample order, and a cell's sums add the rounded products w_t m_t[s] in sample order, so they are
bit-identical however the samples are split across calls.  An observed cell of likelihood zero in any sample is an EngineError
(SBE_ERR_DATA = 4) naming the cell and the sample.  Limits: predict's, 2 .. 2^20 samples, 16 GiB of rows and weights on the device
(store_bytes tells beforehand).

There is no CPU fallback: without the library or a GPU the functions raise.  Handles follow the package's process model
(sbayes_amd/_proc.py): never pickled, forgotten (not destroyed) in a fork()ed child."""
from __future__ import annotations

import ctypes as ct
from dataclasses import dataclass
from pathlib import Path

import numpy as np

from . import _handle, _samples, predict
from ._handle import _ptr, c_handle_p
from .predict import NA, _check_burnin, _check_shape, group_index

ABI_VERSION = 1                          # SBE_LOOPRED_ABI_VERSION of include/sbe_loopred.h
MIN_SAMPLES = 2                          # SBE_ELPD_MIN_SAMPLES
MAX_SAMPLES = 1 << 20                    # SBE_LOOPRED_MAX_SAMPLES
MAX_STORE_BYTES = 1 << 34                # SBE_LOOPRED_MAX_STORE_BYTES
MAX_STAGE_BYTES = predict.MAX_STAGE_BYTES   # SBE_LOOPRED_MAX_STAGE_BYTES
MAX_TILE = predict.MAX_TILE              # SBE_LOOPRED_MAX_TILE

# name -> (restype, argtypes); mirrors include/sbe_loopred.h one to one
PROTOTYPES = {
    **_handle.unit_prototypes("sbe_loopred"),
    "sbe_loopred_create": (ct.c_int, [ct.POINTER(c_handle_p), ct.c_int]),
    "sbe_loopred_store_bytes": (ct.c_int64, [ct.c_int64, ct.c_int64]),
    "sbe_loopred_sample_bytes": (ct.c_int64, [ct.c_int64, ct.c_int64, ct.c_int, ct.c_int, ct.c_int, ct.c_int]),
    "sbe_loopred_lds_max_samples": (ct.c_int64, []),
    "sbe_loopred_set_data": (ct.c_int, [c_handle_p, ct.c_int64, ct.c_int64, ct.c_int, ct.c_int, ct.c_int, ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_int64]),
    "sbe_loopred_reset": (ct.c_int, [c_handle_p]),
    "sbe_loopred_add": (ct.c_int, [c_handle_p, ct.c_int64, ct.c_void_p, ct.c_void_p, ct.c_void_p]),
    "sbe_loopred_weights": (ct.c_int, [c_handle_p, ct.c_void_p, ct.c_void_p, ct.c_void_p]),
    "sbe_loopred_accumulate": (ct.c_int, [c_handle_p, ct.c_int64, ct.c_int64, ct.c_void_p, ct.c_void_p, ct.c_void_p]),
    "sbe_loopred_read": (ct.c_int, [c_handle_p, ct.c_void_p, ct.POINTER(ct.c_int64)]),
    "sbe_loopred_set_feature_tile": (ct.c_int, [c_handle_p, ct.c_int]),
    "sbe_loopred_get_store": (ct.c_int, [c_handle_p, ct.c_void_p, ct.c_void_p]),
}


def load():
    """The engine library with the prototypes of include/sbe_loopred.h attached."""
    return _handle.bind("sbe_loopred", PROTOTYPES, ABI_VERSION)


def store_bytes(n_observed, capacity) -> int:
    """Device bytes of the rows and weights of n_observed cells and `capacity` samples (sbe_loopred_store_bytes)."""
    return int(n_observed) * int(capacity) * 12


def sample_bytes(n_objects, n_features, n_states, n_components, n_clusters, n_rows) -> int:
    """Device bytes one sample of an add or accumulate call takes while the call runs (sbe_loopred_sample_bytes): predict's with
    its likelihood row."""
    return predict.sample_bytes(n_objects, n_features, n_states, n_components, n_clusters, n_rows, True)


def lds_max_samples() -> int:
    """Largest T whose columns the weights kernel stages in LDS; longer columns are read from global memory."""
    return int(load().sbe_loopred_lds_max_samples())


def _group(values, by, observed):
    """The mean of `values` [N,F] over the observed cells: in all, per feature [F] or per object [N] (NaN where none is observed)."""
    if by not in (None, "feature", "object"):
        raise ValueError(f"by={by!r} must be None, 'feature' or 'object'")
    v = np.where(observed, values, 0.0)
    if by is None:
        return float(v.sum() / observed.sum()) if observed.any() else float("nan")
    axis = 0 if by == "feature" else 1
    with np.errstate(invalid="ignore", divide="ignore"):
        return v.sum(axis=axis) / observed.sum(axis=axis)


@dataclass
class LooPredResult:
    """probs [N,F,S]: the leave-one-out predictive of the observed cells, NaN at NA cells; loo_i, k, n_eff [N,F], NaN at NA cells.
    Conditional on the logged effect draws (the module's docstring)."""
    codes: np.ndarray
    probs: np.ndarray
    loo_i: np.ndarray
    k: np.ndarray
    n_eff: np.ndarray
    n_samples: int
    kernel_ms: dict | None = None

    @property
    def observed(self):
        return self.codes != NA

    @property
    def p_obs(self):
        """[N,F]: the leave-one-out probability of the observed state (NaN at NA cells); exp(loo_i) but for rounding."""
        x = np.where(self.observed, self.codes, 0).astype(np.int64)[..., None]
        return np.where(self.observed, np.take_along_axis(self.probs, x, axis=2)[..., 0], np.nan)

    @property
    def predicted(self):
        """int [N,F]: the most probable state, the lowest on ties; -1 at NA cells."""
        return np.where(self.observed, np.where(self.observed[..., None], self.probs, 0.0).argmax(axis=2), -1)

    def accuracy(self, by=None):
        """The share of observed cells whose observed state is the predicted one: held-out imputation accuracy."""
        return _group((self.predicted == self.codes).astype(np.float64), by, self.observed)

    def brier(self, by=None):
        """The mean over observed cells of sum_s (probs[s] - [s == x])^2."""
        onehot = np.arange(self.probs.shape[2])[None, None, :] == self.codes[..., None]
        return _group(np.where(self.observed[..., None], (self.probs - onehot) ** 2, 0.0).sum(axis=2), by, self.observed)

    def log_score(self, by=None):
        """The mean over observed cells of loo_i = log p_loo[x]."""
        return _group(self.loo_i, by, self.observed)

    def calibration(self, bins=10):
        """(count int [bins], mean_predicted [bins], observed_frequency [bins]) over the (observed cell, state) pairs, binned by
        predicted probability in [0, 1] (the last bin closed); NaN in the means of an empty bin."""
        bins = int(bins)
        if bins < 1:
            raise ValueError(f"bins={bins} must be positive")
        obs = self.observed
        p = self.probs[obs]                                              # [M, S]
        hit = (np.arange(p.shape[1])[None, :] == self.codes[obs][:, None])
        which = np.minimum((p * bins).astype(np.int64), bins - 1).ravel()
        count = np.bincount(which, minlength=bins)
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = np.bincount(which, weights=p.ravel(), minlength=bins) / count
            freq = np.bincount(which, weights=hit.ravel().astype(np.float64), minlength=bins) / count
        return count, mean, freq

    def optimism(self, predict_result):
        """dict(accuracy, log_score): the in-sample value minus the leave-one-out one, from a predict.PredictResult of the same
        data and samples."""
        if predict_result.codes.shape != self.codes.shape or not np.array_equal(predict_result.codes, self.codes):
            raise ValueError("the posterior predictive was computed on other data")
        if predict_result.n_samples != self.n_samples:
            raise ValueError(f"the posterior predictive holds {predict_result.n_samples} samples, the leave-one-out predictive {self.n_samples}")
        obs = self.observed
        inside = predict_result.probs
        x = np.where(obs, self.codes, 0).astype(np.int64)[..., None]
        with np.errstate(divide="ignore"):
            log_in = np.log(np.take_along_axis(inside, x, axis=2)[..., 0])
        acc_in = _group((inside.argmax(axis=2) == self.codes).astype(np.float64), None, obs)
        return dict(accuracy=acc_in - self.accuracy(), log_score=_group(log_in, None, obs) - self.log_score())

    def n_bad_k(self, threshold=0.7) -> int:
        """The observed cells whose Pareto k exceeds `threshold` (or is NaN): their weights are unreliable."""
        k = self.k[self.observed]
        return int((~(k <= threshold)).sum())

    def table(self, feature_names=None, state_names=None):
        """(header, rows): one row per observed cell: object, feature, observed, predicted, p_obs, loo_i, k."""
        N, F, _S = self.probs.shape
        fn = list(feature_names) if feature_names is not None else [f"F{f + 1}" for f in range(F)]

        def state(f, s):
            return str(s) if state_names is None else str(state_names[f][s])
        best, p_obs = self.predicted, self.p_obs
        rows = [[n, fn[f], state(f, int(self.codes[n, f])), state(f, int(best[n, f])), float(p_obs[n, f]), float(self.loo_i[n, f]), float(self.k[n, f])]
                for n in range(N) for f in range(F) if self.codes[n, f] != NA]
        return ["object", "feature", "observed", "predicted", "p_obs", "loo_i", "k"], rows

    def feature_table(self, feature_names=None):
        """(header, rows): per feature its observed cells, accuracy, Brier score, mean log score and cells with k > 0.7."""
        F = self.probs.shape[1]
        fn = list(feature_names) if feature_names is not None else [f"F{f + 1}" for f in range(F)]
        acc, brier, score = self.accuracy("feature"), self.brier("feature"), self.log_score("feature")
        bad = (self.observed & ~(self.k <= 0.7)).sum(axis=0)
        rows = [[fn[f], int(self.observed[:, f].sum()), float(acc[f]), float(brier[f]), float(score[f]), int(bad[f])] for f in range(F)]
        return ["feature", "n_observed", "accuracy", "brier", "log_score", "n_bad_k"], rows

    def write_tables(self, out_dir, feature_names=None, state_names=None):
        """loo_predictive.tsv and loo_features.tsv in out_dir; returns the paths."""
        out_dir = Path(out_dir)
        out_dir.mkdir(parents=True, exist_ok=True)
        paths = []
        for name, table in (("loo_predictive.tsv", self.table(feature_names, state_names)), ("loo_features.tsv", self.feature_table(feature_names))):
            _samples.write_tsv(out_dir / name, *table)
            paths.append(out_dir / name)
        return paths


def result_from(codes, p_loo, loo_i, k_i, n_eff, n_samples, kernel_ms=None) -> LooPredResult:
    """The result of the unit's raw outputs: p_loo [N,F,S] (zero at NA cells) and loo_i, k_i, n_eff [M] in column order."""
    codes = np.asarray(codes)
    obs = codes != NA

    def spread(v):
        out = np.full(codes.shape, np.nan)
        out[obs] = v
        return out
    return LooPredResult(codes=codes, probs=np.where(obs[..., None], p_loo, np.nan), loo_i=spread(loo_i), k=spread(k_i), n_eff=spread(n_eff),
                         n_samples=int(n_samples), kernel_ms=kernel_ms)


class LooPredHandle(_samples.SampleHandle):
    """Owner of one sbe_loopred handle: the data, the stored rows and weights and the sums on one device.  The phases in order:
    set_data(.., capacity), add(..) any number of times, weights(), accumulate(..) over the same samples again, result()."""
    _prefix, _noun = "sbe_loopred", "a leave-one-out predictive handle"

    def _clear(self):
        self.n_rows, self.next_t, self._pointwise = 0, 0, None
        self.kernel_ms = dict(add=0.0, weights=0.0, accumulate=0.0)

    def set_data(self, codes, groups, n_groups, n_states, n_clusters, capacity):
        """predict.PredictHandle.set_data's arguments and the number of samples the store takes."""
        capacity = int(capacity)

        def store(codes):
            if not 1 <= capacity <= MAX_SAMPLES:
                raise ValueError(f"capacity={capacity}; the store takes 1 .. {MAX_SAMPLES} (2^20) samples")
            M = int((codes != NA).sum())
            if store_bytes(M, capacity) > MAX_STORE_BYTES:
                raise ValueError(f"the rows and weights of {M} observed cells x {capacity} samples take {store_bytes(M, capacity)} bytes on the device, "
                                 f"the limit is {MAX_STORE_BYTES}")
            return (capacity,)
        self._set_data(codes, groups, n_groups, n_states, n_clusters, store)
        self.n_observed, self.capacity = int((self._codes != NA).sum()), capacity

    def reset(self):
        """Forget the rows, the weights and the sums, keep the data."""
        self._with_data()
        self._check(self._lib.sbe_loopred_reset(self._h))
        self._clear()

    def max_samples(self) -> int:
        """The samples one library call holds."""
        return MAX_STAGE_BYTES // sample_bytes(*self._with_data())

    def add(self, clusters, weights, tables):
        """Phase 1: store the likelihood rows of the samples: clusters uint8 [T,K,N] of 0 / 1, weights float64 [T,F,C], tables
        float64 [T,R,F,S].  Blocks beyond max_samples() go in several library calls."""
        T, blocks = self._blocks(clusters, weights, tables)
        if self.n_rows + T > self.capacity:
            raise ValueError(f"{self.n_rows} samples stored, {T} more exceed the capacity of {self.capacity}")
        for _t0, cl, w, tb in blocks:
            self._check(self._lib.sbe_loopred_add(self._h, cl.shape[0], _ptr(cl), _ptr(w), _ptr(tb)))
            self.n_rows += cl.shape[0]
            self.kernel_ms["add"] += self.last_kernel_ms()
        self._pointwise, self.next_t = None, 0

    def weights(self):
        """Phase 2: PSIS per observed cell over the stored rows; returns (loo_i, k, n_eff), float64 [M] in column order."""
        self._with_data()
        if self.n_rows < MIN_SAMPLES:
            raise ValueError(f"{self.n_rows} samples stored; PSIS needs at least {MIN_SAMPLES} per observation")
        loo_i, k_i, n_eff = (np.empty(max(self.n_observed, 1), dtype=np.float64) for _ in range(3))
        self._pointwise, self.next_t = None, 0
        self._check(self._lib.sbe_loopred_weights(self._h, _ptr(loo_i), _ptr(k_i), _ptr(n_eff)))
        self.kernel_ms["weights"] = self.last_kernel_ms()
        self.kernel_ms["accumulate"] = 0.0
        self._pointwise = tuple(v[:self.n_observed] for v in (loo_i, k_i, n_eff))
        return self._pointwise

    def accumulate(self, clusters, weights, tables):
        """Phase 3: the samples of phase 1 again, in the same order (the next block of them; any split)."""
        if self._pointwise is None:
            self._with_data()
            raise ValueError("no weights yet (weights() comes before accumulate())")
        T, blocks = self._blocks(clusters, weights, tables)
        if self.next_t + T > self.n_rows:
            raise ValueError(f"{self.next_t} of {self.n_rows} samples accumulated, {T} more are too many")
        for _t0, cl, w, tb in blocks:
            self._check(self._lib.sbe_loopred_accumulate(self._h, self.next_t, cl.shape[0], _ptr(cl), _ptr(w), _ptr(tb)))
            self.next_t += cl.shape[0]
            self.kernel_ms["accumulate"] += self.last_kernel_ms()

    def sums(self):
        """(p_loo [N,F,S], the samples accumulated)."""
        N, F, S, _C, _K, _R = self._with_data()
        p = np.empty((N, F, S))
        n = ct.c_int64(0)
        self._check(self._lib.sbe_loopred_read(self._h, _ptr(p), ct.byref(n)))
        return p, n.value

    def store(self, with_weights=True):
        """A test read: (lik float32 [T, M], w float64 [T, M] or None), the store's columns as rows of samples."""
        self._with_data()
        lik = np.empty((self.n_observed, self.n_rows), dtype=np.float32)
        w = np.empty((self.n_observed, self.n_rows), dtype=np.float64) if with_weights else None
        self._check(self._lib.sbe_loopred_get_store(self._h, _ptr(lik), _ptr(w) if with_weights else None))
        return lik.T, (w.T if with_weights else None)

    def result(self) -> LooPredResult:
        if self._pointwise is None:
            self._with_data()
            raise ValueError("no weights yet (weights() comes before result())")
        p, n = self.sums()
        if n != self.n_rows:
            raise ValueError(f"{n} of {self.n_rows} samples accumulated: the second pass is not complete")
        return result_from(self._codes, p, *self._pointwise, n_samples=n, kernel_ms=dict(self.kernel_ms))


def loo_predictive(codes, groups, clusters, weights, tables, burnin=0.1, device=None, n_groups=None) -> LooPredResult:
    """The leave-one-out predictive of T logged samples after burn-in, in predict.posterior_predictive's argument forms: codes
    uint8 [N,F]; groups: uint8 [C-1,N] group indices (with n_groups) or a list of bool [G_c,N] assignments; clusters uint8 [T,K,N];
    weights [T,F,C]; tables [T,R,F,S].  The samples go to the device twice, in blocks of what one call holds."""
    groups, n_groups, clusters, weights, tables, _u = _samples.after_burnin(groups, clusters, weights, tables, burnin, n_groups)
    T = clusters.shape[0]
    if not MIN_SAMPLES <= T <= MAX_SAMPLES:
        raise ValueError(f"{T} samples after burn-in; PSIS needs {MIN_SAMPLES} .. {MAX_SAMPLES} (2^20) per observation")
    h = LooPredHandle(device)
    try:
        h.set_data(codes, groups, n_groups, tables.shape[3], clusters.shape[1], capacity=T)
        h.add(clusters, weights, tables)
        h.weights()
        h.accumulate(clusters, weights, tables)
        return h.result()
    finally:
        h.close()


def main(argv=None):
    ap = _samples.run_parser("python -m sbayes_amd.loopred",
                             "Leave-one-out predictive of every observed cell of an sBayes run, given the logged effect draws: "
                             "held-out imputation accuracy, Brier score and calibration without refitting")
    ap.add_argument("--out", type=Path, default=None, help="directory for loo_predictive.tsv and loo_features.tsv")
    args = ap.parse_args(argv)
    data, clusters, weights, tables, n_groups = _samples.read_run(args)
    res = loo_predictive(data["codes"], data["groups"], clusters, weights, tables, burnin=args.burnin, device=args.device, n_groups=n_groups)
    print(f"{res.n_samples} samples, {int(res.observed.sum())} observed cells (given the logged effect draws): leave-one-out accuracy "
          f"{res.accuracy():.4f}, Brier {res.brier():.4f}, log score {res.log_score():.4f}")
    bad = res.n_bad_k(0.7)
    if bad:
        print(f"warning: {bad} cells with Pareto k > 0.7: their leave-one-out weights are unreliable")
    if args.out:
        res.write_tables(args.out, data["feature_names"], data["state_names"])
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
