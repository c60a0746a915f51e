"""Posterior predictive of the logged samples on the device (include/sbe_predict.h): the probability of every state in
every cell, each component's responsibility for the observed cells, and the pointwise likelihood rows.

A run's stats_K*_*.txt holds one full draw of the mixture model per logged sample -- the weights, a Dirichlet draw of every
cluster's effect and of every confounder group's effect (sbayes/sampling/loggers.py:106-130, 157-228) -- and
clusters_K*_*.txt the membership.  This module puts them back together with the data.  The per-sample mixture row of a
cell, m_t[n,f,.] = sum_c wn_t[n,f,c] theta_t,c[g_c,t(n), f, .], is simulate_features' lh_feature
(sbayes/simulation.py:238-252); averaged over the samples it is

    res = posterior_predictive(codes, groups, clusters, weights, tables, burnin=0.1)
    res.probs [N,F,S]            the posterior predictive probability of every state: imputation for the NA cells
    res.responsibility [N,F,C]   the contact / universal / inheritance share of every observed cell (NaN for NA cells)
    res.impute()                 codes with the NA cells filled by the most probable state, and that state's probability
    res.log_score(codes, mask)   sum over the masked cells of log probs[n, f, codes]: held-out scoring
    res.lik                      with lik=True: float32 [T, N F] in the LikelihoodLogger's layout (NA -> 1.0), for
                                 elpd.psis_loo / elpd.waic / compare when the run's .h5 was never written
    h = PredictHandle(); h.set_data(...); h.accumulate(clusters, weights, tables); h.result()
    python -m sbayes_amd.predict FEATURES FEATURE_STATES STATS CLUSTERS --confounders universal family [--elpd]

The likelihood rows condition on the logged effect draws.  They are not the LikelihoodLogger's rows, which integrate the
effects out and leave the observation itself out of the counts (the collapsed leave-one-out form): an ELPD computed from
them answers for the logged draws, and is not interchangeable with one computed from a likelihood_K*_*.h5.

Numerical contract (tests/_predict_oracle.py restates it in fp64; DESIGN.md section 21 states it): all arithmetic is
float64; a cell's sums add the samples in order, so they are bit-identical from call to call and however the samples are
split across accumulate calls.  Samples are validated on the device before anything is added (EngineError, code
SBE_ERR_DATA = 4, naming the first offender).  Limits: S <= 32 states, C <= 8 components, R <= 256 table rows,
N <= 2^20, F <= 2^16, 4 GiB of accumulators; one call holds at most 256 MiB of samples on the device and accumulate()
splits longer blocks.

There is no CPU fallback: without the library or a GPU the functions raise.  Handles follow the package's process model
(sbayes_amd/_proc.py): never pickled, forgotten (not destroyed) in a fork()ed child."""
from __future__ import annotations

import ctypes as ct
from dataclasses import dataclass
from pathlib import Path

import numpy as np

from . import _handle, _samples
from ._handle import _ptr, c_handle_p
from ._samples import (MAX_ACC_BYTES, MAX_COMPONENTS, MAX_FEATURES, MAX_OBJECTS, MAX_ROWS, MAX_STAGE_BYTES, MAX_STATES, MAX_TILE, NA,  # noqa: F401
                       SUM_TOL, _check_burnin, _check_shape, codes_of, group_index)                # (the limits and checks of the data)

ABI_VERSION = 1                          # SBE_PREDICT_ABI_VERSION of include/sbe_predict.h

# name -> (restype, argtypes); mirrors include/sbe_predict.h one to one (the engine's own table, _lib.PROTOTYPES, is not extended)
PROTOTYPES = {
    **_handle.unit_prototypes("sbe_predict"),
    "sbe_predict_create": (ct.c_int, [ct.POINTER(c_handle_p), ct.c_int]),
    "sbe_predict_sample_bytes": (ct.c_int64, [ct.c_int64, ct.c_int64, ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_int]),
    "sbe_predict_set_data": (ct.c_int, [c_handle_p, ct.c_int64, ct.c_int64, ct.c_int, ct.c_int, ct.c_int, ct.c_void_p, ct.c_void_p, ct.c_void_p]),
    "sbe_predict_reset": (ct.c_int, [c_handle_p]),
    "sbe_predict_accumulate": (ct.c_int, [c_handle_p, ct.c_int64, ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_void_p]),
    "sbe_predict_read": (ct.c_int, [c_handle_p, ct.c_void_p, ct.c_void_p, ct.POINTER(ct.c_int64), ct.POINTER(ct.c_int64)]),
    "sbe_predict_set_feature_tile": (ct.c_int, [c_handle_p, ct.c_int]),
}


def load():
    """The engine library with the prototypes of include/sbe_predict.h attached."""
    return _handle.bind("sbe_predict", PROTOTYPES, ABI_VERSION)


def sample_bytes(n_objects, n_features, n_states, n_components, n_clusters, n_rows, with_lik=False) -> int:
    """Device bytes one sample of an accumulate call takes while the call runs (sbe_predict_sample_bytes)."""
    n, f = int(n_objects), int(n_features)
    return int(n_clusters) * n + 8 * f * int(n_components) + 8 * int(n_rows) * f * int(n_states) + 2 * n + (4 * n * f if with_lik else 0)


@dataclass
class PredictResult:
    """probs [N,F,S] = pred_sum / n_samples; responsibility [N,F,C] = resp_sum / the samples that contributed to the cell
    (NaN for NA cells and for cells no sample contributed to); n_zero: the (sample, observed cell) pairs whose observed state
    had probability 0; lik: float32 [n_samples, N F] or None."""
    codes: np.ndarray
    pred_sum: np.ndarray
    resp_sum: np.ndarray
    n_samples: int
    n_zero: int
    lik: np.ndarray | None = None
    kernel_ms: float = 0.0

    @property
    def probs(self):
        return self.pred_sum / self.n_samples

    @property
    def responsibility(self):
        # every contributing sample adds responsibilities that sum to 1 (but for rounding): their sum counts the samples
        count = np.rint(self.resp_sum.sum(axis=2, keepdims=True))
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where((self.codes != NA)[..., None] & (count > 0), self.resp_sum / count, np.nan)

    def impute(self):
        """(codes with the NA cells filled by the arg-max state, ties to the lowest index; that state's probability [N,F])."""
        best = self.pred_sum.argmax(axis=2)
        filled = np.where(self.codes == NA, best, self.codes).astype(np.uint8)
        return filled, np.take_along_axis(self.pred_sum, best[..., None], axis=2)[..., 0] / self.pred_sum.sum(axis=2)

    def log_score(self, codes, mask):
        """sum over the cells of `mask` of log probs[n, f, codes[n, f]] (held-out scoring: codes are the held-out truth)."""
        codes, mask = np.asarray(codes), np.asarray(mask, dtype=bool)
        if codes.shape != self.codes.shape or mask.shape != self.codes.shape:
            raise ValueError(f"codes and mask must have shape {self.codes.shape}")
        if (codes[mask] >= self.pred_sum.shape[2]).any():
            raise ValueError("a masked cell holds no state (NA or out of range)")
        p = np.take_along_axis(self.probs, np.where(mask, codes, 0).astype(np.int64)[..., None], axis=2)[..., 0]
        with np.errstate(divide="ignore"):
            return float(np.sum(np.log(p[mask])))

    def table(self, feature_names=None, state_names=None, component_names=None, na_only=True):
        """(header, rows): per cell (the NA cells only, or all) the object and feature, the observed and the most probable
        state, its probability and, for observed cells, the responsibilities."""
        N, F, S = self.pred_sum.shape
        C = self.resp_sum.shape[2]
        fn = list(feature_names) if feature_names is not None else [f"F{f + 1}" for f in range(F)]
        cn = list(component_names) if component_names is not None else [f"c{c}" for c in range(C)]

        def state(f, s):
            return str(s) if state_names is None else str(state_names[f][s])
        filled, p = self.impute()
        resp = self.responsibility
        rows = []
        for n in range(N):
            for f in range(F):
                missing = self.codes[n, f] == NA
                if na_only and not missing:
                    continue
                best = int(self.pred_sum[n, f].argmax())
                rows.append([n, fn[f], "" if missing else state(f, int(self.codes[n, f])), state(f, best), float(p[n, f])] +
                            [float(v) for v in resp[n, f]])
        return ["object", "feature", "observed", "predicted", "probability"] + [f"resp_{c}" for c in cn], rows

    def write_table(self, path, **kw):
        _samples.write_tsv(path, *self.table(**kw))


class PredictHandle(_samples.SampleHandle):
    """Owner of one sbe_predict handle: the data and the accumulators on one device.  last_kernel_ms(): the kernels of the
    last library call of accumulate()."""
    _prefix, _noun = "sbe_predict", "a posterior predictive handle"

    def reset(self):
        """Zero the sums, keep the data."""
        self._with_data()
        self._check(self._lib.sbe_predict_reset(self._h))

    def max_samples(self, lik=False) -> int:
        """The samples one library call holds."""
        return MAX_STAGE_BYTES // sample_bytes(*self._with_data(), lik)

    def accumulate(self, clusters, weights, tables, lik=False):
        """Add samples: clusters uint8 [T,K,N] of 0 / 1, weights float64 [T,F,C], tables float64 [T,R,F,S].  Returns the
        float32 [T, N F] likelihood rows with lik=True.  Blocks beyond max_samples() go in several library calls; each call
        validates its samples before it adds them, so an EngineError leaves the samples of the calls before it added."""
        T, blocks = self._blocks(clusters, weights, tables, lik)
        N, F = self.shape[:2]
        rows = np.empty((T, N * F), dtype=np.float32) if lik else None
        self.kernel_ms = 0.0
        for t0, cl, w, tb in blocks:
            out = rows[t0:t0 + cl.shape[0]] if lik else None
            self._check(self._lib.sbe_predict_accumulate(self._h, cl.shape[0], _ptr(cl), _ptr(w), _ptr(tb), _ptr(out) if lik else None))
            self.kernel_ms += self.last_kernel_ms()
        return rows

    def sums(self):
        """(pred_sum [N,F,S], resp_sum [N,F,C], n_samples, n_zero)."""
        N, F, S, C, _K, _R = self._with_data()
        pred, resp = np.empty((N, F, S)), np.empty((N, F, C))
        n, zeros = ct.c_int64(0), ct.c_int64(0)
        self._check(self._lib.sbe_predict_read(self._h, _ptr(pred), _ptr(resp), ct.byref(n), ct.byref(zeros)))
        return pred, resp, n.value, zeros.value

    def result(self, lik=None) -> PredictResult:
        pred, resp, n, zeros = self.sums()
        if n == 0:
            raise ValueError("no sample was accumulated")
        return PredictResult(codes=self._codes, pred_sum=pred, resp_sum=resp, n_samples=n, n_zero=zeros, lik=lik,
                             kernel_ms=getattr(self, "kernel_ms", 0.0))


def posterior_predictive(codes, groups, clusters, weights, tables, burnin=0.1, lik=False, device=None, n_groups=None) -> PredictResult:
    """The posterior predictive of T logged samples after burn-in.  codes uint8 [N,F]; groups: uint8 [C-1,N] group indices
    (with n_groups) or a list of bool [G_c,N] assignments; clusters uint8 [T,K,N]; weights [T,F,C]; tables [T,R,F,S]."""
    groups, n_groups, clusters, weights, tables, _u = _samples.after_burnin(groups, clusters, weights, tables, burnin, n_groups)
    h = PredictHandle(device)
    try:
        h.set_data(codes, groups, n_groups, tables.shape[3], clusters.shape[1])
        rows = h.accumulate(clusters, weights, tables, lik=lik)
        return h.result(rows)
    finally:
        h.close()


# ---- the reference's files ------------------------------------------------------------------------------------
def expected_header(feature_names, state_names, confounders, n_clusters):
    """The parameter columns of a stats file by the logger's rule (loggers.py:106-130), in order: the weights per feature
    (areal, then the confounders), every cluster's effect per feature and state, every confounder group's effect.
    confounders: {name: group names}, in the model's order."""
    names = []
    for f in feature_names:
        names.append(f"w_areal_{f}")
        names += [f"w_{conf}_{f}" for conf in confounders]
    for k in range(n_clusters):
        for i_f, f in enumerate(feature_names):
            names += [f"areal_a{k}_{f}_{s}" for s in state_names[i_f]]
    for conf, group_names in confounders.items():
        for g in group_names:
            for i_f, f in enumerate(feature_names):
                names += [f"{conf}_{g}_{f}_{s}" for s in state_names[i_f]]
    return names


def parameters_from_columns(names, rows, feature_names, state_names, confounders):
    """(weights [T,F,C], tables [T,R,F,S]) of a stats file's columns.  The file's parameter columns -- from the first w_areal_
    column on, as many as the header rule gives -- must equal the expected header; ValueError names the first difference."""
    names = [str(n) for n in names]
    sizes = [n for n in names if n.startswith("size_a")]
    K = len(sizes)
    if K == 0:
        raise ValueError("the stats file has no size_a* column: the number of clusters is unknown")
    want = expected_header(feature_names, state_names, confounders, K)
    first = f"w_areal_{feature_names[0]}"
    if first not in names:
        raise ValueError(f"the stats file has no column {first!r}")
    at = names.index(first)
    have = names[at:at + len(want)]
    for j, (a, b) in enumerate(zip(have, want)):
        if a != b:
            raise ValueError(f"column {at + j} of the stats file is {a!r}, the logger's rule gives {b!r}")
    if len(have) < len(want):
        raise ValueError(f"the stats file ends after column {names[-1]!r}, the logger's rule gives {want[len(have)]!r} next")
    rows = np.asarray(rows, dtype=np.float64)
    T, F, C = rows.shape[0], len(feature_names), 1 + len(confounders)
    S = max(len(s) for s in state_names)
    R = K + sum(len(g) for g in confounders.values())
    weights = rows[:, at:at + F * C].reshape(T, F, C)
    tables = np.zeros((T, R, F, S))
    col = at + F * C
    for r in range(R):
        for f in range(F):
            n = len(state_names[f])
            tables[:, r, f, :n] = rows[:, col:col + n]
            col += n
    return np.ascontiguousarray(weights), tables


def read_parameters(stats_path, feature_names, state_names, confounders):
    """(weights [T,F,C], tables [T,R,F,S]) of a stats_K*_*.txt (diag.read_stats reads it)."""
    from . import diag
    names, rows = diag.read_stats(stats_path)
    return parameters_from_columns(names, rows, feature_names, state_names, confounders)


def read_cluster_samples(clusters_path):
    """uint8 [T,K,N] of a clusters_K*_*.txt (diag.read_clusters reads it)."""
    from . import diag
    names, rows = diag.read_clusters(clusters_path)
    K = int(names[-1].split("_")[0][1:]) + 1
    return np.ascontiguousarray(rows.reshape(rows.shape[0], K, -1).astype(np.uint8))


def read_data(features_csv, feature_states_csv, confounder_columns):
    """dict(codes uint8 [N,F], feature_names, state_names, groups uint8 [C-1,N], confounders {name: group names}) of the
    reference's input files: the features and the order of their states come from the feature_states file (one column
    per feature, its states top down, as sbayes/util.py's encode_states numbers them); a confounder is a column of the
    features file with the groups in sorted order, or, without such a column, the one group <ALL> of every object."""
    import pandas as pd
    from . import assoc
    frame = assoc.read_features_csv(features_csv)
    raw = pd.read_csv(features_csv, dtype=str, keep_default_na=False)
    states = pd.read_csv(feature_states_csv, dtype=str, keep_default_na=False)
    states = states.apply(lambda col: col.str.strip())
    feature_names = [str(c) for c in states.columns]
    state_names, N = [], frame.shape[0]
    codes = np.full((N, len(feature_names)), NA, dtype=np.uint8)
    for k, f in enumerate(feature_names):
        if f not in frame.columns:
            raise ValueError(f"feature {f!r} of the feature_states file is no column of the features file")
        own = [s for s in states[f] if s != ""]
        if len(own) > MAX_STATES:
            raise ValueError(f"feature {f!r} has {len(own)} states; the unit takes at most {MAX_STATES}")
        lookup = {s: c for c, s in enumerate(own)}
        for n, v in enumerate(frame[f]):
            if pd.isna(v):
                continue
            if v not in lookup:
                raise ValueError(f"object {n}: {v!r} is no state of feature {f!r}")
            codes[n, k] = lookup[v]
        state_names.append(own)
    groups, confounders = np.full((len(confounder_columns), N), NA, dtype=np.uint8), {}
    for c, name in enumerate(confounder_columns):
        if name not in raw.columns:
            confounders[name] = ["<ALL>"]
            groups[c] = 0
            continue
        column = raw[name].str.strip()
        group_names = sorted(set(v for v in column if v != ""))
        if len(group_names) >= NA:
            raise ValueError(f"confounder {name!r} has {len(group_names)} groups; the unit takes fewer than {NA}")
        lookup = {g: i for i, g in enumerate(group_names)}
        groups[c] = [lookup.get(v, NA) for v in column]
        confounders[name] = group_names
    return dict(codes=codes, feature_names=feature_names, state_names=state_names, groups=groups, confounders=confounders)


def main(argv=None):
    ap = _samples.run_parser("python -m sbayes_amd.predict",
                             "Posterior predictive of an sBayes run's logged samples: imputation of the missing cells, each "
                             "component's responsibility for the observed cells, and ELPD-LOO given the logged effect draws")
    ap.add_argument("--out-imputed", type=Path, default=None, help="write the NA cells with their most probable state")
    ap.add_argument("--out-responsibility", type=Path, default=None, help="write every cell with the components' responsibilities")
    ap.add_argument("--elpd", action="store_true", help="PSIS-LOO over the likelihood rows (given the logged effect draws)")
    args = ap.parse_args(argv)
    data, clusters, weights, tables, n_groups = _samples.read_run(args)
    res = posterior_predictive(data["codes"], data["groups"], clusters, weights, tables, burnin=args.burnin, lik=args.elpd, device=args.device,
                               n_groups=n_groups)
    filled, p = res.impute()
    missing = data["codes"] == NA
    print(f"{res.n_samples} samples, {int(missing.sum())} missing cells imputed (mean probability of the filled state "
          f"{float(p[missing].mean()) if missing.any() else float('nan'):.4f}), {res.n_zero} observed cells of probability 0")
    names = dict(feature_names=data["feature_names"], state_names=data["state_names"], component_names=["areal", *data["confounders"]])
    if args.out_imputed:
        res.write_table(args.out_imputed, na_only=True, **names)
    if args.out_responsibility:
        res.write_table(args.out_responsibility, na_only=False, **names)
    if args.elpd:
        from . import elpd
        store = elpd._Store(res_device(args.device), res.lik.shape[1], res.lik.shape[0])
        try:
            store.append_rows(res.lik)
            loo_i, k_i, lppd_i, _v = store.compute(0, np.ascontiguousarray(missing.ravel()), False)
        finally:
            store.close()
        loo = elpd._loo(loo_i, k_i, lppd_i, res.lik.shape[0])
        print(f"ELPD-LOO given the logged effect draws: {loo.elpd_loo:.4f} (se {loo.se:.4f}, p_loo {loo.p_loo:.4f}, "
              f"{int((loo.pareto_k > loo.good_k).sum())} observations with k > {loo.good_k:.2f})")
    return 0


def res_device(device):
    if device is None:
        from .registry import default_device
        return default_device()
    return int(device)


if __name__ == "__main__":
    raise SystemExit(main())
