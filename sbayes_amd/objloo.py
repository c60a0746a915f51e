"""Leave-one-object-out ELPD with the cluster membership integrated out, on the device (include/sbe_objloo.h): had this object
(a language, a site) not been documented at all, how well would the fitted model have predicted it, and what would it have
predicted for each of its cells?

elpd.psis_loo and loopred.loo_predictive score one observed cell at a time, and every score is conditional on the object's
logged cluster membership, a per-object latent variable fitted to the very cells being scored.  For comparing numbers of
clusters, or for asking how well the model predicts a new object, the unit is the object with its membership integrated out
(Merkle, Furr & Rabe-Hesketh 2019; the integrated importance sampling of Vehtari et al. 2016).  Per logged sample t and object n
this module forms

    L[t, n] = log sum_j prior[t, n, j] exp(H[t, n, j]),     H[t, n, j] = sum_f log m_j[n, f, x]

over the hypotheses j = 0 ("in no cluster") and j = 1 .. K ("in cluster j - 1"), with contribution's counterfactual rows m0 and
m_k, runs PSIS per object over the T values of L (and, for comparison, over the conditional Cnd = H[z], z the logged membership),
keeps the marginal weights and runs the samples past them a second time:

    res = object_loo(codes, groups, clusters, weights, tables, prior=None, burnin=0.1)
    res.loo_i, res.k_i, res.n_eff, res.lppd_i      [N]: the marginal column; loo_i is a float64 vector, compare takes it as it is
    res.loo_cond_i, res.k_cond_i, res.lppd_cond_i  [N]: the same objects, conditional on the logged membership
    res.membership [N, K+1]                        the Rao-Blackwellised membership probabilities, the mean of p(z_n = j | x_n, ..)
    res.p_loo [N, F, S]                            what the model predicts for every cell of an undocumented object (or None)
    res.elpd, res.se, res.p_eff, res.n_bad_k(0.7), res.accuracy(by), res.brier(by), res.log_score(by), res.table()
    h = ObjLooHandle(); h.set_data(..., capacity=T); h.add(...); h.weights(); h.accumulate(...); h.result()
    python -m sbayes_amd.objloo FEATURES FEATURE_STATES STATS CLUSTERS --confounders universal family --out DIR [--prior FILE.npy]

Caveats.  Everything is CONDITIONAL ON THE LOGGED EFFECT DRAWS, as in predict: leaving an object out removes its influence on the
weighting of the samples, not on a draw already made.  THE PRIOR MUST BE THE MODEL'S CONDITIONAL PRIOR OF THE MEMBERSHIP: the
probability, given the other objects' memberships in the sample, of "no cluster" (column 0) and of each cluster (columns 1 .. K).
Under the uniform area prior (`uniform_area`) that is uniform, the default; otherwise it is the caller's to build, for example
from geo.costs_per_object.  LABELS MUST BE ALIGNED (align) for the columns 1 .. K of `membership` to mean one cluster each; the
scores do not depend on the labels.  PARETO K HAS TO BE READ: with few samples many objects have k > 0.7; they are counted
and flagged, not refitted, and their weights are unreliable.

Numerical contract (tests/_objloo_oracle.py restates it in fp64; DESIGN.md section 32 states it): the rows are contribution's
bit for bit, H is summed in ppc's per-object tree, PSIS is elpd's on the float64 columns with ties in sample order, and a cell's
sums add the rounded products w_t mz_t[s] in sample order, so they are bit-identical however the samples are split across calls.
An observed cell to which no confounder applies, a prior row that is not a distribution and an object of zero likelihood are an
EngineError (SBE_ERR_DATA = 4) naming the offender.  Limits: predict's, 2 .. 2^20 samples, 16 GiB of store on the device
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
from .loopred import _group
from .predict import NA

ABI_VERSION = 1                          # SBE_OBJLOO_ABI_VERSION of include/sbe_objloo.h
MIN_SAMPLES = 2                          # SBE_ELPD_MIN_SAMPLES
MAX_SAMPLES = 1 << 20                    # SBE_OBJLOO_MAX_SAMPLES
MAX_STORE_BYTES = 1 << 34                # SBE_OBJLOO_MAX_STORE_BYTES
MAX_STAGE_BYTES = predict.MAX_STAGE_BYTES   # SBE_OBJLOO_MAX_STAGE_BYTES
MAX_TILE = predict.MAX_TILE              # SBE_OBJLOO_MAX_TILE
SUM_TOL = _samples.SUM_TOL               # SBE_PREDICT_SUM_TOL: how far a prior row's sum may be from 1

# name -> (restype, argtypes); mirrors include/sbe_objloo.h one to one
PROTOTYPES = {
    **_handle.unit_prototypes("sbe_objloo"),
    "sbe_objloo_create": (ct.c_int, [ct.POINTER(c_handle_p), ct.c_int]),
    "sbe_objloo_store_bytes": (ct.c_int64, [ct.c_int64, ct.c_int, ct.c_int64]),
    "sbe_objloo_sample_bytes": (ct.c_int64, [ct.c_int64, ct.c_int64, ct.c_int, ct.c_int, ct.c_int, ct.c_int]),
    "sbe_objloo_lds_max_samples": (ct.c_int64, []),
    "sbe_objloo_set_data": (ct.c_int, [c_handle_p, ct.c_int64, ct.c_int64, ct.c_int, ct.c_int, ct.c_int, ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_int64]),
    "sbe_objloo_reset": (ct.c_int, [c_handle_p]),
    "sbe_objloo_add": (ct.c_int, [c_handle_p, ct.c_int64, ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_void_p]),
    "sbe_objloo_weights": (ct.c_int, [c_handle_p] + [ct.c_void_p] * 8),
    "sbe_objloo_accumulate": (ct.c_int, [c_handle_p, ct.c_int64, ct.c_int64, ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_void_p]),
    "sbe_objloo_read": (ct.c_int, [c_handle_p, ct.c_void_p, ct.POINTER(ct.c_int64)]),
    "sbe_objloo_set_feature_tile": (ct.c_int, [c_handle_p, ct.c_int]),
    "sbe_objloo_get_store": (ct.c_int, [c_handle_p, ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_void_p]),
}
POINTWISE = ("loo_i", "k_i", "n_eff", "lppd_i", "loo_cond_i", "k_cond_i", "lppd_cond_i")


def load():
    """The engine library with the prototypes of include/sbe_objloo.h attached."""
    return _handle.bind("sbe_objloo", PROTOTYPES, ABI_VERSION)


def store_bytes(n_objects, n_clusters, capacity) -> int:
    """Device bytes of the store of n_objects objects, n_clusters clusters and `capacity` samples (sbe_objloo_store_bytes): H and
    a per hypothesis, L, Cnd and w, float64 each."""
    return int(n_objects) * int(capacity) * 8 * (2 * (int(n_clusters) + 1) + 3)


def sample_bytes(n_objects, n_features, n_states, n_components, n_clusters, n_rows) -> int:
    """Device bytes one sample of an add or accumulate call takes while the call runs (sbe_objloo_sample_bytes): predict's, the log
    of every (hypothesis, cell), its sums over the features and the prior."""
    hyp = n_clusters + 1
    return predict.sample_bytes(n_objects, n_features, n_states, n_components, n_clusters, n_rows, False) + 8 * hyp * n_objects * n_features + 16 * hyp * n_objects


def lds_max_samples() -> int:
    """Largest T whose sort keys the weights kernel holds in LDS; longer columns are sorted in global memory."""
    return int(load().sbe_objloo_lds_max_samples())


def broadcast_prior(prior, T, N, K):
    """None, or float64 [T, N, K+1] contiguous, from None, [K+1], [N, K+1] or [T, N, K+1]; the rows are checked here too (the
    device checks them again and names the first offender)."""
    if prior is None:
        return None
    p = np.asarray(prior, dtype=np.float64)
    want = {1: (K + 1,), 2: (N, K + 1), 3: (T, N, K + 1)}.get(p.ndim)
    if want is None or p.shape != want:
        raise ValueError(f"prior must be None, [{K + 1}], [{N}, {K + 1}] or [{T}, {N}, {K + 1}] (no cluster, then the {K} clusters), got shape {p.shape}")
    return np.ascontiguousarray(np.broadcast_to(p, (T, N, K + 1)))


@dataclass
class ObjLooResult:
    """The pointwise vectors [N] of the marginal column (loo_i, k_i, n_eff, lppd_i) and of the conditional one (loo_cond_i,
    k_cond_i, lppd_cond_i), membership [N, K+1], p_loo [N, F, S] or None.  Conditional on the logged effect draws (the module's
    docstring)."""
    codes: np.ndarray
    loo_i: np.ndarray
    k_i: np.ndarray
    n_eff: np.ndarray
    lppd_i: np.ndarray
    loo_cond_i: np.ndarray
    k_cond_i: np.ndarray
    lppd_cond_i: np.ndarray
    membership: np.ndarray
    p_loo: np.ndarray | None
    n_samples: int
    kernel_ms: dict | None = None

    @property
    def observed(self):
        return self.codes != NA

    @property
    def elpd(self) -> float:
        """The sum of loo_i over the objects."""
        return float(np.sum(self.loo_i))

    @property
    def elpd_cond(self) -> float:
        return float(np.sum(self.loo_cond_i))

    @property
    def se(self) -> float:
        """sqrt(N var(loo_i)): over N objects, not N F cells."""
        return float((self.loo_i.size * np.var(self.loo_i)) ** 0.5)

    @property
    def p_eff(self) -> float:
        """sum(lppd_i) - sum(loo_i): the effective number of parameters."""
        return float(np.sum(self.lppd_i) - np.sum(self.loo_i))

    def n_bad_k(self, threshold=0.7, conditional=False) -> int:
        """The objects whose Pareto k exceeds `threshold` (or is NaN): their weights are unreliable."""
        k = self.k_cond_i if conditional else self.k_i
        return int((~(k <= threshold)).sum())

    def _probs(self):
        if self.p_loo is None:
            raise ValueError("no predictive (object_loo(.., predictive=False)): the zero-shot scores need the second pass")
        return self.p_loo

    @property
    def predicted(self):
        """int [N,F]: the most probable state of every cell, the lowest on ties."""
        return self._probs().argmax(axis=2)

    @property
    def p_obs(self):
        """[N,F]: the zero-shot probability of the observed state (NaN at cells without a code)."""
        x = np.where(self.observed, self.codes, 0).astype(np.int64)[..., None]
        return np.where(self.observed, np.take_along_axis(self._probs(), x, axis=2)[..., 0], np.nan)

    def accuracy(self, by=None):
        """The share of observed cells whose observed state is the predicted one: in all, or by="feature" / "object"."""
        return _group((self.predicted == self.codes).astype(np.float64), by, self.observed)

    def brier(self, by=None):
        """The mean over observed cells of sum_s (p_loo[s] - [s == x])^2."""
        p = self._probs()
        onehot = np.arange(p.shape[2])[None, None, :] == self.codes[..., None]
        return _group(np.where(self.observed[..., None], (p - onehot) ** 2, 0.0).sum(axis=2), by, self.observed)

    def log_score(self, by=None):
        """The mean over observed cells of log p_loo[x] (per cell; loo_i scores the object's cells jointly)."""
        with np.errstate(divide="ignore", invalid="ignore"):
            return _group(np.log(self.p_obs), by, self.observed)

    def table(self, object_names=None):
        """(header, rows): one row per object: its cells with a code, loo_i, k, n_eff, lppd_i, the conditional three, the most
        probable membership (0: no cluster) with its probability and, with a predictive, its zero-shot accuracy and log score."""
        N = self.loo_i.size
        names = list(object_names) if object_names is not None else list(range(N))
        best = self.membership.argmax(axis=1)
        header = ["object", "n_observed", "loo_i", "k", "n_eff", "lppd_i", "loo_cond_i", "k_cond", "lppd_cond_i", "membership", "p_membership"]
        rows = [[names[n], int(self.observed[n].sum()), float(self.loo_i[n]), float(self.k_i[n]), float(self.n_eff[n]), float(self.lppd_i[n]),
                 float(self.loo_cond_i[n]), float(self.k_cond_i[n]), float(self.lppd_cond_i[n]), int(best[n]), float(self.membership[n, best[n]])]
                for n in range(N)]
        if self.p_loo is not None:
            acc, score = self.accuracy("object"), self.log_score("object")
            header += ["accuracy", "log_score"]
            rows = [row + [float(acc[n]), float(score[n])] for n, row in enumerate(rows)]
        return header, rows

    def summary_table(self):
        """(header, rows): the totals, one row per column (marginal, conditional)."""
        N = self.loo_i.size
        header = ["column", "n_objects", "n_samples", "elpd", "se", "p_eff", "n_bad_k"]
        cond_se = float((N * np.var(self.loo_cond_i)) ** 0.5)
        rows = [["marginal", N, self.n_samples, self.elpd, self.se, self.p_eff, self.n_bad_k()],
                ["conditional", N, self.n_samples, self.elpd_cond, cond_se, float(np.sum(self.lppd_cond_i) - np.sum(self.loo_cond_i)),
                 self.n_bad_k(conditional=True)]]
        return header, rows

    def write_tables(self, out_dir, object_names=None):
        """object_loo.tsv and object_loo_summary.tsv in out_dir; returns the paths."""
        out_dir = Path(out_dir)
        out_dir.mkdir(parents=True, exist_ok=True)
        paths = []
        for name, table in (("object_loo.tsv", self.table(object_names)), ("object_loo_summary.tsv", self.summary_table())):
            _samples.write_tsv(out_dir / name, *table)
            paths.append(out_dir / name)
        return paths


def result_from(codes, pointwise, membership, p_loo, n_samples, kernel_ms=None) -> ObjLooResult:
    """The result of the unit's raw outputs: the seven pointwise vectors [N] in POINTWISE's order, membership [N, K+1], p_loo
    [N,F,S] or None."""
    vectors = {name: np.ascontiguousarray(v, dtype=np.float64) for name, v in zip(POINTWISE, pointwise)}
    return ObjLooResult(codes=np.asarray(codes), membership=np.asarray(membership), p_loo=p_loo, n_samples=int(n_samples), kernel_ms=kernel_ms, **vectors)


class ObjLooHandle(_samples.SampleHandle):
    """Owner of one sbe_objloo handle: the data, the stored rows and weights and the sums on one device.  The phases in order:
    set_data(.., capacity), add(..) any number of times, weights(), accumulate(..) over the same samples and priors again,
    result()."""
    _prefix, _noun = "sbe_objloo", "a leave-one-object-out handle"

    def _clear(self):
        self.n_rows, self.next_t, self._pointwise = 0, 0, None
        self.kernel_ms = dict(add=0.0, weights=0.0, accumulate=0.0)

    def set_data(self, codes, groups, n_groups, n_states, n_clusters, capacity):
        """predict.PredictHandle.set_data's arguments and the number of samples the store takes."""
        capacity, K = int(capacity), int(n_clusters)

        def store(codes):
            if not 1 <= capacity <= MAX_SAMPLES:
                raise ValueError(f"capacity={capacity}; the store takes 1 .. {MAX_SAMPLES} (2^20) samples")
            N = codes.shape[0]
            if store_bytes(N, K, capacity) > MAX_STORE_BYTES:
                raise ValueError(f"the rows and weights of {N} objects x {K + 1} hypotheses x {capacity} samples take {store_bytes(N, K, capacity)} "
                                 f"bytes on the device, the limit is {MAX_STORE_BYTES}")
            return (capacity,)
        self._set_data(codes, groups, n_groups, n_states, n_clusters, store)
        self.capacity = capacity

    def reset(self):
        """Forget the rows, the weights and the sums, keep the data."""
        self._with_data()
        self._check(self._lib.sbe_objloo_reset(self._h))
        self._clear()

    def max_samples(self) -> int:
        """The samples one library call holds."""
        return MAX_STAGE_BYTES // sample_bytes(*self._with_data())

    def _prior_blocks(self, prior, T, blocks):
        N, _F, _S, _C, K, _R = self.shape
        prior = broadcast_prior(prior, T, N, K)
        return [(t0, cl, w, tb, None if prior is None else prior[t0:t0 + cl.shape[0]]) for t0, cl, w, tb in blocks]

    def add(self, clusters, weights, tables, prior=None):
        """Phase 1: store the rows of the samples: clusters uint8 [T,K,N] of 0 / 1, weights float64 [T,F,C], tables float64
        [T,R,F,S], prior None, [K+1], [N,K+1] or [T,N,K+1].  Blocks beyond max_samples() go in several library calls."""
        T, blocks = self._blocks(clusters, weights, tables)
        if self.n_rows + T > self.capacity:
            raise ValueError(f"{self.n_rows} samples stored, {T} more exceed the capacity of {self.capacity}")
        for _t0, cl, w, tb, pr in self._prior_blocks(prior, T, blocks):
            self._check(self._lib.sbe_objloo_add(self._h, cl.shape[0], _ptr(cl), _ptr(w), _ptr(tb), None if pr is None else _ptr(pr)))
            self.n_rows += cl.shape[0]
            self.kernel_ms["add"] += self.last_kernel_ms()
        self._pointwise, self.next_t = None, 0

    def weights(self):
        """Phase 2: PSIS per object over the stored columns; returns (the seven vectors [N] in POINTWISE's order, membership
        [N, K+1])."""
        N, _F, _S, _C, K, _R = self._with_data()
        if self.n_rows < MIN_SAMPLES:
            raise ValueError(f"{self.n_rows} samples stored; PSIS needs at least {MIN_SAMPLES} per object")
        loo_i, k_i, n_eff, lppd_i, loo_cond_i, k_cond_i, lppd_cond_i = (np.empty(N, dtype=np.float64) for _ in range(7))
        membership = np.empty((N, K + 1), dtype=np.float64)
        self._pointwise, self.next_t = None, 0
        self._check(self._lib.sbe_objloo_weights(self._h, _ptr(loo_i), _ptr(k_i), _ptr(n_eff), _ptr(lppd_i), _ptr(loo_cond_i), _ptr(k_cond_i),
                                                 _ptr(lppd_cond_i), _ptr(membership)))
        self.kernel_ms["weights"] = self.last_kernel_ms()
        self.kernel_ms["accumulate"] = 0.0
        self._pointwise = ((loo_i, k_i, n_eff, lppd_i, loo_cond_i, k_cond_i, lppd_cond_i), membership)
        return self._pointwise

    def accumulate(self, clusters, weights, tables, prior=None):
        """Phase 3: the samples of phase 1 again with their priors, in the same order (the next block of them; any split)."""
        if self._pointwise is None:
            self._with_data()
            raise ValueError("no weights yet (weights() comes before accumulate())")
        T, blocks = self._blocks(clusters, weights, tables)
        if self.next_t + T > self.n_rows:
            raise ValueError(f"{self.next_t} of {self.n_rows} samples accumulated, {T} more are too many")
        for _t0, cl, w, tb, pr in self._prior_blocks(prior, T, blocks):
            self._check(self._lib.sbe_objloo_accumulate(self._h, self.next_t, cl.shape[0], _ptr(cl), _ptr(w), _ptr(tb), None if pr is None else _ptr(pr)))
            self.next_t += cl.shape[0]
            self.kernel_ms["accumulate"] += self.last_kernel_ms()

    def sums(self):
        """(p_loo [N,F,S], the samples accumulated)."""
        N, F, S, _C, _K, _R = self._with_data()
        p = np.empty((N, F, S))
        n = ct.c_int64(0)
        self._check(self._lib.sbe_objloo_read(self._h, _ptr(p), ct.byref(n)))
        return p, n.value

    def store(self, with_weights=True):
        """A test read: (H float64 [N, K+1, T], L [N, T], Cnd [N, T], w [N, T] or None), the store's columns."""
        N, _F, _S, _C, K, _R = self._with_data()
        H = np.empty((N, K + 1, self.n_rows))
        L, Cnd = np.empty((N, self.n_rows)), np.empty((N, self.n_rows))
        w = np.empty((N, self.n_rows)) if with_weights else None
        self._check(self._lib.sbe_objloo_get_store(self._h, _ptr(H), _ptr(L), _ptr(Cnd), _ptr(w) if with_weights else None))
        return H, L, Cnd, w

    def result(self, predictive=True) -> ObjLooResult:
        if self._pointwise is None:
            self._with_data()
            raise ValueError("no weights yet (weights() comes before result())")
        p = None
        if predictive:
            p, n = self.sums()
            if n != self.n_rows:
                raise ValueError(f"{n} of {self.n_rows} samples accumulated: the second pass is not complete")
        return result_from(self._codes, *self._pointwise, p, n_samples=self.n_rows, kernel_ms=dict(self.kernel_ms))


def object_loo(codes, groups, clusters, weights, tables, prior=None, burnin=0.1, predictive=True, device=None, n_groups=None) -> ObjLooResult:
    """The leave-one-object-out ELPD of T logged samples after burn-in, in predict.posterior_predictive's argument forms: codes
    uint8 [N,F]; groups: uint8 [C-1,N] group indices (with n_groups) or a list of bool [G_c,N] assignments; clusters uint8 [T,K,N];
    weights [T,F,C]; tables [T,R,F,S]; prior None (uniform), [K+1], [N,K+1] or one row per sample before burn-in [T,N,K+1].
    predictive=False skips the second pass (p_loo is None).  The samples go to the device in blocks of what one call holds."""
    n_before = np.asarray(clusters).shape[0]
    groups, n_groups, clusters, weights, tables, _u = _samples.after_burnin(groups, clusters, weights, tables, burnin, n_groups)
    T, K, N = clusters.shape
    if prior is not None and np.ndim(prior) == 3:
        if np.shape(prior)[0] != n_before:
            raise ValueError(f"{np.shape(prior)[0]} prior blocks for {n_before} samples")
        prior = np.asarray(prior)[n_before - T:]
    prior = broadcast_prior(prior, T, N, K)
    if not MIN_SAMPLES <= T <= MAX_SAMPLES:
        raise ValueError(f"{T} samples after burn-in; PSIS needs {MIN_SAMPLES} .. {MAX_SAMPLES} (2^20) per object")
    h = ObjLooHandle(device)
    try:
        h.set_data(codes, groups, n_groups, tables.shape[3], K, capacity=T)
        h.add(clusters, weights, tables, prior)
        h.weights()
        if predictive:
            h.accumulate(clusters, weights, tables, prior)
        return h.result(predictive)
    finally:
        h.close()


def main(argv=None):
    ap = _samples.run_parser("python -m sbayes_amd.objloo",
                             "Leave-one-object-out ELPD of an sBayes run with the cluster membership integrated out, given the logged effect "
                             "draws: per object the marginal and the conditional score with their Pareto k, the Rao-Blackwellised membership "
                             "and the zero-shot predictive of every cell")
    ap.add_argument("--prior", type=Path, default=None,
                    help="FILE.npy: the conditional prior of the membership, [K+1], [N, K+1] or [T, N, K+1] (no cluster first); default: uniform")
    ap.add_argument("--out", type=Path, default=None, help="directory for object_loo.tsv and object_loo_summary.tsv")
    args = ap.parse_args(argv)
    data, clusters, weights, tables, n_groups = _samples.read_run(args)
    prior = np.load(args.prior) if args.prior is not None else None
    res = object_loo(data["codes"], data["groups"], clusters, weights, tables, prior=prior, burnin=args.burnin, device=args.device, n_groups=n_groups)
    print(f"{res.n_samples} samples, {res.loo_i.size} objects (given the logged effect draws, membership integrated out): elpd {res.elpd:.2f} "
          f"(se {res.se:.2f}), p_eff {res.p_eff:.2f}; conditional on the logged membership: elpd {res.elpd_cond:.2f}")
    print(f"zero-shot accuracy {res.accuracy():.4f}, Brier {res.brier():.4f}, log score {res.log_score():.4f}")
    bad = res.n_bad_k(0.7)
    if bad:
        print(f"warning: {bad} objects with Pareto k > 0.7: their leave-one-out weights are unreliable")
    if args.out:
        res.write_tables(args.out, data.get("object_names"))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
