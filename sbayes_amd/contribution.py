"""Per-cluster evidence from the logged samples on the device (include/sbe_contrib.h): which features carry cluster k, how
strongly each member belongs, and which non-members would fit.

The posterior predictive (sbayes_amd/predict.py) and its check (sbayes_amd/ppc.py) evaluate the mixture row of a cell under the
membership a sample logged.  This module evaluates the counterfactual rows of the same cell: the object placed in cluster k,
for every k, and in no cluster at all -- the quantity AlterCluster.compute_cluster_posterior evaluates inside the sampler
(sbayes/sampling/operators.py), here after the fact, in log space.  For every logged sample t, cluster k and cell (n, f) with a
code x:  d[t,k,n,f] = log m_k[x] - log m0[x], the log-likelihood ratio of "n in cluster k" against "n in no cluster".

    res = cluster_contribution(codes, groups, clusters, weights, tables, burnin=0.1)
    res.affinity [T,K,N]      sum over f of d, for every object, member or not
    res.gain_feature [T,K,F]  sum over the members of k in sample t of d: what cluster k buys on feature f
    res.gain [T,K]            its sum over the features: the likelihood part of the reference's lh_a<k> column
    res.member [T,K,N]        bool;  res.n_skipped
    res.rank(), res.feature_table(k), res.top_features(k), res.membership_table(), res.write_tables(dir)
    h = ContributionHandle(); h.set_data(...); h.evaluate(clusters, weights, tables); h.result()
    python -m sbayes_amd.contribution FEATURES FEATURE_STATES STATS CLUSTERS --confounders universal family --out DIR

Two caveats.  Labels must be aligned first (sbayes_amd/align.py) for means over samples to refer to one cluster: this module
takes the labels as they are logged.  And a member's affinity is OPTIMISTIC: the cluster's effect draw was fitted with that
member's data, so the data are used twice, as in the posterior predictive check; a non-member's affinity has no such bias.

Numerical contract (tests/_contrib_oracle.py restates it in fp64; DESIGN.md section 24 states it): the row arithmetic is the
posterior predictive's, so m_k of a member is its m[x] bit for bit; the sums run in trees the shape alone fixes, so every output
is bit-identical from call to call, for every tile, and however the samples are split across calls.  Samples are validated on
the device before anything is written (EngineError, code SBE_ERR_DATA = 4, naming the first offender).  The limits are the
posterior predictive's; one call holds at most 256 MiB on the device and evaluate() splits longer blocks.

There is no CPU fallback: without the library or a GPU the functions raise.  Handles follow the package's process model
(sbayes_amd/_proc.py): never pickled, forgotten (not destroyed) in a fork()ed child."""
from __future__ import annotations

import ctypes as ct
import math
from dataclasses import dataclass
from pathlib import Path

import numpy as np

from . import _handle, _samples, predict
from ._handle import _ptr, c_handle_p
from .predict import NA

ABI_VERSION = 1                              # SBE_CONTRIB_ABI_VERSION of include/sbe_contrib.h
MAX_STAGE_BYTES = predict.MAX_STAGE_BYTES    # SBE_CONTRIB_MAX_STAGE_BYTES
MAX_TILE = predict.MAX_TILE                  # SBE_CONTRIB_MAX_TILE

# name -> (restype, argtypes); mirrors include/sbe_contrib.h one to one
PROTOTYPES = {
    **_handle.unit_prototypes("sbe_contrib"),
    "sbe_contrib_create": (ct.c_int, [ct.POINTER(c_handle_p), ct.c_int]),
    "sbe_contrib_sample_bytes": (ct.c_int64, [ct.c_int64, ct.c_int64, ct.c_int, ct.c_int, ct.c_int, ct.c_int]),
    "sbe_contrib_set_data": (ct.c_int, [c_handle_p, ct.c_int64, ct.c_int64, ct.c_int, ct.c_int, ct.c_int, ct.c_void_p, ct.c_void_p, ct.c_void_p]),
    "sbe_contrib_evaluate": (ct.c_int, [c_handle_p, ct.c_int64, ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_void_p,
                                        ct.POINTER(ct.c_int64)]),
    "sbe_contrib_set_feature_tile": (ct.c_int, [c_handle_p, ct.c_int]),
}


def load():
    """The engine library with the prototypes of include/sbe_contrib.h attached."""
    return _handle.bind("sbe_contrib", PROTOTYPES, ABI_VERSION)


def sample_bytes(n_objects, n_features, n_states, n_components, n_clusters, n_rows) -> int:
    """Device bytes one sample of an evaluate call takes while the call runs (sbe_contrib_sample_bytes)."""
    n, f, k = int(n_objects), int(n_features), int(n_clusters)
    return predict.sample_bytes(n, f, n_states, n_components, k, n_rows) + 8 * k * n * f + 8 * k * (n + f)


@dataclass
class ContributionResult:
    """affinity [T,K,N]: per sample the log-likelihood ratio of every object in cluster k against in no cluster; gain_feature
    [T,K,F]: per sample the sum of that ratio's feature term over the cluster's members; member bool [T,K,N]; n_skipped: the
    (sample, cluster, cell) entries that had no ratio (no confounder applies, or m_k = 0)."""
    affinity: np.ndarray
    gain_feature: np.ndarray
    member: np.ndarray
    n_samples: int
    n_skipped: int
    kernel_ms: float = 0.0

    @property
    def gain(self):
        """[T,K]: the sum of gain_feature over the features, exactly rounded (math.fsum), so its order does not matter."""
        T, K, _F = self.gain_feature.shape
        return np.array([[math.fsum(self.gain_feature[t, k]) for k in range(K)] for t in range(T)]).reshape(T, K)   # (+inf stays +inf)

    @property
    def mean_gain(self):
        """[K]: the mean of gain over the samples."""
        return self.gain.mean(axis=0)

    def rank(self):
        """The clusters by mean gain over the samples, descending, ties to the lower index: the reference's rank_clusters rule
        on the likelihood part."""
        mean = self.mean_gain
        return sorted(range(mean.shape[0]), key=lambda k: (-mean[k], k))

    def _cluster(self, k):
        k = int(k)
        if not 0 <= k < self.gain_feature.shape[1]:
            raise ValueError(f"cluster {k} out of range [0, {self.gain_feature.shape[1]})")
        return k

    def feature_table(self, k, names=None):
        """(header, rows) of cluster k per feature: the mean and the sd over the samples of gain_feature, and the share of
        samples in which it is positive; sorted by the mean, descending, ties in index order."""
        k = self._cluster(k)
        g = self.gain_feature[:, k]
        F = g.shape[1]
        names = list(names) if names is not None else [f"F{i + 1}" for i in range(F)]
        if len(names) != F:
            raise ValueError(f"{len(names)} names for {F} features")
        with np.errstate(invalid="ignore"):
            mean, sd, share = g.mean(axis=0), g.std(axis=0), (g > 0).mean(axis=0)
        order = sorted(range(F), key=lambda i: (-mean[i], i))
        return ["feature", "gain_mean", "gain_sd", "share_positive"], [[str(names[i]), float(mean[i]), float(sd[i]), float(share[i])] for i in order]

    def top_features(self, k, n=10, names=None):
        """The first n rows of feature_table(k)."""
        return self.feature_table(k, names)[1][:int(n)]

    def membership_table(self, names=None):
        """(header, rows) per (cluster, object), in index order: the share of samples in which the object is a member, the
        mean affinity, and the share of samples with affinity > 0."""
        _T, K, N = self.affinity.shape
        names = list(names) if names is not None else [str(i) for i in range(N)]
        if len(names) != N:
            raise ValueError(f"{len(names)} names for {N} objects")
        with np.errstate(invalid="ignore"):
            share, mean, positive = self.member.mean(axis=0), self.affinity.mean(axis=0), (self.affinity > 0).mean(axis=0)
        rows = [[k, str(names[n]), float(share[k, n]), float(mean[k, n]), float(positive[k, n])] for k in range(K) for n in range(N)]
        return ["cluster", "object", "member_share", "affinity_mean", "share_affinity_positive"], rows

    def cluster_table(self):
        """(header, rows) per cluster in rank() order: the mean and the sd of gain over the samples, the mean size."""
        gain = self.gain
        size = self.member.sum(axis=2).mean(axis=0)
        with np.errstate(invalid="ignore"):
            rows = [[k, float(gain[:, k].mean()), float(gain[:, k].std()), float(size[k])] for k in self.rank()]
        return ["cluster", "gain_mean", "gain_sd", "size_mean"], rows

    def write_tables(self, directory, feature_names=None, object_names=None):
        """clusters.tsv, membership.tsv and features_a<k>.tsv per cluster into `directory` (created); returns the paths."""
        directory = Path(directory)
        directory.mkdir(parents=True, exist_ok=True)
        paths = [directory / "clusters.tsv", directory / "membership.tsv"]
        _samples.write_tsv(paths[0], *self.cluster_table())
        _samples.write_tsv(paths[1], *self.membership_table(object_names))
        for k in range(self.gain_feature.shape[1]):
            paths.append(directory / f"features_a{k}.tsv")
            _samples.write_tsv(paths[-1], *self.feature_table(k, feature_names))
        return paths


class ContributionHandle(_samples.SampleHandle):
    """Owner of one sbe_contrib handle: the data on one device.  evaluate() appends the rows of its samples; result() returns
    them.  last_kernel_ms(): the kernels of the last library call of evaluate()."""
    _prefix, _noun = "sbe_contrib", "a cluster contribution handle"

    def _clear(self):
        self._rows = {"affinity": [], "gain_feature": [], "member": []}
        self.n_samples, self.n_skipped, self.kernel_ms, self.n_calls = 0, 0, 0.0, 0

    def reset(self):
        """Forget the rows of the samples evaluated so far, keep the data."""
        self._with_data()
        self._clear()

    def max_samples(self) -> int:
        """The samples one library call holds."""
        return MAX_STAGE_BYTES // sample_bytes(*self._with_data())

    def evaluate(self, clusters, weights, tables):
        """Evaluate samples: clusters uint8 [T,K,N] of 0 / 1, weights float64 [T,F,C], tables float64 [T,R,F,S].  Blocks beyond
        max_samples() go in several library calls; each call validates its samples before it writes anything, so an
        EngineError leaves the rows of the calls before it appended."""
        _T, blocks = self._blocks(clusters, weights, tables)
        N, F, _S, _C, K, _R = self.shape
        self.kernel_ms = 0.0
        for _t0, cl, w, tb in blocks:
            n = cl.shape[0]
            affinity, gain = np.empty((n, K, N)), np.empty((n, K, F))
            skipped = ct.c_int64(0)
            self._check(self._lib.sbe_contrib_evaluate(self._h, n, _ptr(cl), _ptr(w), _ptr(tb), _ptr(affinity), _ptr(gain), ct.byref(skipped)))
            self.kernel_ms += self.last_kernel_ms()
            self._rows["affinity"].append(affinity)
            self._rows["gain_feature"].append(gain)
            self._rows["member"].append(cl != 0)
            self.n_samples += n
            self.n_skipped += skipped.value
            self.n_calls += 1

    def result(self) -> ContributionResult:
        self._with_data()
        if self.n_samples == 0:
            raise ValueError("no sample was evaluated")
        return ContributionResult(affinity=np.concatenate(self._rows["affinity"]), gain_feature=np.concatenate(self._rows["gain_feature"]),
                                  member=np.concatenate(self._rows["member"]), n_samples=self.n_samples, n_skipped=self.n_skipped,
                                  kernel_ms=self.kernel_ms)


def cluster_contribution(codes, groups, clusters, weights, tables, burnin=0.1, n_groups=None, device=None) -> ContributionResult:
    """The per-cluster evidence of T logged samples after burn-in.  codes uint8 [N,F]; groups: uint8 [C-1,N] group indices (with
    n_groups) or a list of bool [G_c,N] assignments; clusters uint8 [T,K,N]; weights [T,F,C]; tables [T,R,F,S].  The labels are
    taken as logged (align them first), and a member's affinity is optimistic (its data shaped the cluster's effect draw)."""
    groups, n_groups, clusters, weights, tables, _u = _samples.after_burnin(groups, clusters, weights, tables, burnin, n_groups)
    h = ContributionHandle(device)
    try:
        h.set_data(codes, groups, n_groups, tables.shape[3], clusters.shape[1])
        h.evaluate(clusters, weights, tables)
        return h.result()
    finally:
        h.close()


def main(argv=None):
    ap = _samples.run_parser("python -m sbayes_amd.contribution",
                             "Per-cluster evidence of an sBayes run's logged samples: the likelihood gain of every cluster per "
                             "feature, and every object's affinity to every cluster (labels as logged: align them first; a "
                             "member's affinity is optimistic)")
    ap.add_argument("--out", type=Path, default=None, help="directory for clusters.tsv, membership.tsv and features_a<k>.tsv")
    args = ap.parse_args(argv)
    data, clusters, weights, tables, n_groups = _samples.read_run(args)
    res = cluster_contribution(data["codes"], data["groups"], clusters, weights, tables, burnin=args.burnin, n_groups=n_groups, device=args.device)
    print(f"{res.n_samples} samples, {res.gain_feature.shape[1]} clusters (labels as logged), {res.n_skipped} entries skipped")
    for k, mean, sd, size in res.cluster_table()[1]:
        top = ", ".join(f"{name} {gain:.3f}" for name, gain, _sd, _share in res.top_features(k, 3, data["feature_names"]))
        print(f"  a{k}\tgain {mean:.4f} (sd {sd:.4f})\tmean size {size:.1f}\ttop features: {top}")
    if args.out:
        res.write_tables(args.out, data["feature_names"])
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
