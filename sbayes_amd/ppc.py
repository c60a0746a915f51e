"""Posterior predictive checks on the device (include/sbe_ppc.h): per logged sample one replicated data set drawn from the
fitted model, and the deviance of the replicate next to the deviance of the data, per feature and per object.

The posterior predictive (sbayes_amd/predict.py) puts the fitted model back on the data as probabilities.  This module asks
whether the data look like what the fitted model would produce.  For every logged sample t and every cell (n, f) that has a
code it draws y_t[n,f] from the cell's mixture row m_t[n,f,.] (the row simulate_features draws from,
sbayes/simulation.py:207-255) and takes the discrepancy d = -2 log m_t[n,f,.] at the drawn and at the observed state:

    res = posterior_predictive_check(codes, groups, clusters, weights, tables, burnin=0.1, seed=0)
    res.p_feature [F]     share of samples whose replicated deviance of the feature exceeds the observed one (ties count half)
    res.p_object [N]      the same per object;  res.p_total: on the sum over everything
    res.p_count [F,S]     the same for the number of objects showing state s of feature f: are the frequencies calibrated?
    res.dev_feature [T,2,F], res.dev_object [T,2,N], res.count_rep [T,F,S], res.count_obs [F,S], res.y_rep [T,N,F] or None
    res.table("feature"), res.write_table(path, "object")
    h = PpcHandle(); h.set_data(...); h.check(clusters, weights, tables, seed=1); h.result()
    python -m sbayes_amd.ppc FEATURES FEATURE_STATES STATS CLUSTERS --confounders universal family

A small p says that the model reproduces that feature (object) worse than its own replicates: a candidate for removal or
recoding, next to the chi-squared screening (sbayes_amd/assoc.py).  These p-values condition on the logged effect draws and
use the data twice; they are CONSERVATIVE: under a true model they concentrate around 1/2 more than a uniform variable would,
so a small one is stronger evidence than its size says, and a moderate one is no proof of fit.

Numerical contract (tests/_ppc_oracle.py restates it in fp64; DESIGN.md section 22 states it): the row arithmetic is the
posterior predictive's; the uniform of a cell is Philox4x32-10 under (seed, draw index, n F + f), or the caller's; the sums
run in trees the shape alone fixes, so every output is bit-identical from call to call, for every tile, and however the
samples are split across calls (the handle passes the samples it has checked so far as the first draw index).  Samples are
validated on the device before anything is written (EngineError, code SBE_ERR_DATA = 4, naming the first offender).  The
limits are the posterior predictive's; one call holds at most 256 MiB on the device and check() splits longer blocks.

There is no CPU fallback: without the library or a GPU the functions raise.  Handles follow the package's process model
(sbayes_amd/_proc.py): never pickled, forgotten (not destroyed) in a fork()ed child."""
from __future__ import annotations

import ctypes as ct
from dataclasses import dataclass
from pathlib import Path

import numpy as np

from . import _handle, _samples, predict
from ._handle import _ptr, c_handle_p
from .predict import NA

ABI_VERSION = 1                              # SBE_PPC_ABI_VERSION of include/sbe_ppc.h
MAX_STAGE_BYTES = predict.MAX_STAGE_BYTES    # SBE_PPC_MAX_STAGE_BYTES
MAX_TILE = predict.MAX_TILE                  # SBE_PPC_MAX_TILE

# name -> (restype, argtypes); mirrors include/sbe_ppc.h one to one
PROTOTYPES = {
    **_handle.unit_prototypes("sbe_ppc"),
    "sbe_ppc_create": (ct.c_int, [ct.POINTER(c_handle_p), ct.c_int]),
    "sbe_ppc_sample_bytes": (ct.c_int64, [ct.c_int64, ct.c_int64, ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_int]),
    "sbe_ppc_set_data": (ct.c_int, [c_handle_p, ct.c_int64, ct.c_int64, ct.c_int, ct.c_int, ct.c_int, ct.c_void_p, ct.c_void_p, ct.c_void_p]),
    "sbe_ppc_check": (ct.c_int, [c_handle_p, ct.c_int64, ct.c_int64, ct.c_uint64, ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_void_p,
                                 ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.POINTER(ct.c_int64)]),
    "sbe_ppc_set_feature_tile": (ct.c_int, [c_handle_p, ct.c_int]),
}


def load():
    """The engine library with the prototypes of include/sbe_ppc.h attached."""
    return _handle.bind("sbe_ppc", PROTOTYPES, ABI_VERSION)


def sample_bytes(n_objects, n_features, n_states, n_components, n_clusters, n_rows, with_y_rep=False, with_uniforms=False) -> int:
    """Device bytes one sample of a check call takes while the call runs (sbe_ppc_sample_bytes)."""
    n, f = int(n_objects), int(n_features)
    return (predict.sample_bytes(n, f, n_states, n_components, n_clusters, n_rows) + 16 * n * f + 16 * f + 16 * n + 4 * f * int(n_states) +
            (n * f if with_y_rep else 0) + (8 * n * f if with_uniforms else 0))


def p_value(rep, obs):
    """(#{rep > obs} + #{rep == obs} / 2) / T over the first axis; +inf equals +inf."""
    rep, obs = np.asarray(rep), np.asarray(obs)
    return ((rep > obs).sum(axis=0) + 0.5 * (rep == obs).sum(axis=0)) / rep.shape[0]


@dataclass
class PpcResult:
    """dev_feature [T,2,F] and dev_object [T,2,N]: per sample the observed (index 0) and the replicated (index 1) deviance sums;
    count_rep [T,F,S]: the objects that drew state s; count_obs [F,S]: the objects that show it; y_rep uint8 [T,N,F] or None;
    n_skipped: the (sample, cell) pairs whose mixture row had no mass."""
    codes: np.ndarray
    dev_feature: np.ndarray
    dev_object: np.ndarray
    count_rep: np.ndarray
    count_obs: np.ndarray
    n_samples: int
    n_skipped: int
    y_rep: np.ndarray | None = None
    kernel_ms: float = 0.0

    @property
    def p_feature(self):
        return p_value(self.dev_feature[:, 1], self.dev_feature[:, 0])

    @property
    def p_object(self):
        return p_value(self.dev_object[:, 1], self.dev_object[:, 0])

    @property
    def p_total(self):
        total = self.dev_feature.sum(axis=2)
        return float(p_value(total[:, 1], total[:, 0]))

    @property
    def p_count(self):
        return p_value(self.count_rep, self.count_obs[None])

    @property
    def mean_feature(self):
        """[2,F]: the mean over the samples of the observed and of the replicated deviance."""
        return self.dev_feature.mean(axis=0)

    @property
    def mean_object(self):
        return self.dev_object.mean(axis=0)

    @property
    def n_cells_feature(self):
        return (self.codes != NA).sum(axis=0)

    @property
    def n_cells_object(self):
        return (self.codes != NA).sum(axis=1)

    def table(self, kind="feature", names=None):
        """(header, rows) per feature or per object, in index order: the cells with a code, the mean observed and replicated
        deviance, p, and a flag: `no cells` (p = 0.5 by the tie rule, it says nothing) or `p < 0.05`."""
        if kind not in ("feature", "object"):
            raise ValueError(f"kind={kind!r} must be 'feature' or 'object'")
        feature = kind == "feature"
        p, mean = (self.p_feature, self.mean_feature) if feature else (self.p_object, self.mean_object)
        cells = self.n_cells_feature if feature else self.n_cells_object
        names = list(names) if names is not None else [f"F{i + 1}" if feature else str(i) for i in range(p.shape[0])]
        if len(names) != p.shape[0]:
            raise ValueError(f"{len(names)} names for {p.shape[0]} {kind}s")
        rows = [[str(names[i]), int(cells[i]), float(mean[0, i]), float(mean[1, i]), float(p[i]),
                 "no cells" if cells[i] == 0 else ("p < 0.05" if p[i] < 0.05 else "")] for i in range(p.shape[0])]
        return [kind, "n_cells", "deviance_observed", "deviance_replicated", "p", "flag"], rows

    def worst(self, kind="feature", names=None, k=5):
        """The k rows of table(kind) with the smallest p among those that have cells, ties in index order."""
        _header, rows = self.table(kind, names)
        return sorted((r for r in rows if r[1] > 0), key=lambda r: r[4])[:k]

    def write_table(self, path, kind="feature", names=None):
        _samples.write_tsv(path, *self.table(kind, names))


def count_observed(codes, n_states):
    """int64 [F,S]: the objects that show state s of feature f."""
    codes = np.asarray(codes)
    return np.stack([(codes == s).sum(axis=0) for s in range(int(n_states))], axis=1).astype(np.int64)


class PpcHandle(_samples.SampleHandle):
    """Owner of one sbe_ppc handle: the data on one device.  check() appends the rows of its samples; result() returns them.
    last_kernel_ms(): the kernels of the last library call of check()."""
    _prefix, _noun = "sbe_ppc", "a posterior predictive check handle"

    def _clear(self):
        self._rows = {"dev_feature": [], "dev_object": [], "count_rep": [], "y_rep": []}
        self.n_samples, self.n_skipped, self.kernel_ms = 0, 0, 0.0

    def reset(self):
        """Forget the rows of the samples checked so far (the next sample has draw index 0 again), keep the data."""
        self._with_data()
        self._clear()

    def max_samples(self, replicates=False, uniforms=False) -> int:
        """The samples one library call holds."""
        return MAX_STAGE_BYTES // sample_bytes(*self._with_data(), replicates, uniforms)

    def check(self, clusters, weights, tables, seed=0, uniforms=None, replicates=False):
        """Check samples: clusters uint8 [T,K,N] of 0 / 1, weights float64 [T,F,C], tables float64 [T,R,F,S]; uniforms: None
        (Philox under `seed`, the draw index continues from the samples checked so far) or float64 [T, N F] in [0, 1);
        replicates: keep y_rep.  Blocks beyond max_samples() go in several library calls; each call validates its samples
        before it writes anything, so an EngineError leaves the rows of the calls before it appended."""
        T, blocks = self._blocks(clusters, weights, tables, replicates, uniforms is not None)
        N, F, S = self.shape[:3]
        seed = int(seed)
        if not 0 <= seed < 1 << 64:
            raise ValueError(f"seed={seed} must lie in [0, 2^64)")
        if uniforms is not None:
            uniforms = np.asarray(uniforms)
            if uniforms.dtype != np.float64:
                raise ValueError(f"uniforms must be float64, got {uniforms.dtype}")
            if uniforms.shape not in ((T, N * F), (T, N, F)):
                raise ValueError(f"uniforms must be [{T}, {N * F}] (or [{T}, {N}, {F}]), got shape {uniforms.shape}")
            uniforms = np.ascontiguousarray(uniforms).reshape(T, N * F)
            bad = ~((uniforms >= 0.0) & (uniforms < 1.0))
            if bad.any():
                t, i = np.argwhere(bad)[0]
                raise ValueError(f"uniforms[{t}][{i}]={uniforms[t, i]} is outside [0, 1) or not finite")
        self.kernel_ms = 0.0
        for t0, cl, w, tb in blocks:
            n = cl.shape[0]
            u = uniforms[t0:t0 + n] if uniforms is not None else None
            dev_f, dev_o = np.empty((n, 2, F)), np.empty((n, 2, N))
            count = np.empty((n, F, S), dtype=np.int32)
            y = np.empty((n, N, F), dtype=np.uint8) if replicates else None
            skipped = ct.c_int64(0)
            self._check(self._lib.sbe_ppc_check(self._h, n, self.n_samples, seed, _ptr(cl), _ptr(w), _ptr(tb), _ptr(u) if u is not None else None,
                                                _ptr(y) if replicates else None, _ptr(dev_f), _ptr(dev_o), _ptr(count), ct.byref(skipped)))
            self.kernel_ms += self.last_kernel_ms()
            self._rows["dev_feature"].append(dev_f)
            self._rows["dev_object"].append(dev_o)
            self._rows["count_rep"].append(count)
            self._rows["y_rep"].append(y)
            self.n_samples += n
            self.n_skipped += skipped.value

    def drain_replicates(self):
        """The y_rep blocks of the check() calls since the last drain, in order; the handle forgets them (result().y_rep is then
        None).  For a consumer that takes the replicates block by block (sbayes_amd/pairppc.py)."""
        ys = self._rows["y_rep"]
        out = [y for y in ys if y is not None]
        ys[:] = [None] * len(ys)
        return out

    def result(self) -> PpcResult:
        _N, _F, S, _C, _K, _R = self._with_data()
        if self.n_samples == 0:
            raise ValueError("no sample was checked")
        ys = self._rows["y_rep"]
        return PpcResult(codes=self._codes, dev_feature=np.concatenate(self._rows["dev_feature"]), dev_object=np.concatenate(self._rows["dev_object"]),
                         count_rep=np.concatenate(self._rows["count_rep"]), count_obs=count_observed(self._codes, S), n_samples=self.n_samples,
                         n_skipped=self.n_skipped, y_rep=np.concatenate(ys) if all(y is not None for y in ys) else None, kernel_ms=self.kernel_ms)


def posterior_predictive_check(codes, groups, clusters, weights, tables, burnin=0.1, seed=0, n_groups=None, replicates=False, uniforms=None,
                               device=None) -> PpcResult:
    """The posterior predictive check of T logged samples after burn-in.  codes uint8 [N,F]; groups: uint8 [C-1,N] group indices
    (with n_groups) or a list of bool [G_c,N] assignments; clusters uint8 [T,K,N]; weights [T,F,C]; tables [T,R,F,S]; uniforms:
    None or float64 [T, N F], one row per sample before burn-in."""
    groups, n_groups, clusters, weights, tables, uniforms = _samples.after_burnin(groups, clusters, weights, tables, burnin, n_groups, uniforms)
    h = PpcHandle(device)
    try:
        h.set_data(codes, groups, n_groups, tables.shape[3], clusters.shape[1])
        h.check(clusters, weights, tables, seed=seed, uniforms=uniforms, replicates=replicates)
        return h.result()
    finally:
        h.close()


def main(argv=None):
    ap = _samples.run_parser("python -m sbayes_amd.ppc",
                             "Posterior predictive check of an sBayes run's logged samples: a replicated data set per sample, and "
                             "p-values of the deviance per feature and per object (conservative: given the logged effect draws)", seed=True)
    ap.add_argument("--out-features", type=Path, default=None, help="write the table per feature")
    ap.add_argument("--out-objects", type=Path, default=None, help="write the table per object")
    args = ap.parse_args(argv)
    data, clusters, weights, tables, n_groups = _samples.read_run(args)
    res = posterior_predictive_check(data["codes"], data["groups"], clusters, weights, tables, burnin=args.burnin, seed=args.seed, n_groups=n_groups,
                                     device=args.device)
    print(f"{res.n_samples} samples, p_total {res.p_total:.4f} (conservative: given the logged effect draws), {res.n_skipped} cells skipped")
    for kind, names in (("feature", data["feature_names"]), ("object", None)):
        print(f"the five {kind}s with the smallest p:")
        for name, cells, obs, rep, p, flag in res.worst(kind, names):
            print(f"  {name}\tcells {cells}\tdeviance {obs:.4f} observed, {rep:.4f} replicated\tp {p:.4f}\t{flag}")
    if args.out_features:
        res.write_table(args.out_features, "feature", data["feature_names"])
    if args.out_objects:
        res.write_table(args.out_objects, "object")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
