"""Models compared by their pointwise ELPD on the device: differences with standard errors, stacking and Bayesian-bootstrap
weights (include/sbe_compare.h).

sBayes chooses the number of clusters by running K = 1..n and comparing ELPD-LOO across the runs (sbayes/tools/elpd.py, which
stops at one number per run).  `elpd.psis_loo` / `elpd.waic` give the pointwise values of one run on the device; this module
is the step after them, what `arviz.compare` does with the pointwise values of several runs:

    res = compare({"K3": loo3, "K4": loo4, "K5": loo5})                # LooResult, WaicResult or float64 vectors
    res.names, res.elpd, res.elpd_diff, res.dse, res.weight            # in rank order, best first; print(res.text())
    compare(models, method="bb-pseudo-bma", b_samples=1000, seed=0)    # or "pseudo-bma"
    h = CompareHandle(); h.reset(M, N); h.set_model(k, x); h.totals(); h.stacking(); h.bootstrap(seed, B)
    python -m sbayes_amd.compare RESULTS_DIR [BURNIN] [--method stacking]

Numerical contract (tests/_compare_oracle.py restates it in fp64; DESIGN.md section 20 states it), scale "log" throughout:
elpd = sum_i x_i and se = sqrt(N var(x)) per model (arviz's ELPDData); models ranked by elpd, ties by input order; against
the best model t, elpd_diff = sum_i (x_it - x_ik) and dse = sqrt(N var_i(x_it - x_ik)), both exactly 0 for t.  Stacking
maximises mean_i log(sum_k w_k p_ik) with p_ik = exp(x_ik - max_k x_ik) -- the row shift leaves the maximiser where it is,
and arviz's unshifted exp underflows -- by the EM update of mixture proportions from w = 1/M; gap = max_k g_k - 1 bounds
the distance of the objective from its maximum, and the iteration stops at gap <= tol.  arviz hands the same objective to
SciPy's SLSQP, which returns no such bound; where both were run the objectives they reach agree to 1e-12.  The pseudo-BMA+
weights average softmax(z_b) over Bayesian-bootstrap replicates z_bk = N sum_i(e_bi x_ik) / sum_i e_bi with e = -log(1 - u)
and u the engine's Philox uniforms (seed, draw b, index i): Dirichlet(1, .., 1) weights, arviz's alpha = 1.  The draws are
not SciPy's, so the bootstrap matches an arviz run in distribution, not in value.  Plain pseudo-BMA, softmax of the totals,
is host arithmetic.  Limits: 1 .. 32 models of 1 .. 2^24 values, 1 .. 2^16 replicates, 4 GiB for the store's two images.

There is no CPU fallback: without the library or a GPU the functions raise.  Handles follow the package's process model
(sbayes_amd/_proc.py): never pickled, forgotten (not destroyed) in a fork()ed child."""
from __future__ import annotations

import ctypes as ct
import re
import warnings
from dataclasses import dataclass
from pathlib import Path

import numpy as np

from . import _handle, elpd
from ._handle import _ptr, c_handle_p

ABI_VERSION = 1                          # SBE_COMPARE_ABI_VERSION of include/sbe_compare.h
MAX_MODELS = 32                          # SBE_COMPARE_MAX_MODELS
MAX_POINTS = 1 << 24                     # SBE_COMPARE_MAX_POINTS
MAX_REPLICATES = 1 << 16                 # SBE_COMPARE_MAX_REPLICATES
MAX_IMAGE_BYTES = 1 << 32                # SBE_COMPARE_MAX_IMAGE_BYTES
BLOCK = 256                              # SBE_COMPARE_BLOCK
CHUNK = 4096                             # SBE_COMPARE_CHUNK
RUN = 1024                               # SBE_COMPARE_RUN
BOOT_CHUNK = 1024                        # SBE_COMPARE_BOOT_CHUNK
CHECK_EVERY = 32                         # SBE_COMPARE_CHECK_EVERY
METHODS = ("stacking", "bb-pseudo-bma", "pseudo-bma")

# name -> (restype, argtypes); mirrors include/sbe_compare.h one to one (the engine's own table, _lib.PROTOTYPES, is not extended)
PROTOTYPES = {
    **_handle.unit_prototypes("sbe_compare"),
    "sbe_compare_create": (ct.c_int, [ct.POINTER(c_handle_p), ct.c_int]),
    "sbe_compare_reset": (ct.c_int, [c_handle_p, ct.c_int, ct.c_int64]),
    "sbe_compare_set_model": (ct.c_int, [c_handle_p, ct.c_int, ct.c_void_p]),
    "sbe_compare_totals": (ct.c_int, [c_handle_p, ct.c_void_p, ct.c_void_p]),
    "sbe_compare_differences": (ct.c_int, [c_handle_p, ct.c_int, ct.c_void_p, ct.c_void_p]),
    "sbe_compare_stacking": (ct.c_int, [c_handle_p, ct.c_double, ct.c_int64, ct.c_void_p, ct.POINTER(ct.c_double), ct.POINTER(ct.c_int64)]),
    "sbe_compare_bootstrap": (ct.c_int, [c_handle_p, ct.c_uint64, ct.c_int64, ct.c_void_p, ct.c_void_p, ct.c_void_p]),
    "sbe_compare_set_bootstrap_batch": (ct.c_int, [c_handle_p, ct.c_int64]),
}


def load():
    """The engine library with the prototypes of include/sbe_compare.h attached."""
    return _handle.bind("sbe_compare", PROTOTYPES, ABI_VERSION)


def image_bytes(n_models, n_points) -> int:
    """Device bytes of a store's two images (x, and p for stacking): float64, model-major, N padded to whole chunks."""
    return 2 * int(n_models) * ((int(n_points) + CHUNK - 1) // CHUNK * CHUNK) * 8


# ---- validation (host side, before any library call) -----------------------------------------------------------
def _check_shape(n_models, n_points):
    if not 1 <= n_models <= MAX_MODELS:
        raise ValueError(f"{n_models} models; a comparison takes 1 .. {MAX_MODELS}")
    if not 1 <= n_points <= MAX_POINTS:
        raise ValueError(f"{n_points} pointwise values per model; a comparison takes 1 .. {MAX_POINTS} (2^24)")
    need = image_bytes(n_models, n_points)
    if need > MAX_IMAGE_BYTES:
        raise ValueError(f"a store of {n_models} models x {n_points} points takes {need} bytes on the device, the limit is {MAX_IMAGE_BYTES}")


def _check_replicates(b_samples):
    if isinstance(b_samples, bool) or int(b_samples) != b_samples or not 1 <= b_samples <= MAX_REPLICATES:
        raise ValueError(f"b_samples={b_samples!r} out of range [1, {MAX_REPLICATES}] (2^16)")
    return int(b_samples)


def _check_seed(seed):
    if isinstance(seed, bool) or int(seed) != seed or not 0 <= seed < 1 << 64:
        raise ValueError(f"seed={seed!r} is not an integer in [0, 2^64)")
    return int(seed)


def _check_stop(tol, max_iter):
    tol = float(tol)
    if not (tol > 0.0 and np.isfinite(tol)):
        raise ValueError(f"tol={tol} must be positive and finite")
    if isinstance(max_iter, bool) or int(max_iter) != max_iter or not 1 <= max_iter <= 2 ** 31 - 1:
        raise ValueError(f"max_iter={max_iter!r} out of range [1, 2^31 - 1]")
    return tol, int(max_iter)


def _check_models(models):
    """(names, vectors float64 [N], kind, p, warning) of a dict name -> LooResult | WaicResult | float64 vector."""
    if not isinstance(models, dict):
        raise TypeError(f"models must be a dict of name -> LooResult, WaicResult or float64 vector, got {type(models).__name__}")
    names = [str(n) for n in models]
    if not 1 <= len(names) <= MAX_MODELS:
        raise ValueError(f"{len(names)} models; a comparison takes 1 .. {MAX_MODELS}")
    vectors, kinds, p, warning = [], [], [], []
    for name, m in models.items():
        if isinstance(m, elpd.LooResult):
            v, kind, p_m, warn = m.loo_i, "loo", m.p_loo, m.warning
        elif isinstance(m, elpd.WaicResult):
            v, kind, p_m, warn = m.waic_i, "waic", m.p_waic, m.warning
        else:
            v, kind, p_m, warn = m, None, float("nan"), False
        v = np.asarray(v)
        if v.dtype != np.float64:
            raise TypeError(f"model {name!r}: the pointwise values must be float64, got {v.dtype}")
        if v.ndim != 1:
            raise ValueError(f"model {name!r}: the pointwise values must be a vector, got shape {v.shape}")
        vectors.append(v)
        kinds.append(kind)
        p.append(float(p_m))
        warning.append(bool(warn))
    given = sorted({k for k in kinds if k is not None})
    if len(given) > 1:
        a, b = kinds.index("loo"), kinds.index("waic")
        raise ValueError(f"models {names[a]!r} (LOO) and {names[b]!r} (WAIC) mix the two criteria; compare one kind")
    for name, v in zip(names[1:], vectors[1:]):
        if v.size != vectors[0].size:
            raise ValueError(f"models {names[0]!r} and {name!r} differ in length: {vectors[0].size} and {v.size} pointwise values")
    _check_shape(len(names), vectors[0].size)
    vectors = [np.ascontiguousarray(v) for v in vectors]         # (copies, if any, come after the checks of the sizes)
    for name, v in zip(names, vectors):
        if not np.isfinite(v).all():
            at = int(np.flatnonzero(~np.isfinite(v))[0])
            raise ValueError(f"model {name!r}: pointwise value {at} is {v[at]}, not finite")
    return names, vectors, (given[0] if given else "elpd"), p, warning


class CompareHandle(_handle.UnitHandle):
    """Owner of one sbe_compare handle: the store of M models of N pointwise values on one device.  last_kernel_ms(): the
    kernels of the last totals(), differences(), stacking() or bootstrap()."""
    _prefix, _noun = "sbe_compare", "a model comparison handle"

    def __init__(self, device=None):
        self.n_models = self.n_points = 0
        self._create_on(load, device)

    def reset(self, n_models, n_points):
        """Shape the store: n_models models of n_points values, none of them set."""
        n_models, n_points = int(n_models), int(n_points)
        _check_shape(n_models, n_points)
        self.n_models = self.n_points = 0
        self._check(self._lib.sbe_compare_reset(self._h, n_models, n_points))
        self.n_models, self.n_points = n_models, n_points

    def _check_model(self, k):
        k = int(k)
        if not 0 <= k < self.n_models:
            raise ValueError(f"model {k} out of range [0, {self.n_models})")
        return k

    def set_model(self, k, x):
        """Model k <- x: float64 [n_points] (SBE_ERR_DATA, naming the model, for a value that is not finite)."""
        k = self._check_model(k)
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.shape != (self.n_points,):
            raise ValueError(f"model {k}: {x.shape} values, the store holds vectors of {self.n_points}")
        self._check(self._lib.sbe_compare_set_model(self._h, k, _ptr(x)))

    def _shaped(self):
        if not self.n_models:
            raise ValueError("the store has no shape yet (reset)")

    def totals(self):
        """(elpd, se): float64 [n_models]."""
        self._shaped()
        total, se = np.empty(self.n_models), np.empty(self.n_models)
        self._check(self._lib.sbe_compare_totals(self._h, _ptr(total), _ptr(se)))
        return total, se

    def differences(self, ref):
        """(elpd_diff, dse) against model `ref`: float64 [n_models], exactly 0 at ref."""
        self._shaped()
        ref = self._check_model(ref)
        diff, dse = np.empty(self.n_models), np.empty(self.n_models)
        self._check(self._lib.sbe_compare_differences(self._h, ref, _ptr(diff), _ptr(dse)))
        return diff, dse

    def stacking(self, tol=1e-8, max_iter=100_000):
        """(weights float64 [n_models], gap of those weights, updates that led to them, converged)."""
        self._shaped()
        tol, max_iter = _check_stop(tol, max_iter)
        weights = np.empty(self.n_models)
        gap, updates = ct.c_double(0), ct.c_int64(0)
        self._check(self._lib.sbe_compare_stacking(self._h, tol, max_iter, _ptr(weights), ct.byref(gap), ct.byref(updates)))
        return weights, gap.value, updates.value, gap.value <= tol

    def bootstrap(self, seed=0, b_samples=1000, alpha=1.0, return_z=False):
        """(weights, se) float64 [n_models] of the pseudo-BMA+ weights over b_samples replicates; with return_z also z,
        float64 [b_samples, n_models]."""
        self._shaped()
        if alpha != 1:
            raise ValueError(f"alpha={alpha!r}: the Bayesian bootstrap draws Dirichlet(1, .., 1) weights only")
        seed, b_samples = _check_seed(seed), _check_replicates(b_samples)
        weights, se = np.empty(self.n_models), np.empty(self.n_models)
        z = np.empty((b_samples, self.n_models)) if return_z else None
        self._check(self._lib.sbe_compare_bootstrap(self._h, seed, b_samples, _ptr(weights), _ptr(se), _ptr(z) if return_z else None))
        return (weights, se, z) if return_z else (weights, se)

    def set_bootstrap_batch(self, replicates):
        """Replicates per batch of the bootstrap (a multiple of 64; 0: the default); the results do not depend on it."""
        self._check(self._lib.sbe_compare_set_bootstrap_batch(self._h, int(replicates)))


@dataclass
class CompareResult:
    """The columns of arviz.compare's table, in rank order (best model first): names, rank (0 ..), elpd, p (the effective
    number of parameters; NaN for a bare vector), elpd_diff and dse against the best model, weight, se (of elpd; the
    bootstrap's for "bb-pseudo-bma", as in arviz), warning; order[r]: the input position of the model ranked r.  For
    stacking: gap (the bound on what the objective still lacks), updates, converged."""
    names: list
    rank: np.ndarray
    elpd: np.ndarray
    p: np.ndarray
    elpd_diff: np.ndarray
    weight: np.ndarray
    se: np.ndarray
    dse: np.ndarray
    warning: np.ndarray
    order: np.ndarray
    method: str
    criterion: str = "elpd"
    scale: str = "log"
    gap: float = float("nan")
    updates: int = 0
    converged: bool = True
    kernel_ms: float = 0.0

    def header(self):
        return ["model", "rank", f"elpd_{self.criterion}" if self.criterion != "elpd" else "elpd", f"p_{self.criterion}" if self.criterion != "elpd" else "p",
                "elpd_diff", "weight", "se", "dse", "warning", "scale"]

    def table(self):
        """One row per model, best first, in the order of header()."""
        return [[name, int(self.rank[r]), float(self.elpd[r]), float(self.p[r]), float(self.elpd_diff[r]), float(self.weight[r]),
                 float(self.se[r]), float(self.dse[r]), bool(self.warning[r]), self.scale] for r, name in enumerate(self.names)]

    def text(self):
        """header() and table() as tab-separated lines."""
        def cell(v):
            return v if isinstance(v, str) else (str(v) if isinstance(v, (bool, int)) else f"{v:.10g}")
        return "\n".join(["\t".join(self.header())] + ["\t".join(cell(v) for v in row) for row in self.table()]) + "\n"


def _softmax(z):
    t = np.exp(z - np.max(z))
    return t / np.sum(t)


def compare(models, method="stacking", b_samples=1000, seed=0, tol=1e-8, max_iter=100_000, alpha=1.0, device=None) -> CompareResult:
    """arviz.compare (scale "log") of a dict name -> LooResult, WaicResult or float64 vector of pointwise ELPD values."""
    if method not in METHODS:
        raise ValueError(f"method={method!r} is none of {', '.join(METHODS)}")
    names, vectors, kind, p, warning = _check_models(models)
    tol, max_iter = _check_stop(tol, max_iter)
    b_samples, seed = _check_replicates(b_samples), _check_seed(seed)
    if method == "bb-pseudo-bma" and alpha != 1:
        raise ValueError(f"alpha={alpha!r}: the Bayesian bootstrap draws Dirichlet(1, .., 1) weights only")
    h = CompareHandle(device)
    try:
        h.reset(len(names), vectors[0].size)
        for k, v in enumerate(vectors):
            h.set_model(k, v)
        total, se = h.totals()
        kernel_ms = h.last_kernel_ms()
        order = np.argsort(-total, kind="stable")            # elpd descending, ties by input order
        diff, dse = h.differences(int(order[0]))
        kernel_ms += h.last_kernel_ms()
        gap, updates, converged = float("nan"), 0, True
        if method == "stacking":
            weight, gap, updates, converged = h.stacking(tol, max_iter)
        elif method == "bb-pseudo-bma":
            weight, se = h.bootstrap(seed, b_samples)
        else:
            weight = _softmax(total)
        if method != "pseudo-bma":
            kernel_ms += h.last_kernel_ms()
    finally:
        h.close()
    return CompareResult(names=[names[k] for k in order], rank=np.arange(len(names)), elpd=total[order], p=np.array(p)[order],
                         elpd_diff=diff[order], weight=weight[order], se=se[order], dse=dse[order], warning=np.array(warning)[order],
                         order=order, method=method, criterion=kind, gap=gap, updates=updates, converged=converged, kernel_ms=kernel_ms)


# ---- files -------------------------------------------------------------------------------------------------------
def find_runs(results_dir):
    """{experiment: [(k, run, path)]} of the likelihood_K*_* files below results_dir, as sbayes/tools/elpd.py:71-80 walks
    them (.h5, and the .npz form elpd.read_likelihood also takes): the folders above a file are <experiment>/K<k>, the run
    index follows the last underscore; the files of hot chains (".chain" in the name) are skipped."""
    found = {}
    for path in sorted(Path(results_dir).rglob("likelihood_K*_*")):
        if path.suffix not in (".h5", ".npz") or ".chain" in path.name:
            continue
        folder = re.fullmatch(r"K(\d+)", path.parent.name)
        run = path.stem.rpartition("_")[-1]
        if not folder or not run.isdigit() or len(path.parts) < 3:
            continue
        found.setdefault(path.parts[-3], []).append((int(folder.group(1)), int(run), path))
    return {experiment: sorted(runs) for experiment, runs in found.items()}


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m sbayes_amd.compare",
                                 description="Compare the sBayes runs below a results folder by ELPD-LOO: differences, standard errors and model weights")
    ap.add_argument("results", type=Path, help="folder with the runs' likelihood files (<experiment>/K<k>/likelihood_K<k>_<run>.h5 or .npz)")
    ap.add_argument("burnin", type=float, default=0.1, nargs="?", help="fraction of the samples discarded as burn-in")
    ap.add_argument("--method", choices=METHODS, default="stacking")
    ap.add_argument("--b-samples", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", type=int, default=None)
    args = ap.parse_args(argv)
    found = find_runs(args.results)
    if not found:
        print(f"no likelihood files found below {args.results}")
        return 1
    for experiment, runs in found.items():
        models = {}
        for k, run, path in runs:                               # (a file that cannot be used is skipped with a warning, as the reference's tool does)
            try:
                lh, na = elpd.read_likelihood(path)
                loo = elpd.psis_loo(lh, na_values=na, burnin=args.burnin, device=args.device)
            except Exception as exc:                            # noqa: BLE001
                warnings.warn(f"error in likelihood file '{path}'; it is left out of the comparison: {exc}")
                continue
            if models and loo.loo_i.size != next(iter(models.values())).loo_i.size:
                warnings.warn(f"likelihood file '{path}' holds {loo.loo_i.size} observations, the runs before it "
                              f"{next(iter(models.values())).loo_i.size}; it is left out of the comparison")
                continue
            models[f"K{k}_{run}"] = loo
        if not models:
            warnings.warn(f"{experiment}: no usable likelihood file")
            continue
        res = compare(models, method=args.method, b_samples=args.b_samples, seed=args.seed, device=args.device)
        print(f"{experiment}: {len(models)} runs, {res.method}" + (f", gap {res.gap:.3g} after {res.updates} updates" if res.method == "stacking" else ""))
        print(res.text(), end="")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
