"""Model comparison on the device: PSIS-LOO and WAIC over logged observation likelihoods (include/sbe_elpd.h).

sBayes chooses the number of clusters by running K = 1..n and comparing ELPD-LOO (sbayes/tools/elpd.py): the
LikelihoodLogger rows -- float32 sum_c w * lh_exact per observation and logged sample (loggers.py:354-359) -- are read
back, NA columns and the burn-in dropped, and `arviz.loo` run on their log.  This module does that step on the GPU:

    res = psis_loo(lh, na_values=None, burnin=0.1)     # lh: float32 [S, N*F], as the .h5 `likelihood` earray holds it
    w = waic(lh, na_values=None, burnin=0.1)
    log = LikelihoodLog(model, capacity=1000)          # the rows kept on the engine's device, never copied to the host
    log.append(sample); log.psis_loo(burnin=0.1)
    sbayes_psis_loo(path, burnin=0.1)                  # tools/elpd.py:50 on a .npz (or .h5 when `tables` imports)

Numerical contract (tests/_elpd_oracle.py restates it in NumPy): NA columns are those `na_values` marks, else those
whose every row is isclose(lh, 1); the first int(burnin * S_total) rows are dropped; ll = log(float64(lh)) -- the
reference takes the log in float32, so results differ from an arviz run by about 1e-7 relative; PSIS is arviz's
(`psislw` with reff = 1: one chain, as the reference always has); WAIC is `arviz.waic` with ddof-0 variances.  Both
use arviz's "log" scale.  Limits: 2 .. 2^20 samples after burn-in (SBE_ERR_ARG beyond, with the limit named).

Handles follow the package's process model (sbayes_amd/_proc.py): created lazily in the process that uses them, never
pickled, forgotten (not destroyed) in a fork()ed child, where every further call raises."""
from __future__ import annotations

import ctypes as ct
from dataclasses import dataclass
from pathlib import Path

import numpy as np

from . import _handle
from ._handle import _ptr, c_handle_p

ABI_VERSION = 1                          # SBE_ELPD_ABI_VERSION of include/sbe_elpd.h
MAX_SAMPLES = 1 << 20                    # SBE_ELPD_MAX_SAMPLES

# name -> (restype, argtypes); mirrors include/sbe_elpd.h one to one (the engine's own table, _lib.PROTOTYPES, covers
# the three engine headers and is not extended)
PROTOTYPES = {
    **_handle.unit_prototypes("sbe_elpd"),
    "sbe_elpd_lds_max_samples": (ct.c_int64, []),
    "sbe_elpd_create": (ct.c_int, [ct.POINTER(c_handle_p), ct.c_int, ct.c_int64, ct.c_int64]),
    "sbe_elpd_n_rows": (ct.c_int, [c_handle_p, ct.POINTER(ct.c_int64)]),
    "sbe_elpd_reset": (ct.c_int, [c_handle_p]),
    "sbe_elpd_append_rows": (ct.c_int, [c_handle_p, ct.c_void_p, ct.c_int64]),
    "sbe_elpd_append_engine": (ct.c_int, [c_handle_p, ct.c_void_p, ct.c_int]),
    "sbe_elpd_get_rows": (ct.c_int, [c_handle_p, ct.c_int64, ct.c_int64, ct.c_void_p]),
    "sbe_elpd_compute": (ct.c_int, [c_handle_p, ct.c_int64, ct.c_void_p, ct.c_int, ct.c_void_p, ct.c_void_p, ct.c_void_p,
                                    ct.c_void_p, ct.POINTER(ct.c_int64)]),
}


def load():
    """The engine library with the prototypes of include/sbe_elpd.h attached."""
    return _handle.bind("sbe_elpd", PROTOTYPES, ABI_VERSION)


def lds_max_samples() -> int:
    """Largest S whose columns the kernel stages in LDS; longer columns take the global-memory selection."""
    return int(load().sbe_elpd_lds_max_samples())


@dataclass
class LooResult:
    """The fields of arviz.loo's ELPDData (scale "log"), plus the pointwise values over the kept columns."""
    elpd_loo: float
    se: float
    p_loo: float
    lppd: float
    n_samples: int
    n_data_points: int
    warning: bool
    good_k: float
    loo_i: np.ndarray
    pareto_k: np.ndarray
    scale: str = "log"


@dataclass
class WaicResult:
    """The fields of arviz.waic's ELPDData (scale "log"), plus the pointwise values over the kept columns."""
    elpd_waic: float
    se: float
    p_waic: float
    lppd: float
    n_samples: int
    n_data_points: int
    warning: bool
    waic_i: np.ndarray
    scale: str = "log"


class _Store(_handle.UnitHandle):
    """Owner of one sbe_elpd_store: float32 likelihood rows on one device.  last_kernel_ms(): the column kernel of the last
    compute call."""
    _prefix, _noun = "sbe_elpd", "an ELPD likelihood store"

    def __init__(self, device, n_columns, capacity):
        self.n_columns, self.capacity = int(n_columns), int(capacity)
        self._create_on(load, device, self.n_columns, self.capacity)

    @property
    def n_rows(self) -> int:
        n = ct.c_int64(0)
        self._check(self._lib.sbe_elpd_n_rows(self._h, ct.byref(n)))
        return n.value

    def append_rows(self, rows):
        """rows: float32 [n, n_columns], C order (validated by the caller)."""
        self._check(self._lib.sbe_elpd_append_rows(self._h, _ptr(rows), rows.shape[0]))

    def append_engine(self, eng, slot):
        self._check(self._lib.sbe_elpd_append_engine(self._h, eng._h, int(slot)))

    def rows(self):
        n = self.n_rows
        out = np.empty((n, self.n_columns), dtype=np.float32)
        self._check(self._lib.sbe_elpd_get_rows(self._h, 0, n, _ptr(out)))
        return out

    def reset(self):
        self._check(self._lib.sbe_elpd_reset(self._h))

    def compute(self, burn_rows, na_values, isclose_na):
        """(loo_i, k_i, lppd_i, v_i) over the kept columns; na_values: bool [n_columns] or None (validated by the caller)."""
        m = self.n_columns
        loo_i, k_i, lppd_i, v_i = (np.empty(m, dtype=np.float64) for _ in range(4))
        n_kept = ct.c_int64(0)
        na = None if na_values is None else np.ascontiguousarray(na_values, dtype=np.bool_).view(np.uint8)
        na_addr = None if na is None else _ptr(na)
        self._check(self._lib.sbe_elpd_compute(self._h, int(burn_rows), na_addr, int(bool(isclose_na)), _ptr(loo_i),
                                               _ptr(k_i), _ptr(lppd_i), _ptr(v_i), ct.byref(n_kept)))
        k = n_kept.value
        return loo_i[:k].copy(), k_i[:k].copy(), lppd_i[:k].copy(), v_i[:k].copy()


# ---- validation (host side, before any library call) -----------------------------------------------------------
def _check_lh(lh):
    a = np.asarray(lh)
    if a.dtype != np.float32:
        raise TypeError(f"lh must be float32 (the LikelihoodLogger's column type), got {a.dtype}")
    if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"lh must be [n_samples, n_observations] with both positive, got shape {a.shape}")
    return np.ascontiguousarray(a)


def _check_burnin(burnin, s_total):
    burnin = float(burnin)
    if not 0.0 <= burnin < 1.0:
        raise ValueError(f"burnin={burnin} must lie in [0, 1)")
    burn = int(burnin * s_total)                               # elpd.py:38
    s = s_total - burn
    if not 2 <= s <= MAX_SAMPLES:
        raise ValueError(f"{s} samples after burn-in; PSIS needs 2 .. {MAX_SAMPLES} (2^20) per observation")
    return burn


def _check_na(na_values, m):
    if na_values is None:
        return None
    na = np.asarray(na_values)
    if na.dtype != np.bool_:
        raise TypeError(f"na_values must be bool, got {na.dtype}")
    if na.size != m:
        raise ValueError(f"na_values has {na.size} entries, lh has {m} columns")
    return np.ascontiguousarray(na.ravel())


def _loo(loo_i, k_i, lppd_i, s):
    m = len(loo_i)
    good_k = float(min(1 - 1 / np.log10(s), 0.7))          # np.log10, as arviz.loo: math.log10 differs in the last bit at some S
    elpd = float(np.sum(loo_i))
    lppd = float(np.sum(lppd_i))
    return LooResult(elpd_loo=elpd, se=float((m * np.var(loo_i)) ** 0.5), p_loo=lppd - elpd, lppd=lppd, n_samples=s,
                     n_data_points=m, warning=bool(np.any(k_i > good_k)), good_k=good_k, loo_i=loo_i, pareto_k=k_i)


def _waic(lppd_i, v_i, s):
    m = len(lppd_i)
    waic_i = lppd_i - v_i
    return WaicResult(elpd_waic=float(np.sum(waic_i)), se=float((m * np.var(waic_i)) ** 0.5), p_waic=float(np.sum(v_i)),
                      lppd=float(np.sum(lppd_i)), n_samples=s, n_data_points=m, warning=bool(np.any(v_i > 0.4)),
                      waic_i=waic_i)


def _pointwise(lh, na_values, burnin, device):
    lh = _check_lh(lh)
    s_total, m = lh.shape
    burn = _check_burnin(burnin, s_total)
    na = _check_na(na_values, m)
    if device is None:
        from .registry import default_device
        device = default_device()
    store = _Store(device, m, s_total)
    try:
        store.append_rows(lh)
        return store.compute(burn, na, na is None), s_total - burn
    finally:
        store.close()


def psis_loo(lh, na_values=None, burnin=0.1, device=None) -> LooResult:
    """arviz.loo of a LikelihoodLogger matrix (float32 [S_total, N*F]) as sbayes/tools/elpd.py prepares it."""
    (loo_i, k_i, lppd_i, _v), s = _pointwise(lh, na_values, burnin, device)
    return _loo(loo_i, k_i, lppd_i, s)


def waic(lh, na_values=None, burnin=0.1, device=None) -> WaicResult:
    """arviz.waic of a LikelihoodLogger matrix, prepared like psis_loo's."""
    (_l, _k, lppd_i, v_i), s = _pointwise(lh, na_values, burnin, device)
    return _waic(lppd_i, v_i, s)


class LikelihoodLog:
    """LikelihoodLogger's rows kept on the device of the model's engine: append(sample) stores what
    LikelihoodLogger._write_sample would write for the sample, computed and written on the device."""

    def __init__(self, model, capacity=1000):
        if int(capacity) < 1:
            raise ValueError(f"capacity={capacity} must be positive")
        self.model = model
        self.capacity = int(capacity)
        self._store = None               # created on first use, in the process that uses it

    def _engine(self):
        from .binding import _engine
        return _engine(self.model)

    def _get_store(self, eng):
        if self._store is None or not self._store._h:
            self._store = _Store(eng.device, eng.n_objects * eng.n_features, self.capacity)
        return self._store

    def append(self, sample, slot=0):
        """Append the sample's row: float32(sum_c w * lh_exact), bound as observation_likelihoods(exact=True) binds."""
        from .binding import _bind_slot
        eng = self._engine()
        store = self._get_store(eng)
        if store.n_rows >= self.capacity:
            raise ValueError(f"LikelihoodLog is full: capacity of {self.capacity} rows reached")
        _bind_slot(eng, self.model, sample, slot, with_source=True)
        store.append_engine(eng, slot)

    def __len__(self):
        return 0 if self._store is None else self._store.n_rows

    def rows(self):
        """float32 [n_rows, N*F]: the rows as the .h5 `likelihood` earray would hold them."""
        return self._get_store(self._engine()).rows()

    def reset(self):
        if self._store is not None:
            self._store.reset()

    def na_values(self):
        """bool [N*F]: the model's NA mask, as LikelihoodLogger writes it next to the rows (loggers.py:343-351)."""
        return np.asarray(self.model.data.features.na_values, dtype=bool).ravel()

    def _pointwise(self, burnin, na_values):
        store = self._get_store(self._engine())
        burn = _check_burnin(burnin, store.n_rows)
        na = _check_na(self.na_values() if na_values is None else na_values, store.n_columns)
        return store.compute(burn, na, False), store.n_rows - burn

    def psis_loo(self, burnin=0.1, na_values=None) -> LooResult:
        (loo_i, k_i, lppd_i, _v), s = self._pointwise(burnin, na_values)
        return _loo(loo_i, k_i, lppd_i, s)

    def waic(self, burnin=0.1, na_values=None) -> WaicResult:
        (_l, _k, lppd_i, v_i), s = self._pointwise(burnin, na_values)
        return _waic(lppd_i, v_i, s)

    def close(self):
        if self._store is not None:
            self._store.close()
            self._store = None

    def __getstate__(self):
        raise TypeError("LikelihoodLog holds device memory and is not picklable; re-create it in the new process")


def read_likelihood(path):
    """(lh float32 [S, N*F], na_values bool [N*F] or None) of a likelihood file: .npz with `likelihood` (and
    `na_values`), or the LikelihoodLogger's .h5 when `tables` imports (that route is not exercised by the tests:
    `tables` is not a dependency)."""
    path = Path(path)
    if path.suffix == ".npz":
        with np.load(path, allow_pickle=False) as z:
            return np.asarray(z["likelihood"]), (np.asarray(z["na_values"]) if "na_values" in z.files else None)
    import tables
    with tables.open_file(str(path), mode="r") as f:
        lh = f.root.likelihood[:]
        na = f.root.na_values[:] if "na_values" in f.root else None
    return lh, na


def sbayes_psis_loo(likelihood_path, burnin=0.1, device=None) -> float:
    """sbayes/tools/elpd.py:sbayes_psis_loo: the ELPD-LOO of one run's likelihood file."""
    lh, na = read_likelihood(likelihood_path)
    return psis_loo(lh, na_values=na, burnin=burnin, device=device).elpd_loo
