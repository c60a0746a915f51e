"""Seeded inputs of the power-scaling sensitivity's tests (tests/test_psens_oracle_cpu.py, tests/test_gpu_psens.py).  A plain
helper module: it holds no test.  Every array is made once per process and handed out read-only."""
from functools import lru_cache

import numpy as np

MP_SIZES = (4, 5, 64, 257, 1000)
SORT_SIZES = (4, 5, 255, 256, 257, 1000)


def _frozen(a):
    a.setflags(write=False)
    return a


@lru_cache(maxsize=None)
def values(n, seed):
    """float64 [n]: standard normal draws, no ties."""
    return _frozen(np.random.default_rng(seed).standard_normal(n))


@lru_cache(maxsize=None)
def weights(v, n, seed):
    """float64 [v, n], non-negative with a positive sum: row 0 log-normal, row 1 with its first third zero, row 2 all ones, the
    rest log-normal with a spread that grows."""
    rng = np.random.default_rng(seed)
    w = np.exp(rng.standard_normal((v, n)) * (0.2 + 0.1 * np.arange(v))[:, None])
    if v > 1:
        w[1, :n // 3] = 0.0
    if v > 2:
        w[2] = 1.0
    return _frozen(w)


@lru_cache(maxsize=None)
def columns(n, seed):
    """float64 [n, 7]: normal; three integer values; 0 / 1; zeros of both signs among a few others; log-normal over 12 decades;
    a shuffle of 0 .. n - 1; normal at 1e-20."""
    rng = np.random.default_rng(seed)
    zeros = rng.choice(np.array([-0.0, 0.0, 0.0, -0.0, 1.5, -2.5]), size=n)
    zeros[:2] = (-0.0, 0.0)
    x = np.stack([rng.standard_normal(n), rng.integers(0, 3, n).astype(np.float64), (rng.random(n) < 0.3).astype(np.float64), zeros,
                  np.exp(rng.standard_normal(n) * 6.0), rng.permutation(n).astype(np.float64), rng.standard_normal(n) * 1e-20], axis=1)
    x[:2, 1], x[:2, 2] = (0.0, 2.0), (0.0, 1.0)                              # (never constant)
    return _frozen(x)


INTEGER_COLUMNS = (1, 2, 5)              # of columns(): every gap s[i + 1] - s[i] is 0 or 1, a power of two


@lru_cache(maxsize=None)
def ratios(n, seed, kind):
    """float64 [n]: the values of a component column.  "normal": -x^2 / 2 of normal draws scaled so that PSIS has work to do;
    "ties": the same rounded to a grid, so that the tail holds equal ratios; "heavy": a heavy tail (k well above 0)."""
    rng = np.random.default_rng(seed)
    if kind == "normal":
        r = -0.5 * rng.standard_normal(n) ** 2 * 40.0
    elif kind == "ties":
        r = np.round(-0.5 * rng.standard_normal(n) ** 2 * 40.0)
    elif kind == "heavy":
        r = -rng.pareto(1.5, n) * 30.0
    else:
        raise ValueError(kind)
    return _frozen(r)
