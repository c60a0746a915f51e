"""The fixed cases of the diagnostics tests: seeded columns, shared by tests/test_diag_oracle_cpu.py (which asserts that
every case has a decision margin >= 1e-9 under the checker alone) and tests/test_gpu_diag.py (device against checker).
The checker's result of a case is computed once and shared; nothing changes it."""
from __future__ import annotations

import functools

import numpy as np

from tests import _diag_oracle as orc

MIN_MARGIN = 1e-9


def _binary(rng, m, s, p, stay=0.9):
    x = np.empty((m, s, p))
    x[:, 0] = rng.random((m, p)) < 0.5
    flip = rng.random((m, s, p)) > stay
    for i in range(1, s):
        x[:, i] = np.where(flip[:, i], 1 - x[:, i - 1], x[:, i - 1])
    return x


def _weights_like(rng, m, s, p):
    """Values a stats file holds for a weight: in (0, 1), float32-valued."""
    z = orc.ar1(rng, 0.7, m, s, p)
    return (1.0 / (1.0 + np.exp(-z))).astype(np.float32).astype(np.float64)


def _mixed(rng, m=2, s=120):
    good = orc.ar1(rng, 0.6, m, s, 3, loc=5.0, scale=0.1)
    const = np.full((m, s, 1), 0.25)
    nan = orc.ar1(rng, 0.0, m, s, 1)
    nan[1, 17, 0] = np.nan
    inf = orc.ar1(rng, 0.0, m, s, 1)
    inf[0, s - 1, 0] = np.inf
    return np.concatenate([good[:, :, :1], const, nan, good[:, :, 1:2], inf, _binary(rng, m, s, 1), _weights_like(rng, m, s, 1),
                           good[:, :, 2:]], axis=2)


def _shifted(rng):
    x = orc.ar1(rng, 0.0, 2, 400, 1)
    x[1] += 1.5
    return x


def lds_max_draws():
    from sbayes_amd import diag
    return diag.lds_max_draws()


def _lds_edge(extra):
    rng = np.random.default_rng(4242)
    x = orc.ar1(rng, 0.3, 1, lds_max_draws() + 1, 2, loc=-3.0)
    return x[:, :lds_max_draws() + extra]


# name -> (builder of float64 [M][S][P], keyword arguments of the call)
CASES = {
    "tiny_1x4": (lambda: orc.ar1(np.random.default_rng(11), 0.3, 1, 4, 3), dict(burnin=0.0, split=False)),
    "tiny_1x5": (lambda: orc.ar1(np.random.default_rng(12), 0.3, 1, 5, 3), dict(burnin=0.0, split=False)),
    "tiny_2x6": (lambda: orc.ar1(np.random.default_rng(13), 0.3, 2, 6, 3), dict(burnin=0.0, split=False)),
    "split_3x7": (lambda: orc.ar1(np.random.default_rng(14), 0.3, 3, 15, 3), dict(burnin=0.0, split=True)),       # halves of 7
    "ar09_4x1000": (lambda: orc.ar1(np.random.default_rng(15), 0.9, 4, 1000, 2, loc=2.0), dict()),
    "ar099_4x5000": (lambda: orc.ar1(np.random.default_rng(16), 0.99, 4, 5000, 1), dict()),
    "neg05_2x500": (lambda: orc.ar1(np.random.default_rng(26), -0.5, 2, 500, 1), dict(burnin=0.0, split=False)),   # (a seed at which the floor binds)
    "shifted_2x400": (lambda: _shifted(np.random.default_rng(18)), dict(burnin=0.0, split=False)),
    "binary": (lambda: _binary(np.random.default_rng(19), 2, 300, 1), dict()),
    "weights_f32": (lambda: _weights_like(np.random.default_rng(20), 2, 300, 1), dict()),
    "mixed": (lambda: _mixed(np.random.default_rng(21)), dict()),
    "wide_257": (lambda: orc.ar1(np.random.default_rng(22), 0.5, 2, 60, 257, loc=1.0), dict()),
    "lds_edge": (lambda: _lds_edge(0), dict(burnin=0.0, split=False)),
    "lds_edge_plus_1": (lambda: _lds_edge(1), dict(burnin=0.0, split=False)),
    "global_2x40000": (lambda: orc.ar1(np.random.default_rng(23), 0.9, 2, 40000, 1), dict()),
    "max_lag_hit": (lambda: orc.ar1(np.random.default_rng(15), 0.9, 4, 1000, 2, loc=2.0), dict(max_lag=10)),
    "max_lag_not_hit": (lambda: orc.ar1(np.random.default_rng(15), 0.9, 4, 1000, 2, loc=2.0), dict(max_lag=400)),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(chains float64 [M][S][P] (read-only), keyword arguments, the checker's result)."""
    build, kw = CASES[name]
    x = build()
    x.setflags(write=False)
    return x, dict(kw), orc.diagnose(list(x), **kw)
