"""The range cases of the column kernel (sbayes_amd/csrc/sbe_diag_column.hip.h), shared by tests/test_diag_range_cpu.py (which
asserts under the checker alone that every case covers what it is there for and decides with a safe margin) and
tests/test_gpu_diag_range.py (device against checker).  Three groups, DESIGN.md section 16:

    A  rho_t past entry 2048 (RHO_LDS): the first 2048 entries live in LDS, later ones in the column's slice of a global
       scratch that exists only for n > 2048.  Chains of iid draws, chain m shifted by 1.5 m: the variance between the chains
       keeps every pair sum positive, so the walk runs to its n - 3 bound.
    B  the hand-over between blocks of 32 lags (LAG_BLOCK): walks to the bound, max_lag stops and stops by the rule itself on
       either side of a multiple of 32.
    C  magnitudes: locations to 1e9, scales from 1e-120 to 1e120, and the absolute constant threshold (max - min < 1e-15).

The checker's result of a case is computed once and shared; nothing changes it."""
from __future__ import annotations

import functools

import numpy as np

from tests import _diag_cases as dcases
from tests import _diag_oracle as orc

MIN_MARGIN = 1e-9
RHO_LDS = 2048                  # kRhoLds
LAG_BLOCK = 32                  # kLagBlock
_FLAT = dict(burnin=0.0, split=False)


def shifted(seed, m, n, p, columns=None):
    """orc.ar1(rng, 0.0, m, n, p) with chain k shifted by 1.5 k (in `columns` only, when given)."""
    x = orc.ar1(np.random.default_rng(seed), 0.0, m, n, p)
    cols = slice(None) if columns is None else list(columns)
    for k in range(m):
        x[k][:, cols] += 1.5 * k
    return x


def walk_end(n):
    """n_lags of a column whose first loop runs to its bound: the first odd t with t >= n - 3."""
    return (n - 3) | 1


def max_lag_end(max_lag):
    """n_lags of a column stopped by max_lag alone: the first odd t with t + 2 > max_lag."""
    return (max_lag - 1) | 1


# ---- A: rho_t past entry 2048 -------------------------------------------------------------------------------------------------
ALLOC_N = (2048, 2050, 2051, 2052)          # no scratch; scratch, the walk ends at entry 2047; entries 2048 and 2049 written
SPILL_MAX_LAGS = (2047, 2048, 2049, 2100)


def spill_table():
    """2 x 2400 x 3: columns 0 and 2 shifted (2397 lags), column 1 iid (a few lags), in neighbouring scratch slices."""
    return shifted(201, 2, 2400, 3, columns=(0, 2))


def spill_global():
    """8 x 2300 x 1: M n = 18 400 draws are past the LDS limit, so the column is read from the store and rho_t spills."""
    return shifted(202, 8, 2300, 1)


def spill_edge(n=2051):
    return shifted(401, 2, n, 1)


# ---- B: lag-block edges ---------------------------------------------------------------------------------------------------------
WALK_N = (33, 34, 35, 36, 37, 64, 65, 66, 67, 68, 69, 96, 99)
EDGE_MAX_LAGS = (29, 30, 31, 32, 33, 34, 62, 63, 64, 65, 66)
FREE_MAX_LAGS = (398, 1000)                 # above the 397 lags of shifted_2x400: never met
# n_lags -> (phi, seed) of a 2 x 600 AR(1) column whose walk the rule itself stops there (found by a search over seeds
# 1000 .. 1399 under the checker, the first with a margin >= 1e-6)
RULE_STOPS = {31: (0.9, 1029), 33: (0.9, 1016), 63: (0.97, 1007), 65: (0.97, 1014)}
SUMMARY_WALK_N = (33, 65, 67)


def rule_stop(n_lags):
    phi, seed = RULE_STOPS[n_lags]
    return orc.ar1(np.random.default_rng(seed), phi, 2, 600, 1)


# ---- C: magnitudes and the constant threshold -----------------------------------------------------------------------------------
# name -> (seed, phi, loc, scale): 2 x 600 x 1, default burn-in and split (4 chains of 270 draws)
MAGNITUDES = {
    "loc_m1.2e5_sd30": (601, 0.8, -1.2e5, 30.0),          # a log-likelihood or posterior column
    "loc_1e6": (602, 0.5, 1e6, 1.0),
    "loc_1e9": (603, 0.5, 1e9, 1.0),
    "loc_m1e9_sd1e-3": (604, 0.5, -1e9, 1e-3),
    "scale_1e-120": (605, 0.5, 0.0, 1e-120),              # max - min < 1e-15: constant by the contract; mean and sd are checked
    "scale_1e-14": (606, 0.5, 0.0, 1e-14),
    "scale_1e-7": (607, 0.5, 0.0, 1e-7),                  # a weight near zero
    "scale_1e120": (608, 0.5, 0.0, 1e120),
    "unit": (607, 0.5, 0.0, 1.0),                         # the seed of scale_1e-7
}
THRESHOLD_RANGES = (0.9e-15, float(np.nextafter(1e-15, 0.0)), 1.1e-15)
THRESHOLD_FLAGS = (1, 1, 0, 1)


def magnitude(name):
    seed, phi, loc, scale = MAGNITUDES[name]
    return orc.ar1(np.random.default_rng(seed), phi, 2, 600, 1, loc=loc, scale=scale)


def magnitude_table():
    """Every magnitude column side by side."""
    return np.concatenate([magnitude(name) for name in MAGNITUDES], axis=2)


def threshold_table(s=600, burn=60):
    """2 x 600 x 4.  Columns 0 - 2: an AR(1) column mapped linearly so that the draws kept after burn-in span [0, r] exactly
    (the smallest is 0, the largest fl(1 r) = r); column 3: 1.0 everywhere but one kept draw at 1 + 4 * 2^-52 (range 8.9e-16)."""
    cols = []
    for k, r in enumerate(THRESHOLD_RANGES):
        z = orc.ar1(np.random.default_rng(620 + k), 0.5, 2, s, 1)
        kept = z[:, burn:]
        cols.append((z - kept.min()) / (kept.max() - kept.min()) * r)
    one = np.ones((2, s, 1))
    one[1, s // 2, 0] = 1.0 + 4.0 * 2.0 ** -52
    return np.concatenate(cols + [one], axis=2)


# name -> (builder of float64 [M][S][P], keyword arguments of the call)
CASES = {}
for _n in ALLOC_N:
    CASES[f"alloc_2x{_n}"] = (functools.partial(spill_edge, _n), _FLAT)
CASES["spill_2x2400"] = (spill_table, _FLAT)
CASES["spill_global_8x2300"] = (spill_global, _FLAT)
for _k in SPILL_MAX_LAGS:
    CASES[f"spill_max_lag_{_k}"] = (spill_table, dict(_FLAT, max_lag=_k))
for _n in WALK_N:
    CASES[f"walk_2x{_n}"] = (functools.partial(shifted, 500 + _n, 2, _n, 2), _FLAT)
for _k in EDGE_MAX_LAGS + FREE_MAX_LAGS:
    CASES[f"edge_max_lag_{_k}"] = (dcases.CASES["shifted_2x400"][0], dict(_FLAT, max_lag=_k))
for _k in RULE_STOPS:
    CASES[f"rule_stop_{_k}"] = (functools.partial(rule_stop, _k), _FLAT)
for _name in MAGNITUDES:
    CASES[_name] = (functools.partial(magnitude, _name), dict())
CASES["magnitudes"] = (magnitude_table, dict())
CASES["threshold"] = (threshold_table, dict())

SPILL = ("alloc_2x2051", "alloc_2x2052", "spill_2x2400", "spill_global_8x2300") + tuple(f"spill_max_lag_{k}" for k in SPILL_MAX_LAGS[2:])


@functools.lru_cache(maxsize=None)
def case(name):
    """(chains float64 [M][S][P] (read-only), keyword arguments, the checker's result)."""
    build, kw = CASES[name]
    x = build()
    x.setflags(write=False)
    return x, dict(kw), orc.diagnose(list(x), **kw)


def safe(want):
    """The rule of these cases, per column: constant, or a decision margin >= 1e-9 and above twice the bound on a device's rho
    (the condition under which no decision can flip: tests/_diag_oracle.py)."""
    return ((want["flag"] & orc.FLAG_CONSTANT) != 0) | ((want["margin"] >= MIN_MARGIN) & (want["margin"] > 2 * want["rho_bound"]))


@functools.lru_cache(maxsize=None)
def summary_case(name):
    """(chains, keyword arguments, the summary checker's result) of a case above."""
    from tests import _summary_oracle as sorc
    build, kw = CASES[name]
    x = build()
    x.setflags(write=False)
    return x, dict(kw), sorc.summarize(list(x), **kw)


SUMMARY_CASES = tuple(f"walk_2x{n}" for n in SUMMARY_WALK_N) + tuple(f"rule_stop_{k}" for k in RULE_STOPS) + tuple(MAGNITUDES)
