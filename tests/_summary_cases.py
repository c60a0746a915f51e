"""The fixed cases of the summary tests: seeded columns, shared by tests/test_summary_oracle_cpu.py (which asserts that every
derived column of every case has a decision margin >= 1e-9 and above twice its rho bound under the checker alone) and
tests/test_gpu_summary.py (device against checker).  The checker's result of a case is computed once and shared; nothing
changes it.  Each shape is the smallest at which its mechanism can go wrong: the wave (64), the block (256) and the sorting
network's padding (a power of two, one below, one above), the LDS limit and one past it, more columns than a launch, the
smallest n at which a derived column writes rho_t past the 2048 entries kept in LDS (the spill_* cases: the shifted chains of
tests/_diag_range_cases.py, whose ranks walk to the n - 3 bound as the values do)."""
from __future__ import annotations

import functools

import numpy as np

from tests import _diag_cases as dcases
from tests import _diag_oracle as orc
from tests import _diag_range_cases as rcases
from tests import _summary_oracle as sorc

MIN_MARGIN = 1e-9
EIGHT_PROBS = (0.0, 0.025, 0.25, 0.5, 0.75, 0.9, 0.975, 1.0)


def _flat(rng, total, p=2, phi=0.5):
    """One chain of `total` draws, not split: N = total exactly."""
    return orc.ar1(rng, phi, 1, total, p, loc=1.0)


def _cluster_sizes(rng, m, s, p):
    """Integer columns with heavy ties: the size of a cluster that gains or loses an object now and then."""
    step = rng.integers(-1, 2, size=(m, s, p)) * (rng.random((m, s, p)) < 0.3)
    return np.clip(12 + np.cumsum(step, axis=1), 3, 25).astype(np.float64)


def _all_but_one(m, s):
    x = np.full((m, s, 1), 0.375)
    x[m - 1, s // 3, 0] = 2.5
    return x


def _signed_zeros(rng, m, s):
    """An AR(1) column with a third of its values replaced by +0.0 and -0.0 in turn."""
    x = orc.ar1(rng, 0.4, m, s, 1)
    pick = rng.random((m, s, 1)) < 0.35
    sign = rng.random((m, s, 1)) < 0.5
    x[pick & sign] = 0.0
    x[pick & ~sign] = -0.0
    return x


def _special(rng, m=2, s=120):
    """The mixed columns of the diagnostics' cases (good, constant, NaN, good, inf, 0/1, float32 weights, good), then cluster
    sizes, all equal but one, signed zeros."""
    return np.concatenate([dcases._mixed(rng, m, s), _cluster_sizes(rng, m, s, 2), _all_but_one(m, s), _signed_zeros(rng, m, s)], axis=2)


def _lds_edge(extra):
    rng = np.random.default_rng(5151)
    x = orc.ar1(rng, 0.3, 1, dcases.lds_max_draws() + 1, 2, loc=-3.0)
    return x[:, :dcases.lds_max_draws() + extra]


def _chain_constant(rng, s=40):
    """Two runs: column 0 is 3 all through one and 7 all through the other, column 1 a 0/1 indicator that is 1 in the first
    run only, column 2 an ordinary AR(1).  Every chain of columns 0 and 1 is constant, the chains differ."""
    x = orc.ar1(rng, 0.3, 2, s, 3)
    x[0, :, 0], x[1, :, 0] = 3.0, 7.0
    x[0, :, 1], x[1, :, 1] = 1.0, 0.0
    return x


_FLAT = dict(burnin=0.0, split=False)

# name -> (builder of float64 [M][S][P], keyword arguments of the call)
CASES = {
    "split_1x8": (lambda: orc.ar1(np.random.default_rng(41), 0.3, 1, 8, 3), dict(burnin=0.0)),                 # 2 x 4
    "split_3x14": (lambda: orc.ar1(np.random.default_rng(42), 0.3, 3, 14, 3), dict(burnin=0.0)),               # 6 x 7: N = 42
    "n64": (lambda: _flat(np.random.default_rng(43), 64), _FLAT),
    "n65": (lambda: _flat(np.random.default_rng(44), 65), _FLAT),
    "n255": (lambda: _flat(np.random.default_rng(45), 255), _FLAT),
    "n256": (lambda: _flat(np.random.default_rng(46), 256), _FLAT),
    "n257": (lambda: _flat(np.random.default_rng(47), 257), _FLAT),
    "iid_2x4": (lambda: orc.ar1(np.random.default_rng(48), 0.0, 2, 4, 2), _FLAT),
    "ar05_8x500": (lambda: orc.ar1(np.random.default_rng(49), 0.5, 8, 500, 1), _FLAT),
    "binary": (lambda: dcases._binary(np.random.default_rng(50), 2, 300, 2), dict()),
    "weights_f32": (lambda: dcases._weights_like(np.random.default_rng(51), 2, 300, 2), dict()),
    "special": (lambda: _special(np.random.default_rng(52)), dict()),
    "ar09_4x1000": (lambda: orc.ar1(np.random.default_rng(53), 0.9, 4, 1000, 2, loc=2.0), dict()),
    "wide_257": (lambda: orc.ar1(np.random.default_rng(54), 0.5, 2, 60, 257, loc=1.0), dict()),
    "one_column": (lambda: orc.ar1(np.random.default_rng(55), 0.3, 2, 80, 1), dict()),
    "lds_edge": (lambda: _lds_edge(0), _FLAT),
    "lds_edge_plus_1": (lambda: _lds_edge(1), _FLAT),
    "global_2x40000": (lambda: orc.ar1(np.random.default_rng(56), 0.9, 2, 40000, 2), dict()),
    "probs_0_1": (lambda: orc.ar1(np.random.default_rng(57), 0.3, 2, 90, 2), dict(probs=(0.0, 1.0), hdi_prob=0.5)),
    "eight_probs": (lambda: orc.ar1(np.random.default_rng(58), 0.3, 2, 90, 2), dict(probs=EIGHT_PROBS)),
    "no_probs": (lambda: orc.ar1(np.random.default_rng(59), 0.3, 2, 90, 2), dict(probs=())),
    "hdi_widest": (lambda: orc.ar1(np.random.default_rng(60), 0.3, 1, 10, 2), dict(burnin=0.0, hdi_prob=float(np.nextafter(1.0, 0.0)))),    # floor(hdi_prob N) = N - 1, the widest span: no hdi_prob < 1 rounds hdi_prob N up to N, so the upper clip is never taken
    "hdi_clips_low": (lambda: orc.ar1(np.random.default_rng(61), 0.3, 1, 10, 2), dict(burnin=0.0, hdi_prob=0.01)),      # floor(hdi_prob N) = 0: clipped to 1
    "chain_constant": (lambda: _chain_constant(np.random.default_rng(62)), dict()),                             # W = 0: rhat_rank = +inf
    "max_lag_hit": (lambda: orc.ar1(np.random.default_rng(53), 0.9, 4, 1000, 2, loc=2.0), dict(max_lag=10)),
    "spill_2x2051": (rcases.spill_edge, _FLAT),                                                                 # entries 2048 and 2049, no more
    "spill_2x2400": (rcases.spill_table, _FLAT),                                                                # 3 columns: 12 derived ones
    "spill_global_8x2300": (rcases.spill_global, _FLAT),
}
SPILL = ("spill_2x2051", "spill_2x2400", "spill_global_8x2300")


@functools.lru_cache(maxsize=None)
def case(name):
    """(chains float64 [M][S][P] (read-only), keyword arguments, the checker's result)."""
    build, kw = CASES[name]
    x = build()
    x.setflags(write=False)
    return x, dict(kw), sorc.summarize(list(x), **kw)
