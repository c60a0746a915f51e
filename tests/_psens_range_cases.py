"""Seeded inputs of the PSIS weights' range tests (tests/test_psens_range_cpu.py, tests/test_gpu_psens_range.py): the draw
counts at which k_psens_weights takes another path, ties at the cutoff rank, delta from 1e-8 to 4, log ratios that overflow,
underflow or vanish, unequal and many chains, and the buffers' capacity.  A plain helper module: it holds no test.  Every
array is made once per process and handed out read-only; `reference` runs the checker once per case.

A case: its name, the chains (float64 [S_c, P] each), the rows burnt per chain, the component columns, delta, the store's
capacity and the size of the pieces its rows are appended in (None: one piece), and `expect`: what the case is there for, as
the CPU test asserts it of the checker (per weight vector, in the order alpha < 1, alpha > 1 of each component)."""
import math
from collections import namedtuple
from functools import lru_cache

import numpy as np

from tests import _psens_cases as base
from tests import _psens_oracle as orc

Case = namedtuple("Case", "name chains burn columns delta capacity piece expect")

LDS_MAX_DRAWS = 12_970                    # sbe_psens_lds_max_draws(); the GPU test asserts it of the library
BLOCK = 256                               # threads of the weights kernel's workgroup
KINDS = ("normal", "ties", "heavy")
DRAW_COUNTS = (4, 5, 20, 21, 224, 225, 226, 7281, 7282, 7283, LDS_MAX_DRAWS, LDS_MAX_DRAWS + 1, 50_000)
TIE_COUNTS = (21, 100, 1000)
DELTAS = (1e-8, 1e-6, 1e-4, 0.01, 0.5, 1.0, 4.0)
CAPACITY_DRAWS = 1 << 20
CAPACITY_PROBE_DRAWS = 1 << 17
MAX_TAIL, MAX_M = 3072, 96                # kPsensMaxTail, kPsensMaxM


def _frozen(a):
    a.setflags(write=False)
    return a


def _case(name, x, columns, delta, expect=None, chains=None, burn=None, capacity=None, piece=None):
    chains = [_frozen(np.ascontiguousarray(c, dtype=np.float64)) for c in (chains if chains is not None else [x])]
    burn = list(burn) if burn is not None else [0] * len(chains)
    return Case(name, chains, burn, list(columns), float(delta), capacity or max(len(c) for c in chains), piece, expect or {})


def path_by_size(n):
    return "lds" if n <= LDS_MAX_DRAWS else "global"


# ---- the draw counts ---------------------------------------------------------------------------------------------------
def _draws(n):
    x = np.stack([base.ratios(n, 700 + n + c, kind) for c, kind in enumerate(KINDS)], axis=1)
    tail = int(math.ceil(min(0.2 * n, 3 * math.sqrt(n))))
    expect = dict(tail=tail, path=path_by_size(n))
    if n <= 20:
        expect["k_inf"] = [True] * 6                                         # a tail of at most four: never fitted
    if n in (21, 7281, 7282, 7283):
        expect["above"] = {v: tail for v in (0, 1, 4, 5)}                    # the columns without ties: the whole tail is fitted
    return _case(f"draws_{n}", x, [0, 1, 2], 0.01, expect)


# ---- ties at the cutoff rank -------------------------------------------------------------------------------------------
def with_ties(rng, n, lo, hi):
    """float64 [n], shuffled: n distinct values in (0, 200) whose descending ranks lo .. hi (inclusive, rank 0 the maximum) all
    hold the value of rank hi, and whose ascending ranks lo .. hi all hold the value of rank hi: `lo` values lie strictly beyond
    the tie at either end, so both vectors of a component (the tail of alpha < 1 is the column's lower end) see the same pattern."""
    v = np.sort(rng.choice(np.arange(1, 100 * n + 1), n, replace=False).astype(np.float64)) * (200.0 / (100 * n + 1))
    assert 2 * (hi + 1) <= n
    v[lo:hi + 1] = v[hi]
    v[n - 1 - hi:n - lo] = v[n - 1 - hi]
    return rng.permutation(v)


def _ties(n):
    t = orc.tail_count(n)
    rng = np.random.default_rng(900 + n)
    patterns = [(t - 3, t + 3), (5, t + 2), (4, t), (t, t + 3)]              # the tie covers the cutoff rank t in each
    x = np.stack([with_ties(rng, n, lo, hi) for lo, hi in patterns], axis=1)
    above = {2 * g + v: lo for g, (lo, _hi) in enumerate(patterns) for v in (0, 1)}
    return _case(f"ties_{n}", x, [0, 1, 2, 3], 0.01, dict(tail=t, above=above, k_inf=[lo <= 4 for lo, _hi in patterns for _v in (0, 1)]))


def _equal_tails():
    """N = 25 (a tail of 5).  Column 0: five values at the maximum and five at the minimum, so either vector's tail is five equal
    exceedances, which the checker fits.  Column 1: all but three entries at the maximum: nothing lies above the cutoff for
    alpha > 1, three values do for alpha < 1; raw weights.  Column 2: one value throughout, the rule of equal ratios."""
    rng = np.random.default_rng(925)
    mid = rng.uniform(-50.0, 50.0, 15)
    col0 = rng.permutation(np.concatenate([np.full(5, 80.0), np.full(5, -80.0), mid]))
    col1 = rng.permutation(np.concatenate([np.full(22, 80.0), [-3.0, -41.5, 12.25]]))
    return _case("equal_tails_25", np.stack([col0, col1, np.full(25, -3.0)], axis=1), [0, 1, 2], 0.01,
                 dict(tail=5, above={0: 5, 1: 5, 2: 3, 3: 0, 4: 0, 5: 0}, k_inf=[False, False, True, True, True, True], constant=[4, 5]))


# ---- delta -------------------------------------------------------------------------------------------------------------
def _delta(delta, n):
    if n == 8000:                                                            # a tail above the workgroup; the second column is no component
        x, columns = np.stack([base.ratios(n, 1100 + n, "normal"), base.values(n, 1101 + n)], axis=1), [0]
    else:
        x, columns = np.stack([base.ratios(n, 1100 + n, "normal"), base.ratios(n, 1102 + n, "heavy")], axis=1), [0, 1]
    return _case(f"delta_{delta:g}_n{n}", x, columns, delta, dict(tail=orc.tail_count(n)))


# ---- the ratios' range, N = 1000 ---------------------------------------------------------------------------------------
RANGE_DRAWS = 1000


def _spread_2000():
    """(alpha - 1) x spans 2000 for alpha > 1 (delta = 1) and 1000 for alpha < 1: the ratios crowd below their maximum, so the
    tail is whole and fitted (k far above 0.7 for alpha < 1's vector), and the weights of the draws more than 745 below the
    maximum underflow to exactly 0.  The second column is no component (the sums under these weights are compared too)."""
    r = np.array(base.ratios(RANGE_DRAWS, 1200, "normal"))
    r *= 2000.0 / (r.max() - r.min())
    x = np.stack([r, base.values(RANGE_DRAWS, 1201)], axis=1)
    return _case("spread_2000", x, [0], 1.0, dict(tail=95, above={0: 95, 1: 95}, floored=[False, False], zero_weights=[0, 1], k_unreliable=[0]))


def _heavy_times_50():
    """The heavy column times 50 at delta = 1.  alpha < 1: more than 708 lie between the maximum and the cutoff rank, the cutoff is
    floored at log DBL_MIN and one ratio is left above it; alpha > 1: a whole tail, k above 20, half the weights exactly 0."""
    x = np.array(base.ratios(RANGE_DRAWS, 1210, "heavy"))[:, None] * 50.0
    return _case("heavy_times_50", x, [0], 1.0,
                 dict(tail=95, floored=[True, False], above={0: 1, 1: 95}, k_inf=[True, False], zeros={0: 999}, zero_weights=[1], k_unreliable=[1]))


def _huge_entries():
    """One entry at -1e308 and one at +1e308 among normal draws, delta = 1: alpha - 1 = 1 keeps every ratio finite, maximum minus
    minimum overflows and the minimum's key is -inf; alpha - 1 = -0.5 gives keys down to -1e308."""
    x = np.array(base.values(RANGE_DRAWS, 1220))
    x[3], x[7] = -1e308, 1e308
    return _case("huge_entries", x[:, None], [0], 1.0, dict(floored=[True, True], above={0: 1, 1: 1}, k_inf=[True, True], zeros={0: 999, 1: 999}))


def _tiny_ratios():
    """Log ratios of size 1e-13: after the maximum is subtracted, exp(x) is 1 less a few hundred ulp."""
    x = np.array(base.values(RANGE_DRAWS, 1230)) * 1e-13
    return _case("tiny_ratios", x[:, None], [0], 1.0, dict(tail=95))


def overflow_case():
    """x = 1e308 in one entry at delta = 4: (alpha - 1) x is finite for alpha < 1 and +inf for alpha > 1.  Column 1 of two; column
    0 is a component that is in order."""
    x = np.stack([base.ratios(64, 1240, "normal"), base.values(64, 1241)], axis=1)
    x[11, 1] = 1e308
    return _case("overflow", x, [0, 1], 4.0)


# ---- the chains --------------------------------------------------------------------------------------------------------
def _three_chains():
    """40, 12 and 20 rows, 7, 0 and 8 of them burnt (57 draws), a capacity above every chain, rows appended three at a time;
    the components are columns 2 and 1."""
    x = np.stack([base.values(72, 1300), base.ratios(72, 1301, "heavy"), base.ratios(72, 1302, "normal")], axis=1)
    return _case("three_chains", None, [2, 1], 0.01, dict(tail=12), chains=[x[:40], x[40:52], x[52:]], burn=[7, 0, 8], capacity=64, piece=3)


def _sixty_four_chains():
    """64 chains (SBE_DIAG_MAX_CHAINS) of 4 kept draws (SBE_DIAG_MIN_DRAWS) each after 0, 1 or 2 burnt rows; the component is
    column 1 of two."""
    burn = [c % 3 for c in range(64)]
    rows = [4 + b for b in burn]
    x = np.stack([base.values(sum(rows), 1310), base.ratios(sum(rows), 1311, "normal")], axis=1)
    edges = np.concatenate([[0], np.cumsum(rows)])
    chains = [x[edges[c]:edges[c + 1]] for c in range(64)]
    return _case("sixty_four_chains", None, [1], 0.01, dict(tail=orc.tail_count(256)), chains=chains, burn=burn, capacity=8)


@lru_cache(maxsize=None)
def all_cases():
    """Every case but the capacity one, by name."""
    cases = [_draws(n) for n in DRAW_COUNTS] + [_ties(n) for n in TIE_COUNTS] + [_equal_tails()]
    cases += [_delta(d, n) for d in DELTAS for n in (25, 1000, 8000)]
    cases += [_spread_2000(), _heavy_times_50(), _huge_entries(), _tiny_ratios(), _three_chains(), _sixty_four_chains()]
    return {c.name: c for c in cases}


NAMES = tuple(all_cases())
SUMS_CASES = ("delta_0.01_n8000", "spread_2000", "sixty_four_chains")       # compute() runs after the weights on these
CHAIN_CASES = ("three_chains", "sixty_four_chains")


@lru_cache(maxsize=None)
def long_case(n):
    """One chain of n kept draws after 1000 burnt rows, one normal column, one component: the probe at 2^17 and the capacity
    case at 2^20 (the only size with a tail of kPsensMaxTail and 85 candidates)."""
    x = np.array(base.ratios(n + 1000, 1400 + n.bit_length(), "normal"))[:, None]
    return _case(f"long_{n}", x, [0], 0.01, dict(tail=orc.tail_count(n), path="global"), burn=[1000])


def case(name):
    return all_cases()[name]


def stacked(c):
    return orc.stack(c.chains, c.burn)


def vectors(c):
    """The log ratios of every weight vector of a case, in the unit's order."""
    x = stacked(c)
    return [scale * x[:, col] for col in c.columns for scale in orc.scales(c.delta)]


Reference = namedtuple("Reference", "lws k ess vflag tol_k k_spread lw_spread")


@lru_cache(maxsize=None)
def _reference(c_name, n_long):
    c = long_case(n_long) if n_long else case(c_name)
    with np.errstate(over="ignore"):                                         # (huge_entries: maximum minus minimum is +inf)
        lws, ks, ess, flags = orc.component_weights(stacked(c), c.columns, c.delta)
        spreads = [orc.k_spread(r) for r in vectors(c)]
    dk, dlw = np.array([s[0] for s in spreads]), np.array([s[1] for s in spreads])
    for a in (lws, ks, ess, flags, dk, dlw):
        a.setflags(write=False)
    return Reference(lws, ks, ess, flags, _frozen(orc.K_TOL + orc.K_MARGIN * dk), dk, dlw)


def reference(c):
    """The checker's answer for a case and the tolerance on k per vector (orc.tol_k), computed once per process."""
    return _reference(c.name, len(stacked(c)) if c.name.startswith("long_") else 0)
