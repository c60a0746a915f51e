"""The seeded cases of the feature screening's range tests, shared by tests/test_assoc_cases_cpu.py (which proves under
the checker alone that every case covers what it is meant to cover) and tests/test_gpu_assoc_range.py (device against
checker), and an exact reference of the statistic in rational arithmetic.

Every builder returns (x uint8 [N, F] (read-only), n_states int32 [F]); the checker's result of a case is computed once
and shared, and nothing changes it.

* sweep cases, one per padded state count S_pad (2, 4, 8, 16, 32): a latent state per object, feature f is the latent
  (mod its state count) with probability theta_f and uniform otherwise, theta from 0 to 1, about 3 % NA, state counts
  mixed within (S_pad / 2, S_pad].  N lies off every multiple the kernel pads to, the last tile is partial;
* planted tables: pair (2 k, 2 k + 1) carries table k on its own objects, every other object is NA in both;
* the large case: 2^24 objects, six features, one cell count above 2^24 - 1000;
* the position case: 520 features observed at one object each, between two anchors observed everywhere."""
from __future__ import annotations

import functools
from fractions import Fraction

import numpy as np

from tests import _assoc_oracle as ao

TILE = 32                    # one-hot columns per tile edge of the pair kernel
ROUND = 256                  # objects the codes are padded to (four contraction steps of 64)
HALF = Fraction(1, 2)

# S_pad -> (seed, F, N)
SWEEP = {2: (202, 33, 769), 4: (204, 17, 831), 8: (208, 9, 833), 16: (221, 7, 1023), 32: (203, 7, 1281)}
NA_RATE = 0.03


def tiles_of(f, s_pad):
    """(features per tile edge, tiles, tile pairs) of F features at S_pad."""
    sub = TILE // s_pad
    tiles = -(-f // sub)
    return sub, tiles, tiles * (tiles + 1) // 2


def _sweep_states(rng, s_pad, f):
    """State counts within (S_pad / 2, S_pad], the largest first, the smallest last (at S_pad = 32, where a tile holds one
    feature, the last tile is then partial too), the others drawn."""
    lo = s_pad // 2 + 1
    ns = rng.integers(lo, s_pad + 1, f)
    ns[0], ns[-1] = s_pad, lo
    return ns.astype(np.int32)


def _sweep(s_pad):
    seed, f, n = SWEEP[s_pad]
    rng = np.random.default_rng(seed)
    ns = _sweep_states(rng, s_pad, f)
    # (squared from S_pad = 16 on: with seven features an even spread leaves too many pairs whose p-value underflows)
    theta = (np.linspace(0.0, 1.0, f) ** (2.0 if s_pad >= 16 else 1.0))[rng.permutation(f)]
    latent = rng.integers(0, s_pad, n)
    x = np.empty((n, f), dtype=np.uint8)
    for k in range(f):
        follow = rng.random(n) < theta[k]
        x[:, k] = np.where(follow, latent % ns[k], rng.integers(0, ns[k], n))
    x[rng.random((n, f)) < NA_RATE] = ao.NA
    return x, ns


@functools.lru_cache(maxsize=None)
def sweep(s_pad):
    """(x, n_states, the checker's result) of the sweep case at S_pad."""
    x, ns = _sweep(s_pad)
    x.setflags(write=False)
    ns.setflags(write=False)
    return x, ns, ao.feature_association(x, ns)


# ---- planted tables -------------------------------------------------------------------------------------------------
def _embed(cells, s):
    t = np.zeros((s, s), dtype=np.int64)
    for (a, b), v in cells.items():
        t[a, b] = v
    return t


def _two_by_32():
    t = np.zeros((32, 32), dtype=np.int64)
    t[0] = 1 + np.arange(32) % 3
    t[1] = 1 + (np.arange(32) * 7) % 4
    return t


INDEPENDENT_2X2 = "independent_2x2"
# name -> table (rows: states of feature 2 k, columns: of feature 2 k + 1); the state counts are the table's shape
PLANTED = {
    INDEPENDENT_2X2: np.array([[6, 9], [4, 6]]),               # E = O in every cell: statistic 0, p exactly 1
    "yates_half": np.array([[1, 0], [0, 1]]),                  # |E - O| = 0.5 exactly: the correction removes all of it
    "yates_one": np.array([[2, 0], [0, 2]]),                   # |E - O| = 1: statistic 4 (1/2)^2 / 1 = 1 exactly
    "yates_clamped": np.array([[5, 5], [5, 6]]),               # |E - O| = 5/21 < 0.5: the correction clamps, statistic 0
    "zero_cell": np.array([[7, 0], [3, 9]]),                   # a zero cell with E > 0
    "ends_of_32": _embed({(0, 0): 9, (0, 31): 2, (31, 0): 3, (31, 31): 11}, 32),     # dof 1 with Yates inside S_pad = 32
    "two_by_32": _two_by_32(),                                 # dof 31
    "diagonal_32": np.eye(32, dtype=np.int64),                 # N = 32, dof 961, statistic 992
    "independent_3x3": np.outer([1, 2, 3], [1, 2, 3]),         # E = O: statistic 0 at dof 4
    "never_together": np.zeros((2, 2), dtype=np.int64),        # n = 0 (both features are observed, on other objects)
}
PLANTED_2X2 = [k for k, t in PLANTED.items() if t.shape == (2, 2)]
PLANTED_N = 203
PLANTED_SEED = 77


def _planted(names):
    rng = np.random.default_rng(PLANTED_SEED)
    f = 2 * len(names) + 2
    x = np.full((PLANTED_N, f), ao.NA, dtype=np.uint8)
    ns = np.empty(f, dtype=np.int32)
    for k, name in enumerate(names):
        t = PLANTED[name]
        s = t.shape[0]
        a, b = np.divmod(np.repeat(np.arange(s * s), t.ravel()), s)
        if name == "never_together":                           # each feature observed, on disjoint objects
            at = rng.permutation(PLANTED_N)[:40]
            x[at[:20], 2 * k] = np.arange(20) % 2
            x[at[20:], 2 * k + 1] = np.arange(20) % 2
        else:
            at = rng.permutation(PLANTED_N)[:len(a)]
            order = rng.permutation(len(a))
            x[at, 2 * k], x[at, 2 * k + 1] = a[order], b[order]
        ns[2 * k] = ns[2 * k + 1] = s
    ns[f - 2] = 2                                              # a feature that is NA everywhere
    x[::3, f - 1] = 0                                          # a feature with one state
    ns[f - 1] = 1
    return x, ns


@functools.lru_cache(maxsize=None)
def planted(only_2x2=False):
    """(names, x, n_states, the checker's result): pair (2 k, 2 k + 1) holds PLANTED[names[k]]; the last two features are
    NA everywhere and one-state.  With only_2x2 the 2 x 2 tables alone, so that the call runs at S_pad = 2."""
    names = tuple(PLANTED_2X2 if only_2x2 else PLANTED)
    x, ns = _planted(names)
    x.setflags(write=False)
    ns.setflags(write=False)
    return names, x, ns, ao.feature_association(x, ns)


def planted_table(name, s):
    """PLANTED[name] in the [s, s] frame a call with the largest state count s returns."""
    t = np.zeros((s, s), dtype=np.int64)
    p = PLANTED[name]
    t[:p.shape[0], :p.shape[1]] = p
    return t


# ---- the exact reference -----------------------------------------------------------------------------------------------
def exact_statistic(table):
    """(valid, dof, n, statistic) of one observed table by the contract of tests/_assoc_oracle.py in exact arithmetic:
    occupied rows and columns, E = r c / n, Yates' correction at dof 1; the statistic is a fractions.Fraction."""
    t = np.asarray(table).astype(object)
    r, c = t.sum(axis=1), t.sum(axis=0)
    n = int(r.sum()) if t.size else 0
    rows, cols = [a for a in range(len(r)) if r[a] > 0], [b for b in range(len(c)) if c[b] > 0]
    if len(rows) <= 1 or len(cols) <= 1:
        return False, 0, n, Fraction(0)
    dof = (len(rows) - 1) * (len(cols) - 1)
    stat = Fraction(0)
    for a in rows:
        for b in cols:
            o = Fraction(int(t[a, b]))
            e = Fraction(int(r[a]) * int(c[b]), n)
            if dof == 1:
                d = e - o
                o = o + min(HALF, abs(d)) * (1 if d > 0 else (-1 if d < 0 else 0))
            stat += (o - e) ** 2 / e
    return True, dof, n, stat


def statistic_tolerance(table, exact):
    """The bound on a statistic computed by the contract's fp64 arithmetic against `exact`, as a Fraction:
    ao.statistic_bound(R, C) exact + n 2^-100.  The absolute term covers a Yates term whose exact value is 0: E carries a
    rounding of at most E 2^-52, the clamped difference is then at most that instead of 0, and the term at most
    (E 2^-52)^2 / E <= n 2^-104 per cell."""
    t = np.asarray(table)
    R, C = int(np.count_nonzero(t.sum(axis=1))), int(np.count_nonzero(t.sum(axis=0)))
    return Fraction(float(ao.statistic_bound(R, C))) * exact + Fraction(int(t.sum()), 2 ** 100)


def statistic_within(value, table, exact):
    return abs(Fraction(float(value)) - exact) <= statistic_tolerance(table, exact)


# ---- the large case ----------------------------------------------------------------------------------------------------
LARGE_N = 1 << 24
LARGE_STATES = np.array([2, 2, 3, 3, 32, 2], dtype=np.int32)


def large(n=LARGE_N):
    """(x, n_states) without NA: two binary features that are 0 except at 300 and 260 seeded objects, 40 of them shared (the
    cell (0, 0) of their table is n - 520); two 3-state features, the second a copy of the first changed at 1 object in
    1000; a uniform 32-state feature (S_pad = 32: 21 tile pairs, two launches at n = 2^24); a uniform binary one.  Not
    cached: the codes take 6 n bytes."""
    rng = np.random.default_rng(2024)
    x = np.zeros((n, 6), dtype=np.uint8)
    at = rng.choice(n, 520, replace=False)
    x[at[:300], 0] = 1
    x[at[260:], 1] = 1
    x[:, 2] = rng.integers(0, 3, n, dtype=np.uint8)
    x[:, 3] = x[:, 2]
    moved = rng.choice(n, n // 1000, replace=False)
    x[moved, 3] = (x[moved, 3] + 1 + rng.integers(0, 2, len(moved), dtype=np.uint8)) % 3
    x[:, 4] = rng.integers(0, 32, n, dtype=np.uint8)
    x[:, 5] = rng.integers(0, 2, n, dtype=np.uint8)
    return x, LARGE_STATES.copy()


def bincount_table(x, i, j, s):
    """int64 [s, s]: the table of features i and j of codes without NA (no float32 one-hot at this size)."""
    return np.bincount(x[:, i].astype(np.int64) * s + x[:, j], minlength=s * s).reshape(s, s)


# ---- the position case -------------------------------------------------------------------------------------------------
POSITION_N = 520


@functools.lru_cache(maxsize=None)
def position():
    """(x, n_states, expected n [F, F]): binary; feature 1 + p is observed (state 0) at object p only, features 0 and F - 1
    are anchors observed everywhere with both states.  Every (lane half, dword, nibble) position of the FP4 operand, in each of
    the first eight contraction steps, is then the only object of some feature; the anchors are the row operand of some
    tile pairs and the column operand of others."""
    n = POSITION_N
    rng = np.random.default_rng(520)
    x = np.full((n, n + 2), ao.NA, dtype=np.uint8)
    x[:, 0] = np.arange(n) % 2
    x[:, n + 1] = rng.integers(0, 2, n)
    x[np.arange(n), 1 + np.arange(n)] = 0
    want = np.zeros((n + 2, n + 2), dtype=np.int32)
    want[0, 1:n + 1] = want[n + 1, 1:n + 1] = 1
    want[0, n + 1] = n
    want = want + want.T
    x.setflags(write=False)
    return x, np.full(n + 2, 2, dtype=np.int32), want
