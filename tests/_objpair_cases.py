"""The seeded cases of the object-pair posterior predictive check, shared by tests/test_objpair_oracle_cpu.py (which proves under
the checker alone that every case holds what it claims) and tests/test_gpu_objpair.py (device against checker).  A plain helper
module: it holds no test.

A case is (x uint8 [N, F], n_states int32 [F], y uint8 [T, N, F]), all read-only, and the checker's result, computed once.  The
objects are points in the unit square and their states follow the quarter of the square they lie in, so some pairs agree far more
often than others.  N lies around the 32 objects of a tile (one, two, three and four tiles), F at 1, 3 and 17, and the state
counts are mixed in 1 .. 32 so that E, their sum, lies at the edges of the 256 elements of a round.  Where the shape allows
(N > 2, F > 2) one object and one feature are all NA and the last feature has a single state.  The replicates:

  replicate 0      the data itself: every pair ties (n_equal);
  replicates 1 ..  every column permuted on its own among its observed objects: the data's margins without the pairs;
  replicate 2      also gains cells the data lacks (the unit does not require the data's NA pattern);
  the last one     loses more cells (skipped cells of a check)."""
from __future__ import annotations

import functools

import numpy as np

from tests import _objpair_oracle as orc

NA = orc.NA
T = 5

# name -> (seed, N, F, E or None: as drawn, NA rate)
CASES = {
    "n1": (61, 1, 3, None, 0.0),
    "n2": (62, 2, 1, None, 0.0),
    "n31": (63, 31, 17, 255, 0.2),
    "n32": (64, 32, 17, 256, 0.1),
    "n33": (65, 33, 17, 257, 0.2),
    "n33_f3": (66, 33, 3, None, 0.3),
    "n64": (67, 64, 17, 511, 0.2),
    "n65": (68, 65, 17, 512, 0.1),
    "n65_f1": (69, 65, 1, None, 0.2),
    "n97": (70, 97, 17, 513, 0.2),
}


def state_counts(rng, f, e):
    """int32 [f] in 1 .. 32, mixed, the last one 1 when f > 2, summing to e (None: as drawn)."""
    ns = rng.integers(2, orc.MAX_STATES + 1, f).astype(np.int64)
    if f > 2:
        ns[-1] = 1
    free = f - 1 if f > 2 else f
    if e is not None:
        assert free + (f - free) <= e <= orc.MAX_STATES * free + (f - free)
        k = 0
        while ns.sum() != e:                                      # one state at a time, round the free features
            step = 1 if ns.sum() < e else -1
            if 1 <= ns[k % free] + step <= orc.MAX_STATES:
                ns[k % free] += step
            k += 1
    return ns.astype(np.int32)


def _build(name):
    seed, n, f, e, na_rate = CASES[name]
    rng = np.random.default_rng(seed)
    points = rng.random((n, 2))
    quarter = (points[:, 0] > 0.5).astype(np.int64) * 2 + (points[:, 1] > 0.5)
    ns = state_counts(rng, f, e)
    follow = rng.random((n, f)) < 0.7
    x = np.where(follow, quarter[:, None] % ns[None, :], rng.integers(0, ns[None, :], (n, f))).astype(np.uint8)
    x[rng.random((n, f)) < na_rate] = NA
    if n > 2:
        x[n // 2, :] = NA                                         # one object all NA
    if f > 2:
        x[:, 1] = NA                                              # one feature all NA
    y = np.repeat(x[None], T, axis=0)
    for t in range(1, T):
        for k in range(f):
            at = np.nonzero(x[:, k] != NA)[0]
            y[t, at, k] = x[rng.permutation(at), k]
    gain = (y[2] == NA) & (rng.random((n, f)) < 0.5)
    y[2][gain] = rng.integers(0, ns[None, :], (n, f)).astype(np.uint8)[gain]
    y[-1][rng.random((n, f)) < 0.1] = NA
    return x, ns, y


@functools.lru_cache(maxsize=None)
def case(name):
    """(x, n_states, y, the checker's result) of the case."""
    x, ns, y = _build(name)
    for a in (x, ns, y):
        a.setflags(write=False)
    return x, ns, y, orc.check(x, ns, y)


@functools.lru_cache(maxsize=None)
def limit(kind):
    """The accumulator's limits at N = 33 (two tiles), F = 4096: (x, n_states, y [2, N, F], the checker's result).
      "one_state"  every cell in state 1 of 2: every agree and comparable is 4096, the largest count there is;
      "elements"   every feature of 32 states, E = 131072, the longest contraction axis; seeded codes with some NA."""
    n, f = 33, orc.MAX_FEATURES
    if kind == "one_state":
        ns = np.full(f, 2, dtype=np.int32)
        x = np.ones((n, f), dtype=np.uint8)
        y = np.stack([x, np.zeros_like(x)])
    else:
        rng = np.random.default_rng(71)
        ns = np.full(f, orc.MAX_STATES, dtype=np.int32)
        x = rng.integers(0, 4, (n, f)).astype(np.uint8) * 8 + (np.arange(f) % 8).astype(np.uint8)[None, :]     # four states a feature, up to 31
        x[rng.random((n, f)) < 0.05] = NA
        y = np.stack([x, rng.permuted(x, axis=0)])
    for a in (x, ns, y):
        a.setflags(write=False)
    return x, ns, y, orc.check(x, ns, y)


def hand():
    """Three objects, three features of 2, 3 and 1 states:
          object 0: 0, 2, 0      object 1: 0, NA, 0      object 2: 1, 2, 0
      agree (0,1) = 2 of 2 comparable, (0,2) = 2 of 3, (1,2) = 1 of 2.
    Replicate 0 is the data (three ties).  Replicate 1 sets feature 0 to one state: (0,1) 2 =, (0,2) 3 >, (1,2) 2 >.  Replicate 2
    gives object 1 the state 0 of feature 1 and object 2 the state 0 of feature 0, and loses object 0's feature 2:
    0, 2, NA / 0, 0, 0 / 0, 2, 0: (0,1) 1 <, (0,2) 2 =, (1,2) 2 >."""
    x = np.array([[0, 2, 0], [0, NA, 0], [1, 2, 0]], dtype=np.uint8)
    y1 = x.copy()
    y1[:, 0] = 0
    y2 = np.array([[0, 2, NA], [0, 0, 0], [0, 2, 0]], dtype=np.uint8)
    return x, np.array([2, 3, 1], dtype=np.int32), np.stack([x, y1, y2])
