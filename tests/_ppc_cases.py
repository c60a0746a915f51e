"""Cases of the posterior predictive check shared by tests/test_ppc_oracle_cpu.py, tests/test_ppc_files_cpu.py and
tests/test_gpu_ppc.py: the hand-worked case, the grid and the edge cases with explicit dyadic uniforms, seeded random cases and
the recorded runs (through tests/_predict_cases.py) with their oracle results, each computed once.  A plain helper module: it
holds no test."""
import functools
import math

import numpy as np

from tests import _ppc_oracle as orc
from tests import _predict_cases as recorded_cases
from tests import _predict_oracle as predict_orc

NA = orc.NA
SEED = 2201                               # of the recorded runs' replicates


def _one_confounder(N):
    return np.zeros((1, N), dtype=np.uint8), [1]


def hand():
    """Two objects, one feature of four states, the clusters and one confounder of one group, two samples, all entries dyadic.
    Worked by hand:
      sample 0: object 0 is in the cluster, w~ = (1/2, 1/2), m = (3/8, 0, 3/8, 1/4), cdf = (3/8, 3/8, 3/4, 1), u = 1/2 -> y = 2;
                object 1 is not, w~ = (0, 1), m = (1/4, 0, 1/2, 1/4), cdf = (1/4, 1/4, 3/4, 1), u = 3/4 is on a step -> y = 3
      sample 1: object 0 is not in the cluster, m = (0, 0, 1/2, 1/2), u = 1/4 -> y = 2;
                object 1 is, w~ = (1/4, 3/4), m = (0, 1/4, 3/8, 3/8), cdf = (0, 1/4, 5/8, 1), u = 1/4 is on a step -> y = 2,
                and its observed state 0 has no mass: d_obs = +inf."""
    groups, n_groups = _one_confounder(2)
    case = dict(codes=np.array([[2], [0]], dtype=np.uint8), groups=groups, n_groups=n_groups,
                clusters=np.array([[[1, 0]], [[0, 1]]], dtype=np.uint8), weights=np.array([[[0.5, 0.5]], [[0.25, 0.75]]]),
                tables=np.array([[[[0.5, 0.0, 0.25, 0.25]], [[0.25, 0.0, 0.5, 0.25]]], [[[0.0, 1.0, 0.0, 0.0]], [[0.0, 0.0, 0.5, 0.5]]]]))
    uniforms = np.array([[0.5, 0.75], [0.25, 0.25]])
    d = lambda p: -2.0 * math.log(p)                                                                         # noqa: E731
    want = dict(y_rep=[[[2], [3]], [[2], [2]]], count_rep=[[[0, 0, 1, 1]], [[0, 0, 2, 0]]], n_skipped=0,
                dev_feature=[[[d(0.375) + d(0.25)], [d(0.375) + d(0.25)]], [[math.inf], [d(0.5) + d(0.375)]]],
                dev_object=[[[d(0.375), d(0.25)], [d(0.375), d(0.25)]], [[d(0.5), math.inf], [d(0.5), d(0.375)]]])
    return case, uniforms, want


def grid():
    """One sample, 1024 identical cells (64 objects x 16 features) with m = (1/4, 0, 1/2, 1/4) and u_i = (i + 1/2) / 1024 at cell
    i = n F + f: the states are drawn 256, 0, 512, 256 times."""
    N, F = 64, 16
    case = dict(codes=np.zeros((N, F), dtype=np.uint8), groups=np.zeros((0, N), dtype=np.uint8), n_groups=[],
                clusters=np.ones((1, 1, N), dtype=np.uint8), weights=np.ones((1, F, 1)),
                tables=np.ascontiguousarray(np.broadcast_to(np.array([0.25, 0.0, 0.5, 0.25]), (1, 1, F, 4))))
    return case, ((np.arange(N * F) + 0.5) / (N * F))[None]


TOP = 1.0 - 2.0 ** -53                    # the largest uniform


def edges():
    """Explicit dyadic rows and uniforms at the edges of the draw rule; one sample, the clusters and one confounder of one
    group, both with the same table and the weights (1/2, 1/2), so m is the table's row wherever a component applies.
      features: 0: (0, 1/2, 0, 1/2) zero mass first and in the middle; 1: (1/4, 1/4, 1/2, 0) zero mass last;
                2: (1/2, 0, 1/4, 1/4); 3: all NA
      objects:  0: u = 0;  1: u = 1 - 2^-53;  2, 3: u on the cdf steps;  4: in no cluster and no group: skipped;  5: all NA;
                6: u just below the steps of object 2
      codes:    object 0 shows state 0 of feature 0, which has no mass: d_obs = +inf"""
    rows = np.array([[0.0, 0.5, 0.0, 0.5], [0.25, 0.25, 0.5, 0.0], [0.5, 0.0, 0.25, 0.25], [0.25, 0.25, 0.25, 0.25]])
    N, F = 7, 4
    codes = np.array([[0, 0, 0, NA], [1, 2, 3, NA], [3, 1, 2, NA], [1, 0, 0, NA], [1, 1, 2, NA], [NA] * 4, [3, 2, 0, NA]], dtype=np.uint8)
    groups = np.array([[0, 0, 0, 0, NA, 0, 0]], dtype=np.uint8)
    clusters = np.array([[[1, 1, 0, 1, 0, 1, 1]]], dtype=np.uint8)
    case = dict(codes=codes, groups=groups, n_groups=[1], clusters=clusters, weights=np.full((1, F, 2), 0.5),
                tables=np.ascontiguousarray(np.broadcast_to(rows, (1, 2, F, 4))))
    below = lambda v: np.nextafter(v, 0.0)                                                                   # noqa: E731
    u = np.array([[0.0] * 4, [TOP] * 4, [0.5, 0.25, 0.5, 0.5], [0.5, 0.5, 0.75, 0.5], [0.5] * 4, [0.5] * 4,
                  [below(0.5), below(0.25), below(0.5), 0.5]])
    want_y = [[1, 0, 0, NA], [3, 2, 3, NA], [3, 1, 2, NA], [3, 2, 3, NA], [NA] * 4, [NA] * 4, [1, 0, 0, NA]]
    return case, u.reshape(1, N * F), want_y


def off_one():
    """The largest uniform against totals just above and just below 1 (rows that sum to 1 +- 2^-20, inside the tolerance) and
    trailing states without mass: v = u total stays below total, the draw is the last state with mass."""
    N, F = 2, 2
    e = 2.0 ** -20
    rows = np.array([[0.5, 0.5 + e, 0.0, 0.0], [0.25, 0.75 - e, 0.0, 0.0]])
    case = dict(codes=np.zeros((N, F), dtype=np.uint8), groups=np.zeros((0, N), dtype=np.uint8), n_groups=[],
                clusters=np.ones((1, 1, N), dtype=np.uint8), weights=np.ones((1, F, 1)), tables=np.ascontiguousarray(rows[None, None]))
    return case, np.full((1, N * F), TOP)


# (N, F, S, C, K, group counts or None: seeded) at the edges of the tile plan, T = 3 samples each
SHAPES = [(1, 1, 2, 1, 1, None), (15, 16, 3, 2, 2, None), (16, 16, 3, 2, 2, None), (17, 16, 3, 2, 2, None), (33, 15, 2, 3, 3, None),
          (33, 17, 1, 2, 2, None), (20, 33, 5, 3, 3, None), (9, 5, 32, 1, 2, None), (21, 7, 4, 8, 2, None), (5, 3, 32, 2, 3, (253,))]
T_SHAPES = 3


@functools.lru_cache(maxsize=None)
def synthetic(shape, T=T_SHAPES):
    """(case, seed, the oracle's check of it) for a shape of SHAPES; the margin condition holds (asserted on the CPU)."""
    N, F, S, C, K, counts = shape
    seed = 3000 + N + 7 * F + 31 * S + C
    case = predict_orc.random_case(seed, N, F, S, C, K, T, group_counts=list(counts) if counts else None)
    return case, seed, orc.check(seed=seed, **case)


def recorded(r):
    """The arguments of the oracle's check() for recorded run r."""
    return recorded_cases.case(r)


@functools.lru_cache(maxsize=None)
def recorded_oracle(r):
    return orc.check(seed=SEED, **recorded(r))
