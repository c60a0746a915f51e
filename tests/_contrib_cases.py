"""Cases of the per-cluster evidence unit shared by tests/test_contrib_oracle_cpu.py, tests/test_contrib_files_cpu.py and
tests/test_gpu_contrib.py: the dyadic hand case, the edge cases by construction, seeded random cases and the recorded runs
(through tests/_predict_cases.py) with their oracle results, each computed once.  A plain helper module: it holds no test."""
import functools
import math

import numpy as np

from tests import _contrib_oracle as orc
from tests import _predict_cases as recorded_cases
from tests import _predict_oracle as predict_orc

NA = orc.NA
LOG2 = math.log(2.0)


def hand():
    """Three objects, two features of four states, two clusters and one confounder of one group, two samples with the same
    draws; every entry is dyadic and every m a power of two.  Worked by hand:
      feature 0: w = (1/2, 1/2), the group's row (1/4, 1/4, 1/2, 0): m0 = 1/4, 1/4, 1/2 at the objects' states 0, 1, 2;
                 cluster 0's row (3/4, 1/4, 0, 0): m_0 = 1/2, 1/4, 1/4, d = log 2, 0 (theta_k[x] = m0), -log 2;
                 cluster 1's row (1/4, 3/4, 0, 0): m_1 = 1/4, 1/2, 1/4, d = 0, log 2, -log 2
      feature 1: w = (0, 1): m_k = m0 and d = 0 for every k; object 2 has no code there
      sample 0: a0 = {0}, a1 = {1}, object 2 in no cluster;  sample 1: a0 = {2}, a1 = {0, 1}."""
    row_f1 = [0.5, 0.5, 0.0, 0.0]
    draw = [[[0.75, 0.25, 0.0, 0.0], row_f1], [[0.25, 0.75, 0.0, 0.0], row_f1], [[0.25, 0.25, 0.5, 0.0], row_f1]]
    case = dict(codes=np.array([[0, 0], [1, 1], [2, NA]], dtype=np.uint8), groups=np.zeros((1, 3), dtype=np.uint8), n_groups=[1],
                clusters=np.array([[[1, 0, 0], [0, 1, 0]], [[0, 0, 1], [1, 1, 0]]], dtype=np.uint8),
                weights=np.array([[[0.5, 0.5], [0.0, 1.0]]] * 2), tables=np.array([draw] * 2))
    want = dict(affinity=[[[LOG2, 0.0, -LOG2], [0.0, LOG2, -LOG2]]] * 2, n_skipped=0,
                gain_feature=[[[LOG2, 0.0], [LOG2, 0.0]], [[-LOG2, 0.0], [LOG2, 0.0]]], rank=[1, 0],
                m=[[[0.5, 0.5], [0.25, 0.5], [0.25, 0.0]], [[0.25, 0.5], [0.5, 0.5], [0.25, 0.0]]], m0=[[0.25, 0.5], [0.25, 0.5], [0.5, 0.0]])
    return case, want


def no_mass_outside():
    """m0 = 0 with m_k > 0: two objects, two features of two states, two clusters, one confounder of one group, one sample.  The
    group's row of feature 0 is (1, 0) and both objects show state 1: m0 = 0.  Cluster 0's row (1/2, 1/2) gives m_0 = 1/4 and
    d = +inf; cluster 1's row (1, 0) gives m_1 = 0: skipped.  Feature 1 is ordinary (m0 = 1/2, m_k = 1/2: d = 0).  Object 0 is
    in cluster 0, object 1 in none: affinity[0] = (+inf, +inf), gain_feature[0] = (+inf, 0); cluster 1 has only skipped entries
    on feature 0 and zeros."""
    half = [0.5, 0.5]
    case = dict(codes=np.array([[1, 0], [1, 1]], dtype=np.uint8), groups=np.zeros((1, 2), dtype=np.uint8), n_groups=[1],
                clusters=np.array([[[1, 0], [0, 0]]], dtype=np.uint8), weights=np.array([[[0.5, 0.5], [0.5, 0.5]]]),
                tables=np.array([[[half, half], [[1.0, 0.0], half], [[1.0, 0.0], half]]]))
    want = dict(affinity=[[[math.inf, math.inf], [0.0, 0.0]]], gain_feature=[[[math.inf, 0.0], [0.0, 0.0]]], n_skipped=2)
    return case, want


def without_a_group():
    """An object with no confounder group next to one with a group (seeded, 4 objects x 5 features, C = 3): objects 1 and 3 are
    in no group of either confounder, so exactly their cells with a code are skipped, for every k."""
    case = predict_orc.random_case(2405, 4, 5, 3, 3, 2, 2, na_share=0.2)
    case["groups"][:, [1, 3]] = NA
    case["groups"][0, [0, 2]] = 0                                            # (and the others in at least one)
    return case


# (N, F, S, C, K, group counts or None: seeded), T = 3 samples each: the smallest shapes at which each mechanism can go wrong
SHAPES = [(5, 3, 2, 2, 1, None),
          (17, 7, 5, 3, 3, None),          # N one past the feature tree's 16 lanes
          (33, 65, 4, 2, 2, None),         # F one past a wave
          (21, 130, 3, 8, 4, None),        # C at its limit, a third round of the object tree
          (7, 4, 32, 2, 2, None), (7, 4, 1, 2, 2, None),   # S at both ends
          (6, 2, 2, 2, 255, (1,)),         # one universal group: R = 256
          (9, 5, 3, 1, 2, None)]           # C = 1: every cell is skipped
T_SHAPES = 3


@functools.lru_cache(maxsize=None)
def synthetic(shape, T=T_SHAPES):
    """(case, the oracle's evaluation of it) for a shape of SHAPES."""
    N, F, S, C, K, counts = shape
    seed = 2400 + N + 7 * F + 31 * S + C
    case = predict_orc.random_case(seed, N, F, S, C, K, T, group_counts=list(counts) if counts else None)
    if counts == (1,):
        case["groups"][:] = 0                                                # universal: every object is in the one group
    return case, orc.evaluate(**case)


def recorded(r):
    """The arguments of the oracle's evaluate() for recorded run r."""
    return recorded_cases.case(r)


@functools.lru_cache(maxsize=None)
def recorded_oracle(r):
    return orc.evaluate(**recorded(r))
