"""Cases of the leave-one-out predictive unit shared by tests/test_loopred_oracle_cpu.py, tests/test_loopred_files_cpu.py and
tests/test_gpu_loopred.py: the dyadic hand case, seeded cases per number of samples, the duplicated samples, the column past the
LDS budget and the recorded runs (through tests/_predict_cases.py), each with its oracle result computed once.  A plain helper
module: it holds no test."""
import functools

import numpy as np

from tests import _loopred_oracle as orc
from tests import _predict_cases as recorded_cases
from tests import _predict_oracle as po

NA = orc.NA


def hand():
    """The posterior predictive's hand case (two objects, one feature of two states, the clusters and one confounder, two samples;
    object 0 shows state 0, object 1 is missing and in no group) worked on: lik = (7/8, 1/4) for the one observed cell, T = 2 has a
    tail of one, so the weights are raw: w = (8/7, 4) / (36/7) = (2/9, 7/9); m_0 = (7/8, 1/8), m_1 = (1/4, 3/4):
    p_loo = (2/9 7/8 + 7/9 1/4, 2/9 1/8 + 7/9 3/4) = (7/18, 11/18), loo_i = log 7/18 (the harmonic mean of the two), n_eff = 81/53."""
    case = dict(codes=np.array([[0], [NA]], dtype=np.uint8), groups=np.array([[0, NA]], dtype=np.uint8), n_groups=[1],
                clusters=np.array([[[1, 0]], [[0, 0]]], dtype=np.uint8), weights=np.array([[[0.25, 0.75]], [[0.5, 0.5]]]),
                tables=np.array([[[[0.5, 0.5]], [[1.0, 0.0]]], [[[0.125, 0.875]], [[0.25, 0.75]]]]))
    want = dict(lik=[[0.875], [0.25]], w=[[2 / 9], [7 / 9]], p_loo=[[[7 / 18, 11 / 18]], [[0.0, 0.0]]], n_eff=81 / 53)
    return case, want


def shaped(seed, N, F, S, C, K, T):
    """A seeded case in which every mechanism of the data is present and every observed cell has a positive likelihood in
    every sample: NA cells scattered, the last feature all NA (F >= 2), object 0 in no cluster of any sample, object 1 in no group
    of any confounder, the last object (N >= 3) in neither and without a code; everyone else has at least one component."""
    case = po.random_case(seed, N, F, S, C, K, T, na_share=0.15, out_share=0.25)
    codes, groups, clusters = case["codes"], case["groups"], case["clusters"]
    if F >= 2:
        codes[:, F - 1] = NA
    for n in range(N):
        if C >= 2 and groups[0, n] == NA:
            groups[0, n] = 0                                   # (a component for every sample)
        if C == 1:
            outside = ~clusters[:, :, n].any(axis=1)
            clusters[outside, 0, n] = 1
    if C >= 2:
        clusters[:, :, 0] = 0
        if N >= 2:
            groups[:, 1] = NA
            clusters[:, :, 1] = 0
            clusters[:, 0, 1] = 1
    if N >= 3:
        clusters[:, :, N - 1] = 0
        groups[:, N - 1] = NA
        codes[N - 1, :] = NA
    if (codes[:, :max(F - 1, 1)] == NA).all():
        codes[min(1, N - 1), 0] = 0                            # (at least one observed cell)
    return case


# T -> (seed, N, F, S, C, K, the feature tile the GPU test forces); T = 20 has a tail of four (no fit), T = 21 the first fit.
# The seeds are those for which every column is clear of the fit's branch edges (orc.away_from_edges; checked on the CPU).
BY_SAMPLES = {2: (2602, 4, 3, 2, 2, 1, 1), 20: (2620, 6, 4, 3, 1, 2, 2), 21: (2621, 9, 17, 5, 3, 3, 4), 64: (2664, 7, 5, 4, 2, 3, 2),
              300: (2630, 4, 3, 3, 3, 2, 1)}
SMALLEST = (2601, 2, 1, 2, 1, 1, 2)                            # (seed, N, F, S, C, K, T): one feature, one component


@functools.lru_cache(maxsize=None)
def synthetic(T):
    """(case, the oracle's run of it) for a number of samples of BY_SAMPLES."""
    seed, N, F, S, C, K, _tile = BY_SAMPLES[T]
    case = shaped(seed, N, F, S, C, K, T)
    return case, orc.run(**case)


@functools.lru_cache(maxsize=None)
def smallest():
    case = shaped(*SMALLEST)
    return case, orc.run(**case)


@functools.lru_cache(maxsize=None)
def duplicated():
    """32 samples, each passed twice in a row: T = 64 with exact ties in every column and in the tail."""
    base = shaped(2665, 6, 4, 3, 2, 2, 32)
    case = {k: (np.ascontiguousarray(np.repeat(v, 2, axis=0)) if k in ("clusters", "weights", "tables") else v) for k, v in base.items()}
    return case, orc.run(**case)


@functools.lru_cache(maxsize=None)
def long_column(T):
    """N = 2, F = 2, S = 2, K = 1, C = 1 with T samples (the GPU test: one past what a column's workgroup stages in LDS)."""
    case = po.random_case(2699, 2, 2, 2, 1, 1, T, na_share=0.0, out_share=0.0, states_per_feature=[2, 2])
    return case, orc.run(**case)


BURN = 6                                                       # of the recorded runs' 60 samples at burnin = 0.1


def recorded(r, burn=BURN):
    """The arguments of the oracle's run() for recorded run r after the burn-in."""
    case = recorded_cases.case(r)
    return {k: (v[burn:] if k in ("clusters", "weights", "tables") else v) for k, v in case.items()}


@functools.lru_cache(maxsize=None)
def recorded_oracle(r, burn=BURN):
    return orc.run(**recorded(r, burn))
