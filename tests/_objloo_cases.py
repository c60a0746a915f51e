"""Cases of the leave-one-object-out unit shared by tests/test_objloo_oracle_cpu.py, tests/test_objloo_files_cpu.py and
tests/test_gpu_objloo.py: the dyadic hand case, seeded cases per shape and per number of samples, the duplicated samples, the
column past the LDS budget, the cases with a hypothesis of zero likelihood and the recorded runs (through
tests/_loopred_cases.py), each with its checker result computed once.  A plain helper module: it holds no test."""
import functools

import numpy as np

from tests import _loopred_cases as loopred_cases
from tests import _objloo_oracle as orc
from tests import _predict_oracle as po

NA = orc.NA
SAMPLES = ("clusters", "weights", "tables")


def hand():
    """Two objects, one feature of two states, one cluster, one confounder of one group, two samples, a uniform prior (1/2, 1/2);
    every entry dyadic.  Sample 0: w = (1/2, 1/2), the cluster's row (1/4, 3/4), the group's (1/2, 1/2): m0 = (1/2, 1/2),
    m_1 = (3/8, 5/8).  Sample 1: w = (1/4, 3/4), the cluster's row (1, 0), the group's (1/2, 1/2): m0 = (1/2, 1/2), m_1 = (5/8, 3/8).
    Object 0 shows state 0 and is logged in the cluster in sample 0 only; object 1 has no code.
        object 0: exp(H) = (1/2, 3/8), (1/2, 5/8);  exp(L) = 7/16, 9/16;  exp(Cnd) = 3/8, 1/2
                  T = 2 has a tail of one, so the weights are raw: w = (16/7, 16/9) / (256/63) = (9/16, 7/16),
                  loo_i = log(2 / (16/7 + 16/9)) = log(63/128), lppd_i = log(1/2), n_eff = 256/130;
                  conditional: loo_cond_i = log(2 / (8/3 + 2)) = log(3/7), lppd_cond_i = log(7/16);
                  membership = ((1/4) / (7/16) + (1/4) / (9/16)) / 2 = 32/63 for "no cluster", 31/63 for the cluster;
                  mz = (7/16, 9/16), (9/16, 7/16): p_loo = 9/16 (7/16, 9/16) + 7/16 (9/16, 7/16) = (63/128, 65/128)
        object 1: H = 0, L = Cnd = 0, w = (1/2, 1/2), loo_i = 0, membership (1/2, 1/2), p_loo = (1/2, 1/2), its k infinite too."""
    case = dict(codes=np.array([[0], [NA]], dtype=np.uint8), groups=np.array([[0, 0]], dtype=np.uint8), n_groups=[1],
                clusters=np.array([[[1, 0]], [[0, 0]]], dtype=np.uint8), weights=np.array([[[0.5, 0.5]], [[0.25, 0.75]]]),
                tables=np.array([[[[0.25, 0.75]], [[0.5, 0.5]]], [[[1.0, 0.0]], [[0.5, 0.5]]]]))
    want = dict(expL=[[7 / 16, 1.0], [9 / 16, 1.0]], expCnd=[[3 / 8, 1.0], [1 / 2, 1.0]], w=[[9 / 16, 1 / 2], [7 / 16, 1 / 2]],
                loo_i=[np.log(63 / 128), 0.0], lppd_i=[np.log(1 / 2), 0.0], n_eff=[256 / 130, 2.0], loo_cond_i=[np.log(3 / 7), 0.0],
                lppd_cond_i=[np.log(7 / 16), 0.0], membership=[[32 / 63, 31 / 63], [0.5, 0.5]],
                p_loo=[[[63 / 128, 65 / 128]], [[0.5, 0.5]]])
    return case, want


def shaped(seed, N, F, S, C, K, T):
    """A seeded case in which every observed cell has a confounder and a positive likelihood under every hypothesis: NA cells
    scattered, the last feature all NA (F >= 3), object 0 in no cluster of any sample, the last object (N >= 3) in no cluster and in
    no group and without a code (its cells have no confounder: m0 = 0 there, which only the second pass sees).  With C = 1 no
    confounder exists, so no cell may have a code: all are NA."""
    case = po.random_case(seed, N, F, S, C, K, T, na_share=0.15, out_share=0.25)
    codes, groups, clusters = case["codes"], case["groups"], case["clusters"]
    if C == 1:
        codes[:] = NA
        return case
    if F >= 3:
        codes[:, F - 1] = NA
    groups[0] = np.where(groups[0] == NA, 0, groups[0])                 # (a confounder for every object)
    clusters[:, :, 0] = 0
    if N >= 3:
        clusters[:, :, N - 1] = 0
        groups[:, N - 1] = NA
        codes[N - 1, :] = NA
    if (codes == NA).all():
        codes[0, 0] = 0                                            # (at least one observed cell)
    return case


def seeded_prior(seed, T, N, K, zero=True):
    """A seeded prior [T, N, K+1] of dyadic-free rows that sum to 1 within rounding; with `zero`, object 0's last cluster is
    excluded in every sample (K >= 2; object 0 is logged in no cluster, so its conditional column stays finite)."""
    rng = np.random.default_rng(seed)
    p = rng.gamma(2.0, size=(T, N, K + 1))
    if zero and K >= 2:
        p[:, 0, K] = 0.0
    return p / p.sum(axis=2, keepdims=True)


# name -> (seed, N, F, S, C, K, T, the feature tile the GPU test forces): the tree's edges F = 1, 63, 64, 65, 129; K = 1 and 4;
# C = 1, 2 and 3; N = 1, 2 and 9; S = 2 and 32
BY_SHAPE = {"F1": (3201, 1, 1, 2, 3, 1, 3, 0), "F63": (3263, 2, 63, 32, 3, 4, 3, 0), "F64": (3264, 9, 64, 2, 2, 1, 2, 5),
            "F65": (3265, 9, 65, 5, 3, 4, 3, 16), "F129": (3229, 2, 129, 3, 3, 4, 2, 3), "C1": (3211, 2, 3, 2, 1, 2, 3, 0)}
# T -> (seed, N, F, S, C, K, tile): T = 5 and 20 have a tail of at most four (no fit: k = inf), T = 21 the first fit.  The seeds are
# those for which tests/_psens_oracle.tol_k is finite for every column of both kinds (checked on the CPU).  T = 21 is the case the GPU
# test forces every feature tile on: its two slices of 256 features, 2 x 256 x (R S + C) x 8 bytes with R <= 9 and S = 4, fit the LDS
BY_SAMPLES = {2: (3302, 3, 3, 2, 2, 2, 0), 5: (3305, 4, 3, 3, 2, 2, 1), 20: (3320, 4, 4, 3, 3, 2, 2), 21: (3321, 5, 17, 4, 3, 3, 4),
              64: (3364, 4, 5, 4, 2, 3, 2), 257: (3357, 3, 3, 3, 2, 2, 0)}


@functools.lru_cache(maxsize=None)
def by_shape(name):
    """(case, prior, the checker's run of it) of BY_SHAPE: a seeded prior with an excluded hypothesis where K >= 2."""
    seed, N, F, S, C, K, T, _tile = BY_SHAPE[name]
    case = shaped(seed, N, F, S, C, K, T)
    prior = seeded_prior(seed, T, N, K)
    return case, prior, orc.run(**case, prior=prior)


@functools.lru_cache(maxsize=None)
def synthetic(T):
    """(case, None: the uniform prior, the checker's run) for a number of samples of BY_SAMPLES."""
    seed, N, F, S, C, K, _tile = BY_SAMPLES[T]
    case = shaped(seed, N, F, S, C, K, T)
    return case, None, orc.run(**case)


@functools.lru_cache(maxsize=None)
def duplicated():
    """32 samples, each passed twice in a row: T = 64 with exact ties in every column and in the tail."""
    base = shaped(3365, 4, 4, 3, 2, 2, 32)
    case = {k: (np.ascontiguousarray(np.repeat(v, 2, axis=0)) if k in SAMPLES else v) for k, v in base.items()}
    return case, None, orc.run(**case)


@functools.lru_cache(maxsize=None)
def long_column(T):
    """N = 2, F = 1, S = 2, K = 1, C = 2 with T samples (the GPU test: one past what a column's workgroup sorts in LDS)."""
    case = po.random_case(3399, 2, 1, 2, 2, 1, T, group_counts=[1], na_share=0.0, out_share=0.3, states_per_feature=[2])
    case["groups"][:] = 0
    return case, None, orc.run(**case)


def zero_likelihood(kind):
    """The T = 21 case with sample 4 changed so that the state object 1 shows at feature 0 has no mass in cluster 0's row and in
    the rows of the groups of object 1: m0 = 0 and m_1 = 0 for every object that shows the state there and shares the groups.  All
    objects but object 0 are logged in the last cluster in sample 4.
        "finite"       the other clusters keep their mass: H has -inf entries, L and Cnd stay finite
        "conditional"  object 1 is logged in cluster 0 in sample 4: its Cnd is -inf
        "marginal"     every cluster's row loses the state's mass: L of object 1 is -inf
    Returns (case, (object, sample))."""
    case = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in synthetic(21)[0].items()}
    codes, groups, clusters, tables = case["codes"], case["groups"], case["clusters"], case["tables"]
    K, N = clusters.shape[1:]
    t, n, f = 4, 1, 0
    assert codes[n, f] != NA
    codes[0, f] = NA                                           # (object 0 is logged in no cluster: its Cnd would be H_0)
    x = int(codes[n, f])
    off, _R = po.row_offsets(K, case["n_groups"])
    rows = [0] + [off[c] + int(groups[c - 1, n]) for c in range(1, len(off)) if groups[c - 1, n] != NA]
    if kind == "marginal":
        rows += list(range(1, K))
    tables[t, rows, f, x] = 0.0
    tables[t, rows, f] /= tables[t, rows, f].sum(axis=1, keepdims=True)
    clusters[t] = 0
    clusters[t, K - 1, 1:N - 1] = 1
    if kind == "conditional":
        clusters[t, :, n] = 0
        clusters[t, 0, n] = 1
    assert po.first_offender(clusters, case["weights"], tables) is None
    return case, (n, t)


def recorded(r):
    """The arguments of the checker's run() for recorded run r after the burn-in (tests/_loopred_cases.py)."""
    return loopred_cases.recorded(r)


@functools.lru_cache(maxsize=None)
def recorded_oracle(r):
    return orc.run(**recorded(r))


def all_ratios(run):
    """The vectors of log ratios PSIS sees in a checker's run: -L and -Cnd of every object, as (label, ratios)."""
    return [(f"{name}[{n}]", -run[name][:, n]) for name in ("L", "Cnd") for n in range(run["L"].shape[1])]
