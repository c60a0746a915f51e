"""The contract of the per-cluster evidence unit (include/sbe_contrib.h) in NumPy float64, in the contract's
order, with math.log; the same rows in exact rationals for small cases; and the sums in 50-digit arithmetic (mpmath).  A plain
helper module: it holds no test.

For every sample t, every cell (n, f) with a code x != 255 and every cluster k < K (the object's own membership is not used):
    a_c          = h[n,c] w[f,c] for c >= 1;  a_0 = w[f,0]
    wsum1, wsum0 = a_0 + a_1 + .. and a_1 + a_2 + .., in index order
    w1_c, w0_c   = a_c / wsum1 (c >= 0);  a_c / wsum0 (c >= 1)
    m0           = sum_{c >= 1} w0_c tables[row_c(n), f, x], c in order, every product rounded, then added
    m_k          = w1_0 tables[k, f, x] + sum_{c >= 1} w1_c tables[row_c(n), f, x], the same order, the cluster's term first
    d[t,k,n,f]   = log m_k - log m0;  +inf where m0 = 0
    skipped      wsum0 not > 0: for all k;  m_k not > 0: that (cell, k);  a skipped entry is +0.0 and counts in n_skipped
Outputs per sample: affinity [K,N] = sum_f d (the per-object tree of tests/_ppc_oracle.py: 64 lanes, xor exchanges), gain_feature
[K,F] = sum over the members of k of d (its per-feature tree: 16 lanes, then in order; a non-member adds +0.0).

The device's band for the sums (the form and constant of the posterior predictive check's):
    |dev - oracle| <= 2^-50 (n_terms + 4) sum (|log m_k| + |log m0|),   over the sum's terms, +inf compared by class.
The m's of the device and of this module are bit-identical (the same operations in the same order, nothing contracted), so only
the logs differ: each is within an ulp or so of the exact one, the subtraction adds half an ulp of |d| <= |log m_k| + |log m0|,
and the n_terms - 1 additions half an ulp of the partial sums each.  The magnitudes of the two logs are used, not |d|, because d
is a difference.  reference_sums() evaluates what the contract defines -- the logs of those float64 m's, their difference and
the sums -- in 50 digits, so that it measures exactly what the band is about."""
import math
from fractions import Fraction

import numpy as np

from tests._ppc_oracle import sum_over_features, sum_over_objects
from tests._predict_oracle import NA, cluster_ids, row_offsets
from tests import _predict_oracle as predict_orc

KINDS = predict_orc.KINDS
_LOG = np.frompyfunc(math.log, 1, 1)


def band(n_terms, abs_logs):
    return 2.0 ** -50 * (n_terms + 4) * abs_logs


def log_of(m):
    """math.log of every entry > 0, -inf at 0."""
    m = np.asarray(m, dtype=np.float64)
    out = np.full(m.shape, -np.inf)
    pos = m > 0.0
    out[pos] = _LOG(m[pos]).astype(np.float64)
    return out


def rows_of_sample(codes, groups, n_groups, K, weights_t, tables_t):
    """(m [K,N,F], m0 [N,F], formed bool [N,F], w1_0 [N,F]) of one sample in the contract's operation order; formed: the cell
    has a code and a confounder applies (elsewhere m and m0 are 0)."""
    N, F = codes.shape
    C = weights_t.shape[1]
    off, _R = row_offsets(K, n_groups)
    observed = codes != NA
    x = np.where(observed, codes, 0).astype(np.int64)
    f_idx = np.arange(F)[None, :]
    a = np.zeros((N, F, C))
    a[:, :, 0] = weights_t[None, :, 0]
    theta_x = np.zeros((N, F, C))                                           # tables[row_c(n), f, x], c >= 1
    for c in range(1, C):
        has = groups[c - 1] != NA
        rows = np.where(has, off[c] + groups[c - 1].astype(np.int64), 0)
        a[:, :, c] = np.where(has[:, None], weights_t[None, :, c], 0.0)
        theta_x[:, :, c] = tables_t[rows[:, None], f_idx, x]
    wsum1, wsum0 = np.zeros((N, F)), np.zeros((N, F))
    for c in range(C):
        wsum1 = wsum1 + a[:, :, c]
        if c >= 1:
            wsum0 = wsum0 + a[:, :, c]
    formed = observed & (wsum0 > 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        w1 = np.where(formed[..., None], a / wsum1[..., None], 0.0)
        w0 = np.where(formed[..., None], a / wsum0[..., None], 0.0)
    m0 = np.zeros((N, F))
    for c in range(1, C):
        m0 = m0 + w0[:, :, c] * theta_x[:, :, c]
    m = np.zeros((K, N, F))
    for k in range(K):
        mk = w1[:, :, 0] * tables_t[k][f_idx, x]
        for c in range(1, C):
            mk = mk + w1[:, :, c] * theta_x[:, :, c]
        m[k] = np.where(formed, mk, 0.0)
    return m, np.where(formed, m0, 0.0), formed, w1[:, :, 0]


def evaluate(codes, groups, n_groups, clusters, weights, tables):
    """The outputs of one call over all samples, which must be valid: dict(affinity [T,K,N], gain_feature [T,K,F], member bool
    [T,K,N], n_skipped, and for the tests d [T,K,N,F] (0 where nothing is added), counted bool [T,K,N,F], m [T,K,N,F], m0
    [T,N,F], log_m [T,K,N,F] and log_m0 [T,N,F] (0 where not counted))."""
    T, K, N = clusters.shape
    F = weights.shape[1]
    observed = codes != NA
    out = dict(affinity=np.zeros((T, K, N)), gain_feature=np.zeros((T, K, F)), member=np.zeros((T, K, N), dtype=bool), n_skipped=0,
               d=np.zeros((T, K, N, F)), counted=np.zeros((T, K, N, F), dtype=bool), m=np.zeros((T, K, N, F)), m0=np.zeros((T, N, F)),
               log_m=np.zeros((T, K, N, F)), log_m0=np.zeros((T, N, F)))
    for t in range(T):
        ids, twice = cluster_ids(clusters[t])
        assert twice is None
        m, m0, formed, _w = rows_of_sample(codes, groups, n_groups, K, weights[t], tables[t])
        counted = formed[None] & (m > 0.0)
        log_m0 = log_of(m0)
        log_m = log_of(m)
        with np.errstate(invalid="ignore"):
            d = np.where(counted, log_m - log_m0[None], 0.0)
        out["m"][t], out["m0"][t], out["counted"][t], out["d"][t] = m, m0, counted, d
        out["log_m"][t] = np.where(counted, log_m, 0.0)
        out["log_m0"][t] = np.where(counted.any(axis=0), log_m0, 0.0)
        out["n_skipped"] += int((observed[None] & ~counted).sum())
        for k in range(K):
            member = ids == k
            out["member"][t, k] = member
            out["affinity"][t, k] = sum_over_features(d[k])
            out["gain_feature"][t, k] = sum_over_objects(np.where(member[:, None], d[k], 0.0))
    return out


def terms_and_magnitudes(want):
    """For the band: per output the number of terms of every sum and the sum of |log m_k| + |log m0| over them (+inf logs, where
    m0 = 0, count as 0: such a sum is compared by class).  Returns ((terms, magnitude) of affinity [T,K,N], of gain_feature [T,K,F])."""
    counted, member = want["counted"], want["member"]
    with np.errstate(invalid="ignore"):
        mag = np.where(counted, np.abs(want["log_m"]) + np.abs(want["log_m0"][:, None]), 0.0)
    mag = np.where(np.isinf(mag), 0.0, mag)
    mine = counted & member[..., None]
    return (counted.sum(axis=3), mag.sum(axis=3)), (mine.sum(axis=2), np.where(mine, mag, 0.0).sum(axis=2))


def reference_sums(want):
    """(affinity [T,K,N], gain_feature [T,K,F]) as nested lists of mpmath numbers (mp.dps as the caller set it, 50 in the tests):
    the logs of the oracle's float64 m's, their difference and the sums, each evaluated exactly to that precision."""
    import mpmath
    m, m0, counted, member = want["m"], want["m0"], want["counted"], want["member"]
    T, K, N, F = m.shape
    log0 = {}

    def log(v):
        if v not in log0:
            log0[v] = mpmath.log(mpmath.mpf(v)) if v > 0 else -mpmath.inf
        return log0[v]
    affinity = [[[mpmath.mpf(0)] * N for _ in range(K)] for _ in range(T)]
    gain = [[[mpmath.mpf(0)] * F for _ in range(K)] for _ in range(T)]
    for t, k, n, f in zip(*np.nonzero(counted)):
        d = log(float(m[t, k, n, f])) - log(float(m0[t, n, f]))
        affinity[t][k][n] += d
        if member[t, k, n]:
            gain[t][k][f] += d
    return affinity, gain


def exact_rows(codes, groups, n_groups, clusters, weights, tables):
    """The rows in exact rationals for small cases: dict keyed by (t, k, n, f) of (m_k, m0, w1_0, theta) as Fractions, for every
    cell with a code to which a confounder applies (theta = tables[t, k, f, x])."""
    T, K, N = clusters.shape
    F, C = weights.shape[1:]
    off, _R = row_offsets(K, n_groups)
    out = {}
    for t in range(T):
        for n in range(N):
            comp = [(c, off[c] + int(groups[c - 1][n])) for c in range(1, C) if groups[c - 1][n] != NA]
            for f in range(F):
                x = int(codes[n, f])
                if x == NA:
                    continue
                a0 = Fraction(float(weights[t, f, 0]))
                wsum0 = sum((Fraction(float(weights[t, f, c])) for c, _r in comp), Fraction(0))
                if wsum0 <= 0:
                    continue
                conf = sum((Fraction(float(weights[t, f, c])) * Fraction(float(tables[t, r, f, x])) for c, r in comp), Fraction(0))
                for k in range(K):
                    theta = Fraction(float(tables[t, k, f, x]))
                    out[t, k, n, f] = ((a0 * theta + conf) / (a0 + wsum0), conf / wsum0, a0 / (a0 + wsum0), theta)
    return out


def rank(gain_feature):
    """The clusters by the mean over the samples of the exactly rounded sum over the features, descending, ties to the lower index."""
    T, K, _F = gain_feature.shape
    mean = np.array([[math.fsum(gain_feature[t, k]) for k in range(K)] for t in range(T)]).reshape(T, K).mean(axis=0)
    return sorted(range(K), key=lambda k: (-mean[k], k))
