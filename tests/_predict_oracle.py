"""The contract of the posterior-predictive unit (include/sbe_predict.h) in NumPy float64, with the
kernel's summation order, and an exact form in fractions.Fraction for small cases.  A plain helper module: it holds no test.

One sample t of the logged model, for object n, feature f:
    h[n,0] = (n is in a cluster), h[n,c] = (group_c(n) != none)
    wn[n,f,c] = h w[f,c] / sum_c' h w[f,c']          (the sum over c' = 0, 1, .. in order; 0 where the sum is 0)
    m[n,f,s]  = sum_c wn[n,f,c] * tables[row_c(n), f, s]   (c = 0, 1, .. in order; each product rounded, then added)
    pred_sum += m;  observed x with m[x] > 0: resp_sum[n,f,c] += wn_c tables_c[x] / m[x];  m[x] == 0: n_zero += 1
    lik[t, n F + f] = float32(m[x]), 1.0 for an NA cell
The accumulators add the samples in order.

Error bounds (derived in DESIGN.md section 21 from this operation order; u = 2^-53, gamma(k) = k u / (1 - k u)):
    pred_sum: every term passes C - 1 additions of the weight sum, 1 division, 1 product, C - 1 additions over the
              components and T - 1 additions over the samples: k = T + 2 C - 1 roundings, all terms non-negative, so
              |pred - exact| <= gamma(k) exact + 2 C T 2^-1074 (a quotient and a product may underflow per component and sample)
    resp_sum: numerator C + 1 roundings, denominator 2 C, 1 division, T - 1 additions: k = T + 3 C + 1, and per sample an
              absolute (2 C + 3) 2^-1074 / m[x] where products underflowed
    lik:      float32 rounding of a value with 2 C roundings: (2^-24 + gamma(2 C) (1 + 2^-24)) exact, 2^-150 absolute below 2^-126
"""
from fractions import Fraction

import numpy as np

NA = 255
SUM_TOL = 1e-5
U = 2.0 ** -53
TINY = 2.0 ** -1074
KINDS = ("overlap", "weight entry", "weight sum", "table entry", "table row empty", "table sum")


def gamma(k):
    return k * U / (1 - k * U)


def pred_bound(exact, T, C):
    return gamma(T + 2 * C - 1) * exact + 2 * C * T * TINY


def resp_bound(exact, T, C, inv_m_sum):
    """inv_m_sum [N,F]: the sum over the contributing samples of 1 / m[x]."""
    return gamma(T + 3 * C + 1) * exact + (2 * C + 3) * TINY * inv_m_sum[..., None]


def lik_bound(exact, C):
    eps = gamma(2 * C) * (1 + 2.0 ** -24)
    return np.where(exact >= 2.0 ** -126, (2.0 ** -24 + eps) * exact, 2.0 ** -150 + eps * exact)


def row_offsets(K, n_groups):
    """First table row of every component: the clusters, then the confounders' groups in order; and R."""
    off = [0]
    R = K
    for g in n_groups:
        off.append(R)
        R += int(g)
    return off, R


def cluster_ids(clusters):
    """clusters uint8 [K,N] -> (id int [N], -1 = none; the first object in two clusters or None)."""
    member = clusters != 0
    count = member.sum(axis=0)
    ids = np.where(count > 0, member.argmax(axis=0), -1)
    twice = np.flatnonzero(count > 1)
    return ids, (int(twice[0]) if twice.size else None)


def first_offender(clusters, weights, tables):
    """None, or (sample, kind, position) of the first offender in the header's order: by sample, then by kind (KINDS), then by
    position (object; f C + c; f; (r F + f) S + s; r F + f; r F + f)."""
    T, R, F, S = tables.shape
    C = weights.shape[2]
    for t in range(T):
        _ids, twice = cluster_ids(clusters[t])
        if twice is not None:
            return t, 0, twice
        found = []
        for kind0, rows in ((1, weights[t].reshape(F, C)), (3, tables[t].reshape(R * F, S))):
            bad = ~(rows >= 0.0) | np.isinf(rows)
            bad_row = bad.any(axis=1)
            if bad.any():
                at = int(np.flatnonzero(bad.ravel())[0])
                found.append((kind0, at))
            total = np.zeros(rows.shape[0])
            with np.errstate(invalid="ignore"):
                for i in range(rows.shape[1]):
                    total = total + rows[:, i]
                empty = ~bad_row & ~(rows > 0.0).any(axis=1)
                off = ~bad_row & ~empty & (np.abs(total - 1.0) > SUM_TOL)
            if kind0 == 3 and empty.any():
                found.append((4, int(np.flatnonzero(empty)[0])))
            if kind0 == 1:
                off = ~bad_row & (np.abs(total - 1.0) > SUM_TOL)
            if off.any():
                found.append((kind0 + 1 if kind0 == 1 else 5, int(np.flatnonzero(off)[0])))
        if found:
            kind, at = min(found)
            return t, kind, at
    return None


class Sums:
    """The accumulators of a handle."""

    def __init__(self, N, F, S, C):
        self.pred = np.zeros((N, F, S))
        self.resp = np.zeros((N, F, C))
        self.inv_m = np.zeros((N, F))
        self.n_samples = 0
        self.n_zero = 0


def accumulate(sums, codes, groups, n_groups, clusters, weights, tables):
    """Add the samples (clusters uint8 [T,K,N], weights [T,F,C], tables [T,R,F,S]) to `sums`; returns lik float32 [T, N F].
    The samples must be valid (first_offender(...) is None)."""
    T, K, N = clusters.shape
    F, C = weights.shape[1:]
    S = tables.shape[3]
    off, R = row_offsets(K, n_groups)
    assert tables.shape == (T, R, F, S) and codes.shape == (N, F)
    observed = codes != NA
    x = np.where(observed, codes, 0).astype(np.int64)[..., None]
    h = np.zeros((N, C), dtype=bool)
    rows = np.zeros((N, C), dtype=np.int64)
    for c in range(1, C):
        h[:, c] = groups[c - 1] != NA
        rows[:, c] = np.where(h[:, c], off[c] + groups[c - 1].astype(np.int64), 0)
    lik = np.ones((T, N, F), dtype=np.float32)
    for t in range(T):
        ids, twice = cluster_ids(clusters[t])
        assert twice is None
        h[:, 0] = ids >= 0
        rows[:, 0] = np.where(ids >= 0, ids, 0)
        w = np.where(h[:, None, :], weights[t][None, :, :], 0.0)             # [N,F,C]
        wsum = np.zeros((N, F))
        for c in range(C):
            wsum = wsum + w[:, :, c]
        with np.errstate(invalid="ignore", divide="ignore"):
            wn = np.where((wsum > 0.0)[..., None], w / wsum[..., None], 0.0)
        m = np.zeros((N, F, S))
        mx = np.zeros((N, F))
        part = np.empty((N, F, C))
        for c in range(C):
            theta = tables[t][rows[:, c]]                                    # [N,F,S]
            m = m + wn[:, :, c, None] * theta
            part[:, :, c] = wn[:, :, c] * np.take_along_axis(theta, x, axis=2)[..., 0]
            mx = mx + part[:, :, c]
        sums.pred = sums.pred + m
        adds = observed & (mx > 0.0)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            sums.resp = sums.resp + np.where(adds[..., None], part / mx[..., None], 0.0)
            sums.inv_m = sums.inv_m + np.where(adds, 1.0 / mx, 0.0)
        sums.n_zero += int((observed & ~(mx > 0.0)).sum())
        lik[t] = np.where(observed, mx, 1.0).astype(np.float32)
    sums.n_samples += T
    return lik.reshape(T, N * F)


def run(codes, groups, n_groups, clusters, weights, tables):
    """(Sums, lik) of all samples from empty accumulators."""
    N, F = codes.shape
    sums = Sums(N, F, tables.shape[3], weights.shape[2])
    return sums, accumulate(sums, codes, groups, n_groups, clusters, weights, tables)


def impute(codes, pred_sum):
    """(codes with the NA cells filled by the arg-max state, ties to the lowest index; the filled state's share of the sum)."""
    best = pred_sum.argmax(axis=2)
    filled = np.where(codes == NA, best, codes).astype(np.uint8)
    total = pred_sum.sum(axis=2)
    return filled, np.take_along_axis(pred_sum, best[..., None], axis=2)[..., 0] / total


def exact(codes, groups, n_groups, clusters, weights, tables):
    """The contract in exact arithmetic: (pred_sum [N][F][S], resp_sum [N][F][C], lik [T][N F], inv_m [N][F], n_zero) as nested
    lists of Fractions (small cases only)."""
    T, K, N = clusters.shape
    F, C = weights.shape[1:]
    S = tables.shape[3]
    off, _R = row_offsets(K, n_groups)
    fw = [[[Fraction(float(v)) for v in row] for row in wt] for wt in weights]
    ft = [[[[Fraction(float(v)) for v in st] for st in fr] for fr in tt] for tt in tables]
    pred = [[[Fraction(0)] * S for _ in range(F)] for _ in range(N)]
    resp = [[[Fraction(0)] * C for _ in range(F)] for _ in range(N)]
    inv_m = [[Fraction(0)] * F for _ in range(N)]
    lik = [[Fraction(1)] * (N * F) for _ in range(T)]
    n_zero = 0
    for t in range(T):
        ids, twice = cluster_ids(clusters[t])
        assert twice is None
        for n in range(N):
            comp = [(0, int(ids[n]))] if ids[n] >= 0 else []
            comp += [(c, off[c] + int(groups[c - 1][n])) for c in range(1, C) if groups[c - 1][n] != NA]
            for f in range(F):
                total = sum((fw[t][f][c] for c, _r in comp), Fraction(0))
                wn = {c: (fw[t][f][c] / total if total > 0 else Fraction(0)) for c, _r in comp}
                m = [sum((wn[c] * ft[t][r][f][s] for c, r in comp), Fraction(0)) for s in range(S)]
                pred[n][f] = [a + b for a, b in zip(pred[n][f], m)]
                x = int(codes[n, f])
                if x == NA:
                    continue
                lik[t][n * F + f] = m[x]
                if m[x] > 0:
                    for c, r in comp:
                        resp[n][f][c] += wn[c] * ft[t][r][f][x] / m[x]
                    inv_m[n][f] += 1 / m[x]
                else:
                    n_zero += 1
    return pred, resp, lik, inv_m, n_zero


# ---- seeded cases ---------------------------------------------------------------------------------------------------------
def random_case(seed, N, F, S, C, K, T, group_counts=None, na_share=0.1, out_share=0.2, digits=None, states_per_feature=None):
    """A seeded valid case: dict(codes, groups, n_groups, clusters, weights, tables).  Features have 2 .. S applicable states
    (the table is zero behind them); out_share of the objects are in no cluster of a sample, and in no group of a confounder.
    digits: round the entries as the stats files print them (%.{digits}g), the rows then sum to 1 only within the tolerance."""
    rng = np.random.default_rng(seed)
    n_groups = list(group_counts) if group_counts is not None else [int(rng.integers(1, 4)) for _ in range(C - 1)]
    assert len(n_groups) == C - 1
    _off, R = row_offsets(K, n_groups)
    sf = np.asarray(states_per_feature) if states_per_feature is not None else rng.integers(min(2, S), S + 1, size=F)
    codes = rng.integers(0, 1 << 30, size=(N, F)) % sf[None, :]
    codes = np.where(rng.random((N, F)) < na_share, NA, codes).astype(np.uint8)
    groups = np.full((max(C - 1, 0), N), NA, dtype=np.uint8)
    for c in range(C - 1):
        g = rng.integers(0, n_groups[c], size=N)
        groups[c] = np.where(rng.random(N) < out_share, NA, g)
    clusters = np.zeros((T, K, N), dtype=np.uint8)
    for t in range(T):
        k = rng.integers(0, K, size=N)
        inside = rng.random(N) >= out_share
        clusters[t, k[inside], np.flatnonzero(inside)] = 1
    weights = rng.gamma(1.0, size=(T, F, C))
    weights /= weights.sum(axis=2, keepdims=True)
    tables = rng.gamma(0.7, size=(T, R, F, S)) + 1e-12
    tables *= (np.arange(S)[None, :] < sf[:, None])[None, None]
    tables /= tables.sum(axis=3, keepdims=True)
    if digits is not None:
        fmt = np.vectorize(lambda v: float(f"%.{digits}g" % np.float32(v)))
        weights, tables = fmt(weights), fmt(tables)
    return dict(codes=codes, groups=groups, n_groups=n_groups, clusters=clusters, weights=np.ascontiguousarray(weights),
                tables=np.ascontiguousarray(tables))
