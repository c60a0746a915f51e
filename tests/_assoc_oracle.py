"""NumPy fp64 restatement of the screening loop of sbayes/tools/find_correlated_features.py: for every pair of features
the contingency table over the objects where both are observed (pd.crosstab), then scipy.stats.chi2_contingency
(Pearson's statistic, Yates' correction at one degree of freedom, p-value from the chi-squared survival function).
The checker of sbayes_amd.assoc; tests/golden/assoc.npz holds what pandas and SciPy themselves return.

Numerical contract (sbayes_amd.assoc and the kernels of csrc/sbe_assoc.hip implement the same):

* input `x`: uint8 [N, F] state codes, 255 = not observed; `n_states[f]` bounds the codes of feature f;
* per pair i < j: T[a][b] = #{n : x[n, i] = a and x[n, j] = b}; margins r_a, c_b; total n.  All tables at once are
  X^T X of the one-hot matrix (an NA row is all zero, so it drops the objects pandas drops);
* R = #{a : r_a > 0}, C likewise; the pair is valid iff R > 1 and C > 1 (the tool skips `min(crosstab.shape) <= 1`, and
  pandas only makes rows and columns for states that occur); dof = (R - 1)(C - 1);
* E[a][b] = r_a c_b / n in fp64 (the product of two integers below 2^24 is exact);
* dof == 1 (SciPy's default correction=True): O' = O + sign(E - O) min(0.5, |E - O|), else O' = O;
* statistic = sum of (O' - E)^2 / E over the cells with r_a > 0 and c_b > 0, a major, b minor, in that order;
* pvalue = Q(dof / 2, statistic / 2), the regularized upper incomplete gamma function (scipy.special.chdtrc), by
  `gamma_q` below: Cephes' classical igam / igamc (series of P for x < max(1, a), else the continued fraction of Q),
  with the prefactor x^a e^-x / Gamma(a) by `prefactor`;
* outputs [F, F], mirrored: statistic, pvalue (fp64), dof, n (int32), valid (bool); invalid pairs and the diagonal
  hold statistic 0, pvalue NaN, dof 0 (the diagonal also n 0).

Error bounds the tests use (derived, not tuned): every term of the statistic is non-negative and carries a few
roundings (E: 2, the correction: 2, the square and the quotient: 3), and a sum of R C non-negative terms in any order
adds at most R C more: |statistic - exact| <= (8 + R C) 2^-52 statistic.  `gamma_q` against scipy.special.chdtrc over every
(dof, statistic) of tests/golden/assoc.npz: the largest relative error is GAMMA_Q_MEASURED (at dof 961, where the series
runs over hundreds of terms; 4.2e-14 over the cases with dof <= 81); four times that is the bound on a device p-value
against chdtrc at the device's own statistic (the margin covers the device's exp / log differing from the host's by an
ulp or two).  End to end against the fixture the statistic's own bound enters through the sensitivity of Q to its
argument, |dQ/Q| <= (statistic / 2 + 1) |dx/x|."""
from __future__ import annotations

import math

import numpy as np

NA = 255
MAX_STATES = 32
MAX_ITER = 5000
EPS53 = 2.0 ** -53
DBL_MIN = np.finfo(float).tiny
STIRLING_FROM = 16.0
GAMMA_Q_MEASURED = 3.27e-13         # tests/test_assoc_oracle_cpu.py re-measures it
PVALUE_BOUND = 4 * GAMMA_Q_MEASURED
TWO_PI = 6.283185307179586


def statistic_bound(R, C):
    """Relative bound on the statistic of a table with R x C occupied cells (module docstring)."""
    return (8 + np.asarray(R, dtype=np.float64) * np.asarray(C, dtype=np.float64)) * 2.0 ** -52


def pvalue_bound_end_to_end(statistic, R, C):
    """Relative bound on a p-value against the fixture's: PVALUE_BOUND plus the statistic's bound times (statistic/2 + 1)."""
    return PVALUE_BOUND + (0.5 * np.asarray(statistic, dtype=np.float64) + 1.0) * statistic_bound(R, C)


def upper(a):
    """The pairs i < j of an [F, F] array in the tool's order (combinations)."""
    return np.asarray(a)[np.triu_indices(np.asarray(a).shape[0], 1)]


def one_hot(x, s):
    """float32 [N, F, s]: the one-hot matrix of the codes (NA rows all zero; counts up to 2^24 are exact in float32)."""
    x = np.asarray(x)
    return (x[:, :, None] == np.arange(s, dtype=np.int64)[None, None, :]).astype(np.float32)


def tables(x, n_states=None):
    """int32 [F, F, S, S]: every contingency table at once, X^T X (S = the largest state count)."""
    x = np.asarray(x, dtype=np.uint8)
    s = int(np.max(n_states)) if n_states is not None else int(x[x != NA].max(initial=0)) + 1
    oh = one_hot(x, s)
    n, f = x.shape
    t = oh.reshape(n, f * s).T @ oh.reshape(n, f * s)
    return np.rint(t).astype(np.int32).reshape(f, s, f, s).transpose(0, 2, 1, 3)


def prefactor(a, x):
    """x^a e^-x / Gamma(a).  Below a = 16 through exp(a log x - x - lgamma(a)); from there on with Stirling's series for
    lgamma folded in, exp(a (log1p(mu) - mu) + log(a / 2 pi) / 2 - s(a)) with mu = (x - a) / a, whose terms are of the
    size of the result's logarithm instead of a log x (the rounding of a log x alone would cost 4e-13 at dof 961)."""
    a, x = np.asarray(a, dtype=np.float64), np.asarray(x, dtype=np.float64)
    lg = np.array([math.lgamma(v) for v in a.ravel()]).reshape(a.shape)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        small = np.exp(a * np.log(x) - x - lg)
        mu = (x - a) / a
        w = 1.0 / (a * a)
        st = (1.0 / 12.0 - w * (1.0 / 360.0 - w * (1.0 / 1260.0 - w * (1.0 / 1680.0 - w * (1.0 / 1188.0))))) / a
        large = np.exp(a * (np.log1p(mu) - mu) + 0.5 * np.log(a / TWO_PI) - st)
    return np.where(a < STIRLING_FROM, small, large)


def gamma_q(a, x):
    """Q(a, x) elementwise (float64 [K], flattened), operation for operation what the device evaluates."""
    a, x = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(x, dtype=np.float64))
    a, x = a.ravel().copy(), x.ravel().copy()
    out = np.ones(a.shape, dtype=np.float64)
    pos = x > 0
    out[pos & np.isinf(x)] = 0.0
    todo = pos & ~np.isinf(x)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        ax = prefactor(a, np.where(todo, x, 1.0))
        # the series of P
        ser = todo & ((x < 1.0) | (x < a))
        idx = np.nonzero(ser)[0]
        if idx.size:
            aa, xx = a[idx], x[idx]
            r, c, ans = aa.copy(), np.ones_like(aa), np.ones_like(aa)
            live = np.ones(aa.shape, dtype=bool)
            for _ in range(MAX_ITER):
                r = np.where(live, r + 1.0, r)
                c = np.where(live, c * (xx / r), c)
                ans = np.where(live, ans + c, ans)
                live &= c > ans * EPS53
                if not live.any():
                    break
            out[idx] = 1.0 - ans * ax[idx] / aa
        # the continued fraction of Q
        idx = np.nonzero(todo & ~ser)[0]
        if idx.size:
            big, biginv = 4503599627370496.0, 2.22044604925031308085e-16
            aa, xx = a[idx], x[idx]
            y = 1.0 - aa
            z = xx + y + 1.0
            c = np.zeros_like(aa)
            pkm2, qkm2, pkm1, qkm1 = np.ones_like(aa), xx.copy(), xx + 1.0, z * xx
            ans = pkm1 / qkm1
            live = ax[idx] != 0.0
            for _ in range(MAX_ITER):
                if not live.any():
                    break
                c = c + 1.0
                y = y + 1.0
                z = z + 2.0
                yc = y * c
                pk = pkm1 * z - pkm2 * yc
                qk = qkm1 * z - qkm2 * yc
                ok = qk != 0.0
                r = np.where(ok, pk / np.where(ok, qk, 1.0), 1.0)
                t = np.where(ok, np.abs((ans - r) / r), 1.0)
                ans = np.where(live & ok, r, ans)
                scale = np.where(np.abs(pk) > big, biginv, 1.0)
                npkm2, npkm1, nqkm2, nqkm1 = pkm1 * scale, pk * scale, qkm1 * scale, qk * scale
                pkm2, pkm1 = np.where(live, npkm2, pkm2), np.where(live, npkm1, pkm1)
                qkm2, qkm1 = np.where(live, nqkm2, qkm2), np.where(live, nqkm1, qkm1)
                live = live & (t > EPS53)
            out[idx] = np.where(ax[idx] == 0.0, 0.0, ans * ax[idx])
    return out


def chi2_sf(dof, statistic):
    """The p-value of the contract: Q(dof / 2, statistic / 2)."""
    dof = np.asarray(dof, dtype=np.float64)
    statistic = np.asarray(statistic, dtype=np.float64)
    shape = np.broadcast(dof, statistic).shape
    return gamma_q(0.5 * dof, 0.5 * statistic).reshape(shape)


def table_statistic(t):
    """(valid, dof, n, statistic, R, C) of one observed table (integer [S, S]) by the contract's arithmetic."""
    t = np.asarray(t, dtype=np.float64)
    r, c = t.sum(axis=1), t.sum(axis=0)
    n = r.sum()
    R, C = int(np.count_nonzero(r)), int(np.count_nonzero(c))
    if R <= 1 or C <= 1:
        return False, 0, int(n), 0.0, R, C
    dof = (R - 1) * (C - 1)
    stat = 0.0
    for a in np.nonzero(r)[0]:
        for b in np.nonzero(c)[0]:
            o = t[a, b]
            e = r[a] * c[b] / n
            if dof == 1:
                d = e - o
                o = o + min(0.5, abs(d)) * float(np.sign(d))
            diff = o - e
            stat += diff * diff / e
    return True, dof, int(n), float(stat), R, C


def feature_association(x, n_states=None):
    """dict of [F, F] arrays: statistic, pvalue, dof, n, valid, plus R and C (occupied rows / columns, for the bound)."""
    x = np.asarray(x, dtype=np.uint8)
    f = x.shape[1]
    t = tables(x, n_states)
    stat = np.zeros((f, f))
    dof = np.zeros((f, f), dtype=np.int32)
    n = np.zeros((f, f), dtype=np.int32)
    valid = np.zeros((f, f), dtype=bool)
    R = np.zeros((f, f), dtype=np.int32)
    C = np.zeros((f, f), dtype=np.int32)
    # vectorized over pairs; the cell sum runs a major, b minor, empty rows / columns adding +0.0 (no bit changes)
    r = t.sum(axis=3).astype(np.float64)                       # [F, F, S]
    c = t.sum(axis=2).astype(np.float64)
    nn = r.sum(axis=2)
    R[:] = np.count_nonzero(r, axis=2)
    C[:] = np.count_nonzero(c, axis=2)
    valid[:] = (R > 1) & (C > 1)
    valid[np.arange(f), np.arange(f)] = False
    dof[:] = np.where(valid, (R - 1) * (C - 1), 0)
    n[:] = nn
    n[np.arange(f), np.arange(f)] = 0
    s = t.shape[2]
    with np.errstate(divide="ignore", invalid="ignore"):
        for a in range(s):
            for b in range(s):
                o = t[:, :, a, b].astype(np.float64)
                e = r[:, :, a] * c[:, :, b] / nn
                d = e - o
                oc = np.where(dof == 1, o + np.minimum(0.5, np.abs(d)) * np.sign(d), o)
                diff = oc - e
                term = diff * diff / e
                stat += np.where(valid & (r[:, :, a] > 0) & (c[:, :, b] > 0), term, 0.0)
    stat = np.triu(stat, 1)
    stat = stat + stat.T                                       # mirrored: [j, i] holds what [i, j] holds, bit for bit
    pvalue = np.full((f, f), np.nan)
    pvalue[valid] = chi2_sf(dof[valid], stat[valid])
    return dict(statistic=stat, pvalue=pvalue, dof=dof, n=n, valid=valid, R=R, C=C, tables=t)
