"""The contract of the leave-one-out predictive unit (include/sbe_loopred.h) in NumPy float64, with the
kernels' summation order, and an exact form in fractions.Fraction for cases without smoothing.  It builds on
tests/_predict_oracle.py for the rows and on tests/_elpd_oracle.py:psis_column for the log weights.  A plain helper module: it
holds no test.

    rows      lik[t, j] = float32(m_t[x]) of the observed cells, j in n F + f order: _predict_oracle's lik, NA columns dropped
    weights   per column ll = log(float64(lik)); (lw, k) = psis_column(ll); w = exp(lw); loo_i = logsumexp(lw + ll);
              n_eff = 1 / sum_t w_t^2
    sums      p_loo[n, f, s] = sum_t w_t m_t[n, f, s]: the product rounded, then added, in sample order; zero at NA cells

The mixture rows m_t are computed here for all samples at once (mixture), in _predict_oracle.accumulate's operation order;
tests/test_loopred_oracle_cpu.py checks them against that module bit for bit.

Error bounds of the device against this oracle (u = 2^-53, gamma(k) = k u / (1 - k u)):
    loo_i, k  tests/test_gpu_elpd.py's RTOL = 1e-10 (with its absolute floor of 1e-10, and 1e-9 absolute on k): the project's own
              figure for this arithmetic on the device's libm.
    w_t       the same figure on log w_t: |log w_dev - log w| <= b_t = max(1e-10 |log w_t|, 1e-10).  log w_t = x'_t - log A is what
              the oracle forms; the device forms exp(x'_t) / A.  Both go through the quantities loo_i goes through.
    p_loo     with b = max_t b_t of the column, every w_dev lies within a factor exp(+-b) of w.  The mixture rows use only + * /
              and are within gamma(2 C) of exact on either side (_predict_oracle).  A term w_t m_t[s] is one more rounding, and
              passes at most T - 1 additions; all terms are non-negative.  So
                  |p_dev - p| <= p (expm1(b) (1 + 2 gamma(k)) + 2 gamma(k)),   k = T + 2 C + 1,
              and 2 C T 2^-1074 absolute for products that underflow (probs_bound).
"""
from fractions import Fraction

import numpy as np

from tests import _elpd_oracle as eo
from tests import _predict_oracle as po

NA = po.NA
RTOL = 1e-10                                     # tests/test_gpu_elpd.py's


def mixture(codes, groups, n_groups, clusters, weights, tables):
    """m float64 [T,N,F,S]: the mixture row of every cell and sample, in _predict_oracle.accumulate's operation order."""
    T, K, N = clusters.shape
    F, C = weights.shape[1:]
    S = tables.shape[3]
    off, R = po.row_offsets(K, n_groups)
    assert tables.shape == (T, R, F, S) and codes.shape == (N, F)
    member = clusters != 0
    assert (member.sum(axis=1) <= 1).all(), "an object in two clusters"
    h = np.zeros((T, N, C), dtype=bool)
    rows = np.zeros((T, N, C), dtype=np.int64)
    h[:, :, 0] = member.any(axis=1)
    rows[:, :, 0] = np.where(h[:, :, 0], member.argmax(axis=1), 0)
    for c in range(1, C):
        h[:, :, c] = (groups[c - 1] != NA)[None, :]
        rows[:, :, c] = np.where(h[:, :, c], off[c] + groups[c - 1].astype(np.int64)[None, :], 0)
    w = np.where(h[:, :, None, :], weights[:, None, :, :], 0.0)                  # [T,N,F,C]
    wsum = np.zeros((T, N, F))
    for c in range(C):
        wsum = wsum + w[..., c]
    with np.errstate(invalid="ignore", divide="ignore"):
        wn = np.where((wsum > 0.0)[..., None], w / wsum[..., None], 0.0)
    m = np.zeros((T, N, F, S))
    t_index = np.arange(T)[:, None]
    for c in range(C):
        theta = tables[t_index, rows[:, :, c]]                                   # [T,N,F,S]
        m = m + wn[..., c, None] * theta
    return m


def rows_of(codes, m):
    """lik float32 [T, M] of the observed cells, from the mixture rows."""
    obs = codes != NA
    x = np.where(obs, codes, 0).astype(np.int64)
    mx = np.take_along_axis(m, np.broadcast_to(x[None, ..., None], m.shape[:3] + (1,)), axis=3)[..., 0]
    return mx[:, obs].astype(np.float32)


def first_bad(lik):
    """None, or (column, sample) of the first stored value that is not positive and finite: by column, then by sample."""
    bad = ~(np.isfinite(lik) & (lik > 0))
    if not bad.any():
        return None
    j = int(np.flatnonzero(bad.any(axis=0))[0])
    return j, int(np.flatnonzero(bad[:, j])[0])


def weights_column(lh_col):
    """(w float64 [T], loo_i, k, n_eff) of one column of float32 likelihoods."""
    ll = np.log(np.asarray(lh_col, dtype=np.float64))
    lw, k = eo.psis_column(ll)
    w = np.exp(lw)
    sq = 0.0
    for v in w:                                   # (the device: a fixed tree; the difference is within the bound on n_eff)
        sq += v * v
    return w, eo.logsumexp(lw + ll), float(k), 1.0 / sq


def run(codes, groups, n_groups, clusters, weights, tables):
    """dict(lik [T,M], w [T,M], loo_i [M], k [M], n_eff [M], p_loo [N,F,S], m [T,N,F,S]) of a valid case whose rows are positive."""
    m = mixture(codes, groups, n_groups, clusters, weights, tables)
    lik = rows_of(codes, m)
    assert first_bad(lik) is None
    T, M = lik.shape
    w = np.empty((T, M))
    loo_i, k, n_eff = np.empty(M), np.empty(M), np.empty(M)
    for j in range(M):
        w[:, j], loo_i[j], k[j], n_eff[j] = weights_column(lik[:, j])
    obs = codes != NA
    w_cell = np.zeros((T,) + codes.shape)
    w_cell[:, obs] = w
    p = np.zeros(m.shape[1:])
    for t in range(T):
        p = p + w_cell[t][..., None] * m[t]
    return dict(lik=lik, w=w, loo_i=loo_i, k=k, n_eff=n_eff, p_loo=p, m=m)


def log_w_bound(w):
    """b_t [T,M]: the bound on |log w_dev - log w|."""
    return np.maximum(RTOL * np.abs(np.log(w)), 1e-10)


def probs_bound(p_loo, w, codes, T, C):
    """[N,F,S]: the bound on |p_dev - p_loo| (the module's docstring)."""
    obs = codes != NA
    b = np.zeros(codes.shape)
    b[obs] = log_w_bound(w).max(axis=0)
    g = po.gamma(T + 2 * C + 1)
    return p_loo * (np.expm1(b)[..., None] * (1 + 2 * g) + 2 * g) + 2 * C * T * po.TINY


def branch_margins(lh_col):
    """How far a column is from the edges of _psislw's and _gpdfit's branches, for choosing seeds: dict(tail_len, k, prune: the
    smallest |w_c / (10 eps) - 1| over the fit's candidate weights, clamp: the smallest |smoothed x| over the tail, sigma).  A
    column whose tail has at most 4 elements has no fit: prune and clamp are inf."""
    ll = np.log(np.asarray(lh_col, dtype=np.float64))
    s = len(ll)
    tail_n = int(np.ceil(min(0.2 * s, 3 * np.sqrt(s))))
    x = -ll
    x = x - np.max(x)
    xcutoff = max(np.sort(x)[s - tail_n - 1], np.log(eo.DBL_MIN))
    x_tail = np.sort(x[x > xcutoff])
    out = dict(tail_len=len(x_tail), k=np.inf, prune=np.inf, clamp=np.inf, sigma=np.inf)
    if len(x_tail) <= 4:
        return out
    ary = np.exp(x_tail) - np.exp(xcutoff)
    n = len(ary)
    m_est = 30 + int(n ** 0.5)
    b_ary = 1 - np.sqrt(m_est / (np.arange(1, m_est + 1, dtype=float) - 0.5))
    b_ary /= 3 * ary[int(n / 4 + 0.5) - 1]
    b_ary += 1 / ary[-1]
    with np.errstate(all="ignore"):
        k_ary = np.log1p(-b_ary[:, None] * ary).mean(axis=1)
        len_scale = n * (np.log(-(b_ary / k_ary)) - k_ary - 1)
        wts = 1 / np.exp(len_scale - len_scale[:, None]).sum(axis=1)
    k, sigma = eo.gpdfit(ary)
    out.update(k=float(k), sigma=float(sigma), prune=float(np.min(np.abs(wts / (10 * eo.DBL_EPS) - 1))) if np.isfinite(wts).all() else 0.0)
    if np.isfinite(k):
        with np.errstate(all="ignore"):
            smoothed = np.log(eo.gpinv(np.arange(0.5, n) / n, k, sigma) + np.exp(xcutoff))
        out["clamp"] = float(np.min(np.abs(smoothed))) if np.isfinite(smoothed).all() else 0.0
    return out


def away_from_edges(lik):
    """True when every column of lik [T, M] is clear of the branch edges: k finite wherever there is a fit, sigma > 0, no fit weight
    within 1e-6 (relative) of the pruning threshold, no smoothed value within 1e-9 of the clamp."""
    for j in range(lik.shape[1]):
        g = branch_margins(lik[:, j])
        if g["tail_len"] > 4 and not (np.isfinite(g["k"]) and g["sigma"] > 0 and g["prune"] > 1e-6 and g["clamp"] > 1e-9):
            return False
    return True


def exact_raw(codes, groups, n_groups, clusters, weights, tables):
    """The contract in exact arithmetic for a case whose columns are not smoothed (T <= 20: the tail has at most four elements):
    w_t = (1 / lik_t) / sum_t' (1 / lik_t') with lik_t the float32 value; (w [T][M], p_loo [N][F][S], p_obs_harmonic [M]) as
    Fractions, from _predict_oracle.exact's mixture rows."""
    T, _K, N = clusters.shape
    F, S = weights.shape[1], tables.shape[3]
    assert T <= 20
    cells = [(n, f) for n in range(N) for f in range(F) if codes[n, f] != NA]
    m = []                                                                      # per sample [N][F][S]
    for t in range(T):
        pred, _resp, _lik, _inv, _zero = po.exact(codes, groups, n_groups, clusters[t:t + 1], weights[t:t + 1], tables[t:t + 1])
        m.append(pred)
    lik = [[Fraction(float(np.float32(float(m[t][n][f][int(codes[n, f])])))) for (n, f) in cells] for t in range(T)]
    w = [[None] * len(cells) for _ in range(T)]
    harmonic = []
    p = [[[Fraction(0)] * S for _ in range(F)] for _ in range(N)]
    for j, (n, f) in enumerate(cells):
        total = sum((1 / lik[t][j] for t in range(T)), Fraction(0))
        harmonic.append(T / total)
        for t in range(T):
            w[t][j] = (1 / lik[t][j]) / total
            for s in range(S):
                p[n][f][s] += w[t][j] * m[t][n][f][s]
    return w, p, harmonic
