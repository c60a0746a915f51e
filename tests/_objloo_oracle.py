"""The contract of the leave-one-object-out unit (include/sbe_objloo.h) in NumPy float64, in the header's
order.  It builds on tests/_contrib_oracle.py:rows_of_sample for the counterfactual rows at the observed state, on
tests/_ppc_oracle.py:sum_over_features for the per-object tree and on tests/_elpd_oracle.py:psis_column for the log weights.  A
plain helper module: it holds no test.

    rows      per sample t, object n, hypothesis j (0: no cluster, k + 1: cluster k): H[t, n, j] = sum_f log m_j[n, f, x] in the
              per-object tree, +0.0 for a cell without a code, -inf as a whole where an observed cell has m = 0; an observed cell to
              which no confounder applies is refused (first_unformed)
              a_j = log(prior_j) + H_j;  mx = max_j a_j;  L = mx + log(sum_j exp(a_j - mx)), j in order onto 0;  Cnd = H[z]
    weights   per object and column ll (L, then Cnd): (lw, k) = psis_column(ll); w = exp(lw); loo_i = logsumexp(lw + ll);
              n_eff = 1 / sum_t w_t^2; lppd_i = logsumexp(ll) - log T;  membership[n, j] = (1 / T) sum_t exp(a_j - L), the sums
              in the workgroup's tree (block_tree_sum)
    sums      p_loo[n, f, s] = sum_t w_t(n) mz_t,  mz = sum_j prior_j m_j[n, f, s], j in order onto 0, every product rounded, then
              added; the product with w rounded, then added, in sample order; every cell, with a code or without one

Error bounds of the device against this module (e = 2^-52, one ulp of relative spacing):
    H         tests/_contrib_oracle.band(n_terms, sum |log m|): the m's are bit-identical, only the logs and the order of the
              partial sums' roundings differ (that module's docstring); -inf compared by class.
    L         on the device's own H.  Every elementary function, the device library's and this module's, is taken to be within one
              ulp of the exact value, so the two sides differ by at most 2 e relative per call; an addition of operands that
              differ rounds to results that differ by the operands' difference plus one ulp of the result.  Per (sample, object),
              over the hypotheses with a finite a_j (the others are exactly 0 in the sum on both sides):
                  da_j  = 2 e |log prior_j| + e |a_j|                       the log, then the addition
                  dmx   = max_j da_j
                  dd_j  = da_j + dmx + e |a_j - mx|                          the subtraction
                  dE_j  = E_j (dd_j + 2 e),  E_j = exp(a_j - mx) <= 1         one of the K + 1 exps
                  ds    = sum_j dE_j + K e s,  s = sum_j E_j >= 1             the K additions
                  dlog  = ds / s + 2 e |log s|                               the one log
                  dL    = dmx + dlog + e |L|                                 the last addition
              l_bound() evaluates this; it is some 1e-15 |L| for the cases of the tests.
    phase 2   on the device's own L, Cnd and a: loo, lppd, n_eff and membership at tests/_loopred_oracle.RTOL (the project's figure
              for this arithmetic on the device's libm, with its floor of 1e-10 absolute), k within tests/_psens_oracle.tol_k of the
              column's ratios.
    p_loo     with the device's own w: bit for bit (the rows use + * / only and nothing is contracted).
"""
import math
from fractions import Fraction

import numpy as np

from tests import _contrib_oracle as co
from tests import _elpd_oracle as eo
from tests import _predict_oracle as po
from tests._ppc_oracle import sum_over_features

NA = po.NA
E = 2.0 ** -52
BLOCK = 256                                      # threads of the weights kernel's workgroup


# ---- phase 1 ------------------------------------------------------------------------------------------------------------------------
def uniform_prior(T, N, K):
    return np.full((T, N, K + 1), 1.0 / (K + 1))


def first_unformed(codes, groups, n_groups, K, weights, tables):
    """None, or (sample, object, feature) of the first observed cell to which no confounder applies: by sample, then by cell."""
    for t in range(weights.shape[0]):
        _m, _m0, formed, _w = co.rows_of_sample(codes, groups, n_groups, K, weights[t], tables[t])
        bad = (codes != NA) & ~formed
        if bad.any():
            n, f = (int(v) for v in np.argwhere(bad)[0])
            return t, n, f
    return None


def log_rows(codes, groups, n_groups, K, weights_t, tables_t):
    """log m_j of one sample: float64 [K+1, N, F], +0.0 at cells without a code; every observed cell must be formed."""
    m, m0, formed, _w = co.rows_of_sample(codes, groups, n_groups, K, weights_t, tables_t)
    observed = codes != NA
    assert (formed == observed).all(), "an observed cell to which no confounder applies"
    out = np.zeros((K + 1,) + codes.shape)
    out[0] = np.where(observed, co.log_of(m0), 0.0)
    for k in range(K):
        out[k + 1] = np.where(observed, co.log_of(m[k]), 0.0)
    return out


def hypotheses(codes, groups, n_groups, clusters, weights, tables):
    """(H float64 [T, N, K+1], z int [T, N]: the logged hypothesis of every object, abs_logs [T, N, K+1]: sum |log m| for H's band)."""
    T, K, N = clusters.shape
    H, mag = np.empty((T, N, K + 1)), np.empty((T, N, K + 1))
    z = np.empty((T, N), dtype=np.int64)
    for t in range(T):
        ids, twice = po.cluster_ids(clusters[t])
        assert twice is None
        z[t] = ids + 1
        logs = log_rows(codes, groups, n_groups, K, weights[t], tables[t])
        for j in range(K + 1):
            with np.errstate(invalid="ignore"):
                H[t, :, j] = sum_over_features(logs[j])
            mag[t, :, j] = np.where(np.isinf(logs[j]), 0.0, np.abs(logs[j])).sum(axis=1)
    return H, z, mag


def mix(H, prior, z):
    """(a [.., K+1], L [..], Cnd [..]) of H [.., K+1], prior [.., K+1] and the logged hypotheses z [..]."""
    with np.errstate(divide="ignore", invalid="ignore"):
        a = np.log(prior) + H
        mx = np.full(a.shape[:-1], -np.inf)
        for j in range(a.shape[-1]):
            mx = np.fmax(mx, a[..., j])
        total = np.zeros(a.shape[:-1])
        for j in range(a.shape[-1]):
            total = total + np.exp(a[..., j] - mx)
        L = mx + np.log(total)
    Cnd = np.take_along_axis(H, z[..., None], axis=-1)[..., 0]
    return a, L, Cnd


def first_not_finite(L, Cnd):
    """None, or (object, sample, which) of the first object and sample whose L ("marginal") or Cnd ("conditional") is not finite:
    by object, then by sample; L is named when both are."""
    bad = ~(np.isfinite(L) & np.isfinite(Cnd))                                  # [T, N]
    if not bad.any():
        return None
    n = int(np.flatnonzero(bad.any(axis=0))[0])
    t = int(np.flatnonzero(bad[:, n])[0])
    return n, t, ("marginal" if not np.isfinite(L[t, n]) else "conditional")


def l_bound(H, prior):
    """dL [..]: the bound on |L_device - L| given the same H (the module's docstring)."""
    K = H.shape[-1] - 1
    with np.errstate(divide="ignore", invalid="ignore"):
        lp = np.log(prior)
        a = lp + H
        live = np.isfinite(a)
        mx = np.where(live, a, -np.inf).max(axis=-1, keepdims=True)
        da = np.where(live, 2 * E * np.abs(lp) + E * np.abs(a), 0.0)
        dmx = da.max(axis=-1, keepdims=True)
        d = np.where(live, a - mx, 0.0)
        Ej = np.where(live, np.exp(d), 0.0)
        dE = Ej * (da + dmx + E * np.abs(d) + 2 * E)
        s = Ej.sum(axis=-1)
        ds = dE.sum(axis=-1) + K * E * s
        L = mx[..., 0] + np.log(s)
        return dmx[..., 0] + ds / s + 2 * E * np.abs(np.log(s)) + E * np.abs(L)


# ---- phase 2 ------------------------------------------------------------------------------------------------------------------------
def block_tree_sum(v):
    """The weights kernel's sum of T values: thread i of 256 adds v[i], v[i + 256], .. in order onto 0; the 64 lanes of a wave are
    folded by xor exchanges at distances 32 .. 1; the four waves are added in order."""
    v = np.asarray(v, dtype=np.float64)
    pad = np.zeros(-(-len(v) // BLOCK) * BLOCK)
    pad[:len(v)] = v
    lanes = np.zeros(BLOCK)
    for block in pad.reshape(-1, BLOCK):
        lanes = lanes + block
    waves = lanes.reshape(4, 64)
    o = 32
    while o:
        waves = waves + waves[:, np.arange(64) ^ o]
        o //= 2
    total = waves[0, 0]
    for w in range(1, 4):
        total = total + waves[w, 0]
    return float(total)


def weights_column(ll):
    """(w float64 [T], loo_i, k, n_eff, lppd_i) of one float64 column."""
    ll = np.asarray(ll, dtype=np.float64)
    lw, k = eo.psis_column(ll)
    w = np.exp(lw)
    return w, eo.logsumexp(lw + ll), float(k), 1.0 / block_tree_sum(w * w), eo.logsumexp(ll) - math.log(len(ll))


def phase2(L, Cnd, a):
    """dict of the outputs of sbe_objloo_weights from L, Cnd [T, N] and a [T, N, K+1]: loo_i, k_i, n_eff, lppd_i, loo_cond_i,
    k_cond_i, lppd_cond_i [N], membership [N, K+1] and w [T, N]."""
    T, N = L.shape
    out = {name: np.empty(N) for name in ("loo_i", "k_i", "n_eff", "lppd_i", "loo_cond_i", "k_cond_i", "lppd_cond_i")}
    out["w"] = np.empty((T, N))
    out["membership"] = np.empty((N, a.shape[2]))
    for n in range(N):
        out["w"][:, n], out["loo_i"][n], out["k_i"][n], out["n_eff"][n], out["lppd_i"][n] = weights_column(L[:, n])
        _w, out["loo_cond_i"][n], out["k_cond_i"][n], _n_eff, out["lppd_cond_i"][n] = weights_column(Cnd[:, n])
        for j in range(a.shape[2]):
            with np.errstate(over="ignore"):
                out["membership"][n, j] = block_tree_sum(np.exp(a[:, n, j] - L[:, n])) / T
    return out


# ---- phase 3 ------------------------------------------------------------------------------------------------------------------------
def rows_all_states(codes, groups, n_groups, K, weights_t, tables_t):
    """m_j[n, f, s] of one sample for every cell, with a code or without one, and every state: float64 [K+1, N, F, S], in
    sbe_contrib.h's operation order (w1 is 0 where wsum1 is not > 0, w0 where wsum0 is not > 0)."""
    N, F = codes.shape
    C = weights_t.shape[1]
    S = tables_t.shape[2]
    off, _R = po.row_offsets(K, n_groups)
    f_idx = np.arange(F)[None, :]
    a = np.zeros((N, F, C))
    a[:, :, 0] = weights_t[None, :, 0]
    theta = np.zeros((N, F, C, S))
    for c in range(1, C):
        has = groups[c - 1] != NA
        rows = np.where(has, off[c] + groups[c - 1].astype(np.int64), 0)
        a[:, :, c] = np.where(has[:, None], weights_t[None, :, c], 0.0)
        theta[:, :, c] = tables_t[rows[:, None], f_idx]
    wsum1, wsum0 = np.zeros((N, F)), np.zeros((N, F))
    for c in range(C):
        wsum1 = wsum1 + a[:, :, c]
        if c >= 1:
            wsum0 = wsum0 + a[:, :, c]
    with np.errstate(invalid="ignore", divide="ignore"):
        w1 = np.where((wsum1 > 0.0)[..., None], a / wsum1[..., None], 0.0)
        w0 = np.where((wsum0 > 0.0)[..., None], a / wsum0[..., None], 0.0)
    m = np.zeros((K + 1, N, F, S))
    for c in range(1, C):
        m[0] = m[0] + w0[:, :, c, None] * theta[:, :, c]
    for k in range(K):
        mk = w1[:, :, 0, None] * tables_t[k][None]
        for c in range(1, C):
            mk = mk + w1[:, :, c, None] * theta[:, :, c]
        m[k + 1] = mk
    return m


def accumulate(codes, groups, n_groups, clusters, weights, tables, prior, w):
    """p_loo [N, F, S] from the weights w [T, N]."""
    T, K, N = clusters.shape
    p = np.zeros(codes.shape + (tables.shape[3],))
    for t in range(T):
        m = rows_all_states(codes, groups, n_groups, K, weights[t], tables[t])
        mz = np.zeros(p.shape)
        for j in range(K + 1):
            mz = mz + prior[t, :, j, None, None] * m[j]
        p = p + w[t][:, None, None] * mz
    return p


def run(codes, groups, n_groups, clusters, weights, tables, prior=None):
    """The three phases of a valid case: dict(H, z, mag, a, L, Cnd [T, ..], prior, the outputs of phase2(), p_loo)."""
    T, K, N = clusters.shape
    prior = uniform_prior(T, N, K) if prior is None else np.broadcast_to(np.asarray(prior, dtype=np.float64), (T, N, K + 1))
    H, z, mag = hypotheses(codes, groups, n_groups, clusters, weights, tables)
    a, L, Cnd = mix(H, prior, z)
    assert first_not_finite(L, Cnd) is None
    out = dict(H=H, z=z, mag=mag, a=a, L=L, Cnd=Cnd, prior=prior, **phase2(L, Cnd, a))
    out["p_loo"] = accumulate(codes, groups, n_groups, clusters, weights, tables, prior, out["w"])
    return out


# ---- exact rationals for small cases ----------------------------------------------------------------------------------------------
def exact_marginal(codes, groups, n_groups, clusters, weights, tables, prior):
    """(exp(H) [T][N][K+1], exp(L) [T][N], exp(Cnd) [T][N]) as Fractions from tests/_contrib_oracle.py:exact_rows: the products over
    the observed cells of the exact m_j, and their prior mixture."""
    T, K, N = clusters.shape
    F = codes.shape[1]
    rows = co.exact_rows(codes, groups, n_groups, clusters, weights, tables)
    eH = [[[Fraction(1)] * (K + 1) for _ in range(N)] for _ in range(T)]
    eL = [[Fraction(0)] * N for _ in range(T)]
    eC = [[Fraction(0)] * N for _ in range(T)]
    for t in range(T):
        ids, _twice = po.cluster_ids(clusters[t])
        for n in range(N):
            for f in range(F):
                if codes[n, f] == NA:
                    continue
                for k in range(K):
                    m_k, m0, _w, _theta = rows[t, k, n, f]
                    eH[t][n][k + 1] *= m_k
                eH[t][n][0] *= m0
            eL[t][n] = sum((Fraction(float(prior[t, n, j])) * eH[t][n][j] for j in range(K + 1)), Fraction(0))
            eC[t][n] = eH[t][n][int(ids[n]) + 1]
    return eH, eL, eC
