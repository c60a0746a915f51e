"""The contract of the posterior predictive check (include/sbe_ppc.h) in NumPy float64, in the contract's
order, and an exact form in fractions.Fraction for small cases.  A plain helper module: it holds no test.

Sample t of a call has the draw index tau = first_draw + t.  For every cell (n, f) with a code x != 255:
    wn, m[s]    the posterior predictive's operations in its order (tests/_predict_oracle.py): the normalising sum over c in
                order, one division, m[s] = sum_c wn_c tables[row_c(n), f, s], every product rounded, then added
    cdf_s       = m[0] + .. + m[s] in index order;  total = cdf_{S-1}
    skipped     total not > 0: y = 255, the cell adds to no sum, n_skipped += 1
    u           uniforms[t][n F + f], or philox_uniforms(seed, tau, N F)[n F + f]
    v           = u * total, one rounding
    y           = #{s : cdf_s <= v}, clamped to the last state with m[s] > 0
    d_obs, d_rep = -2 log m[x] (+inf where m[x] = 0), -2 log m[y]
Outputs per sample: y_rep [N,F] (255 for NA and skipped cells), dev_feature [2,F] and dev_object [2,N] (observed, replicated),
count_rep [F,S]; n_skipped for the call.  The sums add the d values of all cells (+0.0 for those without a code or skipped)
in the header's trees: per feature 16 lanes, lane j adds the objects j, j + 16, .. onto 0, then the lanes in order; per object
64 lanes, lane j adds the features j, j + 64, .. onto 0, then xor exchanges at distances 32 .. 1.

check() also returns, per drawn cell, the margin min_s |v - cdf_s| / total: how far the draw is from changing with a rounding.

The device's band for the sums (the form and constant of the Gibbs weights step's):
    |dev - oracle| <= 2^-50 (n_terms + 4) sum |d|,   n_terms the cells in the sum, +inf compared by class.
It covers the two logs per term (the device library's log and NumPy's are each within an ulp or two of the exact one, and
|d| >= 0 adds without cancellation) and n_terms - 1 additions."""
from fractions import Fraction

import numpy as np

from oracle.sbayes_oracle import philox_uniforms
from tests._predict_oracle import NA, cluster_ids, row_offsets
from tests import _predict_oracle as predict_orc

KINDS = (*predict_orc.KINDS, "uniform")
MARGIN = 2.0 ** -40                       # the margin condition: every drawn cell is further than this from a cdf step
FEATURE_LANES, OBJECT_LANES = 16, 64


def dev_band(n_terms, abs_sum):
    return 2.0 ** -50 * (n_terms + 4) * abs_sum


def p_value(rep, obs):
    """(#{rep > obs} + #{rep == obs} / 2) / T over the first axis."""
    rep, obs = np.asarray(rep), np.asarray(obs)
    return ((rep > obs).sum(axis=0) + 0.5 * (rep == obs).sum(axis=0)) / rep.shape[0]


def uniforms_of(seed, first_draw, T, cells):
    """float64 [T, cells]: the Philox uniforms of the draws first_draw .. first_draw + T - 1."""
    return np.stack([philox_uniforms(seed, first_draw + t, cells) for t in range(T)]) if T else np.zeros((0, cells))


def first_offender(clusters, weights, tables, uniforms=None):
    """None, or (sample, kind, position) of the first offender: the posterior predictive's six kinds, then kind 6, a uniform
    outside [0, 1) or not finite, at position n F + f."""
    found = predict_orc.first_offender(clusters, weights, tables)
    if uniforms is not None:
        u = np.asarray(uniforms).reshape(clusters.shape[0], -1)
        bad = np.argwhere(~((u >= 0.0) & (u < 1.0)))
        if bad.size:
            mine = (int(bad[0][0]), 6, int(bad[0][1]))
            found = mine if found is None else min(found, mine)
    return found


def mixture_rows(groups, n_groups, clusters_t, weights_t, tables_t):
    """m [N,F,S] of one sample, in the posterior predictive's operation order."""
    K, N = clusters_t.shape
    F, C = weights_t.shape
    S = tables_t.shape[2]
    off, _R = row_offsets(K, n_groups)
    h = np.zeros((N, C), dtype=bool)
    rows = np.zeros((N, C), dtype=np.int64)
    for c in range(1, C):
        h[:, c] = groups[c - 1] != NA
        rows[:, c] = np.where(h[:, c], off[c] + groups[c - 1].astype(np.int64), 0)
    ids, twice = cluster_ids(clusters_t)
    assert twice is None
    h[:, 0] = ids >= 0
    rows[:, 0] = np.where(ids >= 0, ids, 0)
    w = np.where(h[:, None, :], weights_t[None, :, :], 0.0)             # [N,F,C]
    wsum = np.zeros((N, F))
    for c in range(C):
        wsum = wsum + w[:, :, c]
    with np.errstate(invalid="ignore", divide="ignore"):
        wn = np.where((wsum > 0.0)[..., None], w / wsum[..., None], 0.0)
    m = np.zeros((N, F, S))
    for c in range(C):
        m = m + wn[:, :, c, None] * tables_t[rows[:, c]]
    return m


def sum_over_objects(d):
    """[N,F] -> [F] in the tree of dev_feature."""
    N, F = d.shape
    pad = np.zeros((-(-N // FEATURE_LANES) * FEATURE_LANES, F))
    pad[:N] = d
    lanes = np.zeros((FEATURE_LANES, F))
    for block in pad.reshape(-1, FEATURE_LANES, F):
        lanes = lanes + block
    total = lanes[0]
    for j in range(1, FEATURE_LANES):
        total = total + lanes[j]
    return total


def sum_over_features(d):
    """[N,F] -> [N] in the tree of dev_object."""
    N, F = d.shape
    pad = np.zeros((N, -(-F // OBJECT_LANES) * OBJECT_LANES))
    pad[:, :F] = d
    lanes = np.zeros((N, OBJECT_LANES))
    for block in np.moveaxis(pad.reshape(N, -1, OBJECT_LANES), 1, 0):
        lanes = lanes + block
    o = OBJECT_LANES // 2
    while o:
        lanes = lanes + lanes[:, np.arange(OBJECT_LANES) ^ o]
        o //= 2
    return lanes[:, 0]


def check(codes, groups, n_groups, clusters, weights, tables, seed=0, first_draw=0, uniforms=None):
    """The outputs of one call over all samples, which must be valid: dict(y_rep uint8 [T,N,F], dev_feature [T,2,F],
    dev_object [T,2,N], count_rep int32 [T,F,S], n_skipped, and for the tests d [T,2,N,F] (0 where nothing is added),
    drawn bool [T,N,F], margin [T,N,F] (inf where nothing is drawn), m [T,N,F,S])."""
    T, _K, N = clusters.shape
    F = weights.shape[1]
    S = tables.shape[3]
    observed = codes != NA
    x = np.where(observed, codes, 0).astype(np.int64)[..., None]
    out = dict(y_rep=np.full((T, N, F), NA, dtype=np.uint8), dev_feature=np.zeros((T, 2, F)), dev_object=np.zeros((T, 2, N)),
               count_rep=np.zeros((T, F, S), dtype=np.int32), n_skipped=0, d=np.zeros((T, 2, N, F)), drawn=np.zeros((T, N, F), dtype=bool),
               margin=np.full((T, N, F), np.inf), m=np.zeros((T, N, F, S)))
    for t in range(T):
        m = mixture_rows(groups, n_groups, clusters[t], weights[t], tables[t])
        cdf = np.zeros((N, F, S))
        acc = np.zeros((N, F))
        for s in range(S):
            acc = acc + m[:, :, s]
            cdf[:, :, s] = acc
        total = cdf[:, :, S - 1]
        drawn = observed & (total > 0.0)
        u = (np.asarray(uniforms)[t].reshape(N, F) if uniforms is not None else philox_uniforms(seed, first_draw + t, N * F).reshape(N, F))
        v = u * total
        below = (cdf <= v[..., None]).sum(axis=2)
        last = np.where(m > 0.0, np.arange(S), 0).max(axis=2)
        y = np.minimum(below, last)
        with np.errstate(divide="ignore", invalid="ignore"):
            d_obs = np.where(drawn, -2.0 * np.log(np.take_along_axis(m, x, axis=2)[..., 0]), 0.0)
            d_rep = np.where(drawn, -2.0 * np.log(np.take_along_axis(m, y[..., None], axis=2)[..., 0]), 0.0)
            margin = np.abs(v[..., None] - cdf).min(axis=2) / total
        out["m"][t] = m
        out["drawn"][t] = drawn
        out["margin"][t] = np.where(drawn, margin, np.inf)
        out["y_rep"][t] = np.where(drawn, y, NA)
        out["d"][t, 0], out["d"][t, 1] = d_obs, d_rep
        out["n_skipped"] += int((observed & ~drawn).sum())
        for side, d in enumerate((d_obs, d_rep)):
            out["dev_feature"][t, side] = sum_over_objects(d)
            out["dev_object"][t, side] = sum_over_features(d)
        for s in range(S):
            out["count_rep"][t, :, s] = (drawn & (y == s)).sum(axis=0)
    return out


def exact_draws(codes, groups, n_groups, clusters, weights, tables, uniforms):
    """The contract in exact arithmetic for small cases: (y [T][N][F] with None where nothing is drawn, m [T][N][F][S] as
    Fractions, margin [T][N][F] as Fractions or None).  y = #{s : cdf_s <= u total}; the clamp never acts exactly, since u < 1."""
    T, K, N = clusters.shape
    F, C = weights.shape[1:]
    S = tables.shape[3]
    off, _R = row_offsets(K, n_groups)
    ys, ms, margins = [], [], []
    for t in range(T):
        ids, twice = cluster_ids(clusters[t])
        assert twice is None
        yt, mt, gt = [], [], []
        for n in range(N):
            comp = [(0, int(ids[n]))] if ids[n] >= 0 else []
            comp += [(c, off[c] + int(groups[c - 1][n])) for c in range(1, C) if groups[c - 1][n] != NA]
            yn, mn, gn = [], [], []
            for f in range(F):
                wsum = sum((Fraction(float(weights[t, f, c])) for c, _r in comp), Fraction(0))
                m = [sum((Fraction(float(weights[t, f, c])) / wsum * Fraction(float(tables[t, r, f, s])) for c, r in comp), Fraction(0)) if wsum > 0
                     else Fraction(0) for s in range(S)]
                total = sum(m, Fraction(0))
                mn.append(m)
                if codes[n, f] == NA or total <= 0:
                    yn.append(None)
                    gn.append(None)
                    continue
                v = Fraction(float(uniforms[t, n * F + f])) * total
                cdf = [sum(m[:s + 1], Fraction(0)) for s in range(S)]
                yn.append(sum(1 for c in cdf if c <= v))
                gn.append(min(abs(v - c) for c in cdf) / total)
            yt.append(yn)
            mt.append(mn)
            gt.append(gn)
        ys.append(yt)
        ms.append(mt)
        margins.append(gt)
    return ys, ms, margins
