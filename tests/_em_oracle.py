"""fp64 NumPy restatement of the EM cluster initializer's numerical contract (include/sbe_em.h).

The reference's generate_clusters_em (sbayes/sampling/initializers.py:93-169) runs in float32 (float64 with the
cost-based geo prior) on whatever BLAS the host has.  The device runs every step in fp64 with every sum in a fixed order;
this module restates that contract in the same order where the order is cheap to keep (counts: ascending object; the sums
over states, features and groups: ascending index), so the device agrees with it to a few ulps per step:

  counts[g,f,s] = sum_n z[g,n] [x_nf = s]                 (x = state index, NA = S: NA contributes nothing)
  p             = (counts + 0.5 applicable) / sum_s (counts + 0.5 applicable)
  logp[g,f,s]   = log p;  logp[g,f,S] = log sum_s p          (NA: the reference's all-True _features row)
  ll[g,n]       = sum_f logp[g,f,x_nf]
  cost-based geo prior: zp = softmax(N z[:K], axis=1); geo = -(zp @ cost) / scale / 2;
                        rows >= K = logsumexp(geo[:K]) - log(K N)
  z             = softmax over g of where(available, geo + ll / T_i, -inf)

`discretize` restates discretize_fuzzy_cluster_2 (initializers.py:188-211) and `decision_margin` the distance of each
object's outcome from a tie in it (tests/test_em_oracle_cpu.py uses both)."""
from __future__ import annotations

import numpy as np


def temperatures(n_em_steps: int) -> np.ndarray:
    """T_i = (n_em_steps / (1 + i)) ** 3, the reference's Python doubles."""
    return np.array([(n_em_steps / (1 + i)) ** 3 for i in range(n_em_steps)], dtype=np.float64)


def state_index(features, na_values=None) -> np.ndarray:
    """uint8 [N, F] state index of a one-hot bool block [N, F, S]; S where the observation is missing (no state set)."""
    features = np.asarray(features, dtype=bool)
    s = features.shape[2]
    x = np.argmax(features, axis=2).astype(np.uint8)
    missing = ~features.any(axis=2) if na_values is None else np.asarray(na_values, dtype=bool)
    x[missing] = s
    return x


def em_steps(x, applicable, groups_available, n_clusters, z0, temps, cost=None, scale=None, record=None):
    """z after every step (a list of float64 [G, N] arrays) from z0 over len(temps) steps.  `record` (a dict) receives
    per step the largest |ll| and |geo| over the available (g, n): the inputs of logit_error_bound."""
    x = np.asarray(x).astype(np.intp)
    app = np.asarray(applicable, dtype=bool)
    avail = np.asarray(groups_available, dtype=bool)
    n, f_total = x.shape
    s_total = app.shape[1]
    g_total = avail.shape[0]
    k = int(n_clusters)
    prior = np.where(app, 0.5, 0.0)
    fidx = np.arange(f_total)
    z = np.array(z0, dtype=np.float64)
    out = []
    for t in temps:
        counts = np.zeros((g_total, f_total, s_total + 1))
        for i in range(n):                                   # ascending object per (g, f, s): the device's order
            counts[:, fidx, x[i]] += z[:, i, None]
        c = counts[:, :, :s_total] + prior[None]
        tot = np.zeros((g_total, f_total))
        for s in range(s_total):
            tot += c[:, :, s]
        p = c / tot[:, :, None]
        sp = np.zeros((g_total, f_total))
        for s in range(s_total):
            sp += p[:, :, s]
        with np.errstate(divide="ignore"):
            logp = np.concatenate([np.log(p), np.log(sp)[:, :, None]], axis=2)
        ll = np.zeros((g_total, n))
        for f in range(f_total):
            ll += logp[:, f, x[:, f]]
        if cost is not None:
            a = float(n) * z[:k]
            e = np.exp(a - a.max(axis=1, keepdims=True))
            zp = e / e.sum(axis=1, keepdims=True)
            geo_k = -(zp @ np.asarray(cost, dtype=np.float64)) / scale / 2
            m = geo_k.max()
            fill = (np.log(np.exp(geo_k - m).sum()) + m) - np.log(geo_k.size)
            geo = np.empty((g_total, n))
            geo[:k] = geo_k
            geo[k:] = fill
        else:
            geo = 0.0
        if record is not None:
            record.setdefault("ll_max", []).append(float(np.abs(ll[avail]).max()))
            record.setdefault("geo_max", []).append(float(np.abs(np.broadcast_to(geo, ll.shape)[avail]).max()))
        v = np.where(avail, geo + ll / float(t), -np.inf)
        m = v.max(axis=0)
        e = np.where(avail, np.exp(v - m), 0.0)
        tot = np.zeros(n)
        for g in range(g_total):
            tot += e[g]
        z = e / tot
        out.append(z.copy())
    return out


def discretize(z, n_clusters, min_size, total_size):
    """discretize_fuzzy_cluster_2: bool [K, N] clusters of a soft assignment z [G, N] (rows [0, K) are the clusters)."""
    k = int(n_clusters)
    fz = np.copy(z[:k])
    for c in range(k):
        best = np.argsort(fz[c])[-min_size:]
        fz[:, best] = 0
        fz[c, best] = 1
    best = np.argmax(fz, axis=0)
    best_value = np.max(fz, axis=0)
    threshold = np.sort(best_value)[-total_size]
    best[best_value < threshold] = k
    return np.eye(k + 1, dtype=bool)[best].T[:-1]


def decision_margin(z, n_clusters, min_size, total_size):
    """Per object: how far its outcome in `discretize` is from a tie, as a RELATIVE gap |a - b| / max(a, b) between
    the two values of z compared (softmax errors are relative: a logit error d scales an entry of z by at most
    exp(+-2 d)).  The smallest non-zero one of
      - the gap between its best cluster value and the threshold (sort(best_value)[-total_size]);
      - for an object that passes the threshold, the gap between its best and second-best cluster values;
      - for each cluster row, the gap between its value and the row's min_size-th largest value (or, for one of the
        min_size largest, the (min_size+1)-th): whether the object is forced into the cluster.
    `z` is what discretize sees (rounded to the reference's dtype).  Exact ties (a gap of 0: float32 values saturated at
    1.0) are decided by the method's own tie rule, the same way from any z that rounds to the same values; they do not
    count.  Entries and order statistics of z move by a factor within [1 - r, 1 + r] when every entry does, so an object
    whose margin exceeds 2 r / (1 - r) is discretized the same from both z's."""
    k = int(n_clusters)
    fz = np.array(z[:k], dtype=np.float64)
    n = fz.shape[1]

    def rel(a, b):
        top = np.maximum(np.abs(a), np.abs(b))
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.abs(a - b) / top
        return np.where(r > 0, r, np.inf)                     # (0 / 0 and exact ties: no margin)

    margin = np.full(n, np.inf)
    forced = np.zeros(n, dtype=bool)
    for c in range(k):
        order = np.sort(fz[c])
        if min_size < n:
            hi, lo = order[-min_size], order[-min_size - 1]
            margin = np.minimum(margin, np.where(fz[c] >= hi, rel(fz[c], lo), rel(fz[c], hi)))
        best = np.argsort(fz[c])[-min_size:]
        forced[best] = True
        fz[:, best] = 0
        fz[c, best] = 1
    best_value = np.max(fz, axis=0)
    threshold = np.sort(best_value)[-total_size]
    gap = rel(best_value, threshold)
    if k > 1:
        top2 = np.sort(fz, axis=0)[-2:]
        gap = np.where(best_value >= threshold, np.minimum(gap, rel(top2[1], top2[0])), gap)
    free = ~forced
    margin[free] = np.minimum(margin[free], gap[free])
    return margin


U32 = 2.0 ** -24                                              # float32 unit roundoff


def logit_error_bound(n_features, ll_max, temperature, n_objects=0, geo_max=0.0):
    """Bound d on how far one float32 step of the reference moves a logit geo + ll / T from its exact value: each of the
    F terms log p is off by u (p rounded) + u |log p| (the log rounded), their float32 sum by (F - 1) u sum |log p|,
    the division by T by u |ll / T|; with the geo prior (float64 except softmax(N z) of the float32 z0: N u of the
    exponent) 2 (N + 2) u |geo|."""
    d = (n_features + 2) * U32 * (1.0 + ll_max) / temperature
    if geo_max:
        d += 2 * (n_objects + 2) * U32 * geo_max
    return d


def z_relative_bound(n_features, n_groups, ll_max, temperature, n_objects=0, geo_max=0.0):
    """Relative bound r on one float32 step's z: a logit error d scales exp(v - max) / sum by at most exp(2 d), and the
    float32 softmax itself (exp, the sum over G groups, the division, the rounding of z) adds (G + 3) u."""
    d = logit_error_bound(n_features, ll_max, temperature, n_objects, geo_max)
    return float(np.expm1(2 * d)) + (n_groups + 3) * U32
