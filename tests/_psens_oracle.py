"""NumPy fp64 restatement of the power-scaling sensitivity (sbayes_amd.psens, include/sbe_psens.h, csrc/sbe_psens.hip): the
checker of the unit, in the kernels' order of operations.

The contract, per column x of N stacked draws (chain order, burn-in dropped per chain) and weight vector w [N]:

* xs = x + 0.0; order = stable argsort of xs (ties by sample index); s = xs[order]; q = w[order];
* the prefix sum of q in ONE stated order: with L = ceil(N / 256), chunk t holds the sorted places [t L, (t + 1) L); a chunk
  is added in sequence from 0.0; the 256 chunk totals are added in sequence from 0.0; Qraw_i = (totals before the chunk) +
  (the chunk's sum up to i), Q_i = Qraw_i / (all totals).  prefix_q restates it with two np.cumsum (sequential);
* P_i = (i + 1) / N, M_i = 0.5 (P_i + Q_i), b_i = s[i + 1] - s[i], i = 0 .. N - 2; with log2 0 := 0
      Pint = sum b P;  Qint = sum b Q;  bound = Pint + Qint
      pq = max(0, sum (b P) (log2 P - log2 M) + HALF_INV_LN2 (Qint - Pint))
      qp = max(0, sum (b Q) (log2 Q - log2 M) + HALF_INV_LN2 (Pint - Qint));   js = pq + qp
  every sum: per chunk in sequence from 0.0 (the 256 threads' partials), then `tree` (lanes by xor at 32 .. 1, the four
  waves in index order);
* the same of -x from the same sort: s' = -s[::-1], q' = q[::-1];
* wmean = tree(chunk sums of q s) / (all totals); wsd = sqrt(tree(chunk sums of q ((s - wmean) (s - wmean))) / (all totals));
* a column with a non-finite value: flag 2, NaN everywhere; max - min < 1e-15: flag 1, js = bound = 0, its moments;
* a vector of equal PSIS ratios (VFLAG_CONSTANT) counts as q = 1: Q = P bit for bit, so js = 0 exactly.

Q, P, M and b involve additions, one division and one halving only, so device and checker agree on them bit for bit, and
so on Pint, Qint and bound.  They differ in log2 alone: bound_js gives what that allows (see its docstring).

PSIS is tests/_elpd_oracle.psis_column(-ratios), by construction (component_weights calls it).

The formula is the published one (Kallioinen et al. 2023, the CJS distance of `priorsense` / `arviz.psens`) as far as it can
be restated here; no arviz value was available, so the checker is pinned by closed forms, by a 50-digit evaluation of its own
sums and by invariances (tests/test_psens_oracle_cpu.py)."""
from __future__ import annotations

import math

import numpy as np

from tests import _elpd_oracle as eorc

THREADS, LANES = 256, 64
U = 2.0 ** -53
HALF_INV_LN2 = 0.7213475204444817        # 0.5 / ln 2, the kernels' literal
# The ulp error allowed to the device's float64 log2: no document of the device library that ships with the compiler states one,
# so it was measured against mpmath on (i + 1) / 1000 (tools/psens_speed.py -> profiles/psens/README.md: 0.6148 ulp at the worst
# of the 1000 values on an MI355X, NumPy's 0.4993) and one ulp was added for the values not sampled.  Never set from the kernel's
# agreement with this checker.
LOG2_ULP = 1.62
FLAG_CONSTANT, FLAG_NONFINITE = 1, 2
VFLAG_CONSTANT, VFLAG_UNRELIABLE = 1, 2
OUTPUTS = ("js", "bound", "js_neg", "bound_neg", "wmean", "wsd")


def chunk_len(n):
    return -(-n // THREADS)


def depth(n):
    """Height of the summation tree of n terms: a chunk in sequence, six exchanges, three additions of the waves."""
    return chunk_len(n) + 6 + 3


def tree(partials):
    """The fixed tree over the 256 threads' partials (sbe_unit_device.hip.h: unit_block_reduce)."""
    v = np.asarray(partials, dtype=np.float64).reshape(THREADS // LANES, LANES)
    index = np.arange(LANES)
    o = LANES // 2
    while o:
        v = v + v[:, index ^ o]
        o //= 2
    t = v[0, 0]
    for w in range(1, THREADS // LANES):
        t = t + v[w, 0]
    return float(t)


def _chunk_cumsum(terms):
    """[256, L]: every chunk's running sums in sequence from 0.0 (terms padded with 0.0, which changes no sum)."""
    terms = np.asarray(terms, dtype=np.float64)
    n, length = len(terms), chunk_len(len(terms))
    padded = np.zeros(THREADS * length, dtype=np.float64)
    padded[:n] = terms
    rows = np.concatenate([np.zeros((THREADS, 1)), padded.reshape(THREADS, length)], axis=1)
    return np.cumsum(rows, axis=1)[:, 1:]


def chunk_sums(terms):
    return _chunk_cumsum(terms)[:, -1]


def tree_sum(terms):
    return tree(chunk_sums(terms))


def prefix_q(q):
    """(Q float64 [N], total): the normalised prefix sums of q in the stated order."""
    q = np.asarray(q, dtype=np.float64)
    local = _chunk_cumsum(q)
    scan = np.cumsum(np.concatenate([[0.0], local[:, -1]]))
    raw = (scan[:-1, None] + local).ravel()[:len(q)]
    total = float(scan[-1])
    return raw / total, total


def _log2(v):
    """log2 with log2 0 := 0."""
    out = np.zeros_like(v)
    np.log2(v, out=out, where=v > 0.0)
    return out


def pieces(s, q):
    """P, Q, M, b (float64 [N - 1]) and the total of q, for sorted values s and the weights q in that order."""
    s = np.asarray(s, dtype=np.float64)
    n = len(s)
    big_q, total = prefix_q(q)
    big_q = big_q[:-1]
    big_p = np.arange(1, n, dtype=np.float64) / float(n)
    return big_p, big_q, 0.5 * (big_p + big_q), s[1:] - s[:-1], total


def sums(s, q):
    """dict(js, bound, pint, qint, magnitude) of one direction; magnitude: the A of bound_js."""
    big_p, big_q, mid, b, _total = pieces(s, q)
    l2p, l2q, l2m = _log2(big_p), _log2(big_q), _log2(mid)
    bp, bq = b * big_p, b * big_q
    last = np.zeros(1)                                                       # (place N - 1 adds nothing)
    pint, qint = tree_sum(np.concatenate([bp, last])), tree_sum(np.concatenate([bq, last]))
    spq = tree_sum(np.concatenate([bp * (l2p - l2m), last]))
    sqp = tree_sum(np.concatenate([bq * (l2q - l2m), last]))
    pq = spq + HALF_INV_LN2 * (qint - pint)
    qp = sqp + HALF_INV_LN2 * (pint - qint)
    pq, qp = (0.0 if pq < 0.0 else pq), (0.0 if qp < 0.0 else qp)
    magnitude = float(np.sum(np.abs(b) * (big_p + big_q) * (np.abs(l2p) + np.abs(l2q) + 2.0 * np.abs(l2m)))) + HALF_INV_LN2 * (abs(pint) + abs(qint))
    return dict(js=pq + qp, bound=pint + qint, pint=pint, qint=qint, magnitude=magnitude)


def bound_js(n, magnitude, log2_ulp=LOG2_ULP):
    """What |js_device - js_checker| may be: (L + depth + 4) u A with A = sum b (P + Q) (|log2 P| + |log2 Q| + 2 |log2 M|) +
    (Pint + Qint) / (2 ln 2).  A term (b P) (log2 P - log2 M) carries one rounding of b P, L ulp of each log2, one of the
    difference and one of the product; the tree adds depth roundings of the running sums; Pint and Qint are the same bits on
    both sides."""
    return (log2_ulp + depth(n) + 4) * U * magnitude


def moments(s, q):
    s, q = np.asarray(s, dtype=np.float64), np.asarray(q, dtype=np.float64)
    total = prefix_q(q)[1]
    wmean = tree_sum(q * s) / total
    d = s - wmean
    return wmean, math.sqrt(tree_sum(q * (d * d)) / total)


def column(x, w, vflag=None):
    """One column against V weight vectors: dict of float64 [V] (OUTPUTS, pint, qint, magnitude, magnitude_neg) and `flag`."""
    x = np.asarray(x, dtype=np.float64) + 0.0
    w = np.atleast_2d(np.asarray(w, dtype=np.float64))
    n_vectors = w.shape[0]
    vflag = np.zeros(n_vectors, dtype=np.uint8) if vflag is None else np.asarray(vflag)
    keys = OUTPUTS + ("pint", "qint", "magnitude", "magnitude_neg")
    out = {k: np.full(n_vectors, np.nan) for k in keys}
    if not np.all(np.isfinite(x)):
        out["flag"] = FLAG_NONFINITE
        return out
    constant = bool(x.max() - x.min() < 1e-15)
    out["flag"] = FLAG_CONSTANT if constant else 0
    order = np.argsort(x, kind="stable")
    s = x[order]
    for v in range(n_vectors):
        q = np.ones(len(x)) if vflag[v] & VFLAG_CONSTANT else w[v][order]
        fwd, neg = sums(s, q), sums(-s[::-1], q[::-1])
        out["wmean"][v], out["wsd"][v] = moments(s, q)
        out["pint"][v], out["qint"][v] = fwd["pint"], fwd["qint"]
        out["magnitude"][v], out["magnitude_neg"][v] = fwd["magnitude"], neg["magnitude"]
        for key, value in (("js", fwd["js"]), ("bound", fwd["bound"]), ("js_neg", neg["js"]), ("bound_neg", neg["bound"])):
            out[key][v] = 0.0 if constant else value
    return out


def table(x, w, vflag=None):
    """Every column of x [N, P] against w [V, N]: dict of float64 [V, P] and flag uint8 [P]."""
    x = np.asarray(x, dtype=np.float64)
    cols = [column(x[:, j], w, vflag) for j in range(x.shape[1])]
    out = {k: np.stack([c[k] for c in cols], axis=1) for k in cols[0] if k != "flag"}
    out["flag"] = np.array([c["flag"] for c in cols], dtype=np.uint8)
    return out


# ---- the host's part ----------------------------------------------------------------------------------------------------
def distance(js, bound):
    js, bound = np.asarray(js, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.sqrt(js / bound)
    return np.where(bound == 0.0, 0.0, d)


def cjs(res):
    return np.maximum(distance(res["js"], res["bound"]), distance(res["js_neg"], res["bound_neg"]))


def sensitivity(cjs_rows, delta):
    cjs_rows = np.asarray(cjs_rows)
    return (cjs_rows[0::2] + cjs_rows[1::2]) / (2.0 * math.log2(1.0 + delta))


def stack(chains, burn_rows):
    """The draws the unit sees: every chain's rows after its burn-in, in chain order."""
    return np.concatenate([np.asarray(c, dtype=np.float64)[b:] for c, b in zip(chains, burn_rows)], axis=0)


# ---- the weights ---------------------------------------------------------------------------------------------------------
def scales(delta):
    """alpha - 1 of a component's two vectors."""
    return (1.0 / (1.0 + delta) - 1.0, (1.0 + delta) - 1.0)


def psis_weights(ratios):
    """(log weights [N], k, vflag) of one vector of log ratios."""
    ratios = np.asarray(ratios, dtype=np.float64)
    if ratios.max() - ratios.min() == 0.0:
        return np.full(len(ratios), -math.log(len(ratios))), np.inf, VFLAG_CONSTANT
    lw, k = eorc.psis_column(-ratios)
    return lw, float(k), (VFLAG_UNRELIABLE if k > 0.7 else 0)


def component_weights(x, columns, delta):
    """(log weights [2 G, N], k [2 G], ess [2 G], vflag [2 G]) for the component columns of the stacked draws x [N, P]."""
    lws, ks, flags = [], [], []
    for col in columns:
        for scale in scales(delta):
            lw, k, flag = psis_weights(scale * np.asarray(x, dtype=np.float64)[:, col])
            lws.append(lw)
            ks.append(k)
            flags.append(flag)
    lws = np.stack(lws)
    ess = 1.0 / np.sum(np.exp(lws) ** 2, axis=1)
    return lws, np.array(ks), ess, np.array(flags, dtype=np.uint8)


def powerscale(x, columns, delta):
    """End to end on stacked draws x [N, P]: (sensitivity [G, P], cjs [2 G, P], the table, k, vflag)."""
    lws, ks, _ess, flags = component_weights(x, columns, delta)
    weights = np.where((flags & VFLAG_CONSTANT)[:, None] != 0, 1.0 / x.shape[0], np.exp(lws))
    res = table(x, weights, flags)
    rows = cjs(res)
    return sensitivity(rows, delta), rows, res, ks, flags


# ---- a 50-digit evaluation of `sums` on the checker's own P, Q, M, b (the yardstick's yardstick) -------------------------
def sums_mp(s, q):
    """(js, bound) of one direction in 50 digits, P, Q, M and b taken as the exact doubles the checker forms."""
    import mpmath
    big_p, big_q, mid, b, _total = pieces(s, q)
    with mpmath.workdps(50):
        ln2 = mpmath.log(2)
        pint = qint = spq = sqp = mpmath.mpf(0)
        for p, qv, m, bv in zip(big_p, big_q, mid, b):
            p, qv, m, bv = mpmath.mpf(float(p)), mpmath.mpf(float(qv)), mpmath.mpf(float(m)), mpmath.mpf(float(bv))
            lm = mpmath.log(m) / ln2
            pint += bv * p
            qint += bv * qv
            spq += bv * p * (mpmath.log(p) / ln2 - lm)
            if qv > 0:
                sqp += bv * qv * (mpmath.log(qv) / ln2 - lm)
        half = mpmath.mpf(HALF_INV_LN2)
        pq, qp = spq + half * (qint - pint), sqp + half * (pint - qint)
        js = max(pq, mpmath.mpf(0)) + max(qp, mpmath.mpf(0))
        return js, pint + qint
