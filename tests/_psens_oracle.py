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
sums and by invariances (tests/test_psens_oracle_cpu.py).

For the weights' range tests (tests/test_psens_range_cpu.py, tests/test_gpu_psens_range.py) the module also measures how far
the PSIS checker's own k follows the last bit of its elementary functions (k_spread, tol_k) and evaluates the same steps in 50
digits (psis_weights_mp)."""
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


# ---- the weights over their range (tests/_psens_range_cases.py): the tail's anatomy, the checker's conditioning, 50 digits ---
def tail_count(n):
    """ceil(min(0.2 N, 3 sqrt N)), the tail psis_column asks for."""
    return int(math.ceil(min(0.2 * n, 3 * math.sqrt(n))))


def tail_anatomy(ratios):
    """(tail count asked for, ratios strictly above the cutoff, whether the cutoff is floored at log DBL_MIN), by
    psis_column's first steps."""
    x = np.asarray(ratios, dtype=np.float64)
    with np.errstate(over="ignore"):
        x = x - np.max(x)
    tail_n = tail_count(len(x))
    at_rank = float(np.sort(x)[len(x) - tail_n - 1])
    floor = math.log(eorc.DBL_MIN)
    return tail_n, int(np.sum(x > max(at_rank, floor))), at_rank < floor


class _Jittered:
    """Stands in for a module (numpy, math) inside tests/_elpd_oracle: exp, log1p, log and sqrt give their value moved by -1,
    0 or +1 ulp at random, every other name is the module's.  Zeros and non-finite values stay; sqrt of a plain number (the
    tail count's 3 sqrt S, an integer rule) stays."""
    _moved = ("exp", "log1p", "log", "sqrt")

    def __init__(self, module, rng):
        self._module, self._rng = module, rng

    def __getattr__(self, name):
        f = getattr(self._module, name)
        if name not in self._moved:
            return f

        def moved(v, *args, **kwargs):
            out = f(v, *args, **kwargs)
            if name == "sqrt" and np.ndim(v) == 0:
                return out
            a = np.asarray(out, dtype=np.float64)
            step = self._rng.integers(-1, 2, size=a.shape)
            with np.errstate(over="ignore"):
                b = np.where(step > 0, np.nextafter(a, np.inf), np.where(step < 0, np.nextafter(a, -np.inf), a))
            b = np.where(np.isfinite(a) & (a != 0.0), b, a)
            return b if np.ndim(out) else float(b)
        return moved


class _jitter:
    """Context manager: tests/_elpd_oracle sees _Jittered numpy and math inside it and its own modules again after it."""

    def __init__(self, seed):
        self._rng = np.random.default_rng(seed)

    def __enter__(self):
        self._saved = (eorc.np, eorc.math)
        eorc.np, eorc.math = _Jittered(self._saved[0], self._rng), _Jittered(self._saved[1], self._rng)

    def __exit__(self, *exc):
        eorc.np, eorc.math = self._saved
        return False


def k_spread(ratios, repeats=16, seed=2024):
    """(largest |k' - k|, largest |lw' - lw|) over `repeats` seeded runs of the float64 checker in which every value of exp,
    log1p, log and sqrt formed inside psis_column / gpdfit / gpinv is moved by -1, 0 or +1 ulp at random: how far the
    checker's own k and log weights follow the last bit of its elementary functions.  inf where a run changes whether k
    (or a log weight) is finite or NaN; entries that are -inf or NaN in every run add nothing."""
    ratios = np.asarray(ratios, dtype=np.float64)
    with np.errstate(over="ignore"):
        if ratios.max() - ratios.min() == 0.0:
            return 0.0, 0.0
    lw, k = eorc.psis_column(-ratios)
    dk = dlw = 0.0
    for r in range(repeats):
        with _jitter([seed, r]):
            lw2, k2 = eorc.psis_column(-ratios)
        if np.isfinite(k) and np.isfinite(k2):
            dk = max(dk, abs(float(k2) - float(k)))
        elif not (k == k2 or (np.isnan(k) and np.isnan(k2))):
            dk = math.inf
        same = (lw == lw2) | (np.isnan(lw) & np.isnan(lw2))
        with np.errstate(invalid="ignore"):
            moved = np.abs(lw2 - lw)[~same]
        if moved.size:
            dlw = max(dlw, math.inf if np.isnan(moved).any() else float(moved.max()))
    return dk, dlw


K_TOL, K_MARGIN = 1e-10, 8.0


def tol_k(ratios, repeats=16, seed=2024):
    """What |k_device - k_checker| may be for one vector of log ratios: the project's 1e-10 for well-conditioned fits plus 8
    times the checker's own spread under a +-1 ulp probe (the device's exp and log1p are good to a few
    ulp, not to one; its sums run in another order; sixteen samples miss the worst case).  From the checker alone."""
    return K_TOL + K_MARGIN * k_spread(ratios, repeats, seed)[0]


def psis_weights_mp(ratios):
    """(log weights float64 [N], k) of one vector of log ratios by the steps of psis_column / gpdfit / gpinv in 50 digits, the
    ratios taken as the exact doubles.  For short inputs (N <= 1000)."""
    import mpmath
    ratios = [float(r) for r in np.asarray(ratios, dtype=np.float64)]
    s = len(ratios)
    tail_n = tail_count(s)
    with mpmath.workdps(50):
        mpf = mpmath.mpf
        top = max(ratios)
        x = [mpf(r) - mpf(top) for r in ratios]
        xcutoff = max(sorted(x)[s - tail_n - 1], mpmath.log(mpf(float(eorc.DBL_MIN))))
        expxcutoff = mpmath.exp(xcutoff)
        tail = sorted((i for i in range(s) if x[i] > xcutoff), key=lambda i: (x[i], i))
        n = len(tail)
        k = mpmath.inf
        if n > 4:
            ary = [mpmath.exp(x[i]) - expxcutoff for i in tail]
            m_est = 30 + int(n ** 0.5)
            quart, last = ary[int(n / 4 + 0.5) - 1], ary[-1]
            b_ary = [(1 - mpmath.sqrt(mpf(m_est) / (mpf(j) - mpf(0.5)))) / (3 * quart) + 1 / last for j in range(1, m_est + 1)]
            k_ary = [mpmath.fsum(mpmath.log1p(-b * a) for a in ary) / n for b in b_ary]
            len_scale = [n * (mpmath.log(-(b / kk)) - kk - 1) for b, kk in zip(b_ary, k_ary)]
            weights = [1 / mpmath.fsum(mpmath.exp(lj - li) for lj in len_scale) for li in len_scale]
            kept = [(b, w) for b, w in zip(b_ary, weights) if w >= 10 * mpf(float(eorc.DBL_EPS))]
            wsum = mpmath.fsum(w for _b, w in kept)
            b_post = mpmath.fsum(b * (w / wsum) for b, w in kept)
            k_post = mpmath.fsum(mpmath.log1p(-b_post * a) for a in ary) / n
            sigma = -k_post / b_post
            k = (n * k_post + 5) / (n + 10)
            if sigma <= 0:
                return np.full(s, np.nan), float(k)
            for place, i in enumerate(tail):
                lp = mpmath.log1p(-(mpf(place) + mpf(0.5)) / n)
                gq = -lp if abs(k) < mpf(float(eorc.DBL_EPS)) else mpmath.expm1(-k * lp) / k
                x[i] = min(mpmath.log(gq * sigma + expxcutoff), mpf(0))
        peak = max(x)
        lse = mpmath.log(mpmath.fsum(mpmath.exp(v - peak) for v in x)) + peak
        return np.array([float(v - lse) for v in x]), float(k)
