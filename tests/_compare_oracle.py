"""The contract of the model comparison (include/sbe_compare.h, sbayes_amd/compare.py) restated on the host in fp64, sums by
math.fsum.  A plain helper module: it holds no test.

x is float64 [N, M]: column k holds model k's pointwise ELPD values on the log scale.  arviz is not a dependency, so the
restatement is pinned by known answers (tests/test_compare_oracle_cpu.py), as tests/_elpd_oracle.py is."""
import math

import numpy as np

from oracle import sbayes_oracle as orc


def _fsum_columns(a):
    return np.array([math.fsum(a[:, k]) for k in range(a.shape[1])])


def totals(x):
    """(elpd, se): elpd_k = sum_i x_ik, se_k = sqrt(N var_i(x_ik)), ddof 0 (arviz's ELPDData)."""
    n = x.shape[0]
    total = _fsum_columns(x)
    dev2 = _fsum_columns((x - total / n) ** 2)
    return total, np.sqrt(n * (dev2 / n))


def rank(elpd):
    """Input positions in rank order: elpd descending, ties by input order."""
    return np.argsort(-np.asarray(elpd), kind="stable")


def differences(x, ref):
    """(elpd_diff, dse) against model ref: d_i = x_i,ref - x_ik; exactly 0 at ref."""
    return totals(x[:, [ref]] - x)


def shifted(x):
    """p_ik = exp(x_ik - max_k x_ik)."""
    return np.exp(x - x.max(axis=1, keepdims=True))


def objective(x, w):
    """f(w) = mean_i log(sum_k w_k p_ik), on the shifted p (the shift moves f by a constant)."""
    return math.fsum(np.log(shifted(x) @ np.asarray(w, dtype=np.float64))) / x.shape[0]


def gradient(x, w, exact=True):
    """g_k = mean_i(p_ik / sum_j w_j p_ij)."""
    p = shifted(x)
    r = p / (p @ np.asarray(w, dtype=np.float64))[:, None]
    return (_fsum_columns(r) if exact else r.sum(axis=0)) / x.shape[0]


def gap(x, w):
    """max_k g_k - 1 >= f* - f(w) (concavity, and sum_k w_k g_k = 1)."""
    return float(np.max(gradient(x, w))) - 1.0


def stacking(x, tol=1e-8, max_iter=100_000, exact=True):
    """The EM fixed point from w = 1/M: (weights, gap of those weights, updates that led to them, converged).  The gap is
    looked at after every update (the device looks every CHECK_EVERY: the update counts differ, the contract is the gap).
    exact=False adds with np.sum instead of math.fsum (the speed tool's sizes)."""
    n, m = x.shape
    p = shifted(x)
    w = np.full(m, 1.0 / m)
    for updates in range(max_iter + 1):
        r = p / (p @ w)[:, None]
        g = (_fsum_columns(r) if exact else r.sum(axis=0)) / n
        gap_w = float(np.max(g)) - 1.0
        if gap_w <= tol or updates == max_iter:
            return w, gap_w, updates, gap_w <= tol
        w = w * g
        w = w / np.sum(w)                       # (1 but for rounding: the weights do not drift off the simplex)


def stacking_slsqp(x):
    """arviz.compare's stacking as arviz states it, on this host's SciPy: SLSQP on -sum_i log(exp(x_i) . w) over the first
    M - 1 weights, from w = 1/M, with arviz's bounds, constraints and gradient; exp is not shifted.  Returns the M weights."""
    from scipy.optimize import minimize
    n, m = x.shape
    if m == 1:
        return np.ones(1)
    exp_x = np.exp(x)
    last = m - 1

    def full(w):
        return np.concatenate((w, [max(1.0 - np.sum(w), 0.0)]))

    def neg_score(w):
        return -np.sum(np.log(exp_x @ full(w)))

    def neg_gradient(w):
        d = exp_x @ full(w)
        return -np.array([np.sum((exp_x[:, k] - exp_x[:, last]) / d) for k in range(last)])

    res = minimize(fun=neg_score, x0=np.full(last, 1.0 / m), jac=neg_gradient, bounds=[(0.0, 1.0)] * last,
                   constraints=[{"type": "ineq", "fun": lambda w: 1.0 - np.sum(w)}, {"type": "ineq", "fun": np.sum}])
    return full(res["x"])


def exponentials(seed, b, n):
    """e_bi = -log(1 - u), u the engine's Philox uniform i of draw b under seed: Exp(1), never infinite (1 - u is exact and > 0)."""
    return -np.log(1.0 - orc.philox_uniforms(seed, b, n))


def bootstrap(x, seed, b_samples):
    """(weights [M], se [M], z [B, M], w_b [B, M], bound [B, M]): z_bk = N sum_i(e_bi x_ik) / sum_i e_bi, w_b = softmax(z_b),
    weights = mean_b w_b, se_k = sd_b(z_bk) with ddof 0; bound_bk = N sum_i(e_bi |x_ik|) / sum_i e_bi, the scale of z_bk's
    rounding error."""
    n, m = x.shape
    z, bound = np.empty((b_samples, m)), np.empty((b_samples, m))
    for b in range(b_samples):
        e = exponentials(seed, b, n)
        total = math.fsum(e)
        z[b] = n * _fsum_columns(e[:, None] * x) / total
        bound[b] = n * _fsum_columns(e[:, None] * np.abs(x)) / total
    t = np.exp(z - z.max(axis=1, keepdims=True))
    w_b = t / t.sum(axis=1, keepdims=True)
    weights = _fsum_columns(w_b) / b_samples
    se = np.sqrt(_fsum_columns((z - _fsum_columns(z) / b_samples) ** 2) / b_samples)
    return weights, se, z, w_b, bound


def pseudo_bma(elpd):
    """softmax of the totals."""
    t = np.exp(np.asarray(elpd) - np.max(elpd))
    return t / np.sum(t)


def gamma_values(seed, n, m, spread=0.3):
    """Seeded pointwise values around -2: minus gamma draws (shape 4, scale 0.5), the models shifted against each other."""
    rng = np.random.default_rng(seed)
    return -(rng.gamma(4.0, 0.5, (n, m)) + spread * rng.random(m)[None, :] * rng.random((n, 1)))


def planted(n1, n2, p, q):
    """Two models, n1 observations at (log p, log q) and n2 at (log q, log p); the optimum's w_0 in closed form."""
    x = np.concatenate([np.tile([math.log(p), math.log(q)], (n1, 1)), np.tile([math.log(q), math.log(p)], (n2, 1))])
    w0 = min(1.0, max(0.0, (n1 * p - n2 * q) / ((n1 + n2) * (p - q))))
    return x, w0
