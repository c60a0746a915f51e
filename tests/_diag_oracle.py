"""The convergence diagnostics restated in fp64 NumPy: the checker of sbayes_amd.diag.

`diagnose(chains, burnin, split, max_lag)` follows the contract step by step: per chain the first int(burnin * S_r) rows
are dropped, the chains are cut at the end to the shortest remaining length, with split every chain of n draws becomes
x[:n // 2] and x[-(n // 2):]; then per column

    flags       non-finite value: flag 2, NaN everywhere; max - min < 1e-15: flag 1, ess = M n, rhat NaN, mcse_mean 0
    mu_m        mean of chain m;  d = x[m] - mu_m;  g_m(t) = (1/n) sum_{i < n-t} d[i] d[i+t];  G(t) = mean_m g_m(t)
    mean_var    G(0) n / (n-1);  var_plus = mean_var (n-1)/n + var(mu_m, ddof 1) (0 for one chain)
    rhat        sqrt(var_plus / mean_var);  rho(t) = 1 - (mean_var - G(t)) / var_plus
    rho_t       Geyer's initial positive sequence, then the initial monotone sequence (the loops below, to the letter)
    tau         max(-1 + 2 sum(rho_t[:max_t+1]) + rho_t[max_t+1], 1 / log10(M n));  ess = M n / tau
    mean, sd    over all M n values (sd with ddof 1);  mcse_mean = sd / sqrt(ess)

The means and autocovariances are exact sums (math.fsum), so the checker carries no summation error of its own; what
it does carry -- one rounding in each chain mean, in each d and in each product before the exact sum, 4u G(0) on an
autocovariance at most -- is counted in the bound.

It also returns each column's DECISION MARGIN: the smallest |even + odd| met by the first loop and the smallest
|(rho_t[t+1] + rho_t[t+2]) - (rho_t[t-1] + rho_t[t])| met by the second (and, with max_lag, nothing more: that stop is an
integer comparison).  A device whose rho values are within the bound below of the checker's takes the same decisions
whenever the margin exceeds twice that bound; the fixed cases of the GPU tests have margins >= 1e-9.

BOUNDS (`column_bounds`, per column; u = 2^-53).  A sum of N terms in any fixed order is within (N-1) u sum|terms| of the
exact sum (Higham, Accuracy and Stability, eq. 4.4, first order).  First-order terms are kept and the whole bound is
doubled for the second-order ones (every first-order quantity here is below 1e-9 relative, so the neglected terms are
below 1e-9 of the kept ones).  With A_m = mean|x| and D_m = mean|d| of chain m, D = mean|d| over all chains:

    mu_m        two steps: mu0 = fl(sum x / n) is within e0 = (n-1) u A_m + u |mu_m| of mu_m; the residual sum of
                fl(x - mu0) (n roundings of terms, n-1 of the sum, one division) adds back the difference, leaving
                e_mu = u |mu_m| + (n+1) u (D_m + e0).  e_mu below is the largest over the chains.
    d           d' = fl(x - mu'): |d' - d| <= eps = e_mu + u max|d|
    mean        mean of the M chain means: e_mean = e_mu + (M+1) u |mean|
    sd          sd is the root mean square of the deviations x - mean (times sqrt(N/(N-1)), N = M n), which is
                1-Lipschitz in each deviation under the max norm: deviations are off by eps + e_mean + 2u max|x - mean|,
                the sum of squares adds (N+2) u relative, halved by the root: e_sd = sqrt(N/(N-1)) (eps + e_mean + 2u dev_max)
                + (N/2 + 3) u sd
    G(t)        |sum d'd' - sum dd| / (M n) <= 2 eps D (+ eps^2); products, the sum of at most M n terms and the two
                divisions: (M n + 2) u (1/(M n)) sum|d_i d_{i+t}| <= (M n + 2) u G(0) (Cauchy-Schwarz):
                e_G = (M n + 2) u G(0) + 2 eps D + eps^2 + 4u G(0) (the checker's own)
    mean_var    e_mv = (e_G + 2u G(0)) n/(n-1)
    var_plus    B = var(mu_m): deviations off by 2 e_mu, so |B' - B| <= 4 e_mu sqrt(M/(M-1)) sqrt(B) + 4 e_mu^2 M/(M-1)
                + (M+3) u B = e_B;  e_vp = e_mv + 2u mean_var + e_B + u var_plus
    rhat        relative (e_vp / var_plus + e_mv / mean_var) / 2 + 2u
    rho(t)      q = (mean_var - G(t)) / var_plus: e_rho = (e_mv + e_G) / var_plus + max_t|q| e_vp / var_plus + 3u (1 + max|q|)
                (one figure for all lags of the column)
    tau         the monotone pass replaces values by means of two values (error no larger than the larger, one more
                rounding); with K = max_t + 2 terms: e_tau = 2 K e_rho + (K + 3) u (1 + 2 sum|rho_t|); the floor is
                1-Lipschitz and its own value is within 4u of exact: e_tau = max(e_tau, 4u floor)
    ess         relative e_tau / tau + 2u;  mcse_mean: relative e_sd / sd + half that of ess + 2u

Constant columns are checked on mean and sd alone (same bounds), non-finite columns on their NaNs.  A column that is
constant within every chain while the chains differ (a cluster indicator that never flips within a half) has G(0) = 0:
rhat is +inf by IEEE division and every rho(t) is exactly 1, here and on the device, since every d is exactly zero
when the chain sums are exact; the checker asserts that such a column holds integers."""
from __future__ import annotations

import math

import numpy as np

U = 2.0 ** -53
FLAG_CONSTANT, FLAG_NONFINITE, FLAG_TRUNCATED = 1, 2, 4
FIELDS = ("mean", "sd", "ess", "rhat", "mcse_mean")


def prepare(chains, burnin=0.1, split=True):
    """float64 [M][n][P] after burn-in, the cut to a common length and the split; and the rows cut per chain."""
    chains = [np.asarray(c, dtype=np.float64) for c in chains]
    kept = [c[int(burnin * c.shape[0]):] for c in chains]
    common = min(c.shape[0] for c in kept)
    cut = tuple(c.shape[0] - common for c in kept)
    kept = [c[:common] for c in kept]
    if split:
        h = common // 2
        kept = [part for c in kept for part in (c[:h], c[common - h:])]
    return np.stack(kept), cut


def _fsum_mean(v):
    return math.fsum(v.tolist()) / v.size


def column(x, max_lag=0, exact=True):
    """One column: x float64 [M][n].  A dict of the outputs, the margin and what the bounds need.  exact=False takes the
    autocovariances by direct NumPy sums (what tools/diag_speed.py times as the host's figure; not a checker)."""
    M, n = x.shape
    N = M * n
    nan = float("nan")
    if not np.isfinite(x).all():
        return dict(mean=nan, sd=nan, ess=nan, rhat=nan, mcse_mean=nan, n_lags=0, flag=FLAG_NONFINITE, margin=math.inf)
    mu = np.array([_fsum_mean(x[m]) for m in range(M)])
    mean = math.fsum(x.ravel().tolist()) / N
    dev = x.ravel() - mean
    sd = math.sqrt(math.fsum((dev * dev).tolist()) / (N - 1))
    d = x - mu[:, None]
    aux = dict(mu=mu, A=np.abs(x).mean(axis=1), Dm=np.abs(d).mean(axis=1), D=float(np.abs(d).mean()), dmax=float(np.abs(d).max()),
               devmax=float(np.abs(dev).max()), M=M, n=n)
    if x.max() - x.min() < 1e-15:
        return dict(mean=mean, sd=sd, ess=float(N), rhat=nan, mcse_mean=0.0, n_lags=0, flag=FLAG_CONSTANT, margin=math.inf, aux=aux)

    cache = {}

    def G(t):
        if t not in cache:
            terms = d[:, :n - t] * d[:, t:]
            cache[t] = (math.fsum(terms.ravel().tolist()) if exact else float(terms.sum())) / n / M
        return cache[t]

    mean_var = G(0) * n / (n - 1)
    between = float(np.var(mu, ddof=1)) if M > 1 else 0.0
    var_plus = mean_var * (n - 1) / n + between
    rhat = math.sqrt(var_plus / mean_var) if mean_var > 0 else math.inf       # (IEEE division: every chain constant, the chains differing)

    def rho(t):
        return 1.0 - (mean_var - G(t)) / var_plus

    margin, flag, qmax = math.inf, 0, 0.0
    rho_t = np.zeros(n)
    rho_t[0] = even = 1.0
    odd = rho(1)
    rho_t[1] = odd
    t = 1
    while t < n - 3:
        margin = min(margin, abs(even + odd))                              # read by `> 0` here and by `>= 0` below
        if not even + odd > 0:
            break
        if max_lag > 0 and t + 2 > max_lag:
            flag |= FLAG_TRUNCATED
            break
        even, odd = rho(t + 1), rho(t + 2)
        if even + odd >= 0:
            rho_t[t + 1], rho_t[t + 2] = even, odd
        t += 2
    max_t = t - 2
    if even > 0:
        rho_t[max_t + 1] = even
    t = 1
    replaced = []                                                          # the first entry (t + 1) of every pair the second loop replaces
    while t <= max_t - 2:
        diff = (rho_t[t + 1] + rho_t[t + 2]) - (rho_t[t - 1] + rho_t[t])
        margin = min(margin, abs(diff))
        if diff > 0:
            rho_t[t + 1] = (rho_t[t - 1] + rho_t[t]) / 2
            rho_t[t + 2] = rho_t[t + 1]
            replaced.append(t + 1)
        t += 2
    if mean_var == 0:
        # every d is exactly zero here and on the device (the chain sums of such a column must be exact: asserted), so
        # every G(t) is 0 and every rho(t) exactly 1 on both sides: no rounding that could flip a decision
        assert np.all(x == np.round(x)) and np.abs(x).sum() < 2.0 ** 53, "a column constant within every chain must hold integers"
        margin = math.inf
    tau_raw = -1.0 + 2.0 * float(np.sum(rho_t[:max_t + 1])) + rho_t[max_t + 1]
    floor = 1.0 / math.log10(N)
    tau = max(tau_raw, floor)
    ess = N / tau
    for k in cache:
        qmax = max(qmax, abs((mean_var - cache[k]) / var_plus))
    aux.update(G0=G(0), mean_var=mean_var, var_plus=var_plus, between=between, qmax=qmax, K=max_t + 2, floor=floor,
               abs_rho=float(np.abs(rho_t[:max_t + 2]).sum()), tau=tau)
    return dict(mean=mean, sd=sd, ess=ess, rhat=rhat, mcse_mean=sd / math.sqrt(ess), n_lags=max_t + 2, flag=flag, margin=margin,
                tau=tau, replaced=tuple(replaced), aux=aux)


def column_bounds(c):
    """Absolute bounds on |device - checker| for the five outputs of one column (a dict), by the derivation above."""
    if c["flag"] & FLAG_NONFINITE:
        return {k: 0.0 for k in FIELDS}
    a = c["aux"]
    M, n = a["M"], a["n"]
    N = M * n
    e0 = (n - 1) * U * a["A"] + U * np.abs(a["mu"])
    e_mu = float(np.max(U * np.abs(a["mu"]) + (n + 1) * U * (a["Dm"] + e0)))
    eps = e_mu + U * a["dmax"]
    e_mean = e_mu + (M + 1) * U * abs(c["mean"])
    e_sd = math.sqrt(N / (N - 1)) * (eps + e_mean + 2 * U * a["devmax"]) + (N / 2 + 3) * U * c["sd"]
    out = {"mean": 2 * e_mean, "sd": 2 * e_sd}
    if c["flag"] & FLAG_CONSTANT:
        out.update(ess=0.0, rhat=0.0, mcse_mean=0.0)
        return out
    G0, mv, vp, B = a["G0"], a["mean_var"], a["var_plus"], a["between"]
    e_G = (N + 2) * U * G0 + 2 * eps * a["D"] + eps * eps + 4 * U * G0
    e_mv = (e_G + 2 * U * G0) * n / (n - 1)
    e_B = 0.0
    if M > 1:
        e_B = 4 * e_mu * math.sqrt(M / (M - 1)) * math.sqrt(B) + 4 * e_mu * e_mu * M / (M - 1) + (M + 3) * U * B
    e_vp = e_mv + 2 * U * mv + e_B + U * vp
    e_rho = (e_mv + e_G) / vp + a["qmax"] * e_vp / vp + 3 * U * (1 + a["qmax"])
    K = a["K"]
    e_tau = max(2 * K * e_rho + (K + 3) * U * (1 + 2 * a["abs_rho"]), 4 * U * a["floor"])
    rel_ess = e_tau / a["tau"] + 2 * U
    out["rhat"] = 2 * c["rhat"] * ((e_vp / vp + e_mv / mv) / 2 + 2 * U) if mv > 0 else 0.0      # (+inf on both sides)
    out["ess"] = 2 * c["ess"] * rel_ess
    out["mcse_mean"] = 2 * c["mcse_mean"] * (e_sd / c["sd"] + rel_ess / 2 + 2 * U)
    out["rho"] = 2 * e_rho
    return out


def diagnose(chains, burnin=0.1, split=True, max_lag=0):
    """The outputs as arrays over the columns, with `margin`, `bound` (a dict of arrays like the outputs), `rho_bound`,
    `replaced` (per column the first entries of the pairs the monotone pass replaced), `cut`, `n_chains` and `n_draws`."""
    x, cut = prepare(chains, burnin, split)
    M, n, P = x.shape
    cols = [column(np.ascontiguousarray(x[:, :, j]), max_lag) for j in range(P)]
    bnds = [column_bounds(c) for c in cols]
    res = {k: np.array([c[k] for c in cols], dtype=np.float64) for k in FIELDS}
    res["n_lags"] = np.array([c["n_lags"] for c in cols], dtype=np.int32)
    res["flag"] = np.array([c["flag"] for c in cols], dtype=np.uint8)
    res["margin"] = np.array([c["margin"] for c in cols])
    res["bound"] = {k: np.array([b[k] for b in bnds]) for k in FIELDS}
    res["rho_bound"] = np.array([b.get("rho", 0.0) for b in bnds])
    res["replaced"] = [c.get("replaced", ()) for c in cols]
    res.update(cut=cut, n_chains=M, n_draws=n)
    return res


def fractions(got, want):
    """Per field, the largest |got - want| / bound over the columns (0 / 0 counts as 0); NaN must meet NaN."""
    out = {}
    for k in FIELDS:
        g, w, b = np.asarray(getattr(got, k)), want[k], want["bound"][k]
        assert np.array_equal(np.isnan(g), np.isnan(w)), (k, g, w)
        ok = ~np.isnan(w)
        with np.errstate(invalid="ignore"):
            err = np.where(g[ok] == w[ok], 0.0, np.abs(g[ok] - w[ok]))         # (equal infinities count as equal)
        with np.errstate(divide="ignore", invalid="ignore"):
            frac = np.where(err == 0, 0.0, err / b[ok])
        out[k] = float(frac.max(initial=0.0))
    return out


# ---- seeded test columns -----------------------------------------------------------------------------------------
def ar1(rng, phi, m, s, p=1, loc=0.0, scale=1.0):
    """m chains of s draws of p independent stationary AR(1) columns: float64 [m][s][p]."""
    e = rng.standard_normal((m, s, p))
    x = np.empty((m, s, p))
    x[:, 0] = e[:, 0]
    c = np.sqrt(1.0 - phi * phi)                                           # (phi: a number, or one value per column)
    for i in range(1, s):
        x[:, i] = phi * x[:, i - 1] + c * e[:, i]
    return loc + scale * x
