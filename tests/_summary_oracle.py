"""The posterior summary restated in fp64 NumPy: the checker of sbayes_amd.summary.

`summarize(chains, burnin, split, max_lag, probs, hdi_prob)` follows the contract step by step.  Burn-in, cut and split
are those of tests/_diag_oracle.py (`prepare`); then per column, over the N = M n draws that remain, x <- x + 0.0 (a -0
never reaches an output) and s = the ascending sort of the N values:

    flags        non-finite value: flag 2, NaN everywhere.  max - min < 1e-15: flag 1, quantiles and HDI as computed,
                 rhat_rank NaN, ess_bulk = ess_tail = N
    quantile(p)  h = (N-1) p; k = floor(h); g = h - k; s[k] + (s[min(k+1, N-1)] - s[k]) g, in that order
    HDI          inc = floor(hdi_prob N) clipped to [1, N-1]; (s[i], s[i+inc]) at the lowest i of least s[i+inc] - s[i]
    ranks        r = (lower_bound + upper_bound + 1) / 2 in s: average ranks, exact half-integers
    z(x)         ndtri((r - 0.375) / (N + 0.25))
    derived      zb = z(x); zf = z(|x - quantile(0.5)|) (its own sort); i05 = [x <= quantile(0.05)], i95 = [x <= quantile(0.95)]
    flat         a column constant within every chain (the chains differing) has W = 0: R-hat is +inf and every rho(t) is 1
                 whatever the chains' values are.  There zb and zf hold 2 r instead of z: integers whose chain sums are exact,
                 so both sides see W = 0 exactly (a z would leave W to the rounding of a chain's mean)
    outputs      every derived column through `_diag_oracle.column` (its rule for a constant column included):
                 ess_bulk = ess(zb); ess_tail = min(ess(i05), ess(i95)); rhat_rank = the larger of rhat(zb) and rhat(zf),
                 a NaN side ignored; flag ORs FLAG_TRUNCATED over the five passes
    mean, sd, ess, rhat, mcse_mean, n_lags: those of `_diag_oracle.column` on x

Quantiles, HDI, ranks and the indicators are exact selections and one fixed expression: the device gives the same bits.
ess_tail comes from exact 0/1 columns, so `_diag_oracle.column_bounds` applies to it unchanged.  ess_bulk and rhat_rank
come from PERTURBED inputs: the device's ndtri is within C_NDTRI u max(1, |z|) of the exact z (DESIGN.md section 18 counts
its roundings) and this checker's (scipy.special.ndtri) within 8 u max(1, |z|) (asserted against mpmath in
tests/test_summary_oracle_cpu.py), so the two sides' derived columns differ by at most

    delta = (C_NDTRI + 8) u max(1, max|z|)

per value.  `bounds_with_input_error(c, delta)` is the derivation of `_diag_oracle.column_bounds` with a chain mean off by
delta more (e_mu + delta) and a centred value off by 2 delta more (eps + 2 delta); at delta = 0 it is `column_bounds`."""
from __future__ import annotations

import math

import numpy as np
from scipy.special import ndtri

from tests import _diag_oracle as orc

U = orc.U
C_NDTRI = 40                                  # |z_dev - z| <= C_NDTRI u max(1, |z|): DESIGN.md section 18
C_CHECKER = 8                                 # |scipy ndtri - z| <= C_CHECKER u max(1, |z|): asserted on the CPU
FLAG_CONSTANT, FLAG_NONFINITE, FLAG_TRUNCATED = orc.FLAG_CONSTANT, orc.FLAG_NONFINITE, orc.FLAG_TRUNCATED
DERIVED = ("zb", "zf", "i05", "i95")
DEFAULT_PROBS = (0.05, 0.5, 0.95)


def quantile(s, p):
    """The contract's quantile of the ascending s at probability p."""
    N = s.size
    h = (N - 1) * float(p)
    k = math.floor(h)
    g = h - k
    lo, hi = float(s[k]), float(s[min(k + 1, N - 1)])
    with np.errstate(all="ignore"):
        return float(np.float64(lo) + np.float64(hi - lo) * np.float64(g))


def hdi_span(hdi_prob, N):
    return int(min(max(math.floor(float(hdi_prob) * N), 1), N - 1))


def hdi(s, hdi_prob):
    inc = hdi_span(hdi_prob, s.size)
    width = s[inc:] - s[:s.size - inc]
    i = int(np.argmin(width))                                              # (the first of equal widths)
    return float(s[i]), float(s[i + inc])


def ranks(v):
    """Average ranks of the values of v (any shape) among themselves: exact half-integers."""
    s = np.sort(v.ravel())
    return (np.searchsorted(s, v, side="left") + np.searchsorted(s, v, side="right") + 1) / 2.0


def rank_probability(r, N):
    return (r - 0.375) / (N + 0.25)


def z_of(v, flat=False):
    """z of the average ranks of v; for a column constant within every chain (flat) twice the average ranks instead."""
    return 2.0 * ranks(v) if flat else ndtri(rank_probability(ranks(v), v.size))


def derive(x):
    """x float64 [M][n], finite -> dict of the four derived columns [M][n], the ranks and the three quantiles they use."""
    x = x + 0.0
    s = np.sort(x.ravel())
    q05, q50, q95 = quantile(s, 0.05), quantile(s, 0.5), quantile(s, 0.95)
    flat = bool(np.all(x == x[:, :1]))
    return dict(flat=flat, zb=z_of(x, flat), zf=z_of(np.abs(x - q50), flat), i05=(x <= q05).astype(np.float64), i95=(x <= q95).astype(np.float64),
                rank=ranks(x), q05=q05, q50=q50, q95=q95)


def delta_of(z):
    return (C_NDTRI + C_CHECKER) * U * max(1.0, float(np.abs(z).max()))


def bounds_with_input_error(c, delta):
    """`_diag_oracle.column_bounds` for a column whose every value the device holds within delta of the checker's."""
    if c["flag"] & FLAG_NONFINITE:
        return {k: 0.0 for k in orc.FIELDS}
    a = c["aux"]
    M, n = a["M"], a["n"]
    N = M * n
    e0 = (n - 1) * U * a["A"] + U * np.abs(a["mu"])
    e_mu = float(np.max(U * np.abs(a["mu"]) + (n + 1) * U * (a["Dm"] + e0))) + delta
    eps = e_mu + U * a["dmax"] + delta                                     # (the checker's eps + 2 delta)
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
    out["rhat"] = 2 * c["rhat"] * ((e_vp / vp + e_mv / mv) / 2 + 2 * U) if mv > 0 else 0.0
    out["ess"] = 2 * c["ess"] * rel_ess
    out["mcse_mean"] = 2 * c["mcse_mean"] * (e_sd / c["sd"] + rel_ess / 2 + 2 * U)
    out["rho"] = 2 * e_rho
    return out


def _nanmax(a, b):
    return b if math.isnan(a) else (a if math.isnan(b) else max(a, b))


def column(x, max_lag=0, probs=DEFAULT_PROBS, hdi_prob=0.94, exact=True):
    """One column: x float64 [M][n].  A dict of the outputs, with per derived column its checker result, its bound and its
    margin (`parts`).  exact=False takes the autocovariances by direct NumPy sums (what tools/summary_speed.py times as the
    host's figure; not a checker)."""
    N = x.size
    nan = float("nan")
    base = orc.column(x, max_lag, exact)
    out = {k: base[k] for k in orc.FIELDS + ("n_lags", "flag", "margin")}
    out["base"] = base
    if base["flag"] & FLAG_NONFINITE:
        out.update(quantiles=[nan] * len(probs), hdi_lo=nan, hdi_hi=nan, ess_bulk=nan, ess_tail=nan, rhat_rank=nan, parts={},
                   bound=dict(ess_bulk=0.0, ess_tail=0.0, rhat_rank=0.0))
        return out
    xs = x + 0.0
    s = np.sort(xs.ravel())
    out["quantiles"] = [quantile(s, p) for p in probs]
    out["hdi_lo"], out["hdi_hi"] = hdi(s, hdi_prob)
    if base["flag"] & FLAG_CONSTANT:
        out.update(ess_bulk=float(N), ess_tail=float(N), rhat_rank=nan, parts={}, bound=dict(ess_bulk=0.0, ess_tail=0.0, rhat_rank=0.0))
        return out
    d = derive(x)
    parts = {}
    for name in DERIVED:
        c = orc.column(np.ascontiguousarray(d[name]), max_lag, exact)
        delta = delta_of(d[name]) if name in ("zb", "zf") and not d["flat"] else 0.0
        b = bounds_with_input_error(c, delta)
        parts[name] = dict(col=c, bound=b, margin=c["margin"], rho_bound=b.get("rho", 0.0), delta=delta)
        out["flag"] |= c["flag"] & FLAG_TRUNCATED
    out["parts"] = parts
    out["derived"] = d
    out["ess_bulk"] = parts["zb"]["col"]["ess"]
    e05, e95 = parts["i05"]["col"]["ess"], parts["i95"]["col"]["ess"]
    out["ess_tail"] = min(e05, e95)
    rb, rf = parts["zb"]["col"]["rhat"], parts["zf"]["col"]["rhat"]
    out["rhat_rank"] = _nanmax(rb, rf)
    # a min or max of two values, each within its bound of the device's, is within the larger bound of the device's
    out["bound"] = dict(ess_bulk=parts["zb"]["bound"]["ess"],
                        ess_tail=max(parts["i05"]["bound"]["ess"], parts["i95"]["bound"]["ess"]),
                        rhat_rank=max(parts["zb"]["bound"]["rhat"], parts["zf"]["bound"]["rhat"]))
    return out


BIT_EQUAL = ("quantiles", "hdi_lo", "hdi_hi")
BOUNDED = ("ess_bulk", "ess_tail", "rhat_rank")


def summarize(chains, burnin=0.1, split=True, max_lag=0, probs=DEFAULT_PROBS, hdi_prob=0.94, exact=True):
    """The outputs as arrays over the columns, with `margin` (the least over the column's five passes), `margin_ok` (every
    pass's margin >= 1e-9 and above twice its rho bound), `bound`, `cut`, `n_chains`, `n_draws` and `columns` (the dicts)."""
    x, cut = orc.prepare(chains, burnin, split)
    M, n, P = x.shape
    cols = [column(np.ascontiguousarray(x[:, :, j]), max_lag, probs, hdi_prob, exact) for j in range(P)]
    res = {k: np.array([c[k] for c in cols], dtype=np.float64) for k in orc.FIELDS + ("hdi_lo", "hdi_hi") + BOUNDED}
    res["quantiles"] = np.array([c["quantiles"] for c in cols], dtype=np.float64).reshape(P, len(probs)).T.copy()
    res["n_lags"] = np.array([c["n_lags"] for c in cols], dtype=np.int32)
    res["flag"] = np.array([c["flag"] for c in cols], dtype=np.uint8)
    res["bound"] = {k: np.array([c["bound"][k] for c in cols]) for k in BOUNDED}
    margins = [[c["margin"]] + [p["margin"] for p in c["parts"].values()] for c in cols]
    res["margin"] = np.array([min(m) for m in margins])
    res["margin_ok"] = np.array([all(p["margin"] >= 1e-9 and p["margin"] > 2 * p["rho_bound"] for p in c["parts"].values()) for c in cols])
    res.update(cut=cut, n_chains=M, n_draws=n, columns=cols)
    return res


def fractions(got, want):
    """Per bounded field, the largest |got - want| / bound over the columns (0 / 0 counts as 0); NaN must meet NaN."""
    out = {}
    for k in BOUNDED:
        g, w, b = np.asarray(getattr(got, k)), want[k], want["bound"][k]
        assert np.array_equal(np.isnan(g), np.isnan(w)), (k, g, w)
        ok = ~np.isnan(w)
        with np.errstate(invalid="ignore"):
            err = np.where(g[ok] == w[ok], 0.0, np.abs(g[ok] - w[ok]))
        with np.errstate(divide="ignore", invalid="ignore"):
            frac = np.where(err == 0, 0.0, err / b[ok])
        out[k] = float(frac.max(initial=0.0))
    return out
