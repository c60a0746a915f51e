"""NumPy restatement of the deterministic part of sBayes' GibbsSampleWeights._propose (sbayes/sampling/operators.py:597-676):
the checker of sbayes_amd.wgibbs and of the kernels of csrc/sbe_wgibbs.hip.  tests/golden/wgibbs.npz holds what the
reference itself computed.

State of a sample, as the engine slot holds it:
  w          float32 [F, C]   raw weights
  patterns   bool [P, C]      distinct rows of has_components (np.unique(axis=0) order), pid int [N] the row of every object
  src        int [N, F]       source component of every observation, -1 where none is set
  na         bool [N, F]      missing observations
The draws of a proposal: i1, i2 (two components), a2 float64 [F] (the beta draw), u float32 [F] (the uniforms).

Numerical contract:

* `pair_counts`: per feature, the objects whose pattern has both components and whose source is i1 (column 0) / i2 (column
  1): np.sum(source[has_both], axis=0)[:, [i1, i2]] of the reference.  NA observations count for neither.  Exact.
* `propose_weights`: float32, bit for bit the reference's w_new: w02 = w[:, i1] + w[:, i2] (float32);
  w_new[:, i1] = float32((1 - a2) * w02), w_new[:, i2] = float32(a2 * w02) (float64 products, rounded once); every row
  divided by its float32 sum in NumPy's order for a contiguous axis of C <= 8 terms; a2_old = w[:, i2] / w02 (float32).
* `log_ratio`: float64 per feature, no lgamma anywhere -- ln B(alpha) of the Dirichlet density and betaln of the beta
  density are the same on both sides of the Metropolis ratio:
    d_lh    = sum over the non-NA observations n of log wn_new[pid(n), f, src(n, f)] - log wn_old[pid(n), f, src(n, f)]
              with wn_* the float32 per-pattern normalised weights (`normalized_weights`: normalize_weights of the
              reference, likelihood.py:171-190); an observation without a source component contributes log 0 on both sides
    d_prior = sum_c (alpha - 1) (log w_new - log w); a term with alpha == 1 is 0 whatever w is (SciPy's xlogy)
    d_q     = (A - 1) (log a2_old - log a2) + (B - 1) (log1p(-a2_old) - log1p(-a2)); a term whose coefficient is 0 is 0
    log_p   = (d_lh + d_prior + d_q) / T
  accept = float64(u) < exp(log_p): a NaN rejects, as `u < nan` does in the reference; the result is where(accept, w_new, w).
  Beside log_p the function returns S, the sum of |coefficient * log| over every term, and the number of terms: the
  error band of an any-order float64 evaluation is eps = 2^-50 (n_terms + 4) S / T (`device_band`).
* Against the reference (`reference_bound`): the reference adds N float32 logs per feature in float32, twice:
  |log p_ref - log p| <= (N + 1) 2^-24 S_lh / T + 1e-12 with S_lh the sum of |log| over both likelihood sums."""
from __future__ import annotations

import numpy as np


def state_of(has_components, source, na):
    """(patterns, pid, src) from the reference's arrays: has_components bool [N, C], source bool [N, F, C]."""
    patterns, pid = np.unique(np.asarray(has_components, dtype=bool), axis=0, return_inverse=True)
    source = np.asarray(source, dtype=bool)
    src = np.where(source.any(axis=-1), source.argmax(axis=-1), -1).astype(np.int16)
    src[np.asarray(na, dtype=bool)] = -1
    return patterns, np.asarray(pid).reshape(-1).astype(np.int64), src


def normalized_weights(w, patterns):
    """float32 [P, F, C]: the reference's normalize_weights per distinct pattern."""
    wp = np.asarray(patterns, dtype=bool)[:, None, :] * np.asarray(w, dtype=np.float32)[None, :, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        wp /= np.sum(wp, axis=-1, keepdims=True)
    return wp


def pair_counts(patterns, pid, src, na, i1, i2):
    """int64 [F, 2]."""
    patterns = np.asarray(patterns, dtype=bool)
    has_both = (patterns[:, i1] & patterns[:, i2])[np.asarray(pid)]
    sel = has_both[:, None] & ~np.asarray(na, dtype=bool)
    src = np.asarray(src)
    return np.stack([(sel & (src == i1)).sum(axis=0), (sel & (src == i2)).sum(axis=0)], axis=1).astype(np.int64)


def beta_parameters(counts, concentration_array, i1, i2, prior_temperature):
    """float64 [F, 2]: (A, B) = (1 + c2, 1 + c1), c = (counts + concentration_array[:, [i1, i2]]) / T."""
    c = (np.asarray(counts) + np.asarray(concentration_array)[:, [i1, i2]]) / prior_temperature
    return np.stack([1 + c[:, 1], 1 + c[:, 0]], axis=1).astype(np.float64)


def propose_weights(w, i1, i2, a2):
    """(w_new float32 [F, C], a2_old float32 [F])."""
    w = np.asarray(w, dtype=np.float32)
    a2 = np.asarray(a2, dtype=np.float64)
    w02 = w[:, i1] + w[:, i2]
    w_new = w.copy()
    w_new[:, i1] = (1 - a2) * w02
    w_new[:, i2] = a2 * w02
    with np.errstate(invalid="ignore", divide="ignore"):
        w_new = (w_new / np.sum(w_new, axis=-1, keepdims=True)).astype(np.float32)
        a2_old = w[:, i2] / w02
    return w_new, a2_old


def _coef_log(coef, value):
    """coef * value with the xlogy convention: 0 where coef == 0, whatever value is."""
    with np.errstate(invalid="ignore"):
        return np.where(coef == 0, 0.0, coef * value)


def log_ratio(w, w_new, a2_old, patterns, pid, src, na, a2, alpha, beta_ab, prior_temperature):
    """dict of float64 [F] arrays: d_lh, d_prior, d_q, log_p, S (sum of |coefficient * log|), S_lh, n_terms."""
    w = np.asarray(w, dtype=np.float32)
    w_new = np.asarray(w_new, dtype=np.float32)
    F, C = w.shape
    pid, src, na = np.asarray(pid), np.asarray(src), np.asarray(na, dtype=bool)
    a2 = np.asarray(a2, dtype=np.float64)
    a2o = np.asarray(a2_old, dtype=np.float32).astype(np.float64)
    alpha = np.asarray(alpha, dtype=np.float64)
    ab = np.asarray(beta_ab, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        lo_t = np.log(normalized_weights(w, patterns).astype(np.float64))          # [P, F, C]
        ln_t = np.log(normalized_weights(w_new, patterns).astype(np.float64))
        f_idx = np.arange(F)[None, :]
        s = np.where(src >= 0, src, 0)
        lo = np.where(src >= 0, lo_t[pid[:, None], f_idx, s], -np.inf)
        ln = np.where(src >= 0, ln_t[pid[:, None], f_idx, s], -np.inf)
        d_lh = np.where(na, 0.0, ln - lo).sum(axis=0)
        s_lh = np.where(na, 0.0, np.abs(ln) + np.abs(lo)).sum(axis=0)
        lw, lwn = np.log(w.astype(np.float64)), np.log(w_new.astype(np.float64))
        d_prior = _coef_log(alpha - 1, lwn - lw).sum(axis=1)
        s_prior = (_coef_log(np.abs(alpha - 1), np.abs(lwn)) + _coef_log(np.abs(alpha - 1), np.abs(lw))).sum(axis=1)
        ca, cb = ab[:, 0] - 1, ab[:, 1] - 1
        la, lao, lb, lbo = np.log(a2), np.log(a2o), np.log1p(-a2), np.log1p(-a2o)
        d_q = _coef_log(ca, lao - la) + _coef_log(cb, lbo - lb)
        s_q = (_coef_log(np.abs(ca), np.abs(lao)) + _coef_log(np.abs(ca), np.abs(la))
               + _coef_log(np.abs(cb), np.abs(lbo)) + _coef_log(np.abs(cb), np.abs(lb)))
        log_p = (d_lh + d_prior + d_q) / prior_temperature
    n_terms = 2 * (~na).sum(axis=0) + 2 * C + 4
    return dict(d_lh=d_lh, d_prior=d_prior, d_q=d_q, log_p=log_p, S=s_lh + s_prior + s_q, S_lh=s_lh,
                n_terms=n_terms.astype(np.int64))


def decide(u, log_p):
    """bool [F]: float64(u) < exp(log_p); NaN rejects."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(u, dtype=np.float32).astype(np.float64) < np.exp(np.asarray(log_p, dtype=np.float64))


def device_band(terms, prior_temperature):
    """float64 [F]: any-order float64 summation of n_terms terms plus a few ulp per log / log1p, a factor of about 4 to
    spare.  Infinite or NaN where S is: such a feature's log_p is infinite or NaN on both sides."""
    return 2.0 ** -50 * (terms["n_terms"] + 4) * terms["S"] / prior_temperature


def reference_bound(terms, n_objects, prior_temperature):
    """float64 [F]: the worst case of the reference's two serial float32 sums of float32 logs."""
    return (n_objects + 1) * 2.0 ** -24 * terms["S_lh"] / prior_temperature + 1e-12


def log_margin(u, log_p):
    """|log u - log p| per feature (inf for u == 0 or an infinite log_p): how far a decision is from flipping."""
    with np.errstate(divide="ignore", invalid="ignore"):
        m = np.abs(np.log(np.asarray(u, dtype=np.float32).astype(np.float64)) - np.asarray(log_p, dtype=np.float64))
    return np.where(np.isnan(m), np.inf, m)


def step(w, patterns, pid, src, na, i1, i2, a2, u, alpha, beta_ab, prior_temperature):
    """The whole deterministic step: (weights_out float32 [F, C], accept bool [F], terms dict, w_new)."""
    w = np.asarray(w, dtype=np.float32)
    w_new, a2_old = propose_weights(w, i1, i2, a2)
    terms = log_ratio(w, w_new, a2_old, patterns, pid, src, na, a2, alpha, beta_ab, prior_temperature)
    accept = decide(u, terms["log_p"])
    return np.where(accept[:, None], w_new, w), accept, terms, w_new
