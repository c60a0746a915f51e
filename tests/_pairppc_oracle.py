"""NumPy fp64 restatement of the pairwise posterior predictive check (include/sbe_pairppc.h, sbayes_amd/pairppc.py).  A plain
helper module: it holds no test.

Contract:

* data `x` uint8 [N, F], 255 = not observed, `n_states` int32 [F]; the observed statistic, dof, n and valid of every pair are
  tests/_assoc_oracle.py's (feature_association): counts from X^T X, dof from the occupied rows and columns, Pearson terms in
  fp64 with Yates' correction at dof 1, summed a major, b minor;
* replicates `y` uint8 [T, N, F], each code below n_states[f] or 255.  For every replicate t in order and every pair i < j that
  is valid on the data: s = the statistic of the replicate's table by the same arithmetic; a table with dof 0 has s = 0 and
  n_degenerate += 1; exactly one of n_greater, n_equal, n_less += 1 by comparing s and stat_obs; sum += s; sumsq += s * s
  (the product rounded, then added);
* pairs that are not valid on the data, and the diagonal, stay at 0; every [F, F] output is mirrored; stat_rep [T, F, F] holds
  the s values (0 where nothing is accumulated).

Bounds the tests use: a device statistic lies within bound = ao.statistic_bound(R, C) (relative) of the oracle's, R and C the
occupied rows and columns of that replicate's table.  A count of the device may differ from the oracle's, per pair, by at most
the number of replicates whose oracle value satisfies |s - stat_obs| <= bound * max(s, stat_obs), with that same bound
(`near`)."""
from __future__ import annotations

import numpy as np

from tests import _assoc_oracle as ao

NA = ao.NA
INT_FIELDS = ("n_greater", "n_equal", "n_less", "n_degenerate")


def accumulate(stat_obs, valid_obs, stat_rep, dof_rep=None):
    """The counts and sums of the contract's loop from per-replicate statistics [T, F, F], added one by one in replicate order.
    dof_rep [T, F, F]: the replicates' dof (None: no n_degenerate).  Works on the upper triangle and mirrors."""
    f = stat_obs.shape[0]
    live = np.triu(np.asarray(valid_obs, dtype=bool), 1)
    out = {k: np.zeros((f, f), dtype=np.int32) for k in INT_FIELDS}
    total, sq = np.zeros((f, f)), np.zeros((f, f))
    for t in range(stat_rep.shape[0]):
        s = np.where(live, stat_rep[t], 0.0)
        out["n_greater"] += live & (s > stat_obs)
        out["n_equal"] += live & (s == stat_obs)
        out["n_less"] += live & (s < stat_obs)
        if dof_rep is not None:
            out["n_degenerate"] += live & (dof_rep[t] == 0)
        total = total + s
        sq = sq + s * s
    out["sum"], out["sumsq"] = total, sq
    return {k: v + v.T for k, v in out.items()}


def check(x, n_states, y):
    """dict: stat_obs, dof_obs, n_obs, valid_obs, R_obs, C_obs; stat_rep, dof_rep, R_rep, C_rep [T, F, F]; the four counts, sum,
    sumsq [F, F]; n_replicates."""
    x, y = np.asarray(x, dtype=np.uint8), np.asarray(y, dtype=np.uint8)
    obs = ao.feature_association(x, n_states)
    valid = obs["valid"]
    t_n, f = y.shape[0], x.shape[1]
    stat_rep = np.zeros((t_n, f, f))
    dof_rep = np.zeros((t_n, f, f), dtype=np.int32)
    r_rep = np.zeros((t_n, f, f), dtype=np.int32)
    c_rep = np.zeros((t_n, f, f), dtype=np.int32)
    for t in range(t_n):
        rep = ao.feature_association(y[t], n_states)
        stat_rep[t] = np.where(valid, rep["statistic"], 0.0)           # (a replicate's dof 0 table holds statistic 0 already)
        dof_rep[t], r_rep[t], c_rep[t] = rep["dof"], rep["R"], rep["C"]
    out = accumulate(obs["statistic"], valid, stat_rep, dof_rep)
    out.update(stat_obs=obs["statistic"], dof_obs=obs["dof"], n_obs=obs["n"], valid_obs=valid, R_obs=obs["R"], C_obs=obs["C"],
               stat_rep=stat_rep, dof_rep=dof_rep, R_rep=r_rep, C_rep=c_rep, n_replicates=t_n)
    return out


def near(want):
    """int [F, F]: per pair the replicates whose oracle statistic lies within its bound of stat_obs (module docstring)."""
    bound = ao.statistic_bound(want["R_rep"], want["C_rep"])
    s, o = want["stat_rep"], want["stat_obs"][None]
    close = want["valid_obs"][None] & (np.abs(s - o) <= bound * np.maximum(s, o))
    return close.sum(axis=0)


def p_value(res):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(res["valid_obs"], (res["n_greater"] + 0.5 * res["n_equal"]) / res["n_replicates"], np.nan)
