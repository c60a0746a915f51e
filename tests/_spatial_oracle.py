"""The contract of the spatial posterior predictive check (include/sbe_spatial.h) restated in NumPy: the checker of
tests/test_gpu_spatial.py, itself checked against a literal triple loop and closed forms in tests/test_spatial_oracle_cpu.py.
A plain helper module: it holds no test.

Every quantity is an integer, so the device's result must EQUAL this one: no tolerance, no measured bound.

  data        x uint8 [N, F], 255 = not observed; n_states int32 [F], each in [1, 32]
  classes     band uint8 [N, N], entry (i, j) a class b < B or 255 (pair not counted), symmetric, the diagonal ignored
  one data set y:
      agree[b, f]            = #{i < j : band[i, j] = b, y[i, f] and y[j, f] are codes, y[i, f] = y[j, f]}
      comparable[b, f]       = the same without the equality
      local_agree[b, i]      = sum over f of #{j != i : band[i, j] = b, both are codes, y[i, f] = y[j, f]}
      local_comparable[b, i] = the same without the equality
      total[b]               = sum over f of agree[b, f]
  replicates  y uint8 [T, N, F]; per replicate and entry of agree, local_agree and total exactly one of n_greater, n_equal,
              n_less grows by comparing with the observed value; sum += v, sumsq += v * v for agree and local_agree."""
from __future__ import annotations

import numpy as np

NA = 255
MAX_OBJECTS, MAX_FEATURES, MAX_STATES, MAX_BANDS = 4096, 4096, 32, 8
INT64_MAX, INT32_MAX = 2 ** 63 - 1, 2 ** 31 - 1
STATS = ("agree", "comparable", "local_agree", "local_comparable", "total")
ACCUMULATORS = tuple(f"{k}_{c}" for k in "fi" for c in ("greater", "equal", "less", "sum", "sumsq")) + ("t_greater", "t_equal", "t_less")


def max_replicates(n_objects, n_features):
    """The replicates below which no int64 sum of squares (and no int32 count) can overflow: agree <= N (N - 1) / 2 and
    local_agree <= (N - 1) F in one replicate."""
    n, f = int(n_objects), int(n_features)
    if not (1 <= n <= MAX_OBJECTS and 1 <= f <= MAX_FEATURES):
        return 0
    most = max(n * (n - 1) // 2, (n - 1) * f)
    return INT32_MAX if most == 0 else min(INT32_MAX, INT64_MAX // (most * most))


def check_band(band, n_bands):
    """None, or the message of the first offence in the order of the contract: the first entry off the diagonal that is neither
    below B nor 255, else the first (i, j) that differs from (j, i)."""
    band = np.asarray(band)
    n = band.shape[0]
    off = ~np.eye(n, dtype=bool)
    bad = off & (band != NA) & (band >= n_bands)
    if bad.any():
        i, j = np.argwhere(bad)[0]
        return f"band[{i}][{j}]={int(band[i, j])} is neither below n_bands={n_bands} nor 255"
    bad = off & (band != band.T)
    if bad.any():
        i, j = np.argwhere(bad)[0]
        return f"band[{i}][{j}]={int(band[i, j])} differs from band[{j}][{i}]={int(band[j, i])}"
    return None


def statistics(y, band, n_bands):
    """The five arrays of one data set y [N, F] (int64 each), every pair compared cell by cell."""
    y, band = np.asarray(y), np.asarray(band)
    n, f_n = y.shape
    member = [(band == b) & ~np.eye(n, dtype=bool) for b in range(n_bands)]
    out = dict(agree=np.zeros((n_bands, f_n), dtype=np.int64), comparable=np.zeros((n_bands, f_n), dtype=np.int64),
               local_agree=np.zeros((n_bands, n), dtype=np.int64), local_comparable=np.zeros((n_bands, n), dtype=np.int64))
    for f in range(f_n):
        c = y[:, f]
        seen = c != NA
        both = seen[:, None] & seen[None, :]
        same = both & (c[:, None] == c[None, :])
        for b in range(n_bands):
            a, q = same & member[b], both & member[b]
            twice_a, twice_q = int(a.sum()), int(q.sum())
            assert twice_a % 2 == 0 and twice_q % 2 == 0           # (every pair from both ends)
            out["agree"][b, f], out["comparable"][b, f] = twice_a // 2, twice_q // 2
            out["local_agree"][b] += a.sum(axis=1)
            out["local_comparable"][b] += q.sum(axis=1)
    out["total"] = out["agree"].sum(axis=1)
    assert np.array_equal(out["local_agree"].sum(axis=1), 2 * out["total"])
    return out


def accumulate(obs, reps):
    """The accumulators after the replicates' statistics `reps` (a list of statistics() results) against the observed `obs`."""
    acc = {}
    for key, stat in (("f", "agree"), ("i", "local_agree"), ("t", "total")):
        shape = obs[stat].shape
        v = np.array([r[stat] for r in reps], dtype=np.int64).reshape((len(reps),) + shape)
        acc[f"{key}_greater"] = (v > obs[stat]).sum(axis=0).astype(np.int32)
        acc[f"{key}_equal"] = (v == obs[stat]).sum(axis=0).astype(np.int32)
        acc[f"{key}_less"] = (v < obs[stat]).sum(axis=0).astype(np.int32)
        if key != "t":
            acc[f"{key}_sum"] = v.sum(axis=0)
            acc[f"{key}_sumsq"] = (v * v).sum(axis=0)
    return acc


def check(x, n_states, band, n_bands, y):
    """Everything the unit returns for data x, classes band and replicates y [T, N, F]: `<stat>_obs` and `<stat>_rep` [T, ...] of
    the five arrays, the accumulators (ACCUMULATORS) and n_replicates."""
    x, y, ns = np.asarray(x), np.asarray(y), np.asarray(n_states)
    assert x.dtype == np.uint8 and y.dtype == np.uint8 and y.shape[1:] == x.shape and 1 <= n_bands <= MAX_BANDS
    assert ((ns >= 1) & (ns <= MAX_STATES)).all() and check_band(band, n_bands) is None
    for a in (x, y):
        assert ((a == NA) | (a < ns)).all()
    assert y.shape[0] <= max_replicates(*x.shape)
    obs = statistics(x, band, n_bands)
    reps = [statistics(y[t], band, n_bands) for t in range(y.shape[0])]
    out = {f"{k}_obs": v for k, v in obs.items()}
    for k in STATS:
        out[f"{k}_rep"] = np.array([r[k] for r in reps], dtype=np.int64).reshape((len(reps),) + obs[k].shape)
    out.update(accumulate(obs, reps))
    out["n_replicates"] = y.shape[0]
    return out
