"""The checker of sbayes_amd.align: the contract of include/sbe_align.h restated in NumPy, in exact integers.

Assignment rule: for an integer agreement matrix d[K][K] the permutation p maximises sum_i d[i][p[i]]; among the
maximisers it is the one whose sequence (p[0], ..., p[K-1]) is lexicographically smallest.  The solver here is brute
force over the K! permutations in lexicographic order (itertools.permutations yields them so), keeping the first that
attains the maximum; it uses no SciPy.  Wherever the optimum is unique it equals the reference's
scipy.optimize.linear_sum_assignment(d, maximize=True)[1]; count_optimal() says where that is."""
from __future__ import annotations

from functools import lru_cache
from itertools import permutations

import numpy as np


@lru_cache(maxsize=None)
def _all_perms(k):
    return np.array(list(permutations(range(k))), dtype=np.intp)            # lexicographic order


def _values(d):
    d = np.asarray(d)
    assert d.ndim == 2 and d.shape[0] == d.shape[1] and d.dtype.kind in "iu", (d.shape, d.dtype)
    k = d.shape[0]
    perms = _all_perms(k)
    return perms, d.astype(np.int64)[np.arange(k)[None, :], perms].sum(axis=1)


def best_permutation(d):
    """The rule's permutation of an integer matrix d [K][K]: int64 [K]."""
    perms, values = _values(d)
    return perms[int(np.argmax(values))].astype(np.int64)                   # (argmax: the first maximum, lexicographic order)


def best_value(d) -> int:
    return int(_values(d)[1].max())


def count_optimal(d) -> int:
    """How many permutations attain the maximum of d."""
    values = _values(d)[1]
    return int(np.count_nonzero(values == values.max()))


def agreement(a, b):
    """d[i][j] = sum_n a[i][n] b[j][n], int64."""
    return np.asarray(a, dtype=np.int64) @ np.asarray(b, dtype=np.int64).T


def within(clusters, seed_rows=0, with_d=False):
    """The permutations P_s of one run, int64 [S, K].  clusters: 0/1 [S, K, N].  with_d: also the matrices d [S, K, K]."""
    c = np.asarray(clusters).astype(np.int64)
    s_n, k, _n = c.shape
    m = min(int(seed_rows), s_n)
    w = max(m, 1)
    total = c[:m].sum(axis=0)
    perms = np.zeros((s_n, k), dtype=np.int64)
    ds = np.zeros((s_n, k, k), dtype=np.int64)
    for s in range(s_n):
        d = total @ c[s].T
        p = best_permutation(d)
        total += w * c[s][p]
        perms[s], ds[s] = p, d
    return (perms, ds) if with_d else perms


def counts(clusters, perms=None, burn=0):
    """cnt[i][n] = sum over s >= burn of c[s][P_s[i]][n], int64 [K, N]; perms None: as logged."""
    c = np.asarray(clusters).astype(np.int64)
    if perms is not None:
        c = np.take_along_axis(c, np.asarray(perms, dtype=np.intp)[:, :, None], axis=1)
    return c[int(burn):].sum(axis=0)


def across(count_list, pivot=0):
    """(Q int64 [R, K], d int64 [R, K, K]) for the runs' counts against the pivot's."""
    ds = np.stack([agreement(count_list[pivot], cb) for cb in count_list])
    return np.stack([best_permutation(d) for d in ds]), ds


def align_runs(runs, pivot=0, within_seed=None, burnin=0.0):
    """What sbayes_amd.align.align_runs returns, as a dict: perms, run_perms, total_perms, counts, agreement."""
    perms = [np.tile(np.arange(r.shape[1]), (r.shape[0], 1)) if within_seed is None else within(r, within_seed) for r in runs]
    burn = [int(float(burnin) * r.shape[0]) for r in runs]
    cnt = [counts(r, None if within_seed is None else p, b) for r, p, b in zip(runs, perms, burn)]
    q, ds = across(cnt, pivot)
    return {"perms": perms, "run_perms": q, "total_perms": [p[:, qq] for p, qq in zip(perms, q)],
            "counts": np.stack([cb[qq] for cb, qq in zip(cnt, q)]), "agreement": ds, "burn_rows": burn}
