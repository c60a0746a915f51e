"""The contract of the object-pair posterior predictive check (include/sbe_objpair.h) restated in NumPy: the checker of
tests/test_gpu_objpair.py, itself checked against literal loops and against tests/_spatial_oracle.py in
tests/test_objpair_oracle_cpu.py.  A plain helper module: it holds no test.

Every quantity is an integer, so the device's result must EQUAL this one: no tolerance, no measured bound.

  data        x uint8 [N, F], 255 = not observed; n_states int32 [F], each in [1, 32]
  one data set y, for i != j (the diagonal is 0 everywhere):
      agree[i, j]      = #{f : y[i, f] and y[j, f] are codes, y[i, f] = y[j, f]}
      comparable[i, j] = the same without the equality
  replicates  y uint8 [T, N, F]; per replicate and pair exactly one of n_greater, n_equal, n_less grows by comparing the
              replicate's agree with agree_obs; sum += v, sumsq += v * v.

The checker compares the cells feature by feature.  It shares nothing with the device's way of counting (a product of one-hot
rows); elements() restates only the sizes of that product, for the tests of the cases and of replicate_bytes."""
from __future__ import annotations

import numpy as np

NA = 255
MAX_OBJECTS, MAX_FEATURES, MAX_STATES = 4096, 4096, 32
INT32_MAX = 2 ** 31 - 1
ROUND, TILE = 256, 32                     # the contraction axis in whole rounds, the objects in whole tiles
MAX_STAGE_BYTES = 256 << 20
ACCUMULATORS = ("n_greater", "n_equal", "n_less", "sum", "sumsq")


def max_replicates(n_objects, n_features):
    """The replicates a handle accumulates: the int32 counts bind (sumsq <= n 2^24 is far from 2^63); 0 beyond the limits."""
    n, f = int(n_objects), int(n_features)
    return INT32_MAX if 1 <= n <= MAX_OBJECTS and 1 <= f <= MAX_FEATURES else 0


def elements(n_states):
    """(E, E_pad): the one-hot elements of a row, and E in whole rounds."""
    e = int(np.asarray(n_states, dtype=np.int64).sum())
    return e, -(-e // ROUND) * ROUND


def replicate_bytes(n_objects, n_features, n_elements, with_agree_rep=False):
    """Device bytes of one replicate of a call: the upload, the packed rows (a nibble per element) of the objects in whole tiles,
    and the replicate's own counts if asked for; 0 beyond the limits."""
    n, f, e = int(n_objects), int(n_features), int(n_elements)
    if max_replicates(n, f) == 0 or not f <= e <= MAX_STATES * f:
        return 0
    return n * f + (-(-n // TILE) * TILE) * (-(-e // ROUND) * ROUND) // 2 + (4 * n * n if with_agree_rep else 0)


def statistics(y):
    """(agree, comparable) int64 [N, N] of one data set y [N, F], the cells compared feature by feature."""
    y = np.asarray(y)
    n, f_n = y.shape
    agree, comparable = np.zeros((n, n), dtype=np.int64), np.zeros((n, n), dtype=np.int64)
    for f in range(f_n):
        c = y[:, f]
        seen = c != NA
        both = seen[:, None] & seen[None, :]
        comparable += both
        agree += both & (c[:, None] == c[None, :])
    np.fill_diagonal(agree, 0)
    np.fill_diagonal(comparable, 0)
    return agree, comparable


def check(x, n_states, y):
    """Everything the unit returns for data x and replicates y [T, N, F]: agree_obs, comparable_obs, agree_rep [T, N, N], the
    accumulators (ACCUMULATORS) and n_replicates."""
    x, y, ns = np.asarray(x), np.asarray(y), np.asarray(n_states)
    assert x.dtype == np.uint8 and y.dtype == np.uint8 and y.shape[1:] == x.shape
    assert ((ns >= 1) & (ns <= MAX_STATES)).all() and ns.shape == (x.shape[1],)
    for a in (x, y):
        assert ((a == NA) | (a < ns)).all()
    assert y.shape[0] <= max_replicates(*x.shape)
    n = x.shape[0]
    agree_obs, comparable_obs = statistics(x)
    rep = np.zeros((y.shape[0], n, n), dtype=np.int64)
    for t in range(y.shape[0]):
        rep[t] = statistics(y[t])[0]
    off = ~np.eye(n, dtype=bool)
    return dict(agree_obs=agree_obs.astype(np.int32), comparable_obs=comparable_obs.astype(np.int32), agree_rep=rep.astype(np.int32),
                n_greater=((rep > agree_obs) & off).sum(axis=0).astype(np.int32), n_equal=((rep == agree_obs) & off).sum(axis=0).astype(np.int32),
                n_less=((rep < agree_obs) & off).sum(axis=0).astype(np.int32), sum=rep.sum(axis=0), sumsq=(rep * rep).sum(axis=0),
                n_replicates=y.shape[0])
