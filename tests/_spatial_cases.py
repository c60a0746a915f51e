"""The seeded cases of the spatial posterior predictive check, shared by tests/test_spatial_oracle_cpu.py (which proves under the
oracle alone that every case holds what it claims) and tests/test_gpu_spatial.py (device against oracle).  A plain helper module:
it holds no test.

A case is (x uint8 [N, F], n_states int32 [F], band uint8 [N, N], B, y uint8 [T, N, F]), all read-only, and the oracle's result,
computed once.  The objects are points in the unit square and their states follow the quarter of the square they lie in, so
near pairs agree more often than far ones.  N lies around the 64 objects of a mask word and the 128 of a count block, F around the
16 features of the default tile, S at 2 and at the limit of 32, B at 1 and 8.  The diagonal of band holds junk (it is ignored).
The replicates keep the data's missingness except the last one, which loses more cells (skipped cells of a check):

  replicate 0      the data itself: every entry ties (n_equal);
  replicates 1 ..  every column permuted on its own among its observed objects: the data's margins without the geography."""
from __future__ import annotations

import functools

import numpy as np

from tests import _spatial_oracle as orc

NA = orc.NA
TILE = 16                                # the default features per tile of the count kernel (csrc/sbe_spatial.hip)

# name -> (seed, N, F, S, B, T, NA rate, classes, all-NA object or None, all-NA feature or None)
# classes: "quantile" B classes of equal size over all pairs; "knn" one class over the union 6-nearest-neighbour graph;
#          "unequal" class 0 the nearest 1 % of the pairs, class 1 the next 60 %, the rest not counted; "none" nothing counted
CASES = {
    "n1": (21, 1, 3, 3, 1, 3, 0.0, "quantile", None, None),
    "n2": (22, 2, TILE + 1, 2, 1, 4, 0.0, "quantile", None, None),
    "n63": (23, 63, TILE - 1, 4, 8, 5, 0.2, "quantile", 5, 2),
    "n64": (24, 64, TILE, 32, 1, 5, 0.2, "knn", None, None),
    "n65": (25, 65, TILE + 1, 5, 3, 5, 0.2, "quantile", 64, 16),
    "n127": (26, 127, 1, 2, 8, 5, 0.1, "quantile", None, None),
    "n128": (27, 128, 9, 7, 2, 5, 0.3, "unequal", 0, None),
    "n129": (28, 129, 2 * TILE + 1, 3, 1, 4, 0.0, "knn", None, None),
    "n257": (29, 257, 5, 32, 8, 3, 0.2, "quantile", 256, 4),
    "none_counted": (30, 65, 4, 3, 2, 3, 0.1, "none", None, None),
    # the most objects the unit takes: 64 mask words, four chunks of 16 per lane
    "n4096": (31, 4096, 3, 3, 2, 2, 0.1, "unequal", 4095, None),
}
LARGE = ("n4096",)                       # (too many pairs for the literal loop, and for more than one pass on the device)


def bands(kind, points, n_bands, rng):
    """band uint8 [N, N] of the points' plane distances by `kind`, with junk on the diagonal."""
    n = points.shape[0]
    diff = points[:, None, :] - points[None, :, :]
    cost = np.sqrt((diff * diff).sum(axis=2))
    band = np.full((n, n), NA, dtype=np.uint8)
    upper = cost[np.triu_indices(n, 1)]
    if kind == "quantile" and upper.size:
        edges = np.quantile(upper, (np.arange(n_bands) + 1.0) / n_bands)
        band = np.minimum(np.searchsorted(edges, cost, side="left"), n_bands - 1).astype(np.uint8)
    elif kind == "unequal" and upper.size:
        edges = np.quantile(upper, [0.01, 0.61])
        cls = np.searchsorted(edges, cost, side="left")
        band = np.where(cls < 2, cls, NA).astype(np.uint8)
    elif kind == "knn" and n > 1:
        away = cost + np.where(np.eye(n, dtype=bool), np.inf, 0.0)
        near = np.argsort(away, axis=1, kind="stable")[:, :min(6, n - 1)]
        adj = np.zeros((n, n), dtype=bool)
        adj[np.repeat(np.arange(n), near.shape[1]), near.ravel()] = True
        band = np.where(adj | adj.T, 0, NA).astype(np.uint8)
    band[np.arange(n), np.arange(n)] = rng.integers(0, 256, n).astype(np.uint8)      # (ignored whatever it holds)
    return band


def _build(name):
    seed, n, f, s, b, t_n, na_rate, kind, na_object, na_feature = CASES[name]
    rng = np.random.default_rng(seed)
    points = rng.random((n, 2))
    quarter = (points[:, 0] > 0.5).astype(np.int64) * 2 + (points[:, 1] > 0.5)
    ns = rng.integers(2, s + 1, f).astype(np.int32)
    ns[0] = s
    if f > 2:
        ns[-1] = 1                                                # a feature of one state: it agrees wherever it is observed
    follow = rng.random((n, f)) < 0.7
    x = np.where(follow, quarter[:, None] % ns[None, :], rng.integers(0, ns[None, :], (n, f))).astype(np.uint8)
    x[rng.random((n, f)) < na_rate] = NA
    if na_object is not None:
        x[na_object, :] = NA
    if na_feature is not None:
        x[:, na_feature] = NA
    y = np.repeat(x[None], t_n, axis=0)
    for t in range(1, t_n):
        for k in range(f):
            at = np.nonzero(x[:, k] != NA)[0]
            y[t, at, k] = x[rng.permutation(at), k]
    if t_n > 1:
        y[-1][rng.random((n, f)) < 0.1] = NA
    return x, ns, bands(kind, points, b, rng), b, y


@functools.lru_cache(maxsize=None)
def case(name):
    """(x, n_states, band, B, y, the oracle's result) of the case."""
    x, ns, band, b, y = _build(name)
    for a in (x, ns, band, y):
        a.setflags(write=False)
    return x, ns, band, b, y, orc.check(x, ns, band, b, y)


def constant(n, f):
    """Every cell in one state, one class over the complete graph: agree = comparable = n (n - 1) / 2 for every feature and
    local_agree = (n - 1) f for every object."""
    x = np.full((n, f), 1, dtype=np.uint8)
    band = np.zeros((n, n), dtype=np.uint8)
    return x, np.full(f, 2, dtype=np.int32), band, 1


def halves(n, h, f):
    """The first h objects in state 0, the other n - h in state 1; class 0 within the halves, class 1 across:
    agree[0] = C(h, 2) + C(n - h, 2) = comparable[0], agree[1] = 0, comparable[1] = h (n - h)."""
    x = np.zeros((n, f), dtype=np.uint8)
    x[h:] = 1
    first = np.arange(n) < h
    band = np.where(first[:, None] == first[None, :], 0, 1).astype(np.uint8)
    return x, np.full(f, 2, dtype=np.int32), band, 2


def hand():
    """Four objects on a line, 0 - 1 - 2 - 3, class 0 the three edges, class 1 the pairs two steps apart, (0, 3) not counted; two
    features: 0, 0, 1, 1 and 0, NA, 0, 2.
      feature 0: edges (0,1) agree, (1,2) differ, (2,3) agree: agree[0] = 2 of 3; two steps: (0,2), (1,3) differ: agree[1] = 0 of 2
      feature 1: edges: only (2,3) comparable, differs: 0 of 1; two steps: (0,2) agree, (1,3) not comparable: 1 of 1
    local_agree[0] = 1, 1, 1, 1; local_agree[1] = 1, 0, 1, 0; total = 2, 1.  Replicate 0 is the data; replicate 1 sets feature 0
    to 0, 0, 0, 0 (agree[0][0] = 3 > 2, agree[1][0] = 2 > 0) and keeps feature 1."""
    x = np.array([[0, 0], [0, 255], [1, 0], [1, 2]], dtype=np.uint8)
    band = np.array([[9, 0, 1, 255], [0, 9, 0, 1], [1, 0, 9, 0], [255, 1, 0, 9]], dtype=np.uint8)
    y1 = x.copy()
    y1[:, 0] = 0
    return x, np.array([2, 3], dtype=np.int32), band, 2, np.stack([x, y1])
