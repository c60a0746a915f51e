"""The checker of sbayes_amd.partdist: the contract of include/sbe_partdist.h restated in NumPy.  A plain helper module: it
holds no test.

Runs are 0/1 arrays [S_r, K, N] with disjoint areas.  A sample is a partition of the N objects into K + 1 blocks: block 0
the objects in no area, blocks 1..K the areas.  Samples are ordered by (run, sample).  For samples x and y:
    n[k][l] = sum_i x[k][i] y[l][i];  a_k, b_l the area sizes.  The extended table E is (K+1) x (K+1):
        E[k][l] = n[k][l] (k, l >= 1),  E[k][0] = a_k - sum_l n[k][l],  E[0][l] = b_l - sum_k n[k][l],
        E[0][0] = N - sum a - sum b + sum n;  the extended sizes a+ = (N - sum a, a_1 .. a_K), b+ likewise.
    binder(x,y) = sum_k a_k^2 + sum_l b_l^2 - 2 sum_kl n[k][l]^2: the ordered object pairs, diagonal included, that share an
        area in exactly one of the two samples.  For a selection with similarity counts C (tests/_consensus_oracle.py):
        sum_t binder(s,t) = score[s] + sum_ij C[i][j].
    sumsq(x,y) = sum_kl E[k][l]^2.
    vi(x,y) = max(0, ((h_x + h_y) - 2 j) / N), x the EARLIER of the two samples, h_x = sum_{k=0..K} L[a+_k], h_y likewise,
        j = sum_{k=0..K} sum_{l=0..K} L[E[k][l]] with k major and l minor; every sum left to right from 0.0 in float64;
        L = xlogx(N): L[0] = 0, L[m] = m * log(m) as NumPy computes it.  The device is handed this table and never takes
        a log, so it agrees with this module bit for bit.
    sums: binder_sum[s][r'] = sum_{t in r'} binder(s,t) in exact integers; vi_sum[s][r'] in the tree of tree_sum: 64 lanes,
        lane j adds t = j, j + 64, .. of run r' onto 0.0, then xor exchanges at distances 32 .. 1.

Bounds.  u = 2^-53.  vi adds n_terms = 2 (K + 1) + (K + 1)^2 entries of L, none negative, in three chains, then one
addition, one exact doubling, one subtraction and one division: against the exact value of the same expression over the
same table the error is at most (n_terms + 3) 2^-52 S / N with S = h_x + h_y + 2 j the sum of the terms' magnitudes (first
order in u, stated with 2 u for u).  The table itself: NumPy's m log m is within XLOGX_REL of the exact product, relatively
(measured against mpmath at 50 digits for every m <= 16384 by tests/test_partdist_oracle_cpu.py: 1.85 u, recorded as 2 u);
it enters with a factor 4 of margin.  vi_bound() is the sum of the two.  The true VI of two equal partitions is 0, so
under other labels the computed value lies in [0, vi_bound]."""
from __future__ import annotations

import numpy as np

LANES = 64
XLOGX_REL = 2.0 * 2.0 ** -53              # the recorded relative error of NumPy's m log m over m <= 16384 (measured: 1.85 u)


def xlogx(n_objects):
    m = np.arange(int(n_objects) + 1, dtype=np.float64)
    table = np.zeros(int(n_objects) + 1, dtype=np.float64)
    table[1:] = m[1:] * np.log(m[1:])
    return table


def positions(runs):
    """One array per run: the ordinal of every sample in (run, sample) order."""
    at = np.cumsum([0] + [np.asarray(r).shape[0] for r in runs])
    return [np.arange(at[r], at[r + 1]) for r in range(len(runs))]


def tables(xs, ys):
    """n int64 [R, C, K, K] of samples xs [R, K, N] against ys [C, K, N]."""
    return np.einsum("rkn,cln->rckl", np.asarray(xs).astype(np.int64), np.asarray(ys).astype(np.int64))


def sizes(xs):
    return np.asarray(xs).astype(np.int64).sum(axis=2)


def extended(n, a, b, n_objects):
    """E int64 [.., K+1, K+1], a+ and b+ int64 [.., K+1] from tables [.., K, K] and sizes [.., K]."""
    n = np.asarray(n, dtype=np.int64)
    k = n.shape[-1]
    e = np.zeros(n.shape[:-2] + (k + 1, k + 1), dtype=np.int64)
    e[..., 1:, 1:] = n
    e[..., 1:, 0] = a - n.sum(axis=-1)
    e[..., 0, 1:] = b - n.sum(axis=-2)
    e[..., 0, 0] = int(n_objects) - a.sum(axis=-1) - b.sum(axis=-1) + n.sum(axis=(-1, -2))
    a_plus = np.concatenate([(int(n_objects) - a.sum(axis=-1))[..., None], a], axis=-1)
    b_plus = np.concatenate([(int(n_objects) - b.sum(axis=-1))[..., None], b], axis=-1)
    return e, a_plus, b_plus


def chain(terms):
    """The sum of float64 terms [.., m] along the last axis, left to right from 0.0."""
    acc = np.zeros(terms.shape[:-1], dtype=np.float64)
    for q in range(terms.shape[-1]):
        acc = acc + terms[..., q]
    return acc


def measures(n, a, b, n_objects, swap=None, table=None):
    """(binder int64, vi float64, sumsq int64), each [R, C], from tables n [R, C, K, K] and sizes a [R, K], b [C, K].  swap:
    boolean [R, C], True where the column's sample is the earlier of the two (default: nowhere)."""
    n = np.asarray(n, dtype=np.int64)
    a = np.broadcast_to(np.asarray(a, dtype=np.int64)[:, None, :], n.shape[:3])
    b = np.broadcast_to(np.asarray(b, dtype=np.int64)[None, :, :], n.shape[:3])
    binder = (a * a).sum(axis=-1) + (b * b).sum(axis=-1) - 2 * (n * n).sum(axis=(-1, -2))
    if swap is not None:                                                    # x is the earlier sample
        s3, s4 = swap[:, :, None], swap[:, :, None, None]
        n, a, b = np.where(s4, np.swapaxes(n, -1, -2), n), np.where(s3, b, a), np.where(s3, a, b)
    e, a_plus, b_plus = extended(n, a, b, n_objects)
    assert e.min() >= 0 and e.sum(axis=(-1, -2)).min() == e.sum(axis=(-1, -2)).max() == int(n_objects), "the areas of a sample are not disjoint"
    sumsq = (e * e).sum(axis=(-1, -2))
    L = xlogx(n_objects) if table is None else table
    h_x, h_y = chain(L[a_plus]), chain(L[b_plus])
    j = chain(L[e.reshape(e.shape[:-2] + (-1,))])                           # k major, l minor
    vi = np.maximum(0.0, ((h_x + h_y) - 2.0 * j) / float(n_objects))
    return binder, vi, sumsq


def block(xs, ys, pos_x=None, pos_y=None):
    """(binder, vi, sumsq) [R, C] of samples xs against ys; pos_x, pos_y: their ordinals in (run, sample) order (default: xs
    before ys)."""
    n_objects = np.asarray(xs).shape[2]
    swap = None if pos_x is None else np.asarray(pos_x)[:, None] > np.asarray(pos_y)[None, :]
    return measures(tables(xs, ys), sizes(xs), sizes(ys), n_objects, swap)


def tree_sum(values):
    """The contract's tree along the last axis: lane j adds the entries j, j + 64, .. onto 0.0, then the lanes are exchanged
    by xor at distances 32 .. 1.  Every lane ends with the same value; lane 0's is returned."""
    v = np.asarray(values, dtype=np.float64)
    lanes = np.zeros(v.shape[:-1] + (LANES,), dtype=np.float64)
    for t0 in range(0, v.shape[-1], LANES):
        piece = v[..., t0:t0 + LANES]
        lanes[..., :piece.shape[-1]] = lanes[..., :piece.shape[-1]] + piece
    index = np.arange(LANES)
    o = LANES // 2
    while o:
        lanes = lanes + lanes[..., index ^ o]
        o //= 2
    return lanes[..., 0]


def sums(runs, selection=None):
    """(binder_sum int64, vi_sum float64), each [T_sel, R_sel], over the runs of `selection` (indices; default: all)."""
    selection = list(range(len(runs))) if selection is None else list(selection)
    pos = positions(runs)
    rows_b, rows_v = [], []
    for a in selection:
        if not len(runs[a]):
            continue
        cols_b, cols_v = [], []
        for b in selection:
            if len(runs[b]):
                binder, vi, _ = block(runs[a], runs[b], pos[a], pos[b])
                cols_b.append(binder.sum(axis=1))
                cols_v.append(tree_sum(vi))
            else:
                cols_b.append(np.zeros(len(runs[a]), dtype=np.int64))
                cols_v.append(np.zeros(len(runs[a])))
        rows_b.append(np.stack(cols_b, axis=1))
        rows_v.append(np.stack(cols_v, axis=1))
    return np.concatenate(rows_b), np.concatenate(rows_v)


def n_terms(n_clusters):
    return 2 * (n_clusters + 1) + (n_clusters + 1) ** 2


def vi_bound(n_clusters, n_objects, magnitude):
    """The bound of the module's docstring; magnitude: S = h_x + h_y + 2 j (vi_magnitude)."""
    return ((n_terms(n_clusters) + 3) * 2.0 ** -52 + 4.0 * XLOGX_REL) * magnitude / float(n_objects)


def vi_magnitude(n, a, b, n_objects):
    """S = h_x + h_y + 2 j, float64 [R, C] (the order does not matter here)."""
    n = np.asarray(n, dtype=np.int64)
    a = np.broadcast_to(np.asarray(a, dtype=np.int64)[:, None, :], n.shape[:3])
    b = np.broadcast_to(np.asarray(b, dtype=np.int64)[None, :, :], n.shape[:3])
    e, a_plus, b_plus = extended(n, a, b, n_objects)
    L = xlogx(n_objects)
    return L[a_plus].sum(axis=-1) + L[b_plus].sum(axis=-1) + 2.0 * L[e].sum(axis=(-1, -2))


def tree_bound(values):
    """|tree_sum - exact sum| for non-negative terms [.., S]: a lane adds ceil(S / 64) terms, six exchanges follow."""
    v = np.asarray(values, dtype=np.float64)
    return (-(-v.shape[-1] // LANES) + 6) * 2.0 ** -52 * np.abs(v).sum(axis=-1)


def adjusted_rand(e):
    """The textbook adjusted Rand index of one extended table, in exact fractions (1 where the denominator is 0)."""
    from fractions import Fraction
    from math import comb
    e = np.asarray(e, dtype=np.int64)
    index = sum(comb(int(v), 2) for v in e.ravel())
    rows, cols = sum(comb(int(v), 2) for v in e.sum(axis=1)), sum(comb(int(v), 2) for v in e.sum(axis=0))
    pairs = comb(int(e.sum()), 2)
    if pairs == 0:
        return 1.0
    expected = Fraction(rows * cols, pairs)
    den = Fraction(rows + cols, 2) - expected
    return 1.0 if den == 0 else float((index - expected) / den)
