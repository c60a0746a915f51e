"""The checker of sbayes_amd.partdist (tests/_partdist_oracle.py) against brute force from label vectors: Binder's distance by
counting object pairs, the variation of information by mpmath at 50 digits from its definition, the adjusted Rand index from
the textbook formula, and the identity that ties the distances to the consensus scores (tests/_consensus_oracle.py)."""
import math
from fractions import Fraction

import mpmath as mp
import numpy as np
import pytest

from sbayes_amd import partdist
from tests import _consensus_oracle as consensus_orc
from tests import _partdist_cases as cases
from tests import _partdist_oracle as orc

CASES = [(7, 1, 1, 6100), (9, 2, 13, 6101), (8, 3, 40, 6102), (6, 5, 33, 6103), (5, 8, 70, 6104)]


def brute_binder(lx, ly):
    """Ordered object pairs, diagonal included, that share an area in exactly one of the two samples."""
    same_x = (lx[:, None] == lx[None, :]) & (lx[:, None] > 0)
    same_y = (ly[:, None] == ly[None, :]) & (ly[:, None] > 0)
    return int((same_x != same_y).sum())


def exact_vi(lx, ly):
    """2 H(X,Y) - H(X) - H(Y) of the (K+1)-block partitions, in nats, at 50 digits."""
    n = len(lx)

    def entropy(keys):
        _, counts = np.unique(keys, return_counts=True, axis=0)
        return -sum(mp.mpf(int(c)) / n * mp.log(mp.mpf(int(c)) / n) for c in counts)
    return 2 * entropy(np.stack([lx, ly], axis=1)) - entropy(lx[:, None]) - entropy(ly[:, None])


def test_the_table_of_m_log_m_is_within_the_recorded_error_for_every_m():
    mp.mp.dps = 50
    table = orc.xlogx(16384)
    assert table[0] == 0.0 and table[1] == 0.0 and np.array_equal(table, partdist.xlogx(16384))
    worst = mp.mpf(0)
    for m in range(2, 16385):
        exact = m * mp.log(m)
        worst = max(worst, abs(mp.mpf(float(table[m])) - exact) / exact)
    print(f"largest relative error of m log m over m <= 16384: {float(worst) / 2.0 ** -53:.3f} u")
    assert float(worst) <= orc.XLOGX_REL


@pytest.mark.parametrize("s,k,n,seed", CASES)
def test_binder_vi_and_rand_equal_brute_force_from_the_labels(s, k, n, seed):
    mp.mp.dps = 50
    c = cases.disjoint(s, k, n, seed)
    labels = cases.labels_of(c)
    pos = np.arange(s)
    binder, vi, sumsq = orc.block(c, c, pos, pos)
    tables, a = orc.tables(c, c), orc.sizes(c)
    bound = orc.vi_bound(k, n, orc.vi_magnitude(tables, a, a, n))
    ari = partdist.adjusted_rand(sumsq, a, a, n)
    rand = partdist.rand_index(sumsq, a, a, n)
    for x in range(s):
        for y in range(s):
            assert binder[x, y] == brute_binder(labels[x], labels[y]), (x, y)
            exact = exact_vi(labels[x], labels[y])
            assert abs(mp.mpf(float(vi[x, y])) - exact) <= bound[x, y], (x, y, vi[x, y], float(exact), bound[x, y])
            e, _, _ = orc.extended(tables[x, y], a[x], a[y], n)
            assert e.sum() == n and sumsq[x, y] == (e * e).sum()
            want = orc.adjusted_rand(e)
            assert abs(ari[x, y] - want) <= 4 * 2.0 ** -53 * abs(want), (x, y)          # two conversions and one division
            agree = sum(1 for i in range(n) for j in range(i) if (labels[x][i] == labels[x][j]) == (labels[y][i] == labels[y][j]))
            assert rand[x, y] == (agree / math.comb(n, 2) if n > 1 else 1.0)
    assert np.array_equal(vi, vi.T) and (vi >= 0.0).all() and not np.diag(vi).any() and not np.diag(binder).any()
    assert np.array_equal(binder, binder.T) and np.array_equal(sumsq, sumsq.T)
    assert np.array_equal(np.diag(ari), np.ones(s))


def test_the_adjusted_rand_index_of_known_tables():
    # Hubert & Arabie's form on a table worked by hand: rows (2, 2), columns (2, 2), table [[1, 1], [1, 1]]
    e = np.array([[1, 1], [1, 1]])
    assert orc.adjusted_rand(e) == float(Fraction(0 - Fraction(2 * 2, 6), 2 - Fraction(2 * 2, 6))) == -0.5
    got = partdist.adjusted_rand(np.array([[4]]), np.array([[2]]), np.array([[2]]), 4)     # one area of two objects each side, blocks 0 of two
    assert got.shape == (1, 1) and got[0, 0] == -0.5
    # denominators of 0: one block on both sides, and every block a single object
    assert partdist.adjusted_rand(np.array([[25]]), np.array([[5]]), np.array([[5]]), 5)[0, 0] == 1.0
    assert partdist.adjusted_rand(np.array([[2]]), np.array([[1]]), np.array([[1]]), 2)[0, 0] == 1.0
    assert partdist.adjusted_rand(np.array([[1]]), np.array([[1]]), np.array([[0]]), 1)[0, 0] == 1.0


@pytest.mark.parametrize("lengths,k,n,seed", [((6, 4), 3, 37, 6200), ((5, 1, 7), 5, 20, 6201), ((9,), 8, 64, 6202), ((3, 3), 1, 11, 6203)])
def test_the_binder_sums_are_the_consensus_scores_plus_the_sum_of_the_counts(lengths, k, n, seed):
    runs = [cases.disjoint(s, k, n, seed + r) for r, s in enumerate(lengths)]
    counts, t = consensus_orc.similarity(runs)
    binder_sum, vi_sum = orc.sums(runs)
    scores = np.concatenate([consensus_orc.scores(r, counts, t) for r in runs])
    assert np.array_equal(binder_sum.sum(axis=1), scores + int(counts.sum()))
    # the tree against the exact sum of the same terms
    pos = orc.positions(runs)
    for a in range(len(runs)):
        at = pos[a][0]
        for b in range(len(runs)):
            _, vi, _ = orc.block(runs[a], runs[b], pos[a], pos[b])
            for s in range(lengths[a]):
                exact = math.fsum(vi[s])
                assert abs(vi_sum[at + s, b] - exact) <= orc.tree_bound(vi[s])


def test_equal_partitions_under_other_labels_lie_within_the_bound_and_the_same_labels_give_zero():
    k, n = 5, 257
    c = cases.disjoint(12, k, n, 6300, outside=0.2)
    moved = c[:, [3, 0, 4, 1, 2], :]
    pos = np.arange(12)
    binder, vi, sumsq = orc.block(c, moved, pos, pos + 12)
    a = orc.sizes(c)
    bound = orc.vi_bound(k, n, orc.vi_magnitude(orc.tables(c, moved), a, orc.sizes(moved), n))
    own = (a * a).sum(axis=1) + (n - a.sum(axis=1)) ** 2
    assert not np.diag(binder).any() and np.array_equal(np.diag(sumsq), own)
    assert (np.diag(vi) >= 0.0).all() and (np.diag(vi) <= np.diag(bound)).all() and np.diag(bound).max() < 1e-12
    _, same, _ = orc.block(c, c.copy(), pos, pos + 12)
    assert not np.diag(same).any()                                          # the zeros of E add +0.0: exactly 0.0
    # vi(y, x) = vi(x, y): the earlier sample is x from whichever side the pair is seen
    _, back, _ = orc.block(moved, c, pos + 12, pos)
    assert np.array_equal(back, vi.T)


def test_the_tree_is_64_lanes_then_xor_exchanges():
    v = np.random.default_rng(6400).random(150)
    lanes = [0.0] * 64
    for t, value in enumerate(v):
        lanes[t % 64] += value
    o = 32
    while o:
        lanes = [lanes[j] + lanes[j ^ o] for j in range(64)]
        o //= 2
    assert len(set(lanes)) == 1 and orc.tree_sum(v) == lanes[0]
    assert orc.tree_sum(np.zeros(0)) == 0.0 and orc.tree_sum(np.array([3.5])) == 3.5


def test_the_host_side_readings_of_the_sums():
    binder_sum = np.array([[0 + 4, 6], [4 + 0, 2], [6, 0], ], dtype=np.int64)      # runs of 2 and 1 samples
    vi_sum = np.array([[0.5, 0.25], [0.5, 0.75], [1.0, 0.0]])
    b, v = partdist.mean_run_distances(binder_sum, vi_sum, [2, 1])
    assert b[0, 0] == 8 / 2 and b[0, 1] == 8 / 2 and b[1, 0] == 6 / 2 and np.isnan(b[1, 1])
    assert v[0, 0] == 1.0 / 2 and v[0, 1] == 1.0 / 2 and v[1, 0] == 0.5 and np.isnan(v[1, 1])
    assert partdist.argmin_loss([np.array([5, 3, 3]), np.array([3, 9])]) == (0, 1)
    assert partdist.argmin_loss([np.array([5.0, 4.0]), np.array([3.0, 3.0])]) == (1, 0)
    with pytest.raises(ValueError, match="no sample"):
        partdist.argmin_loss([np.zeros(0)])
    d = [np.array([0.0, 1.0, 2.0, 3.0]), np.arange(4.0, 20.0)]              # 20 samples
    assert partdist.ball_radius(d, 0.95) == 18.0 and partdist.ball_radius(d, 1.0) == 19.0 and partdist.ball_radius(d, 0.05) == 0.0
    assert partdist.ball_radius(d, 0.951) == 19.0
