"""CPU checks of the partition search's checker (tests/_partsearch_oracle.py) against definitions it does not share: the
scores against the loss recomputed from scratch, the sweeps' monotony, local optimality, the brute-force optimum of small
cases and tests/_partdist_oracle.py's losses."""
import numpy as np
import pytest

from tests import _partdist_oracle as partdist_orc
from tests import _partsearch_cases as cases
from tests import _partsearch_oracle as orc

SHAPES = [(9, 2, 7), (33, 5, 65), (40, 8, 300)]


def _moved(c, i, q):
    out = c.copy()
    out[i] = q
    return out


@pytest.mark.parametrize("n,k,t", SHAPES)
def test_the_scores_are_the_change_of_the_loss_sum_recomputed_from_scratch(n, k, t):
    y, _ = cases.noisy(n + t, n, k, t)
    c = cases.random_starts(5, n, k, 1)[0][0]
    table = orc.xlogx(n)
    dl = table[1:] - table[:-1]
    for i in range(0, n, max(1, n // 7)):
        p = int(c[i])
        e, a = orc.tables(c, y, k), np.bincount(c, minlength=k + 1).astype(np.int64)
        yi = y[:, i].astype(np.int64)
        e[p, yi, np.arange(t)] -= 1
        a[p] -= 1
        g_vi, s = orc.scores(e, a, yi, "vi", dl)
        g_binder, _ = orc.scores(e, a, yi, "binder", dl)
        sums = [orc.evaluate([_moved(c, i, q)], y, k) for q in range(k + 1)]
        slack = [orc.sum_bound(_moved(c, i, q), y, k) for q in range(k + 1)]
        for q in range(k + 1):
            # Binder: exact
            assert int(sums[q][3][0]) - int(sums[p][3][0]) == int(g_binder[q]) - int(g_binder[p])
            # VI: N (sum(q) - sum(p)) = g(q) - g(p) within the bounds of both sums and both scores (module docstring)
            lhs = n * (float(sums[q][2][0]) - float(sums[p][2][0]))
            bound = n * (slack[q] + slack[p]) + orc.g_bound(t, dl[a[q]], s[q]) + orc.g_bound(t, dl[a[p]], s[p])
            assert abs(lhs - (g_vi[q] - g_vi[p])) <= bound + 2.0 ** -52 * abs(lhs), (i, q)


@pytest.mark.parametrize("loss", cases.LOSSES)
@pytest.mark.parametrize("n,k,t", SHAPES)
def test_sweeps_never_raise_the_loss_and_end_in_a_local_optimum(loss, n, k, t):
    y, _ = cases.noisy(3 * n + t, n, k, t)
    init, order = cases.random_starts(11, n, k, 2)
    for s in range(2):
        got = orc.search(y, k, loss, init[s], order[s], 40)
        assert got.converged == 1 and got.sweeps >= 2 and np.isnan(got.trace[got.sweeps:]).all()
        assert got.trace[got.sweeps - 1] == (got.vi_sum if loss == "vi" else got.binder_sum)
        # no single move lowers the loss sum
        _, _, vi_sum, binder_sum = orc.evaluate([got.labels], y, k)
        here = float(vi_sum[0]) if loss == "vi" else int(binder_sum[0])
        slack = 0 if loss == "binder" else 2 * orc.sum_bound_any(k, n, t)
        for i in range(n):
            for q in range(k + 1):
                other = orc.evaluate([_moved(got.labels, i, q)], y, k)
                there = float(other[2][0]) if loss == "vi" else int(other[3][0])
                assert there >= here - slack, (i, q)


@pytest.mark.parametrize("loss", cases.LOSSES)
def test_the_vi_trace_rises_by_no_more_than_the_bound(loss):
    n, k, t = 33, 5, 65
    y, _ = cases.noisy(77, n, k, t)
    init, order = cases.random_starts(12, n, k, 3)
    for s in range(3):
        got = orc.search(y, k, loss, init[s], order[s], 40)
        start = orc.evaluate([init[s]], y, k)
        before = float(start[2][0]) if loss == "vi" else float(start[3][0])
        assert got.sweeps >= 2
        for w in range(got.sweeps):
            # the exact loss falls by the exact scores of the sweep's moves; the computed scores were negative
            bound = 0.0 if loss == "binder" else got.slack[w] + 2 * orc.sum_bound_any(k, n, t)
            assert got.trace[w] - before <= bound
            before = got.trace[w]


@pytest.mark.parametrize("loss", cases.LOSSES)
def test_the_best_of_eight_starts_is_the_brute_force_optimum(loss):
    assert len(cases.BRUTE_SEEDS) >= 24
    for seed in cases.BRUTE_SEEDS:
        y, k = cases.brute(seed)
        cands, vi_sum, binder_sum = cases.brute_force(y, k)
        init, order = cases.starts_of(y, k, 8, seed, loss)
        got = cases.oracle_starts(y, k, loss, init, order, 64)
        assert all(g.converged for g in got)
        medoid = orc.evaluate([init[0]], y, k)
        if loss == "binder":
            assert min(g.binder_sum for g in got) == int(binder_sum.min()), seed
            assert got[0].binder_sum <= int(medoid[3][0])
        else:
            best = min(got, key=lambda g: g.vi_sum)
            slack = 2 * orc.sum_bound(best.labels, y, k)
            assert abs(best.vi_sum - float(vi_sum.min())) <= slack, seed
            assert got[0].vi_sum <= float(medoid[2][0]) + slack


@pytest.mark.parametrize("n,k,t", SHAPES)
def test_the_losses_are_the_partition_distances_checkers(n, k, t):
    y, _ = cases.noisy(n, n, k, t)
    c = cases.random_starts(3, n, k, 2)[0]
    c[1][c[1] == k] = 0                                       # an empty block
    vi, binder, vi_sum, binder_sum = orc.evaluate(c, y, k)
    want_b, want_v, _ = partdist_orc.block(orc.rows_of(c, k), orc.rows_of(y, k))
    assert np.array_equal(binder, want_b) and np.array_equal(vi, want_v)
    assert np.array_equal(binder_sum, want_b.sum(axis=1))
    assert np.array_equal(orc.labels_of(orc.rows_of(y, k)), y)
    # the tree: within tree_bound's form of the plain sum, and exact where every value is a small integer
    assert np.all(np.abs(vi_sum - vi.sum(axis=1)) <= (-(-t // 256) + 8) * 2.0 ** -52 * vi.sum(axis=1))
    ints = np.arange(1000, dtype=np.float64)
    assert orc.block_tree(ints) == ints.sum() and orc.block_tree(ints[:1]) == 0.0 and orc.block_tree(ints[:2]) == 1.0


def test_both_branches_of_the_tie_rule_are_taken_under_binder():
    y, k, init, order = cases.contradictory()
    ties = np.sum([orc.search(y, k, "binder", init[s], order[s], 8).ties for s in range(init.shape[0])], axis=0)
    assert ties[0] > 0 and ties[1] > 0, ties


def test_a_start_one_move_from_the_common_partition_reaches_it_at_zero():
    truth = cases.noisy(4, 33, 5, 1)[1]
    y = np.repeat(truth[None], 65, axis=0)
    init = truth.copy()
    init[7] = (init[7] + 1) % 6
    for loss in cases.LOSSES:
        got = orc.search(y, 5, loss, init, np.arange(33), 8)
        assert np.array_equal(got.labels, truth) and got.vi_sum == 0.0 and got.binder_sum == 0 and (got.sweeps, got.moves, got.converged) == (2, 1, 1)
