"""Known answers that pin the host restatement of the model comparison (tests/_compare_oracle.py): arviz is not a
dependency, so closed forms and invariants stand in for it."""
import math

import numpy as np
import pytest

from tests import _compare_oracle as co

TOL = 1e-8


def test_totals_ranking_and_differences_follow_the_direct_formulas():
    x = co.gamma_values(3, 257, 4)
    elpd, se = co.totals(x)
    assert np.allclose(elpd, x.sum(axis=0), rtol=1e-13) and np.allclose(se, np.sqrt(257 * x.var(axis=0)), rtol=1e-12)
    order = co.rank(elpd)
    assert list(elpd[order]) == sorted(elpd, reverse=True)
    assert list(co.rank([1.0, 3.0, 3.0, 2.0])) == [1, 2, 3, 0]                 # ties by input order
    top = int(order[0])
    diff, dse = co.differences(x, top)
    d = x[:, [top]] - x
    assert np.allclose(diff, d.sum(axis=0), rtol=1e-12, atol=1e-12) and np.allclose(dse, np.sqrt(257 * d.var(axis=0)), rtol=1e-12)
    assert np.allclose(diff, elpd[top] - elpd, rtol=1e-12, atol=1e-10)
    assert diff[top] == 0.0 and dse[top] == 0.0 and np.all(diff >= 0)


def test_stacking_of_one_model_is_one():
    w, gap, updates, converged = co.stacking(co.gamma_values(1, 50, 1))
    assert list(w) == [1.0] and gap == 0.0 and updates == 0 and converged


@pytest.mark.parametrize("n1,n2,p,q,interior", [(700, 300, 0.6, 0.2, True), (400, 600, 0.5, 0.25, True), (900, 100, 0.6, 0.2, False),
                                                (100, 900, 0.6, 0.2, False)])
def test_stacking_meets_the_planted_two_model_optimum(n1, n2, p, q, interior):
    x, w0 = co.planted(n1, n2, p, q)
    assert (0.0 < w0 < 1.0) == interior
    w, gap, _updates, converged = co.stacking(x, tol=TOL)
    assert converged and 0.0 <= gap <= TOL
    # f is strongly concave along w_0 with f'' <= -c, c = ((p - q) / max(p, q))^2 (both denominators are at most max(p, q)), and
    # f* - f(w) <= gap: (c / 2) (w_0 - w_0*)^2 <= gap
    c = ((p - q) / max(p, q)) ** 2
    assert abs(w[0] - w0) <= math.sqrt(2 * gap / c) + 1e-12
    assert abs(w.sum() - 1.0) <= 1e-14


def test_a_duplicated_column_shares_the_single_columns_weight():
    x = co.gamma_values(5, 400, 3)
    w, gap, _u, _c = co.stacking(x, tol=TOL)
    twice = np.concatenate([x, x[:, [1]]], axis=1)
    w2, gap2, _u2, _c2 = co.stacking(twice, tol=TOL)
    merged = np.array([w2[0], w2[1] + w2[3], w2[2]])
    assert abs(co.objective(twice, w2) - co.objective(x, merged)) <= 1e-14       # the same mixture
    assert abs(co.objective(twice, w2) - co.objective(x, w)) <= gap + gap2
    # along any direction d the objective's curvature is -mean_i((p_i . d) / (p_i . w))^2 <= -d' (P'P / N) d, as p_i . w <= 1 for the
    # shifted p; with lam the smallest eigenvalue of P'P / N and f* - f(w) <= gap: (lam / 2) |w - w*|^2 <= gap for both sets of weights
    p = co.shifted(x)
    lam = float(np.linalg.eigvalsh(p.T @ p / p.shape[0])[0])
    assert lam > 0
    assert np.linalg.norm(merged - w) <= math.sqrt(2 * gap / lam) + math.sqrt(2 * gap2 / lam) + 1e-12


def test_a_dominated_model_ends_below_tol():
    x = co.gamma_values(7, 300, 2)
    x = np.concatenate([x, x[:, [0]] - 0.5], axis=1)                               # pointwise below model 0
    w, gap, _u, converged = co.stacking(x, tol=TOL)
    assert converged and gap <= TOL and w[2] < TOL


@pytest.mark.parametrize("n,m,seed", [(257, 4, 11), (4099, 8, 12)])
def test_the_fixed_point_is_no_worse_than_slsqp(n, m, seed):
    x = co.gamma_values(seed, n, m)
    w, gap, _u, converged = co.stacking(x, tol=TOL)
    w_slsqp = co.stacking_slsqp(x)
    assert converged and gap <= TOL
    f_em, f_slsqp = co.objective(x, w), co.objective(x, w_slsqp)
    print(f"n={n} m={m}: f_em={f_em!r} f_slsqp={f_slsqp!r} gap={gap:.3g}")
    assert f_em >= f_slsqp - TOL
    assert abs(w_slsqp.sum() - 1.0) <= 1e-9 and np.all(w_slsqp >= -1e-12)
    assert abs(co.gap(x, w) - gap) <= 1e-15


def test_the_update_is_monotone_and_stays_on_the_simplex():
    x = co.gamma_values(13, 200, 5)
    last = -np.inf
    for it in (1, 2, 4, 8, 16, 32):
        w, _gap, updates, _c = co.stacking(x, tol=1e-300, max_iter=it)
        f = co.objective(x, w)
        assert updates == it and f >= last and abs(w.sum() - 1.0) <= 1e-14 and np.all(w >= 0)
        last = f
    w, gap, updates, converged = co.stacking(x, tol=TOL, max_iter=3)
    assert updates == 3 and not converged and gap == co.gap(x, w) > TOL


BOOT_SEED, BOOT_B = 2024, 400


def test_bootstrap_rows_sum_to_one_and_recentre_on_the_totals():
    x = co.gamma_values(17, 300, 3)
    weights, se, z, w_b, bound = co.bootstrap(x, BOOT_SEED, BOOT_B)
    assert np.all(np.abs(w_b.sum(axis=1) - 1.0) <= 1e-15) and abs(weights.sum() - 1.0) <= 1e-14
    elpd, _se = co.totals(x)
    # the seed was checked to satisfy this before it was committed (5 standard errors of the mean)
    assert np.all(np.abs(z.mean(axis=0) - elpd) <= 5 * se / math.sqrt(BOOT_B)), (z.mean(axis=0) - elpd, se / math.sqrt(BOOT_B))
    assert np.allclose(se, z.std(axis=0), rtol=1e-12) and np.all(bound >= np.abs(z))


def test_bootstrap_of_identical_columns_is_uniform():
    x = np.repeat(co.gamma_values(19, 120, 1), 4, axis=1)
    weights, se, z, _w_b, _bound = co.bootstrap(x, 5, 20)
    assert np.array_equal(weights, np.full(4, 0.25)) and np.all(se == se[0]) and se[0] > 0
    assert np.all(z == z[:, [0]])


def test_bootstrap_of_one_model():
    x = co.gamma_values(23, 90, 1)
    weights, se, z, w_b, _bound = co.bootstrap(x, 7, 10)
    assert list(weights) == [1.0] and np.all(w_b == 1.0) and se[0] > 0 and z.shape == (10, 1)
    e = co.exponentials(7, 3, 90)
    assert np.all(e > 0) and np.all(np.isfinite(e)) and z[3, 0] == 90 * math.fsum(e * x[:, 0]) / math.fsum(e)


def test_plain_pseudo_bma_is_the_softmax_of_the_totals():
    w = co.pseudo_bma([-1000.0, -1001.0, -2000.0])
    assert abs(w[0] - 1 / (1 + math.exp(-1))) <= 1e-15 and w[2] == 0.0 and abs(w.sum() - 1.0) <= 1e-15
