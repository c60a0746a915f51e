"""Known answers that pin tests/_elpd_oracle.py (the NumPy restatement of arviz.loo / arviz.waic over a LikelihoodLogger
matrix): arviz is not a dependency, so the restatement is checked by what PSIS-LOO and WAIC must give on inputs
whose answer is known in closed form."""
import math

import numpy as np
import pytest

from tests import _elpd_oracle as eo


def _col(lh):
    return eo.column_stats(np.asarray(lh, dtype=np.float32))


@pytest.mark.parametrize("seed", range(4))
def test_short_column_is_the_unsmoothed_harmonic_mean(seed):
    """S = 5: T = 1, the tail has at most one element, k = inf and the importance weights are the raw 1/lh: loo_i is
    the harmonic-mean estimate -log(mean(1/lh))."""
    lh = np.random.default_rng(seed).uniform(0.05, 1.0, 5).astype(np.float32)
    loo_i, k, _lppd, _v = _col(lh)
    assert k == np.inf
    want = -math.log(np.mean(1 / lh.astype(np.float64)))
    assert abs(loo_i - want) <= 1e-14 * abs(want)


def test_heavy_ties_leave_a_tail_too_short_to_fit():
    """S = 100, T = 20: the 21st smallest value is tied with 96 others, so only the 3 smaller values form the tail."""
    lh = np.array([0.5] * 97 + [0.1, 0.2, 0.3], dtype=np.float32)
    np.random.default_rng(1).shuffle(lh)
    loo_i, k, _lppd, _v = _col(lh)
    assert k == np.inf
    want = -math.log(np.mean(1 / lh.astype(np.float64)))
    assert abs(loo_i - want) <= 1e-14 * abs(want)


@pytest.mark.parametrize("s", [5, 64, 1000])
def test_constant_column(s):
    lh = np.full(s, 0.3, dtype=np.float32)
    loo_i, k, lppd_i, v_i = _col(lh)
    ll = math.log(np.float64(np.float32(0.3)))
    assert k == np.inf and 0.0 <= v_i <= 1e-28          # (zero up to the rounding of the mean)
    assert abs(loo_i - ll) <= 1e-14 * abs(ll) and abs(lppd_i - ll) <= 1e-14 * abs(ll)


@pytest.mark.parametrize("k", [0.2, 0.5, 0.9])
def test_gpdfit_recovers_the_shape_of_exact_gpd_draws(k):
    rng = np.random.default_rng(int(k * 10))
    u = rng.uniform(size=10_000)
    x = np.sort(((1 - u) ** (-k) - 1) / k)            # GPD(k, sigma = 1) by inversion
    k_hat, sigma = eo.gpdfit(x)
    assert abs(k_hat - k) < 0.1
    assert abs(sigma - 1) < 0.1


def test_smoothing_happens_on_a_heavy_tail():
    """lh uniform on (0, 1): the importance ratios 1/lh have tail index 1, k near 1 (> 0.7: a warning)."""
    lh = np.random.default_rng(3).uniform(1e-4, 1, 4000).astype(np.float32)
    loo_i, k, lppd_i, _v = _col(lh)
    assert 0.7 < k < 1.5
    raw = -math.log(np.mean(1 / lh.astype(np.float64)))
    assert loo_i != raw and loo_i <= lppd_i


@pytest.mark.parametrize("s", [64, 1000, 4000])
def test_loo_does_not_depend_on_the_order_of_the_samples(s):
    rng = np.random.default_rng(s)
    lh = np.exp(rng.standard_t(3, s) - 2).astype(np.float32)
    a = _col(lh)
    b = _col(rng.permutation(lh))
    assert abs(a[0] - b[0]) <= 1e-13 * abs(a[0])
    assert a[1] == pytest.approx(b[1], rel=1e-12, abs=1e-12)


def test_burnin_drops_int_of_burnin_times_the_rows():
    rng = np.random.default_rng(7)
    lh = rng.uniform(0.1, 1, (10, 3)).astype(np.float32)
    for burnin, drop in [(0.0, 0), (0.15, 1), (0.19, 1), (0.2, 2), (0.55, 5)]:
        loo_i, k_i, lppd_i, v_i, s = eo.pointwise(lh, na_values=np.zeros(3, bool), burnin=burnin)
        assert s == 10 - drop
        want = np.array([eo.column_stats(lh[drop:, j]) for j in range(3)])
        np.testing.assert_array_equal(np.stack([loo_i, k_i, lppd_i, v_i], axis=1), want)


def test_na_rules():
    """na_values drops the columns it marks; without it, the columns whose every row is isclose(lh, 1) -- over all
    rows, burn-in included (elpd.py:27-39)."""
    rng = np.random.default_rng(8)
    lh = rng.uniform(0.1, 0.9, (20, 5)).astype(np.float32)
    lh[:, 1] = 1.0
    lh[:, 3] = np.float32(1 + 5e-6)          # within rtol 1e-5
    lh[:, 4] = 1.0
    lh[0, 4] = 1.5                            # a burn-in row that is not close to 1: the column is kept
    assert list(eo.kept_columns(lh)) == [True, False, True, False, True]
    loo_i, *_rest, s = eo.pointwise(lh, burnin=0.1)
    assert len(loo_i) == 3 and s == 18
    na = np.array([False, False, True, False, False])
    loo_i2, *_rest = eo.pointwise(lh, na_values=na, burnin=0.1)
    assert len(loo_i2) == 4
    assert loo_i2[0] == loo_i[0] and loo_i2[1] == pytest.approx(math.log(1.0), abs=1e-15)


def test_waic_against_the_direct_formula():
    rng = np.random.default_rng(9)
    lh = np.exp(rng.normal(-1, 0.7, (500, 40))).astype(np.float32)
    _loo, _k, lppd_i, v_i, s = eo.pointwise(lh, na_values=np.zeros(40, bool), burnin=0.0)
    ll = np.log(lh.astype(np.float64))
    waic_i = np.log(np.mean(np.exp(ll), axis=0)) - np.var(ll, axis=0)
    np.testing.assert_allclose(lppd_i - v_i, waic_i, rtol=1e-13)
    t = eo.totals(_loo, _k, lppd_i, v_i, s)
    assert t["p_waic"] == pytest.approx(np.var(ll, axis=0).sum(), rel=1e-13)
    assert t["n_data_points"] == 40 and t["n_samples"] == 500


def test_values_that_are_not_positive_and_finite_are_refused():
    lh = np.full((10, 2), 0.5, dtype=np.float32)
    lh[4, 1] = 0.0
    with pytest.raises(ValueError, match="positive and finite"):
        eo.pointwise(lh, burnin=0.0)


# ---- known answers across the sample range (the device is held to the same ones: tests/test_gpu_elpd_range.py) ----
def _beta_bernoulli(s, seed, n=20, ones=14, a=1.0, b=1.0):
    """The two distinct columns of a Beta-Bernoulli model under s exact posterior draws (y = 1, y = 0) and the exact
    log leave-one-out predictive of each: p(y_i | y_-i) = (a + sum_{j != i} y_j) / (a + b + n - 1) for y_i = 1."""
    theta = np.random.default_rng(seed).beta(a + ones, b + n - ones, s)
    exact = [math.log((a + ones - 1) / (a + b + n - 1)), math.log(1 - (a + ones) / (a + b + n - 1))]
    return theta.astype(np.float32), (1 - theta).astype(np.float32), exact


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_beta_bernoulli_smoothed_loo_at_2_20_samples(seed):
    """A smoothed loo_i tied to a known value: at S = 2^20 (T = 3072, 85 fit candidates) PSIS recovers the exact
    leave-one-out predictive.  Over seeds 0 .. 15 the error was at most 7.8e-4 (k = 0.003 .. 0.17): 2e-3 has margin."""
    c1, c0, exact = _beta_bernoulli(1 << 20, seed)
    for col, want in ((c1, exact[0]), (c0, exact[1])):
        loo_i, k, _lppd, _v = _col(col)
        assert 0 < k < 0.5
        assert abs(loo_i - want) <= 2e-3, (loo_i, want)


@pytest.mark.parametrize("s", [2, 3, 4, 20])
def test_columns_up_to_20_samples_are_never_smoothed(s):
    """T = ceil(min(0.2 S, 3 sqrt(S))) <= 4 up to S = 20: k = inf, loo_i = -log(mean(1/lh)), lppd_i = log(mean(lh)),
    v_i = var(log lh)."""
    lh = np.random.default_rng(s).uniform(0.01, 1.0, s).astype(np.float32)
    x = lh.astype(np.float64)
    loo_i, k, lppd_i, v_i = _col(lh)
    assert k == np.inf
    assert loo_i == pytest.approx(-math.log(np.mean(1 / x)), rel=1e-14)
    assert lppd_i == pytest.approx(math.log(np.mean(x)), rel=1e-14)
    assert v_i == pytest.approx(np.var(np.log(x)), rel=1e-12, abs=1e-300)


def test_21_samples_fit_five_distinct_tail_values_but_not_four():
    """S = 21, T = 5: the sixth smallest value is the cutoff.  Five distinct values below it are fitted; a tie of the
    fifth and sixth smallest leaves four, unsmoothed (the harmonic mean)."""
    v = np.linspace(0.05, 0.95, 21)
    loo_i, k, _lppd, _v = _col(v)
    assert np.isfinite(k) and loo_i != pytest.approx(-math.log(np.mean(1 / v.astype(np.float32).astype(float))), rel=1e-9)
    tied = v.copy()
    tied[5] = tied[4]
    x = tied.astype(np.float32).astype(np.float64)
    loo_i, k, _lppd, _v = _col(tied)
    assert k == np.inf
    assert loo_i == pytest.approx(-math.log(np.mean(1 / x)), rel=1e-14)


def test_good_k_uses_arviz_log10():
    """arviz.loo forms good_k with np.log10; math.log10 differs in the last bit at S = 11, 40, 43, 119, ... and the
    reported good_k (and the warning at a k that equals it) must be arviz's."""
    from sbayes_amd import elpd
    for s in (11, 40, 43, 119, 1002, 1 << 20):
        z = np.zeros(1)
        assert elpd._loo(z, z, z, s).good_k == eo.totals(z, z, z, z, s)["good_k"] == min(1 - 1 / np.log10(s), 0.7)
