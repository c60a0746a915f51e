"""CPU checks of the summary's checker (tests/_summary_oracle.py): each formula of the contract against an independent
statement of it (np.quantile, a brute-force HDI, scipy's rankdata, ndtri at 40 digits), the bounds with an input error
against the diagnostics' bounds, two known answers, and the decision margins of every fixed case of the GPU tests."""
import math

import mpmath
import numpy as np
import pytest
from scipy.special import ndtri
from scipy.stats import rankdata

from tests import _diag_oracle as orc
from tests import _summary_cases as cases
from tests import _summary_oracle as sorc

U = 2.0 ** -53


def test_quantile_is_within_one_ulp_of_numpy():
    rng = np.random.default_rng(1)
    worst = 0.0
    for n in (8, 9, 42, 64, 65, 255, 257, 1000, 17920):
        for scale in (1.0, 1e-3, 1e6):
            s = np.sort(rng.standard_normal(n) * scale + scale)
            for p in (0.0, 0.05, 0.25, 0.5, 0.9, 0.975, 1.0):
                got, want = sorc.quantile(s, p), float(np.quantile(s, p))
                worst = max(worst, abs(got - want) / np.spacing(abs(want)))
    print(f"[summary-bound] quantile against np.quantile: {worst:.3g} ulp")
    assert worst <= 1.0
    s = np.array([1.0, 2.0, 4.0, 8.0])
    assert [sorc.quantile(s, p) for p in (0.0, 0.5, 1.0, 1 / 3)] == [1.0, 3.0, 8.0, 2.0]


def test_hdi_against_a_brute_force_search():
    rng = np.random.default_rng(2)
    for n, prob in ((8, 0.94), (42, 0.5), (100, 0.94), (257, 0.9), (10, 0.01), (10, float(np.nextafter(1.0, 0.0)))):
        for ties in (False, True):
            s = np.sort(np.round(rng.standard_normal(n), 1) if ties else rng.standard_normal(n))
            inc = min(max(int(math.floor(prob * n)), 1), n - 1)
            best = min(range(n - inc), key=lambda i: (s[i + inc] - s[i], i))
            assert sorc.hdi(s, prob) == (s[best], s[best + inc]) and sorc.hdi_span(prob, n) == inc
    assert sorc.hdi(np.array([0.0, 2.0, 2.5, 3.0]), 0.5) == (2.0, 3.0) and sorc.hdi(np.array([0.0, 1.0, 2.0, 3.0]), 0.5) == (0.0, 2.0)


def test_ranks_equal_scipy_rankdata():
    rng = np.random.default_rng(3)
    for v in (rng.standard_normal((4, 50)), rng.integers(0, 5, (3, 40)).astype(float), np.zeros((2, 8)),
              np.array([[0.0, -0.0, 1.0, 0.0]]) + 0.0):
        r = sorc.ranks(v)
        assert np.array_equal(r.ravel(), rankdata(v.ravel(), method="average")) and np.all(2 * r == np.round(2 * r))


def test_the_checkers_ndtri_is_within_8u_of_40_digits_on_the_rank_grid_of_2_pow_20():
    mpmath.mp.dps = 40
    N = 1 << 20
    rng = np.random.default_rng(4)
    r = np.concatenate([np.arange(1, 201), np.arange(N - 199, N + 1), rng.integers(1, N + 1, 3000)]).astype(np.float64)
    r[3:-3:7] += 0.5                                                        # (half-integers occur with ties)
    r = np.minimum(r, N)
    p = sorc.rank_probability(r, N)
    assert p.min() == 0.625 / (N + 0.25) and p.max() == (N - 0.375) / (N + 0.25)
    z = ndtri(p)
    worst = 0.0
    for pi, zi in zip(p, z):
        exact = mpmath.sqrt(2) * mpmath.erfinv(2 * mpmath.mpf(float(pi)) - 1)
        worst = max(worst, float(abs(mpmath.mpf(float(zi)) - exact) / (U * max(1.0, abs(float(exact))))))
    print(f"[summary-bound] scipy ndtri against 40 digits: {worst:.3g} u max(1, |z|) of {sorc.C_CHECKER}")
    assert worst <= sorc.C_CHECKER == 8 and np.abs(z).max() < 5.0
    assert sorc.C_NDTRI <= 64


def test_bounds_with_input_error_equal_the_diagnostics_bounds_at_zero_and_grow_with_delta():
    x = orc.ar1(np.random.default_rng(5), 0.6, 4, 200, 3, loc=2.0)
    x[:, :, 2] = 0.25
    for j in range(3):
        c = orc.column(np.ascontiguousarray(x[:, :, j]))
        assert sorc.bounds_with_input_error(c, 0.0) == orc.column_bounds(c)
        if j < 2:
            b0, b1 = orc.column_bounds(c), sorc.bounds_with_input_error(c, 1e-13)
            assert all(b1[k] > b0[k] for k in b0)
            assert b1["mean"] - b0["mean"] == pytest.approx(2e-13, rel=1e-6)
    bad = orc.column(np.array([[1.0, np.nan, 2.0, 3.0]]))
    assert sorc.bounds_with_input_error(bad, 1e-13) == orc.column_bounds(bad)


def _student_chains(seed, m=4, s=1000, scale_last=3.0):
    rng = np.random.default_rng(seed)
    x = rng.standard_t(2.0, size=(m, s, 1))
    x[m - 1] *= scale_last
    return x


def test_known_answer_rank_rhat_sees_a_scaled_heavy_tailed_chain_the_classic_one_does_not():
    """Four chains of Student-t (2 degrees of freedom) draws, the last scaled by 3: the chains agree in location, so the
    classic split R-hat stays below 1.02; the folded rank-normalised R-hat exceeds 1.05."""
    res = sorc.summarize(list(_student_chains(7)), burnin=0.0)
    print(f"[summary-known] rhat {res['rhat'][0]:.4f} rhat_rank {res['rhat_rank'][0]:.4f}")
    assert res["rhat"][0] < 1.02 and res["rhat_rank"][0] > 1.05
    col = res["columns"][0]
    assert col["parts"]["zf"]["col"]["rhat"] == res["rhat_rank"][0] > col["parts"]["zb"]["col"]["rhat"]


def test_iid_normal_has_bulk_and_tail_ess_of_the_order_of_the_draws():
    x = np.random.default_rng(8).standard_normal((4, 1000, 1))
    res = sorc.summarize(list(x), burnin=0.0, split=False)
    n = 4000
    assert 0.7 * n < res["ess_bulk"][0] < 1.3 * n and 0.5 * n < res["ess_tail"][0] < 1.5 * n
    assert abs(res["rhat_rank"][0] - 1.0) < 0.01
    assert np.allclose(res["quantiles"][:, 0], np.quantile(x, (0.05, 0.5, 0.95)), rtol=4 * U, atol=0.0)


def test_flagged_columns_follow_the_contract():
    x = np.zeros((2, 10, 3))
    x[:, :, 0] = 0.25
    x[:, :, 1] = np.random.default_rng(9).standard_normal((2, 10))
    x[1, 3, 1] = np.inf
    x[:, :, 2] = np.where(np.arange(10) % 2 == 0, 0.0, -0.0)                 # +0 and -0: constant, and +0 in every output
    res = sorc.summarize(list(x), burnin=0.0)
    assert res["flag"].tolist() == [1, 2, 1]
    assert res["quantiles"][:, 0].tolist() == [0.25] * 3 and (res["hdi_lo"][0], res["hdi_hi"][0]) == (0.25, 0.25)
    assert res["ess_bulk"][0] == res["ess_tail"][0] == 20.0 and math.isnan(res["rhat_rank"][0])
    for k in ("hdi_lo", "hdi_hi", "ess_bulk", "ess_tail", "rhat_rank", "mean"):
        assert math.isnan(res[k][1]), k
    assert np.isnan(res["quantiles"][:, 1]).all()
    assert not np.signbit(res["quantiles"][:, 2]).any() and not np.signbit(res["hdi_lo"][2])


def test_a_column_constant_within_every_chain_has_an_infinite_rank_rhat_from_exact_integers():
    x, kw, want = cases.case("chain_constant")
    assert np.isinf(want["rhat_rank"][:2]).all() and np.isinf(want["rhat"][:2]).all() and np.isfinite(want["rhat_rank"][2])
    assert want["flag"].tolist() == [0, 0, 0] and (want["bound"]["rhat_rank"][:2] == 0.0).all()
    for j in (0, 1):
        c = want["columns"][j]
        d = c["derived"]
        assert d["flat"] and np.array_equal(d["zb"], 2.0 * d["rank"]) and np.all(d["zb"] == np.round(d["zb"]))
        assert all(p["delta"] == 0.0 and p["margin"] == math.inf for p in c["parts"].values())
        assert c["ess_bulk"] == c["ess"]                                     # rho = 1 at every lag, whatever the values
    assert not want["columns"][2]["derived"]["flat"]


def test_truncation_in_a_derived_pass_reaches_the_flag():
    x, kw, want = cases.case("max_lag_hit")
    assert np.all(want["flag"] == sorc.FLAG_TRUNCATED)
    assert all(p["col"]["flag"] == sorc.FLAG_TRUNCATED for c in want["columns"] for p in c["parts"].values())


@pytest.mark.parametrize("name", list(cases.CASES))
def test_every_derived_column_of_every_fixed_case_has_a_safe_decision_margin(name):
    """>= 1e-9 and above twice its rho bound (the bound with the input error for zb and zf): the device, whose rho values are
    within the bound of the checker's, then takes the checker's decisions."""
    _x, _kw, want = cases.case(name)
    least = math.inf
    for c in want["columns"]:
        assert c["margin"] >= cases.MIN_MARGIN
        for which, p in c["parts"].items():
            assert p["margin"] >= cases.MIN_MARGIN and p["margin"] > 2 * p["rho_bound"], (name, which, p["margin"], p["rho_bound"])
            least = min(least, p["margin"])
    print(f"[summary-bound] {name}: least margin of a derived column {least:.3g}")
    assert want["margin_ok"].all()
