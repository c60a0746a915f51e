"""The diagnostics checker (tests/_diag_oracle.py) against known answers, the decision margins of the fixed cases the GPU
tests use, and the readers of the reference's files (sbayes_amd.diag.read_stats / read_clusters)."""
import math

import numpy as np
import pytest

from tests import _diag_cases as cases
from tests import _diag_oracle as orc
from sbayes_amd import diag


@pytest.mark.parametrize("phi", [0.0, 0.5, 0.9])
def test_ar1_tau_is_the_theoretical_one_within_the_spread_of_the_columns(phi):
    """tau = (1 + phi) / (1 - phi) for AR(1).  12 seeded columns of 4 x 4000: the mean of their estimates lies within four
    standard errors (their own spread / sqrt(12)) plus the estimator's small-sample bias (2 %) of it."""
    x = orc.ar1(np.random.default_rng(100 + int(10 * phi)), phi, 4, 4000, 12)
    res = orc.diagnose(list(x), burnin=0.0, split=False)
    tau = 16000 / res["ess"]
    want = (1 + phi) / (1 - phi)
    assert abs(tau.mean() - want) <= 4 * tau.std(ddof=1) / math.sqrt(12) + 0.02 * want, (tau.mean(), want)
    assert np.all(np.abs(res["rhat"] - 1) < 0.01)
    assert np.allclose(res["mcse_mean"], res["sd"] / np.sqrt(res["ess"]), rtol=1e-15)


def test_iid_columns_have_about_one_draw_per_draw_and_the_pooled_moments():
    x = orc.ar1(np.random.default_rng(7), 0.0, 3, 2000, 6, loc=10.0, scale=2.0)
    res = orc.diagnose(list(x), burnin=0.1, split=True)
    assert (res["n_chains"], res["n_draws"]) == (6, 900)
    kept = np.stack([c[200:] for c in x])
    assert np.allclose(res["mean"], kept.mean(axis=(0, 1)), rtol=1e-13)
    assert np.allclose(res["sd"], kept.reshape(-1, 6).std(axis=0, ddof=1), rtol=1e-13)
    assert np.all(np.abs(res["ess"] / 5400 - 1) < 0.15)


def test_the_floor_binds_for_anticorrelated_draws():
    x, kw, res = cases.case("neg05_2x500")
    assert res["ess"][0] == 1000 / (1 / math.log10(1000)) == 1000 * math.log10(1000)


def test_constant_and_non_finite_columns_are_flagged_and_do_not_fail():
    x, kw, res = cases.case("mixed")
    assert res["flag"].tolist() == [0, 1, 2, 0, 2, 0, 0, 0]
    assert res["mean"][1] == 0.25 and res["sd"][1] == 0 and res["ess"][1] == 4 * 54 and math.isnan(res["rhat"][1]) and res["mcse_mean"][1] == 0
    for j in (2, 4):
        assert all(math.isnan(res[k][j]) for k in orc.FIELDS) and res["n_lags"][j] == 0
    assert np.isfinite(res["ess"][[0, 3, 5, 6, 7]]).all()


def test_split_drops_the_middle_draw_of_an_odd_length_and_burnin_follows_drop_burnin():
    x = np.arange(2 * 21 * 1, dtype=np.float64).reshape(2, 21, 1)
    parts, cut = orc.prepare(list(x), burnin=0.1, split=True)          # int(0.1 * 21) = 2 dropped, 19 left, halves of 9
    assert parts.shape == (4, 9, 1) and cut == (0, 0)
    assert parts[0, :, 0].tolist() == list(range(2, 11)) and parts[1, :, 0].tolist() == list(range(12, 21))
    parts, cut = orc.prepare([x[0], x[1][:15]], burnin=0.0, split=False)
    assert parts.shape == (2, 15, 1) and cut == (6, 0)
    assert diag._plan([21, 21], 0.1, True) == ([2, 2], (0, 0), 4, 9)


@pytest.mark.parametrize("name,n_lags", [("tiny_1x4", 1), ("tiny_1x5", 3), ("tiny_2x6", 3)])
def test_the_smallest_shapes_have_defined_values(name, n_lags):
    x, kw, res = cases.case(name)
    assert np.isfinite(res["ess"]).all() and np.isfinite(res["rhat"]).all() and (res["ess"] > 0).all()
    assert res["n_lags"].tolist() == [n_lags] * 3
    if name == "tiny_1x4":                                                  # no pair of lags fits: tau is the floor
        assert np.all(res["ess"] == 4 * math.log10(4))


def test_max_lag_truncates_and_says_so():
    hit, free = cases.case("max_lag_hit")[2], cases.case("max_lag_not_hit")[2]
    assert np.all(hit["flag"] == orc.FLAG_TRUNCATED) and np.all(hit["n_lags"] == 9)       # pairs up to lags (8, 9) <= 10
    assert np.all(free["flag"] == 0) and np.array_equal(free["n_lags"], cases.case("ar09_4x1000")[2]["n_lags"])
    assert np.all(hit["ess"] > free["ess"])


@pytest.mark.parametrize("name", list(cases.CASES))
def test_every_fixed_case_decides_with_a_margin(name):
    """At a margin of 1e-9 the discrete decisions (stop, keep, monotone replacement) cannot flip under rounding: the
    checker's own bound on a device's rho is orders below it."""
    x, kw, res = cases.case(name)
    assert res["margin"].min() >= cases.MIN_MARGIN
    assert 2 * res["rho_bound"].max() < cases.MIN_MARGIN
    for k in orc.FIELDS:
        b = res["bound"][k]
        assert np.all(b >= 0) and np.all(np.isfinite(b))
    varying = res["flag"] == 0
    assert np.all(res["bound"]["ess"][varying] < 1e-8 * res["ess"][varying])


def test_bounds_scale_with_the_offset_of_a_column():
    """A column far from zero loses digits in its mean: the bound on the mean grows with the offset, the bound on ess
    hardly does (the mean is taken in two steps)."""
    base = orc.ar1(np.random.default_rng(5), 0.5, 2, 200, 1)
    near, far = orc.diagnose(list(base), 0.0, False), orc.diagnose(list(base + 1e6), 0.0, False)
    assert far["bound"]["mean"][0] > 1e3 * near["bound"]["mean"][0]
    assert far["bound"]["ess"][0] < 10 * near["bound"]["ess"][0] + 1e-6


def test_read_stats_keeps_the_numeric_columns_in_file_order(tmp_path):
    p = tmp_path / "stats_K2_0.txt"
    p.write_text("Sample\tposterior\tw_areal_f1\tsample_id\n0\t-10.5\t0.25\t0\n100\t-9.25\t0.5\t0\n200\t-9\t1e-3\t0\n")
    names, rows = diag.read_stats(p)
    assert names == ["Sample", "posterior", "w_areal_f1", "sample_id"]
    assert rows.dtype == np.float64 and rows.tolist() == [[0, -10.5, 0.25, 0], [100, -9.25, 0.5, 0], [200, -9, 1e-3, 0]]
    q = tmp_path / "stats_with_text.txt"
    q.write_text("Sample\tlabel\tx\n0\ta\t1.5\n1\tb\tnan\n")
    names, rows = diag.read_stats(q)
    assert names == ["Sample", "x"] and rows[:, 0].tolist() == [0, 1] and rows[0, 1] == 1.5 and math.isnan(rows[1, 1])


def test_read_clusters_gives_indicator_columns(tmp_path):
    p = tmp_path / "clusters_K2_0.txt"
    p.write_text("0110\t1000\n0100\t1001\n\n")
    names, rows = diag.read_clusters(p)
    assert names == ["a0_0", "a0_1", "a0_2", "a0_3", "a1_0", "a1_1", "a1_2", "a1_3"]
    assert rows.dtype == np.float64 and rows.tolist() == [[0, 1, 1, 0, 1, 0, 0, 0], [0, 1, 0, 0, 1, 0, 0, 1]]
    p.write_text("0110\t100\n")
    with pytest.raises(ValueError, match="2 clusters of 4 objects"):
        diag.read_clusters(p)
    p.write_text("0120\t1000\n")
    with pytest.raises(ValueError, match="other than 0 and 1"):
        diag.read_clusters(p)


def test_runs_are_joined_on_their_common_columns(tmp_path):
    a, b = tmp_path / "s0.txt", tmp_path / "s1.txt"
    a.write_text("Sample\tx\ty\tsample_id\n0\t1\t2\t0\n1\t3\t4\t0\n")
    b.write_text("Sample\ty\tz\tx\tsample_id\n0\t5\t0\t6\t1\n1\t7\t0\t8\t1\n")
    ca, cb = tmp_path / "c0.txt", tmp_path / "c1.txt"
    ca.write_text("01\n11\n")
    cb.write_text("10\n00\n")
    names, runs = diag._load_runs([a, b], [ca, cb])
    assert names == ["x", "y", "a0_0", "a0_1"]
    assert runs[0].tolist() == [[1, 2, 0, 1], [3, 4, 1, 1]] and runs[1].tolist() == [[6, 5, 1, 0], [8, 7, 0, 0]]
    with pytest.raises(ValueError, match="1 cluster files for 2 stats files"):
        diag._load_runs([a, b], [ca])
