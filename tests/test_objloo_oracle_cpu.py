"""CPU checks of the checker of the leave-one-object-out unit (tests/_objloo_oracle.py) and of the cases the GPU tests use
(tests/_objloo_cases.py): against exact rationals on small cases, against the posterior predictive's rows, the one-hot prior, the
fixed tree, the figures of the two recorded runs, and the seeds (every column's Pareto k is well conditioned)."""
import math
from fractions import Fraction

import numpy as np
import pytest

from sbayes_amd import objloo
from tests import _contrib_oracle as co
from tests import _loopred_cases as loopred_cases
from tests import _loopred_oracle as lo
from tests import _objloo_cases as cases
from tests import _objloo_oracle as orc
from tests import _ppc_oracle as ppc_orc
from tests import _predict_oracle as po
from tests import _psens_oracle as ps


def test_the_hand_case_is_what_the_docstring_works_out():
    case, want = cases.hand()
    got = orc.run(**case)
    assert np.allclose(np.exp(got["L"]), want["expL"], rtol=1e-15, atol=0) and np.allclose(np.exp(got["Cnd"]), want["expCnd"], rtol=1e-15, atol=0)
    assert got["L"][:, 1].tolist() == [0.0, 0.0] and got["H"][:, 1].tolist() == [[0.0, 0.0], [0.0, 0.0]]
    for name in ("w", "n_eff", "membership", "p_loo"):
        assert np.allclose(got[name], want[name], rtol=1e-14, atol=0), name
    for name in ("loo_i", "lppd_i", "loo_cond_i", "lppd_cond_i"):
        assert np.allclose(got[name], want[name], rtol=1e-14, atol=1e-16), name
    assert np.isinf(got["k_i"]).all() and np.isinf(got["k_cond_i"]).all() and got["z"].tolist() == [[1, 0], [0, 0]]


@pytest.mark.parametrize("name", ["F1", "F65", "hand", 5])
def test_the_rows_against_exact_rationals(name):
    """exp(H), exp(L) and exp(Cnd) against the products of the exact m_j over the observed cells and their prior mixture.  Every m
    is within gamma(2 C) of exact and a log within an ulp, so |H - log exact| <= n_cells gamma(2 C + 2) + the band of the sum; L adds
    its own bound (the checker's docstring) and the rounding of the prior's log, which l_bound holds."""
    if name == "hand":
        case, prior = cases.hand()[0], None
    else:
        case, prior, _run = cases.by_shape(name) if isinstance(name, str) else cases.synthetic(name)
    T, K, N = case["clusters"].shape
    C = case["weights"].shape[2]
    prior = orc.uniform_prior(T, N, K) if prior is None else prior
    H, z, mag = orc.hypotheses(**case)
    a, L, Cnd = orc.mix(H, prior, z)
    eH, eL, eC = orc.exact_marginal(**case, prior=prior)
    n_cells = (case["codes"] != orc.NA).sum(axis=1)

    def log_of(q):
        return math.log(float(q)) if q > 0 else -math.inf      # (the quotient correctly rounded: an ulp of its log at most)
    for t in range(T):
        for n in range(N):
            bound = n_cells[n] * po.gamma(2 * C + 2) + co.band(n_cells[n], mag[t, n].max()) + 2.0 ** -52
            for j in range(K + 1):
                assert abs(H[t, n, j] - log_of(eH[t][n][j])) <= bound, (t, n, j)
            assert abs(Cnd[t, n] - log_of(eC[t][n])) <= bound
            assert abs(L[t, n] - log_of(eL[t][n])) <= bound + orc.l_bound(H[t, n], prior[t, n]) + 2.0 ** -52 * abs(L[t, n]), (t, n)


@pytest.mark.parametrize("T", [5, 21])
def test_cnd_is_the_sum_of_the_logs_of_the_posterior_predictives_rows(T):
    case, _prior, run = cases.synthetic(T)
    m = lo.mixture(**case)                                       # [T,N,F,S] in _predict_oracle's order, under the logged membership
    obs = case["codes"] != orc.NA
    x = np.where(obs, case["codes"], 0).astype(np.int64)
    for t in range(T):
        mx = np.take_along_axis(m[t], x[..., None], axis=2)[..., 0]
        want = ppc_orc.sum_over_features(np.where(obs, co.log_of(np.where(obs, mx, 1.0)), 0.0))
        assert np.array_equal(run["Cnd"][t], want)


def test_the_rows_of_every_state_are_the_evidence_units_rows_at_the_observed_state():
    case, _prior, _run = cases.synthetic(21)
    K = case["clusters"].shape[1]
    obs = case["codes"] != orc.NA
    x = np.where(obs, case["codes"], 0).astype(np.int64)[None, ..., None]
    for t in (0, 7):
        m, m0, formed, _w = co.rows_of_sample(case["codes"], case["groups"], case["n_groups"], K, case["weights"][t], case["tables"][t])
        full = orc.rows_all_states(case["codes"], case["groups"], case["n_groups"], K, case["weights"][t], case["tables"][t])
        at_x = np.take_along_axis(full, np.broadcast_to(x, full.shape[:3] + (1,)), axis=3)[..., 0]
        assert (formed == obs).all() and np.array_equal(at_x[0][obs], m0[obs]) and np.array_equal(at_x[1:][:, obs], m[:, obs])
        # the last object has no confounder and no code: "no cluster" predicts nothing for it, the clusters predict their rows
        assert not full[0, -1].any() and np.array_equal(full[1:, -1], case["tables"][t][:K])
        assert np.allclose(full[:, :-1].sum(axis=3), 1.0, rtol=0, atol=1e-12)


@pytest.mark.parametrize("name", ["F63", "F129"])
def test_a_one_hot_prior_at_the_logged_membership_gives_the_conditional_column_bit_for_bit(name):
    case, _prior, _run = cases.by_shape(name)
    H, z, _mag = orc.hypotheses(**case)
    onehot = (np.arange(H.shape[2])[None, None, :] == z[..., None]).astype(np.float64)
    a, L, Cnd = orc.mix(H, onehot, z)
    assert np.array_equal(L, Cnd) and np.isfinite(L).all() and (np.isinf(a).sum(axis=2) == H.shape[2] - 1).all()


def test_the_fixed_tree_is_a_sum():
    rng = np.random.default_rng(5)
    for n in (1, 2, 63, 64, 255, 256, 257, 1000):
        v = rng.random(n)
        assert abs(orc.block_tree_sum(v) - math.fsum(v)) <= po.gamma(n) * math.fsum(v)
    assert orc.block_tree_sum([0.5, 0.25]) == 0.75 and orc.block_tree_sum(np.ones(300)) == 300.0
    # thread i adds the values i, i + 256, .. first: two half-ulps meet in thread 1 and survive, or meet 1.0 one by one and do not
    v = np.zeros(258)
    v[0], v[1], v[257] = 1.0, 2.0 ** -53, 2.0 ** -53
    assert orc.block_tree_sum(v) == 1.0 + 2.0 ** -52
    v[257], v[256] = 0.0, 2.0 ** -53
    assert orc.block_tree_sum(v) == 1.0


@pytest.mark.parametrize("r,by_cell,cond,marg,bad_cond,bad_marg,median_cond,median_marg",
                         [(0, -2045.2, -2048.5, -2070.7, 17, 8, 0.48, 0.40), (1, -2030.1, -2034.8, -2067.6, 20, 12, 0.51, 0.40)])
def test_the_recorded_runs_reproduce_the_worked_figures(r, by_cell, cond, marg, bad_cond, bad_marg, median_cond, median_marg):
    """100 objects x 36 features, K = 3, 54 samples after burn-in, a uniform prior: the ELPD by cell (the leave-one-out predictive's),
    the object-level ELPD under the logged membership and with the membership integrated out, and the objects with k > 0.7."""
    run = cases.recorded_oracle(r)
    assert run["L"].shape == (54, 100) and run["H"].shape == (54, 100, 4)
    assert round(float(loopred_cases.recorded_oracle(r)["loo_i"].sum()), 1) == by_cell
    assert round(float(run["loo_cond_i"].sum()), 1) == cond and round(float(run["loo_i"].sum()), 1) == marg
    assert int((run["k_cond_i"] > 0.7).sum()) == bad_cond and int((run["k_i"] > 0.7).sum()) == bad_marg
    assert round(float(np.median(run["k_cond_i"])), 2) == median_cond and round(float(np.median(run["k_i"])), 2) == median_marg
    assert np.allclose(run["membership"].sum(axis=1), 1.0, rtol=0, atol=1e-12) and np.allclose(run["p_loo"].sum(axis=2), 1.0, rtol=0, atol=1e-7)
    assert (run["L"] >= run["Cnd"] + math.log(0.25) - 1e-12).all()          # the marginal holds the logged hypothesis's term
    # every column's k is well conditioned: the bound on the device's k is the project's floor
    tol = np.array([ps.tol_k(ratios) for _label, ratios in cases.all_ratios(run)])
    assert tol.shape == (200,) and (tol >= 1e-10).all() and (tol < 1.01e-10).all()


def _seeded_runs():
    yield from ((f"T={T}", cases.synthetic(T)[2]) for T in cases.BY_SAMPLES)
    yield "duplicated", cases.duplicated()[2]
    yield "long", cases.long_column(objloo.lds_max_samples() + 1)[2]


def test_the_seeds_leave_no_column_whose_k_is_excused():
    """tests/_psens_oracle.tol_k is finite (and near its floor) for every column of both kinds of every seeded case the GPU test
    compares k on; the sample counts cover a tail of at most four values (k = inf) and the first fit."""
    for label, run in _seeded_runs():
        tol = np.array([ps.tol_k(ratios) for _l, ratios in cases.all_ratios(run)])
        assert np.isfinite(tol).all() and (tol < 1e-9).all(), (label, tol.max())
    for T in cases.BY_SAMPLES:
        run = cases.synthetic(T)[2]
        assert np.isinf(run["k_i"]).all() == np.isinf(run["k_cond_i"]).all() == (T <= 20), T
    assert np.isfinite(cases.synthetic(21)[2]["k_i"][:4]).all() and np.isinf(cases.synthetic(21)[2]["k_i"][4])    # (a constant column: no tail)
    dup = cases.duplicated()[2]
    assert np.array_equal(dup["L"][0::2], dup["L"][1::2]) and (dup["w"][0::2] <= dup["w"][1::2]).all()
    assert (dup["w"][0::2] < dup["w"][1::2]).any(axis=0)[:3].all()      # of two equal samples the earlier one sits lower in the tail


def test_the_cases_with_a_hypothesis_of_zero_likelihood():
    for kind, which in (("finite", None), ("conditional", "conditional"), ("marginal", "marginal")):
        case, (n, t) = cases.zero_likelihood(kind)
        assert orc.first_unformed(case["codes"], case["groups"], case["n_groups"], case["clusters"].shape[1], case["weights"], case["tables"]) is None
        H, z, _mag = orc.hypotheses(**case)
        _a, L, Cnd = orc.mix(H, orc.uniform_prior(*H.shape[:2], H.shape[2] - 1), z)
        assert np.isneginf(H[t, n, 0]) and np.isneginf(H[t, n, 1]) and not np.isposinf(H).any() and not np.isnan(H).any()
        assert orc.first_not_finite(L, Cnd) == (None if which is None else (n, t, which))
    # an excluded hypothesis (prior 0) is -inf in a and leaves L finite; excluding them all does not
    H = np.array([[-1.0, -2.0, -3.0]])
    a, L, _c = orc.mix(H, np.array([[0.0, 0.5, 0.5]]), np.array([1]))
    assert np.isneginf(a[0, 0]) and L[0] == pytest.approx(math.log(0.5 * math.exp(-2) + 0.5 * math.exp(-3)), rel=1e-15)
    assert np.isnan(orc.mix(np.array([[-np.inf, -2.0]]), np.array([[1.0, 0.0]]), np.array([1]))[1][0])


def test_an_observed_cell_without_a_confounder_is_found():
    case, _prior, _run = cases.synthetic(5)
    groups = case["groups"].copy()
    groups[:, 2] = orc.NA
    f = int(np.flatnonzero(case["codes"][2] != orc.NA)[0])
    assert orc.first_unformed(case["codes"], groups, case["n_groups"], 2, case["weights"], case["tables"]) == (0, 2, f)
    with pytest.raises(AssertionError, match="no confounder applies"):
        orc.log_rows(case["codes"], groups, case["n_groups"], 2, case["weights"][0], case["tables"][0])


def test_the_bound_on_l_covers_a_perturbed_evaluation():
    """l_bound against L recomputed with every log and exp moved by one ulp either way at random (the device's library differs from
    this one by such steps): the bound holds and is of the order of an ulp of L."""
    case, prior, run = cases.by_shape("F65")
    H, bound = run["H"], orc.l_bound(run["H"], prior)
    assert (bound > 0).all() and (bound < 64 * 2.0 ** -52 * np.maximum(np.abs(run["L"]), 1.0)).all()
    rng = np.random.default_rng(11)

    def moved(v):
        step = rng.integers(-1, 2, size=np.shape(v))
        return np.where(np.isfinite(v) & (v != 0), np.where(step > 0, np.nextafter(v, np.inf), np.where(step < 0, np.nextafter(v, -np.inf), v)), v)
    for _ in range(8):
        with np.errstate(divide="ignore"):
            a = moved(np.log(prior)) + H
        mx = a.max(axis=2)
        total = np.zeros(mx.shape)
        for j in range(a.shape[2]):
            total = total + moved(np.exp(a[..., j] - mx))
        assert (np.abs((mx + moved(np.log(total))) - run["L"]) <= bound).all()


def test_exact_fractions_are_exact():
    case, _want = cases.hand()
    eH, eL, eC = orc.exact_marginal(**case, prior=orc.uniform_prior(2, 2, 1))
    assert eH[0][0] == [Fraction(1, 2), Fraction(3, 8)] and eL[1][0] == Fraction(9, 16) and eC[0][0] == Fraction(3, 8) and eL[0][1] == 1
