"""CPU checks of the leave-one-out predictive's checker (tests/_loopred_oracle.py) and of its cases (tests/_loopred_cases.py): the
oracle against exact rationals where no column is smoothed, the identities its results satisfy, the tie rule, and that the cases
are what they claim to be."""
from fractions import Fraction

import numpy as np
import pytest

from tests import _elpd_oracle as eo
from tests import _loopred_cases as cases
from tests import _loopred_oracle as orc
from tests import _predict_oracle as po

ALL = [("T", T) for T in cases.BY_SAMPLES] + [("smallest", None), ("duplicated", None)]


def _get(kind, T):
    return cases.synthetic(T) if kind == "T" else getattr(cases, kind)()


def test_the_mixture_rows_are_the_posterior_predictive_oracles_bit_for_bit():
    for kind, T in ALL:
        case, want = _get(kind, T)
        sums, lik = po.run(**case)
        pred = np.zeros_like(sums.pred)
        for m in want["m"]:
            pred = pred + m
        assert np.array_equal(pred, sums.pred)
        obs = case["codes"] != orc.NA
        assert np.array_equal(lik[:, obs.ravel()], want["lik"]) and (lik[:, ~obs.ravel()] == 1).all()


def test_the_hand_case():
    case, want = cases.hand()
    got = orc.run(**case)
    assert got["lik"].tolist() == want["lik"] and np.isinf(got["k"]).all()
    assert np.allclose(got["w"], want["w"], rtol=1e-15, atol=0) and np.allclose(got["p_loo"], want["p_loo"], rtol=4e-16, atol=0)
    assert got["n_eff"][0] == pytest.approx(want["n_eff"], rel=1e-15) and got["loo_i"][0] == pytest.approx(np.log(7 / 18), rel=1e-15)


@pytest.mark.parametrize("T", [2, 20])
def test_raw_weights_against_exact_rationals(T):
    """T <= 20: the tail has at most four elements, nothing is smoothed, and the weights are the normalised 1 / lik exactly."""
    case, got = cases.synthetic(T)
    assert np.isinf(got["k"]).all()
    w, p, harmonic = orc.exact_raw(**case)
    M = got["lik"].shape[1]
    assert len(harmonic) == M
    for j in range(M):
        for t in range(T):
            assert abs(Fraction(float(got["w"][t, j])) - w[t][j]) <= 1e-14 * w[t][j]
        assert abs(Fraction(float(np.exp(got["loo_i"][j]))) - harmonic[j]) <= 1e-14 * harmonic[j]
        assert abs(Fraction(float(got["n_eff"][j])) - 1 / sum(w[t][j] ** 2 for t in range(T))) <= 1e-13 * T
    N, F, S = got["p_loo"].shape
    for n in range(N):
        for f in range(F):
            for s in range(S):
                assert abs(Fraction(float(got["p_loo"][n, f, s])) - p[n][f][s]) <= 1e-14 * p[n][f][s]
    # (the bound of the GPU test is no tighter than what the oracle itself keeps against the exact value)
    exact = np.array([[[float(v) for v in fs] for fs in ns] for ns in p])
    assert (np.abs(got["p_loo"] - exact) <= orc.probs_bound(got["p_loo"], got["w"], case["codes"], T, case["weights"].shape[2])).all()


@pytest.mark.parametrize("kind,T", ALL)
def test_the_identities_of_a_result(kind, T):
    case, got = _get(kind, T)
    obs = case["codes"] != orc.NA
    n_samples = got["lik"].shape[0]
    assert np.allclose(got["w"].sum(axis=0), 1.0, rtol=0, atol=1e-13) and (got["w"] > 0).all()
    # sum_s probs = sum_t w_t sum_s m_t[s]
    w_cell = np.zeros((n_samples,) + obs.shape)
    w_cell[:, obs] = got["w"]
    assert np.allclose(got["p_loo"].sum(axis=2), (w_cell * got["m"].sum(axis=3)).sum(axis=0), rtol=1e-13, atol=0)
    assert not got["p_loo"][~obs].any()
    # probs[x] = exp(loo_i), but for the float32 rounding of the rows
    x = np.where(obs, case["codes"], 0).astype(np.int64)
    p_obs = np.take_along_axis(got["p_loo"], x[..., None], axis=2)[..., 0][obs]
    assert np.allclose(p_obs, np.exp(got["loo_i"]), rtol=2.0 ** -23, atol=0)
    assert ((got["n_eff"] >= 1 - 1e-12) & (got["n_eff"] <= n_samples * (1 + 1e-12))).all()


def test_a_constant_column_has_uniform_weights():
    case, _got = cases.synthetic(64)
    same = {k: (np.ascontiguousarray(np.repeat(v[:1], 64, axis=0)) if k in ("clusters", "weights", "tables") else v) for k, v in case.items()}
    got = orc.run(**same)
    assert (got["lik"] == got["lik"][0]).all() and np.isinf(got["k"]).all()
    assert np.allclose(got["w"], 1 / 64, rtol=1e-15, atol=0) and np.allclose(got["n_eff"], 64, rtol=1e-14, atol=0)
    assert np.allclose(got["p_loo"], got["m"][0] * (case["codes"] != orc.NA)[..., None], rtol=1e-14, atol=0)


def test_the_tie_rule_on_duplicated_samples():
    """Of two equal samples in the tail the earlier one takes the lower position in ascending x, so the smaller smoothed weight."""
    case, got = cases.duplicated()
    lik, w = got["lik"], got["w"]
    assert np.array_equal(lik[0::2], lik[1::2]) and np.isfinite(got["k"]).all()
    assert (w[0::2] <= w[1::2]).all()
    for j in range(lik.shape[1]):
        assert (w[0::2, j] < w[1::2, j]).any()
        # the statement itself: positions by (x ascending, sample ascending); the smoothed values ascend along them
        x = -np.log(lik[:, j].astype(np.float64))
        (tail,) = np.where(x > np.sort(x)[64 - 13 - 1])               # (T = 64: a tail of at most ceil(12.8) = 13)
        along = tail[np.lexsort((tail, x[tail]))]
        assert len(tail) > 4 and (np.diff(w[along, j]) >= 0).all()


def test_the_cases_are_what_they_claim_to_be():
    for kind, T in ALL:
        case, got = _get(kind, T)
        assert po.first_offender(case["clusters"], case["weights"], case["tables"]) is None
        assert orc.first_bad(got["lik"]) is None and orc.away_from_edges(got["lik"]), (kind, T)
        assert not np.isnan(got["k"]).any() and np.isfinite(got["loo_i"]).all()
    for T, (_seed, N, F, S, C, K, tile) in cases.BY_SAMPLES.items():
        case, got = cases.synthetic(T)
        assert 2 <= N <= 9 and 1 <= F <= 17 and 2 <= S <= 5 and 1 <= C <= 3 and 1 <= K <= 3 and (F + tile - 1) // tile >= 2
        codes = case["codes"]
        assert (codes[:, F - 1] == orc.NA).all() and (codes[N - 1] == orc.NA).all() and (codes[:, :F - 1] == orc.NA).any() and (codes != orc.NA).any()
        assert not case["clusters"][:, :, N - 1].any() and (case["groups"][:, N - 1] == orc.NA).all()
        if C >= 2:
            assert not case["clusters"][:, :, 0].any() and (case["groups"][:, 1] == orc.NA).all()
        tail = int(np.ceil(min(0.2 * T, 3 * np.sqrt(T))))
        assert np.isinf(got["k"]).all() == (tail <= 4)
    assert int(np.ceil(0.2 * 20)) == 4 and int(np.ceil(0.2 * 21)) == 5
    assert np.isfinite(cases.synthetic(21)[1]["k"]).any() and np.isfinite(cases.synthetic(300)[1]["k"]).all()


def test_branch_margins_see_the_edges():
    rng = np.random.default_rng(5)
    col = np.exp(rng.normal(-1.5, 0.8, 200)).astype(np.float32)
    g = orc.branch_margins(col)
    assert g["tail_len"] == 40 and np.isfinite(g["k"]) and g["k"] == eo.column_stats(col)[1] and g["sigma"] > 0
    assert orc.branch_margins(col[:20])["tail_len"] == 4 and np.isinf(orc.branch_margins(col[:20])["prune"])
    assert orc.first_bad(np.array([[0.5, 0.25], [0.5, 0.0], [np.inf, 0.5]], dtype=np.float32)) == (0, 2)
