"""CPU checks of the oracle of the per-cluster evidence unit (tests/_contrib_oracle.py) against the contract of
include/sbe_contrib.h: the sums against 50-digit arithmetic, the rows against exact rationals, the dyadic hand case, the skip rules
by construction, and the host arithmetic of sbayes_amd/contribution.py's result: gain, rank() and the tables."""
import math
from fractions import Fraction

import mpmath
import numpy as np
import pytest

from sbayes_amd import contribution
from tests import _contrib_cases as cases
from tests import _contrib_oracle as orc
from tests import _predict_oracle as predict_orc

NA = orc.NA


def _within_a_quarter(want, label):
    """The oracle's sums against reference_sums(), in units of the device band; +inf by class."""
    mpmath.mp.dps = 50
    exact_aff, exact_gain = orc.reference_sums(want)
    (aff_terms, aff_mag), (gain_terms, gain_mag) = orc.terms_and_magnitudes(want)
    worst = 0.0
    for got, exact, terms, mag in ((want["affinity"], exact_aff, aff_terms, aff_mag), (want["gain_feature"], exact_gain, gain_terms, gain_mag)):
        for idx in np.ndindex(got.shape):
            ref = exact[idx[0]][idx[1]][idx[2]]
            if ref == mpmath.inf:
                assert got[idx] == math.inf
                continue
            band = orc.band(int(terms[idx]), float(mag[idx]))
            err = abs(mpmath.mpf(float(got[idx])) - ref)
            assert err <= band / 4, (label, idx, float(err), band)
            worst = max(worst, float(err / band) if band else 0.0)
    print(f"{label}: worst error of the oracle's sums {worst:.3g} of the device band")
    return worst


@pytest.mark.parametrize("shape", cases.SHAPES, ids=str)
def test_the_oracle_lies_within_a_quarter_of_the_band_of_50_digits_on_the_seeded_cases(shape):
    _case, want = cases.synthetic(shape)
    _within_a_quarter(want, str(shape))


def test_the_oracle_lies_within_a_quarter_of_the_band_of_50_digits_on_the_other_cases():
    for label, case in (("hand", cases.hand()[0]), ("no mass outside", cases.no_mass_outside()[0]), ("without a group", cases.without_a_group())):
        _within_a_quarter(orc.evaluate(**case), label)
    for r in (0, 1):                                                          # the recorded runs: their first two samples
        want = cases.recorded_oracle(r)
        _within_a_quarter({k: (v[:2] if isinstance(v, np.ndarray) else v) for k, v in want.items()}, f"run {r}")


def test_the_rows_are_the_exact_ones_on_the_dyadic_case_and_the_identity_holds():
    """exp(-d) (1 - w1_0) = 1 - w1_0 theta_0[k,f,x] / m_k in rationals, with exp(-d) = m0 / m_k: the strict form of "m_k of a
    member is the posterior predictive's m[x]".  On the dyadic case nothing rounds, so the float64 rows are the rationals."""
    case, want = cases.hand()
    got = orc.evaluate(**case)
    exact = orc.exact_rows(**case)
    assert len(exact) == 2 * 2 * 5                                            # samples x clusters x cells with a code
    for (t, k, n, f), (mk, m0, w10, theta) in exact.items():
        assert Fraction(float(got["m"][t, k, n, f])) == mk and Fraction(float(got["m0"][t, n, f])) == m0
        assert m0 / mk * (1 - w10) == 1 - w10 * theta / mk
    assert got["m"][0].tolist() == want["m"] and got["m0"][0].tolist() == want["m0"]
    # on a seeded case the identity holds for the exact rows, and the float64 rows are within their roundings of them
    case, got = cases.synthetic(cases.SHAPES[1])
    C = case["weights"].shape[2]
    for (t, k, n, f), (mk, m0, w10, theta) in orc.exact_rows(**case).items():
        assert m0 / mk * (1 - w10) == 1 - w10 * theta / mk
        assert abs(Fraction(float(got["m"][t, k, n, f])) - mk) <= predict_orc.gamma(2 * C) * mk
        assert abs(Fraction(float(got["m0"][t, n, f])) - m0) <= predict_orc.gamma(2 * C) * m0


def test_a_members_row_is_the_posterior_predictives_bit_for_bit():
    """m_k of a member of k and m0 of an object in no cluster are the posterior predictive's m[x] (its lik row is float32(m[x]))."""
    for shape in cases.SHAPES[:4]:
        case, got = cases.synthetic(shape)
        T, K, N = case["clusters"].shape
        F = case["weights"].shape[1]
        _sums, lik = predict_orc.run(**case)
        lik = lik.reshape(T, N, F)
        formed = (case["codes"] != NA) & (case["groups"] != NA).any(axis=0)[:, None]   # (the seeded weights are all positive)
        assert formed.any()
        for t in range(T):
            ids, _ = predict_orc.cluster_ids(case["clusters"][t])
            for n in range(N):
                row = got["m"][t, ids[n], n] if ids[n] >= 0 else got["m0"][t, n]
                assert np.array_equal(row.astype(np.float32)[formed[n]], lik[t, n][formed[n]]), (shape, t, n)


def test_the_hand_case():
    case, want = cases.hand()
    got = orc.evaluate(**case)
    assert got["affinity"].tolist() == want["affinity"] and got["gain_feature"].tolist() == want["gain_feature"]
    assert got["n_skipped"] == 0 and orc.rank(got["gain_feature"]) == want["rank"]
    assert got["d"][0, 0, 1, 0] == 0.0 and not np.signbit(got["d"][0, 0, 1, 0]) and (got["d"] < 0).sum() == 4   # theta_k[x] = m0: d = +0.0 exactly
    assert (got["d"][:, :, :, 1] == 0.0).all() and got["counted"][:, :, :2, 1].all()                    # w[f,0] = 0: d = 0 for every k, counted


def test_the_skip_rules_by_construction():
    # m0 = 0 with m_k > 0 is +inf in both sums; m_k = 0 is skipped
    case, want = cases.no_mass_outside()
    got = orc.evaluate(**case)
    assert got["affinity"].tolist() == want["affinity"] and got["gain_feature"].tolist() == want["gain_feature"] and got["n_skipped"] == want["n_skipped"]
    # an object without a group: exactly its cells with a code are skipped, for every k
    case = cases.without_a_group()
    got = orc.evaluate(**case)
    T, K, _N = case["clusters"].shape
    observed = case["codes"] != NA
    assert not got["counted"][:, :, [1, 3]].any() and got["counted"][:, :, [0, 2]].all(axis=(0, 1))[observed[[0, 2]]].all()
    assert got["n_skipped"] == T * K * int(observed[[1, 3]].sum()) and (got["affinity"][:, :, [1, 3]] == 0.0).all()
    assert not np.signbit(got["affinity"][:, :, [1, 3]]).any()
    # C = 1: no confounder applies anywhere
    case, got = cases.synthetic(cases.SHAPES[-1])
    T, K, _N = case["clusters"].shape
    assert got["n_skipped"] == T * K * int((case["codes"] != NA).sum()) and not got["counted"].any()
    for name in ("affinity", "gain_feature"):
        assert (got[name] == 0.0).all() and not np.signbit(got[name]).any()
    # NA cells are not counted: a case without any code skips nothing
    blank = dict(case, codes=np.full_like(case["codes"], NA))
    assert orc.evaluate(**blank)["n_skipped"] == 0


def _result(got, burn=0):
    return contribution.ContributionResult(affinity=got["affinity"][burn:], gain_feature=got["gain_feature"][burn:], member=got["member"][burn:],
                                           n_samples=got["affinity"].shape[0] - burn, n_skipped=got["n_skipped"])


def test_gain_is_the_exactly_rounded_sum_and_rank_breaks_ties_to_the_lower_index():
    case, got = cases.synthetic(cases.SHAPES[3])
    res = _result(got)
    gain = res.gain
    assert gain.shape == (3, 4)
    for t in range(3):
        for k in range(4):
            exact = sum((Fraction(float(v)) for v in got["gain_feature"][t, k]), Fraction(0))
            assert gain[t, k] == float(exact)                                 # (Fraction -> float rounds to nearest even, as fsum does)
            assert gain[t, k] == math.fsum(got["gain_feature"][t, k][::-1])  # the order does not matter
    assert res.rank() == orc.rank(got["gain_feature"]) == sorted(range(4), key=lambda k: (-gain.mean(axis=0)[k], k))
    # ties, and an infinite gain
    tied = contribution.ContributionResult(affinity=np.zeros((2, 4, 1)), member=np.zeros((2, 4, 1), dtype=bool), n_samples=2, n_skipped=0,
                                           gain_feature=np.array([[[1.0, 2.0], [3.0, 0.0], [0.5, 0.5], [4.0, 0.0]],
                                                                  [[1.0, 2.0], [0.0, 3.0], [0.5, 0.5], [0.0, 4.0]]]))
    assert tied.gain.tolist() == [[3.0, 3.0, 1.0, 4.0]] * 2 and tied.rank() == [3, 0, 1, 2]
    tied.gain_feature[1, 2, 0] = math.inf
    assert tied.gain[1, 2] == math.inf and tied.rank() == [2, 3, 0, 1]
    case, want = cases.hand()
    assert _result(orc.evaluate(**case)).rank() == want["rank"]


def test_the_tables(tmp_path):
    case, got = cases.synthetic(cases.SHAPES[1])                              # 17 x 7, K = 3, T = 3
    res = _result(got)
    header, rows = res.feature_table(1)
    assert header == ["feature", "gain_mean", "gain_sd", "share_positive"] and len(rows) == 7
    mean = got["gain_feature"][:, 1].mean(axis=0)
    order = sorted(range(7), key=lambda i: (-mean[i], i))
    assert [r[0] for r in rows] == [f"F{i + 1}" for i in order] and [r[1] for r in rows] == [float(mean[i]) for i in order]
    assert [r[2] for r in rows] == [float(got["gain_feature"][:, 1, i].std()) for i in order]
    assert [r[3] for r in rows] == [float((got["gain_feature"][:, 1, i] > 0).mean()) for i in order]
    names = [f"feat{i}" for i in range(7)]
    assert res.top_features(1, 3, names) == res.feature_table(1, names)[1][:3] and res.top_features(1)[0][0] == f"F{order[0] + 1}"
    with pytest.raises(ValueError, match="6 names for 7 features"):
        res.feature_table(0, names[:-1])
    with pytest.raises(ValueError, match=r"cluster 3 out of range \[0, 3\)"):
        res.feature_table(3)
    header, rows = res.membership_table()
    assert header == ["cluster", "object", "member_share", "affinity_mean", "share_affinity_positive"] and len(rows) == 3 * 17
    k, n = 2, 5
    row = rows[k * 17 + n]
    assert row[:2] == [2, "5"] and row[2] == float(got["member"][:, k, n].mean()) and row[3] == float(got["affinity"][:, k, n].mean())
    assert row[4] == float((got["affinity"][:, k, n] > 0).mean())
    assert sum(r[2] for r in rows) == pytest.approx(got["member"].sum() / 3)
    with pytest.raises(ValueError, match="2 names for 17 objects"):
        res.membership_table(["a", "b"])
    header, rows = res.cluster_table()
    assert header == ["cluster", "gain_mean", "gain_sd", "size_mean"] and [r[0] for r in rows] == res.rank()
    assert [r[3] for r in rows] == [float(got["member"][:, k].sum(axis=1).mean()) for k in res.rank()]
    paths = res.write_tables(tmp_path / "out", names)
    assert [p.name for p in paths] == ["clusters.tsv", "membership.tsv", "features_a0.tsv", "features_a1.tsv", "features_a2.tsv"]
    lines = (tmp_path / "out" / "features_a1.tsv").read_text().splitlines()
    assert lines[0].split("\t") == ["feature", "gain_mean", "gain_sd", "share_positive"] and len(lines) == 8
    assert lines[1].split("\t")[0] == f"feat{order[0]}" and float(lines[1].split("\t")[1]) == pytest.approx(mean[order[0]], rel=1e-9)
    assert len((tmp_path / "out" / "membership.tsv").read_text().splitlines()) == 1 + 3 * 17
