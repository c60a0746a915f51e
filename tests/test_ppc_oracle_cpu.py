"""CPU checks of the oracle of the posterior predictive check (tests/_ppc_oracle.py) against the contract of include/sbe_ppc.h:
the hand-worked case, the draw rule on a grid and at its edges, the draws against exact rationals, the deviance sums against
mpmath, skipped cells, the p-value arithmetic and the split of the draw index.  Every case that draws from Philox is also held
to the margin condition the GPU tests rely on: every drawn cell is further than 2^-40 from a cdf step."""
import math
from fractions import Fraction

import mpmath
import numpy as np
import pytest

from sbayes_amd import ppc
from tests import _ppc_cases as cases
from tests import _ppc_oracle as orc

NA = orc.NA


def test_the_hand_case():
    case, uniforms, want = cases.hand()
    assert orc.first_offender(case["clusters"], case["weights"], case["tables"], uniforms) is None
    got = orc.check(uniforms=uniforms, **case)
    assert got["y_rep"].tolist() == want["y_rep"] and got["count_rep"].tolist() == want["count_rep"] and got["n_skipped"] == 0
    assert got["dev_feature"].tolist() == want["dev_feature"] and got["dev_object"].tolist() == want["dev_object"]
    assert got["m"][0, 0, 0].tolist() == [0.375, 0.0, 0.375, 0.25] and got["m"][1, 1, 0].tolist() == [0.0, 0.25, 0.375, 0.375]
    res = ppc.PpcResult(codes=case["codes"], dev_feature=got["dev_feature"], dev_object=got["dev_object"], count_rep=got["count_rep"],
                        count_obs=ppc.count_observed(case["codes"], 4), n_samples=2, n_skipped=0)
    assert res.p_feature.tolist() == [0.25] and res.p_object.tolist() == [0.5, 0.25] and res.p_total == 0.25
    assert res.count_obs.tolist() == [[1, 0, 1, 0]] and res.p_count.tolist() == [[0.0, 0.5, 0.75, 0.75]]


def test_the_draw_rule_on_a_grid():
    case, uniforms = cases.grid()
    got = orc.check(uniforms=uniforms, **case)
    assert [int((got["y_rep"] == s).sum()) for s in range(4)] == [256, 0, 512, 256]
    assert got["count_rep"].sum(axis=(0, 1)).tolist() == [256, 0, 512, 256] and got["n_skipped"] == 0
    assert (np.diff(got["y_rep"].ravel().astype(int)) >= 0).all()          # the draw is monotone in u


def test_a_uniform_on_a_step_goes_to_the_next_state_and_zero_to_the_first_with_mass():
    case, uniforms, want_y = cases.edges()
    got = orc.check(uniforms=uniforms, **case)
    assert got["y_rep"][0].tolist() == want_y
    # no state of zero mass is ever drawn, on any of these edges
    m_y = np.take_along_axis(got["m"], np.where(got["drawn"], got["y_rep"], 0).astype(np.int64)[..., None], axis=3)[..., 0]
    assert (m_y[got["drawn"]] > 0).all()
    # the skipped object, the NA object and the NA feature
    assert got["n_skipped"] == 3 and not got["drawn"][0, 4].any() and not got["drawn"][0, 5].any() and not got["drawn"][0, :, 3].any()
    assert (got["d"][0, :, 4] == 0).all() and (got["dev_object"][0, :, 4] == 0).all() and (got["dev_feature"][0, :, 3] == 0).all()
    assert got["count_rep"][0, 3].tolist() == [0, 0, 0, 0] and got["count_rep"][0].sum() == 15
    # an observed state without mass
    assert got["d"][0, 0, 0, 0] == math.inf and got["dev_feature"][0, 0, 0] == math.inf and np.isfinite(got["dev_feature"][0, 1]).all()
    p = ppc.p_value(got["dev_feature"][:, 1], got["dev_feature"][:, 0])
    assert p[0] == 0.0 and p[3] == 0.5                                      # +inf observed: p = 0; no cells: a tie
    ys, _ms, _margins = orc.exact_draws(uniforms=uniforms, **case)
    assert [[NA if y is None else y for y in row] for row in ys[0]] == want_y


def test_the_clamp_acts_only_where_v_equals_the_total():
    """A valid uniform is below 1 and a valid cell's total is within 2e-5 of 1, so u total rounds below total (the largest
    uniform against totals on both sides of 1); the clamp is reached with u = 1, which the device's validation refuses."""
    case, uniforms = cases.off_one()
    got = orc.check(uniforms=uniforms, **case)
    total = got["m"].sum(axis=3)
    assert (uniforms.reshape(total.shape) * total < total).all() and (got["y_rep"] == 1).all()
    assert total[0, 0].tolist() == [1 + 2.0 ** -20, 1 - 2.0 ** -20]
    ones = np.ones_like(uniforms)
    assert orc.first_offender(case["clusters"], case["weights"], case["tables"], ones) == (0, 6, 0)
    clamped = orc.check(uniforms=ones, **case)                              # v == total: every cdf step is <= v, the count is S
    assert (clamped["y_rep"] == 1).all() and (clamped["margin"] == 0).all()
    case, _u, _y = cases.edges()
    clamped = orc.check(uniforms=np.ones((1, 28)), **case)
    assert clamped["y_rep"][0, 0].tolist() == [3, 2, 3, NA]


@pytest.mark.parametrize("shape", [s for s in cases.SHAPES if s[0] * s[1] <= 300 and s[2] <= 5], ids=str)
def test_the_draws_match_exact_rationals_where_the_margin_allows(shape):
    case, seed, got = cases.synthetic(shape)
    N, F = case["codes"].shape
    T = case["clusters"].shape[0]
    uniforms = orc.uniforms_of(seed, 0, T, N * F)
    ys, ms, margins = orc.exact_draws(uniforms=uniforms, **case)
    compared = 0
    for t in range(T):
        for n in range(N):
            for f in range(F):
                if ys[t][n][f] is None:
                    assert not got["drawn"][t, n, f] and got["y_rep"][t, n, f] == NA
                    continue
                assert got["drawn"][t, n, f] and abs(float(margins[t][n][f]) - got["margin"][t, n, f]) <= 2.0 ** -45
                if margins[t][n][f] > Fraction(orc.MARGIN):
                    assert got["y_rep"][t, n, f] == ys[t][n][f]
                    compared += 1
    assert compared == int(got["drawn"].sum()) > 0                          # (the margin condition: nothing was left out)


@pytest.mark.parametrize("shape", cases.SHAPES, ids=str)
def test_the_margin_condition_holds_for_the_seeded_cases(shape):
    _case, _seed, got = cases.synthetic(shape)
    assert got["margin"][got["drawn"]].min() > orc.MARGIN
    assert (got["y_rep"][~got["drawn"]] == NA).all() and (got["count_rep"].sum(axis=2) == got["drawn"].sum(axis=1)).all()


def test_the_margin_condition_holds_for_the_longer_seeded_case():
    _case, _seed, got = cases.synthetic((33, 15, 2, 3, 3, None), T=7)      # the split test's
    assert got["margin"][got["drawn"]].min() > orc.MARGIN and got["drawn"].shape[0] == 7


@pytest.mark.parametrize("r", [0, 1])
def test_the_margin_condition_holds_for_the_recorded_runs(r):
    got = cases.recorded_oracle(r)
    smallest = got["margin"][got["drawn"]].min()
    print(f"run {r}: smallest margin {smallest:.3g}")
    assert smallest > orc.MARGIN and smallest > 5e-8
    assert got["n_skipped"] == 0 and int(got["drawn"][0].sum()) == 3600 - 92 and np.isfinite(got["dev_feature"]).all()
    p = orc.p_value(got["dev_feature"][:, 1], got["dev_feature"][:, 0])
    assert p.min() >= 0.1 and 0.7 <= np.median(p) <= 1.0                    # (the issue's prototype: 0.20 / 0.43 to 1.0, median 0.9)


def test_the_deviance_sums_lie_within_a_quarter_of_the_device_band_of_mpmath():
    mpmath.mp.dps = 50
    shape = cases.SHAPES[6]                                                 # 20 x 33 x 5, three components
    case, seed, got = cases.synthetic(shape)
    N, F = case["codes"].shape
    T = case["clusters"].shape[0]
    uniforms = orc.uniforms_of(seed, 0, T, N * F)
    _ys, ms, _margins = orc.exact_draws(uniforms=uniforms, **case)
    worst = 0.0
    for t in range(T):
        exact = [[[mpmath.mpf(0)] * F for _ in range(N)] for _ in range(2)]
        for n in range(N):
            for f in range(F):
                if not got["drawn"][t, n, f]:
                    continue
                for side, s in enumerate((int(case["codes"][n, f]), int(got["y_rep"][t, n, f]))):
                    m = ms[t][n][f][s]
                    exact[side][n][f] = -2 * mpmath.log(mpmath.mpf(m.numerator) / mpmath.mpf(m.denominator)) if m > 0 else mpmath.inf
        for side in range(2):
            for f in range(F):
                column = [exact[side][n][f] for n in range(N)]
                if any(v == mpmath.inf for v in column):
                    assert got["dev_feature"][t, side, f] == math.inf
                    continue
                band = orc.dev_band(int(got["drawn"][t, :, f].sum()), float(sum(abs(v) for v in column)))
                err = abs(mpmath.mpf(float(got["dev_feature"][t, side, f])) - sum(column))
                worst = max(worst, float(err / band) if band else float(err))
                assert err <= band / 4
            for n in range(N):
                row = exact[side][n]
                if any(v == mpmath.inf for v in row):
                    assert got["dev_object"][t, side, n] == math.inf
                    continue
                band = orc.dev_band(int(got["drawn"][t, n].sum()), float(sum(abs(v) for v in row)))
                err = abs(mpmath.mpf(float(got["dev_object"][t, side, n])) - sum(row))
                worst = max(worst, float(err / band) if band else float(err))
                assert err <= band / 4
    print(f"worst error of the oracle's sums: {worst:.3g} of the device band")


def test_the_trees_add_every_cell_once():
    rng = np.random.default_rng(5)
    for N, F in [(1, 1), (15, 63), (16, 64), (17, 65), (33, 130)]:
        d = rng.random((N, F))
        assert np.allclose(orc.sum_over_objects(d), d.sum(axis=0), rtol=1e-14) and np.allclose(orc.sum_over_features(d), d.sum(axis=1), rtol=1e-14)
    d = np.ones((40, 70))                                                   # small integers add exactly in any order
    assert orc.sum_over_objects(d).tolist() == [40.0] * 70 and orc.sum_over_features(d).tolist() == [70.0] * 40


def test_the_p_value_counts_ties_half_and_takes_infinities():
    inf = math.inf
    rep = np.array([[1.0, 2.0, inf, 0.0], [3.0, 2.0, inf, 0.0], [2.0, 2.0, 1.0, 0.0], [0.0, 1.0, inf, 0.0]])
    obs = np.array([[2.0, 2.0, inf, 0.0]] * 4)
    assert orc.p_value(rep, obs).tolist() == [(1 + 0.5) / 4, 1.5 / 4, 1.5 / 4, 0.5]
    assert ppc.p_value(rep, obs).tolist() == orc.p_value(rep, obs).tolist()
    assert orc.p_value(np.array([[5.0]]), np.array([[inf]])).tolist() == [0.0]
    empty = ppc.PpcResult(codes=np.array([[NA, 0]], dtype=np.uint8), dev_feature=np.zeros((3, 2, 2)), dev_object=np.zeros((3, 2, 1)),
                          count_rep=np.zeros((3, 2, 1), dtype=np.int32), count_obs=np.array([[0], [1]]), n_samples=3, n_skipped=0)
    header, rows = empty.table("feature")
    assert header == ["feature", "n_cells", "deviance_observed", "deviance_replicated", "p", "flag"]
    assert rows[0] == ["F1", 0, 0.0, 0.0, 0.5, "no cells"] and rows[1][:2] == ["F2", 1] and rows[1][5] == ""
    assert empty.p_count.tolist() == [[0.5], [0.0]] and [r[0] for r in empty.worst("feature")] == ["F2"]


def test_the_draw_index_makes_the_split_explicit():
    case, seed, whole = cases.synthetic(cases.SHAPES[4])
    part = lambda a, b: {k: (v[a:b] if k in ("clusters", "weights", "tables") else v) for k, v in case.items()}    # noqa: E731
    pieces = [orc.check(seed=seed, first_draw=a, **part(a, b)) for a, b in ((0, 1), (1, 3))]
    for key in ("y_rep", "dev_feature", "dev_object", "count_rep"):
        assert np.array_equal(np.concatenate([p[key] for p in pieces]), whole[key])
    assert sum(p["n_skipped"] for p in pieces) == whole["n_skipped"]
    again = orc.check(seed=seed, first_draw=0, **part(1, 3))                # the wrong index draws other replicates
    assert not np.array_equal(again["y_rep"], whole["y_rep"][1:])
    u = orc.uniforms_of(seed, 0, 3, 33 * 15)
    assert np.array_equal(orc.uniforms_of(seed, 1, 2, 33 * 15), u[1:]) and ((u >= 0) & (u < 1)).all()


def test_the_seventh_kind_of_offender_is_ordered_like_the_others():
    case, uniforms, _want = cases.hand()
    bad = uniforms.copy()
    bad[1, 0] = 1.0
    assert orc.first_offender(case["clusters"], case["weights"], case["tables"], bad) == (1, 6, 0)
    bad[0, 1] = math.nan
    assert orc.first_offender(case["clusters"], case["weights"], case["tables"], bad) == (0, 6, 1)
    tables = case["tables"].copy()
    tables[0, 1, 0, 2] = 0.75                                               # a sum, in the same sample: the earlier kind wins
    assert orc.first_offender(case["clusters"], case["weights"], tables, bad) == (0, 5, 1)
    bad[0, 1] = -0.5
    tables[0, 1, 0, 2], tables[1, 0, 0, 0] = 0.5, -1.0                      # an entry, in the later sample: the earlier sample wins
    assert orc.first_offender(case["clusters"], case["weights"], tables, bad) == (0, 6, 1)
    assert orc.KINDS[6] == "uniform" and len(orc.KINDS) == 7
