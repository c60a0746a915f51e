"""CPU checks of the posterior predictive's oracle (tests/_predict_oracle.py) against the contract in exact arithmetic, under
the bounds derived from the operation order, and against known answers of simulate_features'
formula."""
from fractions import Fraction

import numpy as np
import pytest

from sbayes_amd import predict
from tests import _predict_oracle as orc


def _float(q):
    try:
        return float(q)
    except OverflowError:
        return float("inf")


def _as_float(nested):
    return np.vectorize(_float, otypes=[np.float64])(np.array(nested, dtype=object))


def _against_exact(case, T, C):
    sums, lik = orc.run(**case)
    pred, resp, lik_x, inv_m, n_zero = orc.exact(**case)
    pred_f, resp_f, inv_f = _as_float(pred), _as_float(resp), _as_float(inv_m)
    # the difference in exact arithmetic: a float64 is a Fraction
    worst = {}
    for name, have, want, bound in (("pred", sums.pred, pred, orc.pred_bound(pred_f, T, C)),
                                    ("resp", sums.resp, resp, orc.resp_bound(resp_f, T, C, inv_f))):
        ratio = 0.0
        for idx in np.ndindex(have.shape):
            w = want[idx[0]][idx[1]][idx[2]]
            if np.isinf(bound[idx]):                         # 1 / m[x] beyond the float64 range: a ratio of denormals carries no bound
                continue
            err = abs(Fraction(float(have[idx])) - w)
            assert err <= Fraction(float(bound[idx])) * (1 + Fraction(1, 1 << 40)), (name, idx, float(err), float(bound[idx]))
            if bound[idx] > 0:
                ratio = max(ratio, float(err) / float(bound[idx]))
        worst[name] = ratio
    assert sums.n_zero == n_zero and sums.n_samples == T
    lik_f = _as_float(lik_x)
    lb = orc.lik_bound(lik_f, C)
    for t, i in np.ndindex(lik.shape):
        assert abs(Fraction(float(lik[t, i])) - lik_x[t][i]) <= Fraction(float(lb[t, i])) * (1 + Fraction(1, 1 << 40)), (t, i)
    return worst


@pytest.mark.parametrize("seed,N,F,S,C,K,T,digits", [(1, 5, 3, 3, 3, 2, 7, None), (2, 4, 2, 5, 1, 1, 3, None), (3, 3, 2, 2, 8, 3, 5, None),
                                                     (4, 6, 3, 5, 3, 3, 40, 8), (5, 2, 2, 4, 2, 1, 300, 8)])
def test_the_oracle_meets_the_exact_form_under_the_derived_bound(seed, N, F, S, C, K, T, digits):
    case = orc.random_case(seed, N, F, S, C, K, T, digits=digits)
    assert orc.first_offender(case["clusters"], case["weights"], case["tables"]) is None
    worst = _against_exact(case, T, C)
    print(f"seed {seed}: worst error / bound: pred {worst['pred']:.3f}, resp {worst['resp']:.3f}")


def test_weights_scaled_over_thirty_decades_and_denormal_entries():
    case = orc.random_case(11, 4, 3, 3, 3, 2, 20)
    rng = np.random.default_rng(12)
    w = case["weights"] * 10.0 ** rng.uniform(-30, 0, size=case["weights"].shape)
    w[0, 0] = [1.0, 1e-300, 1e-300]
    case["weights"] = w / w.sum(axis=2, keepdims=True)
    tb = case["tables"]
    tb[1, :, 0, 0] = 5e-324                                  # denormal entries, in every row and in one row alone
    tb[2, 0, 1, 1] = 1e-310
    tb /= tb.sum(axis=3, keepdims=True)
    assert ((tb > 0) & (tb < 2.0 ** -1022)).sum() >= tb.shape[1] + 1
    assert orc.first_offender(case["clusters"], case["weights"], tb) is None
    _against_exact(case, 20, 3)


def test_known_answers_of_the_mixture_formula():
    """Two objects, one feature of two states, clusters + one confounder; by hand."""
    codes = np.array([[0], [orc.NA]], dtype=np.uint8)
    groups = np.array([[0, orc.NA]], dtype=np.uint8)        # object 1 is in no group
    clusters = np.array([[[1, 0]], [[0, 0]]], dtype=np.uint8)   # sample 0: object 0 in the cluster; sample 1: nobody
    weights = np.array([[[0.25, 0.75]], [[0.5, 0.5]]])
    tables = np.array([[[[0.5, 0.5]], [[1.0, 0.0]]], [[[0.125, 0.875]], [[0.25, 0.75]]]])   # [T][R = 2][F = 1][S = 2]
    sums, lik = orc.run(codes, groups, [1], clusters, weights, tables)
    # sample 0, object 0: both components, 0.25 (0.5, 0.5) + 0.75 (1, 0) = (0.875, 0.125); sample 1: the confounder alone, (0.25, 0.75)
    assert sums.pred[0, 0].tolist() == [0.875 + 0.25, 0.125 + 0.75]
    # object 1: no component in either sample -> w = 0, m = 0
    assert sums.pred[1, 0].tolist() == [0.0, 0.0]
    # responsibilities of object 0 for its state 0: sample 0: (0.125, 0.75) / 0.875; sample 1: (0, 1)
    assert sums.resp[0, 0].tolist() == [0.125 / 0.875, 0.75 / 0.875 + 1.0]
    assert sums.resp[1, 0].tolist() == [0.0, 0.0] and sums.n_zero == 0
    assert lik.tolist() == [[0.875, 1.0], [0.25, 1.0]]
    filled, p = orc.impute(codes, sums.pred + np.array([[[0, 0]], [[1.0, 3.0]]]))
    assert filled.tolist() == [[0], [1]] and p[1, 0] == 0.75


def test_a_cell_without_any_component_counts_as_zero_probability():
    codes = np.array([[1]], dtype=np.uint8)
    clusters = np.zeros((2, 1, 1), dtype=np.uint8)
    sums, lik = orc.run(codes, np.zeros((0, 1), np.uint8), [], clusters, np.ones((2, 1, 1)), np.full((2, 1, 1, 2), 0.5))
    assert sums.n_zero == 2 and not sums.pred.any() and not sums.resp.any() and lik.tolist() == [[0.0], [0.0]]


def _valid():
    return orc.random_case(21, 6, 4, 3, 3, 2, 5)


@pytest.mark.parametrize("name,kind,at", [("overlap", 0, 4), ("nan", 3, (2 * 4 + 1) * 3 + 2), ("negative", 3, 5), ("row sum", 5, 1 * 4 + 3),
                                          ("weight sum", 2, 2), ("negative weight", 1, 2 * 3 + 1), ("empty row", 4, 7)])
def test_the_first_offender_is_named_in_the_contracts_order(name, kind, at):
    case = _valid()
    cl, w, tb = case["clusters"], case["weights"], case["tables"]
    if name == "overlap":
        cl[3, :, 4] = 1
        cl[4, :, 1] = 1                                      # a later sample does not count
    elif name == "nan":
        tb[3, 2, 1, 2] = np.nan
        tb[3, 3, 0, 0] *= 1.5                                # a wrong sum in the same sample comes after any bad entry
    elif name == "negative":
        tb[3, 0, 1, 2] = -1e-9
    elif name == "row sum":
        tb[3, 1, 3] *= 1.001
    elif name == "weight sum":
        w[3, 2] *= 0.99
        tb[3, 0, 0] *= 1.001                                 # weights come before tables
    elif name == "negative weight":
        w[3, 2, 1] = -0.5
    elif name == "empty row":
        tb[3, 1, 3] = 0.0
    assert orc.first_offender(cl, w, tb) == (3, kind, at)


def test_sums_within_the_tolerance_pass_and_the_module_mirrors_it():
    case = _valid()
    case["tables"][0, 0, 0] *= 1 + 9e-6
    case["weights"][0, 0] *= 1 - 9e-6
    assert orc.first_offender(case["clusters"], case["weights"], case["tables"]) is None
    assert predict.SUM_TOL == orc.SUM_TOL == 1e-5 and predict.NA == orc.NA == 255


def test_splitting_the_samples_leaves_the_oracles_sums_bit_identical():
    case = orc.random_case(31, 7, 5, 4, 3, 2, 9)
    whole, lik = orc.run(**case)
    parts = orc.Sums(7, 5, 4, 3)
    data = (case["codes"], case["groups"], case["n_groups"])
    rows = [orc.accumulate(parts, *data, case["clusters"][a:b], case["weights"][a:b], case["tables"][a:b]) for a, b in ((0, 2), (2, 9))]
    assert np.array_equal(parts.pred, whole.pred) and np.array_equal(parts.resp, whole.resp) and np.array_equal(np.concatenate(rows), lik)
