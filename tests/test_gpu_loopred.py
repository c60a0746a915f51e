"""GPU checks of the leave-one-out predictive (include/sbe_loopred.h, sbayes_amd/loopred.py): against the oracle
(tests/_loopred_oracle.py) under the bounds its docstring derives, every cell, none left out; against the existing units byte for
byte (the stored rows are predict's lik, loo_i and k are elpd's on those rows); bit-identical reads for every split of the samples
over the calls of either pass, every feature tile and after a reset; the column past the LDS budget
and the duplicated samples; the errors; and loo_predictive on the recorded runs."""
import ctypes as ct
from functools import lru_cache

import numpy as np
import pytest

from sbayes_amd import elpd, loopred, predict
from sbayes_amd._handle import EngineError, _ptr
from tests import _loopred_cases as cases
from tests import _loopred_oracle as orc
from tests import _predict_oracle as po
from tests.test_gpu_elpd import RTOL, check_k, close

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE, ERR_DATA = 1, 3, 4
SAMPLES = ("clusters", "weights", "tables")


def _set(h, case, capacity=None):
    h.set_data(case["codes"], case["groups"], case["n_groups"], case["tables"].shape[3], case["clusters"].shape[1],
               capacity=capacity or case["clusters"].shape[0])


def _pass(call, case, splits):
    T = case["clusters"].shape[0]
    edges = [0, *(splits or []), T]
    for a, b in zip(edges, edges[1:]):
        call(*(case[k][a:b] for k in SAMPLES))


def _run(h, case, add_splits=None, acc_splits=None):
    """The three phases on a handle that holds the data; dict(lik, w, loo_i, k, n_eff, p_loo)."""
    _pass(h.add, case, add_splits)
    loo_i, k, n_eff = h.weights()
    _pass(h.accumulate, case, acc_splits)
    lik, w = h.store()
    p, n = h.sums()
    assert n == case["clusters"].shape[0] == h.n_rows
    return dict(lik=lik, w=w, loo_i=loo_i.copy(), k=k.copy(), n_eff=n_eff.copy(), p_loo=p)


def _device(case, tile=0, **splits):
    h = loopred.LooPredHandle(0)
    try:
        _set(h, case)
        h.set_feature_tile(tile)
        return _run(h, case, **splits)
    finally:
        h.close()


def _same(a, b):
    return all(np.array_equal(a[key], b[key], equal_nan=True) for key in a)


def _check(dev, want, case, label):
    """The device's result against the oracle's, every cell; prints the worst error in units of its bound."""
    T, C = case["clusters"].shape[0], case["weights"].shape[2]
    assert np.array_equal(dev["lik"], want["lik"])
    close(dev["loo_i"], want["loo_i"])
    check_k(dev["k"], want["k"])
    b = orc.log_w_bound(want["w"])
    ew = np.abs(np.log(dev["w"]) - np.log(want["w"]))
    eb = orc.probs_bound(want["p_loo"], want["w"], case["codes"], T, C)
    ep = np.abs(dev["p_loo"] - want["p_loo"])
    en = np.abs(dev["n_eff"] - want["n_eff"]) / want["n_eff"]
    nb = np.expm1(2 * b.max(axis=0)) + 2 * po.gamma(T + 2)
    el = np.abs(dev["loo_i"] - want["loo_i"]) / np.maximum(RTOL * np.abs(want["loo_i"]), 1e-10)
    print(f"{label}: worst error / bound: loo_i {el.max():.3g}, log w {(ew / b).max():.3g}, p_loo {(ep[eb > 0] / eb[eb > 0]).max():.3g}, "
          f"n_eff {(en / nb).max():.3g}")
    assert (ew <= b).all() and (ep <= eb).all() and (en <= nb).all()
    assert not dev["p_loo"][case["codes"] == loopred.NA].any()


# ---- against the oracle ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", sorted(cases.BY_SAMPLES))
def test_sample_counts_against_the_oracle(T):
    case, want = cases.synthetic(T)
    tile = cases.BY_SAMPLES[T][6]
    dev = _device(case, tile=tile)
    _check(dev, want, case, f"T={T}")
    assert np.isinf(dev["k"]).all() == (T <= 20)


def test_the_smallest_case_against_the_oracle():
    case, want = cases.smallest()
    _check(_device(case), want, case, "smallest")


def test_the_hand_case():
    case, want = cases.hand()
    dev = _device(case)
    assert dev["lik"].tolist() == want["lik"] and np.isinf(dev["k"]).all()
    assert np.allclose(dev["w"], want["w"], rtol=1e-14, atol=0) and np.allclose(dev["p_loo"], want["p_loo"], rtol=1e-14, atol=0)
    assert dev["n_eff"][0] == pytest.approx(want["n_eff"], rel=1e-14) and dev["loo_i"][0] == pytest.approx(np.log(7 / 18), rel=1e-14)


def test_duplicated_samples_tie_in_every_column_and_in_the_tail():
    case, want = cases.duplicated()
    dev = _device(case)
    _check(dev, want, case, "duplicated")
    assert np.array_equal(dev["lik"][0::2], dev["lik"][1::2]) and (dev["w"][0::2] <= dev["w"][1::2]).all()
    assert ((dev["w"][0::2] < dev["w"][1::2]).any(axis=0)).all()          # of two equal samples the earlier one sits lower in the tail


def test_a_column_past_the_lds_budget():
    T = elpd.lds_max_samples() + 1
    assert T > loopred.lds_max_samples()
    case, want = cases.long_column(T)
    dev = _device(case)
    _check(dev, want, case, f"T={T}")
    _against_the_units(case, dev)


# ---- against the existing units, byte for byte --------------------------------------------------------------------------------------
def _against_the_units(case, dev):
    h = predict.PredictHandle(0)
    try:
        h.set_data(case["codes"], case["groups"], case["n_groups"], case["tables"].shape[3], case["clusters"].shape[1])
        lik = h.accumulate(case["clusters"], case["weights"], case["tables"], lik=True)
    finally:
        h.close()
    na = (case["codes"] == predict.NA).ravel()
    assert np.array_equal(lik[:, ~na], dev["lik"]) and (lik[:, na] == 1).all()
    loo = elpd.psis_loo(lik, na_values=na, burnin=0.0, device=0)
    assert np.array_equal(loo.loo_i, dev["loo_i"]) and np.array_equal(loo.pareto_k, dev["k"], equal_nan=True)


@pytest.mark.parametrize("T", [2, 21, 300])
def test_the_rows_are_predicts_and_loo_and_k_are_elpds(T):
    case, _want = cases.synthetic(T)
    _against_the_units(case, _default(T))


@lru_cache(maxsize=None)
def _default(T):
    return _device(cases.synthetic(T)[0])


# ---- bit-identical reads ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [1, 2, 3, 5, 16, 256])
def test_a_forced_feature_tile_changes_no_bit(tile):
    assert _same(_default(21), _device(cases.synthetic(21)[0], tile=tile))


def test_the_reads_do_not_depend_on_how_the_samples_are_split():
    case, _want = cases.synthetic(64)
    whole = _default(64)
    for add_splits, acc_splits in ((list(range(1, 64)), None), (None, list(range(1, 64))), ([7], [33, 40]), ([1, 2, 63], [31, 32])):
        assert _same(whole, _device(case, add_splits=add_splits, acc_splits=acc_splits)), (add_splits, acc_splits)
    h = loopred.LooPredHandle(0)
    try:                                                       # after a reset, and with room to spare in the store
        _set(h, case, capacity=100)
        first = _run(h, case, [5], [60])
        h.reset()
        assert h.sums()[1] == 0 and not h.sums()[0].any() and h.store(with_weights=False)[0].shape == (0, first["lik"].shape[1])
        assert _same(whole, first) and _same(whole, _run(h, case))
        # weights() again starts the second pass over; a further add discards the weights
        h.weights()
        assert h.sums()[1] == 0 and not h.sums()[0].any()
        _pass(h.accumulate, case, [20])
        assert np.array_equal(h.sums()[0], whole["p_loo"])
        h.add(*(case[k][:3] for k in SAMPLES))
        assert h._lib.sbe_loopred_accumulate(h._h, 0, 1, *(_ptr(case[k]) for k in SAMPLES)) == ERR_STATE and "no weights yet" in h._last_error()
    finally:
        h.close()


# ---- errors ----------------------------------------------------------------------------------------------------------------------------
def _raw(h, name, *args):
    return getattr(h._lib, f"sbe_loopred_{name}")(h._h, *args)


def test_the_call_sequence_is_checked():
    case, _want = cases.synthetic(21)
    cl, w, tb = (case[k] for k in SAMPLES)
    out = np.zeros(256)
    n = ct.c_int64(0)
    h = loopred.LooPredHandle(0)
    try:
        for rc in (_raw(h, "reset"), _raw(h, "add", 1, _ptr(cl), _ptr(w), _ptr(tb)), _raw(h, "weights", _ptr(out), _ptr(out), _ptr(out)),
                   _raw(h, "accumulate", 0, 1, _ptr(cl), _ptr(w), _ptr(tb)), _raw(h, "read", None, ct.byref(n)), _raw(h, "get_store", None, None)):
            assert rc == ERR_STATE and "sbe_loopred_set_data comes first" in h._last_error()
        _set(h, case)
        # T = 0 and T = 1: no weights
        assert _raw(h, "weights", _ptr(out), _ptr(out), _ptr(out)) == ERR_STATE and "0 samples stored" in h._last_error()
        h.add(cl[:1], w[:1], tb[:1])
        assert _raw(h, "weights", _ptr(out), _ptr(out), _ptr(out)) == ERR_STATE and "1 samples stored; PSIS needs at least 2" in h._last_error()
        # accumulate before weights
        h.add(cl[1:], w[1:], tb[1:])
        assert _raw(h, "accumulate", 0, 21, _ptr(cl), _ptr(w), _ptr(tb)) == ERR_STATE and "no weights yet" in h._last_error()
        assert _raw(h, "get_store", None, _ptr(out)) == ERR_STATE
        # the store is full
        assert _raw(h, "add", 1, _ptr(cl), _ptr(w), _ptr(tb)) == ERR_ARG and "store overflow: 21 samples + 1 exceed the capacity of 21" in h._last_error()
        h.weights()
        # a wrong t0, a gap, past the end
        for t0, count in ((1, 1), (0, 22), (5, 3)):
            assert _raw(h, "accumulate", t0, count, _ptr(cl), _ptr(w), _ptr(tb)) == ERR_STATE and "in order without gaps, the next sample is 0" in h._last_error()
        h.accumulate(cl[:4], w[:4], tb[:4])
        later = tuple(np.ascontiguousarray(v[6:]) for v in (cl, w, tb))
        assert _raw(h, "accumulate", 6, 2, *(_ptr(v) for v in later)) == ERR_STATE and "the next sample is 4" in h._last_error()
        assert _raw(h, "accumulate", 0, 4, _ptr(cl), _ptr(w), _ptr(tb)) == ERR_STATE
        with pytest.raises(ValueError, match="4 of 21 samples accumulated: the second pass is not complete"):
            h.result()
        h.accumulate(cl[4:], w[4:], tb[4:])
        assert np.array_equal(h.sums()[0], _default(21)["p_loo"]) and np.array_equal(h.result().loo_i[case["codes"] != 255], _default(21)["loo_i"])
    finally:
        h.close()


def test_a_changed_sample_in_the_second_pass_is_refused_and_named():
    case, _want = cases.synthetic(21)
    cl, w, tb = (case[k] for k in SAMPLES)
    h = loopred.LooPredHandle(0)
    try:
        _set(h, case)
        h.add(cl, w, tb)
        h.weights()
        h.accumulate(cl[:5], w[:5], tb[:5])
        before = h.sums()
        other = tb[5:].copy()
        other[3] = tb[0]                                       # sample 8 is another draw: valid, but not the one stored
        with pytest.raises(EngineError, match="sample 8: its likelihood row differs from the one sbe_loopred_add stored") as err:
            h.accumulate(cl[5:], w[5:], other)
        assert err.value.code == ERR_DATA
        after = h.sums()
        assert after[1] == before[1] == 5 and np.array_equal(after[0], before[0])
        swapped = np.ascontiguousarray(cl[5:][::-1])           # the samples in another order: the first of them differs
        with pytest.raises(EngineError, match="sample 5: its likelihood row differs"):
            h.accumulate(swapped, np.ascontiguousarray(w[5:][::-1]), np.ascontiguousarray(tb[5:][::-1]))
        h.accumulate(cl[5:], w[5:], tb[5:])                    # the handle is usable afterwards
        assert np.array_equal(h.sums()[0], _default(21)["p_loo"])
    finally:
        h.close()


def test_a_zero_likelihood_names_the_cell_and_the_sample():
    case, _want = cases.synthetic(21)
    cl, w, tb = case["clusters"], case["weights"], case["tables"].copy()
    n, f = (int(v) for v in np.argwhere(case["codes"] != 255)[40])
    x = int(case["codes"][n, f])
    tb[5, :, f, x] = 0.0
    tb[5, :, f] /= tb[5, :, f].sum(axis=1, keepdims=True)
    tb[9, :, f, x] = 0.0
    tb[9, :, f] /= tb[9, :, f].sum(axis=1, keepdims=True)
    assert po.first_offender(cl, w, tb) is None
    first = int(np.flatnonzero(case["codes"][:, f] == x)[0])                 # the first cell, in n F + f order, that shows the state
    lik = orc.rows_of(case["codes"], orc.mixture(case["codes"], case["groups"], case["n_groups"], cl, w, tb))
    j, t = orc.first_bad(lik)
    assert t == 5 and tuple(np.argwhere(case["codes"] != 255)[j]) == (first, f)
    h = loopred.LooPredHandle(0)
    try:
        _set(h, case)
        h.add(cl, w, tb)
        with pytest.raises(EngineError, match=rf"cell \(object {first}, feature {f}\), sample 5: the likelihood of the observed state is zero") as err:
            h.weights()
        assert err.value.code == ERR_DATA
        assert _raw(h, "accumulate", 0, 1, _ptr(cl), _ptr(w), _ptr(tb)) == ERR_STATE
        h.reset()
        assert _same(_default(21), _run(h, case))
    finally:
        h.close()


def _spoil(case, name):
    cl, w, tb = (case[k].copy() for k in SAMPLES)
    if name == "overlap":
        cl[3, 0, 4] = cl[3, 2, 4] = 1
        return (cl, w, tb), "sample 3: object 4 is in more than one cluster"
    if name == "nan":
        tb[2, 4, 3, 1] = np.nan
        return (cl, w, tb), r"sample 2: tables\[4\]\[3\]\[1\] \(row, feature, state\) is negative or not finite"
    if name == "row sum":
        tb[4, 2, 1] *= 1.001
        return (cl, w, tb), "sample 4: table row 2, feature 1 sums further than 1e-05 from 1"
    w[0, 3] *= 0.99
    return (cl, w, tb), "sample 0: the weights of feature 3 sum further than 1e-05 from 1"


@pytest.mark.parametrize("name", ["overlap", "nan", "row sum", "weight sum"])
def test_bad_samples_are_refused_in_either_pass(name):
    case, _want = cases.synthetic(21)
    bad, match = _spoil(case, name)
    assert po.first_offender(*bad) is not None
    h = loopred.LooPredHandle(0)
    try:
        _set(h, case)
        with pytest.raises(EngineError, match=match) as err:
            h.add(*bad)
        assert err.value.code == ERR_DATA and h.n_rows == 0 and h.store(with_weights=False)[0].shape[0] == 0
        _pass(h.add, case, None)
        h.weights()
        with pytest.raises(EngineError, match=match):
            h.accumulate(*bad)
        assert h.sums()[1] == 0 and not h.sums()[0].any()
        _pass(h.accumulate, case, [9])
        assert np.array_equal(h.sums()[0], _default(21)["p_loo"])
    finally:
        h.close()


def test_the_data_and_the_store_limit_are_checked():
    h = loopred.LooPredHandle(0)
    try:
        codes = np.zeros((4, 3), dtype=np.uint8)
        codes[2, 1] = 2
        with pytest.raises(EngineError, match=r"codes\[2\]\[1\]=2 is neither a state below 2 nor 255") as err:
            h.set_data(codes, np.zeros((0, 4), np.uint8), [], 2, 1, capacity=5)
        assert err.value.code == ERR_DATA
        groups = np.array([[0, 1, 2, 255]], dtype=np.uint8)
        with pytest.raises(EngineError, match=r"groups\[0\]\[2\]=2 is neither a group below 2 nor 255"):
            h.set_data(np.zeros((4, 3), np.uint8), groups, [2], 2, 1, capacity=5)
        wide = np.zeros((1 << 10, 1 << 10), dtype=np.uint8)
        for capacity, text in ((0, "capacity=0"), ((1 << 20) + 1, "capacity=1048577"), (1 << 20, "take 13194139533312 bytes on the device, the limit is 17179869184")):
            assert _raw(h, "set_data", 1 << 10, 1 << 10, 2, 1, 1, _ptr(wide), None, None, capacity) == ERR_ARG and text in h._last_error(), capacity
        assert _raw(h, "set_feature_tile", 257) == ERR_ARG
        # every cell NA: nothing to weigh, nothing is added
        case = {**cases.synthetic(2)[0]}
        case["codes"] = np.full_like(case["codes"], 255)
        got = _run_all_na(h, case)
        assert got[0].size == 0 and not got[1].any()
    finally:
        h.close()


def _run_all_na(h, case):
    _set(h, case)
    _pass(h.add, case, None)
    loo_i, _k, _n_eff = h.weights()
    _pass(h.accumulate, case, None)
    return loo_i, h.sums()[0]


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [0, 1])
def test_loo_predictive_on_the_recorded_runs(r):
    full = cases.recorded(r, burn=0)
    case, want = cases.recorded(r), cases.recorded_oracle(r)
    res = loopred.loo_predictive(full["codes"], full["groups"], full["clusters"], full["weights"], full["tables"], burnin=0.1, device=0,
                                 n_groups=full["n_groups"])
    obs = case["codes"] != loopred.NA
    assert res.n_samples == 54 and res.probs.shape == (100, 36, 5) and np.isnan(res.probs[~obs]).all() and all(v > 0 for v in res.kernel_ms.values())
    close(res.loo_i[obs], want["loo_i"])
    check_k(res.k[obs], want["k"])
    eb = orc.probs_bound(want["p_loo"], want["w"], case["codes"], 54, 3)
    ep = np.abs(np.where(obs[..., None], res.probs, 0.0) - want["p_loo"])
    print(f"recorded run {r}: worst p_loo error / bound {(ep[eb > 0] / eb[eb > 0]).max():.3g}; accuracy {res.accuracy():.4f}, Brier {res.brier():.4f}, "
          f"log score {res.log_score():.4f}, {res.n_bad_k()} cells with k > 0.7")
    assert (ep <= eb).all()
    assert np.allclose(res.p_obs[obs], np.exp(res.loo_i[obs]), rtol=2.0 ** -22, atol=0)
    assert res.n_bad_k() == int((want["k"] > 0.7).sum())
    # the optimism of the in-sample fit, from the posterior predictive of the same samples
    inside = predict.posterior_predictive(full["codes"], full["groups"], full["clusters"], full["weights"], full["tables"], burnin=0.1, device=0,
                                          n_groups=full["n_groups"])
    assert res.optimism(inside)["log_score"] > 0
