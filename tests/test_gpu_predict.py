"""GPU checks of the posterior predictive (include/sbe_predict.h, sbayes_amd/predict.py) against the oracle
(tests/_predict_oracle.py) under the bounds derived from the operation order: device and oracle each lie
within the bound of the exact value, so they differ by at most twice the bound."""
import ctypes as ct
from functools import lru_cache

import numpy as np
import pytest

from sbayes_amd import elpd, predict
from sbayes_amd._handle import EngineError, _ptr
from tests import _predict_cases as cases
from tests import _predict_oracle as orc

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE, ERR_DATA = 1, 3, 4


def _set(h, case, S=None, K=None):
    h.set_data(case["codes"], case["groups"], case["n_groups"], S or case["tables"].shape[3], K or case["clusters"].shape[1])


def _device(case, lik=True, tile=0, splits=None):
    """(pred_sum, resp_sum, n_samples, n_zero, lik) of the device for a case, the samples split at `splits`."""
    T = case["clusters"].shape[0]
    with_handle = predict.PredictHandle(0)
    try:
        _set(with_handle, case)
        with_handle.set_feature_tile(tile)
        edges = [0, *(splits or []), T]
        rows = [with_handle.accumulate(case["clusters"][a:b], case["weights"][a:b], case["tables"][a:b], lik=lik) for a, b in zip(edges, edges[1:])]
        return (*with_handle.sums(), np.concatenate(rows) if lik else None)
    finally:
        with_handle.close()


def _check(dev, want, T, C):
    """The device's result against the oracle's (Sums, lik); prints the worst error in units of the bound."""
    pred, resp, n_samples, n_zero, lik = dev
    sums, lik_want = want
    pb = 2 * orc.pred_bound(sums.pred, T, C) * (1 + 1e-9)
    rb = 2 * orc.resp_bound(sums.resp, T, C, sums.inv_m) * (1 + 1e-9)
    lb = 2 * orc.lik_bound(lik_want.astype(np.float64), C)
    ep, er, el = np.abs(pred - sums.pred), np.abs(resp - sums.resp), np.abs(lik.astype(np.float64) - lik_want)
    print(f"pred: max err {ep.max():.3g} ({'bit-identical' if np.array_equal(pred, sums.pred) else 'differs'}), "
          f"resp: {er.max():.3g} ({'bit-identical' if np.array_equal(resp, sums.resp) else 'differs'}), lik: {el.max():.3g}, "
          f"n_zero {n_zero} / {sums.n_zero}")
    assert (ep <= pb).all() and (er <= rb).all() and (el <= lb).all()
    assert n_samples == T == sums.n_samples and n_zero == sums.n_zero


# ---- the recorded runs ------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _recorded_oracle(r):
    return orc.run(**cases.case(r))


@pytest.mark.parametrize("r", [0, 1])
def test_the_recorded_runs_match_the_oracle(r):
    case, want = cases.case(r), _recorded_oracle(r)
    dev = _device(case)
    _check(dev, want, 60, 3)
    na = case["codes"] == predict.NA
    assert (dev[4][:, na.ravel()] == 1).all() and dev[3] == 0
    res = predict.PredictResult(codes=case["codes"], pred_sum=dev[0], resp_sum=dev[1], n_samples=dev[2], n_zero=dev[3], lik=dev[4])
    filled, p = res.impute()
    filled_want, p_want = orc.impute(case["codes"], want[0].pred)
    assert np.array_equal(filled, filled_want) and np.abs(p - p_want).max() <= 1e-12
    assert np.allclose(np.nansum(res.responsibility, axis=2)[~na], 1.0, rtol=0, atol=1e-12) and np.isnan(res.responsibility[na]).all()
    # LOO given the logged draws, from the device's rows and from the oracle's
    loo = elpd.psis_loo(dev[4], na_values=na.ravel(), burnin=0.0, device=0)
    loo_want = elpd.psis_loo(want[1], na_values=na.ravel(), burnin=0.0, device=0)
    assert loo.elpd_loo == loo_want.elpd_loo and np.array_equal(loo.loo_i, loo_want.loo_i) and loo.n_data_points == 3600 - 92


def test_the_one_call_form_discards_the_burn_in():
    case, want = cases.case(0), None
    res = predict.posterior_predictive(case["codes"], case["groups"], case["clusters"], case["weights"], case["tables"], burnin=0.1, lik=True, device=0,
                                       n_groups=case["n_groups"])
    kept = {k: (v[6:] if k in ("clusters", "weights", "tables") else v) for k, v in case.items()}
    want = orc.run(**kept)
    _check((res.pred_sum, res.resp_sum, res.n_samples, res.n_zero, res.lik), want, 54, 3)
    assert res.probs.shape == (100, 36, 5) and res.kernel_ms > 0


# ---- seeded synthetic cases ---------------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 2, 1, 1, 1), (33, 7, 3, 3, 3, 2), (257, 65, 5, 3, 3, 61), (33, 65, 32, 8, 3, 2), (257, 7, 2, 8, 1, 61), (1, 65, 5, 1, 3, 2),
          (257, 1, 32, 3, 1, 1), (33, 1, 3, 8, 3, 61)]


@lru_cache(maxsize=None)
def _synthetic(shape, **kw):
    N, F, S, C, K, T = shape
    case = orc.random_case(1000 + sum(shape), N, F, S, C, K, T, **dict(kw))
    assert orc.first_offender(case["clusters"], case["weights"], case["tables"]) is None
    return case, orc.run(**case)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "N{}-F{}-S{}-C{}-K{}-T{}".format(*s))
def test_synthetic_cases_match_the_oracle(shape):
    case, want = _synthetic(shape)
    _check(_device(case), want, shape[5], shape[3])


def test_the_largest_table_runs_at_a_tile_of_one_feature():
    """R = 256 rows of S = 32 states: two slices of one feature take 128 KiB of LDS."""
    case = orc.random_case(77, 5, 3, 32, 2, 3, 3, group_counts=[253])
    want = orc.run(**case)
    _check(_device(case), want, 3, 2)
    h = predict.PredictHandle(0)
    try:
        _set(h, case)
        h.set_feature_tile(2)                                # two features: 256 KiB, refused; the handle stays usable
        with pytest.raises(EngineError, match="bytes of LDS") as err:
            h.accumulate(case["clusters"], case["weights"], case["tables"])
        assert err.value.code == ERR_ARG and h.sums()[2] == 0
        h.set_feature_tile(1)
        h.accumulate(case["clusters"], case["weights"], case["tables"])
        assert np.array_equal(h.sums()[0], _device(case)[0])
    finally:
        h.close()


@pytest.mark.parametrize("tile", [1, 2, 3, 7, 16, 64, 256])
def test_a_forced_feature_tile_changes_no_bit(tile):
    shape = (33, 7, 3, 3, 3, 5)
    case, _want = _synthetic(shape)
    a, b = _tile_default(shape), _device(case, tile=tile)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


@lru_cache(maxsize=None)
def _tile_default(shape):
    return _device(_synthetic(shape)[0])


# ---- split invariance --------------------------------------------------------------------------------------------------------
def test_the_sums_do_not_depend_on_how_the_samples_are_split():
    case, want = _synthetic((33, 7, 5, 3, 3, 61), out_share=0.3)
    whole = _device(case)
    _check(whole, want, 61, 3)
    for splits in (None, list(range(1, 61)), [7]):            # a second identical call, 61 calls of one sample, 7 + 54
        other = _device(case, splits=splits)
        assert all(np.array_equal(x, y) for x, y in zip(whole, other)), splits
    assert whole[3] == want[0].n_zero


# ---- edge cases ----------------------------------------------------------------------------------------------------------------
def _edge(name):
    N, F, S, C, K, T = 33, 7, 4, 3, 3, 4
    case = orc.random_case(500, N, F, S, C, K, T, na_share=1.0 if name == "all NA" else 0.0 if name == "no NA" else 0.1)
    if name == "object in no cluster":
        case["clusters"][:, :, 5] = 0
    elif name == "object in no group":
        case["groups"][:, 5] = predict.NA
    elif name == "zero probability state":
        case["codes"][:, 2] = 1                               # every object shows state 1 of feature 2, which no row allows
        tb = case["tables"]
        tb[:, :, 2, 1] = 0.0
        tb[:, :, 2, 0] += 1e-3                                # (keeps a positive entry in the row)
        tb[:, :, 2] /= tb[:, :, 2].sum(axis=2, keepdims=True)
    elif name == "tiny weights":
        w = case["weights"]
        w[:, :, 0], w[:, :, 1], w[:, :, 2] = 1e-300, 1.0, 1e-300
    elif name == "denormal entries":
        tb = case["tables"]
        tb[1, :, 0, 0] = 5e-324
        tb[2, 0, 1, 1] = 1e-310
        tb /= tb.sum(axis=3, keepdims=True)
    return case, T, C


@pytest.mark.parametrize("name", ["all NA", "no NA", "object in no cluster", "object in no group", "zero probability state", "tiny weights",
                                  "denormal entries"])
def test_edge_cases_match_the_oracle(name):
    case, T, C = _edge(name)
    assert orc.first_offender(case["clusters"], case["weights"], case["tables"]) is None
    want = orc.run(**case)
    dev = _device(case)
    _check(dev, want, T, C)
    if name == "all NA":
        assert not dev[1].any() and (dev[4] == 1).all() and dev[3] == 0
    if name == "zero probability state":
        assert dev[3] >= 33 * T and not dev[1][:, 2].any() and not dev[4].reshape(T, 33, 7)[:, :, 2].any()
    if name == "object in no cluster":
        assert not dev[1][5, :, 0].any()


def test_one_component_and_objects_outside_every_cluster():
    """C = 1: an object in no cluster has no component at all: m = 0, lik = 0, counted in n_zero, no responsibility."""
    case = orc.random_case(600, 33, 7, 3, 1, 3, 2, na_share=0.0, out_share=0.0)
    case["clusters"][:, :, 4] = 0
    want = orc.run(**case)
    dev = _device(case)
    _check(dev, want, 2, 1)
    assert dev[3] == 2 * 7 and not dev[0][4].any() and not dev[1][4].any() and not dev[4].reshape(2, 33, 7)[:, 4].any()


# ---- errors --------------------------------------------------------------------------------------------------------------------
def _spoil(case, name):
    cl, w, tb = case["clusters"].copy(), case["weights"].copy(), case["tables"].copy()
    if name == "overlap":
        cl[3, 0, 4] = cl[3, 2, 4] = 1
        return (cl, w, tb), "sample 3: object 4 is in more than one cluster"
    if name == "nan":
        tb[2, 4, 3, 1] = np.nan
        return (cl, w, tb), r"sample 2: tables\[4\]\[3\]\[1\] \(row, feature, state\) is negative or not finite"
    if name == "negative":
        tb[1, 0, 6, 0] = -1e-12
        return (cl, w, tb), r"sample 1: tables\[0\]\[6\]\[0\]"
    if name == "row sum":
        tb[4, 2, 1] *= 1.001
        return (cl, w, tb), "sample 4: table row 2, feature 1 sums further than 1e-05 from 1"
    w[0, 3] *= 0.99
    return (cl, w, tb), "sample 0: the weights of feature 3 sum further than 1e-05 from 1"


@pytest.mark.parametrize("name", ["overlap", "nan", "negative", "row sum", "weight sum"])
def test_bad_samples_are_refused_before_anything_is_added(name):
    case, _want = _synthetic((33, 7, 3, 3, 3, 5))
    (cl, w, tb), match = _spoil(case, name)
    kind = {"overlap": 0, "nan": 3, "negative": 3, "row sum": 5, "weight sum": 2}[name]
    assert orc.first_offender(cl, w, tb)[1] == kind
    h = predict.PredictHandle(0)
    try:
        _set(h, case)
        h.accumulate(case["clusters"][:2], case["weights"][:2], case["tables"][:2])
        before = h.sums()
        with pytest.raises(EngineError, match=match) as err:
            h.accumulate(cl, w, tb, lik=True)
        assert err.value.code == ERR_DATA
        after = h.sums()
        assert all(np.array_equal(x, y) for x, y in zip(before, after))
        h.accumulate(case["clusters"][2:], case["weights"][2:], case["tables"][2:])          # the handle is usable afterwards
        assert all(np.array_equal(x, y) for x, y in zip(h.sums(), _tile_default((33, 7, 3, 3, 3, 5))[:4]))
    finally:
        h.close()


def test_the_call_sequence_and_the_data_are_checked():
    h = predict.PredictHandle(0)
    try:
        n, z = ct.c_int64(0), ct.c_int64(0)
        buf = np.zeros(64)
        assert h._lib.sbe_predict_reset(h._h) == ERR_STATE and "sbe_predict_set_data comes first" in h._last_error()
        assert h._lib.sbe_predict_accumulate(h._h, 1, _ptr(buf), _ptr(buf), _ptr(buf), None) == ERR_STATE
        assert h._lib.sbe_predict_read(h._h, None, None, ct.byref(n), ct.byref(z)) == ERR_STATE
        codes = np.zeros((4, 3), dtype=np.uint8)
        codes[2, 1] = 2
        with pytest.raises(EngineError, match=r"codes\[2\]\[1\]=2 is neither a state below 2 nor 255") as err:
            h.set_data(codes, np.zeros((0, 4), np.uint8), [], 2, 1)
        assert err.value.code == ERR_DATA
        groups = np.array([[0, 1, 2, 255]], dtype=np.uint8)
        with pytest.raises(EngineError, match=r"groups\[0\]\[2\]=2 is neither a group below 2 nor 255"):
            h.set_data(np.zeros((4, 3), np.uint8), groups, [2], 2, 1)
        with pytest.raises(ValueError, match="no data yet"):
            h.reset()
        # set_data resets the sums, reset keeps the data
        case, _want = _synthetic((33, 7, 3, 3, 3, 5))
        _set(h, case)
        h.accumulate(case["clusters"], case["weights"], case["tables"])
        h.reset()
        assert h.sums()[2:] == (0, 0) and not h.sums()[0].any()
        h.accumulate(case["clusters"], case["weights"], case["tables"])
        assert np.array_equal(h.sums()[0], _tile_default((33, 7, 3, 3, 3, 5))[0])
        _set(h, case)
        assert h.sums()[2:] == (0, 0) and not h.sums()[1].any()
        with pytest.raises(ValueError, match="no sample was accumulated"):
            h.result()
    finally:
        h.close()


# ---- limits ----------------------------------------------------------------------------------------------------------------------
def _raw_set_data(h, N, F, S, C, K, n_groups):
    codes, groups = np.zeros(16, np.uint8), np.zeros(16, np.uint8)          # (never read: the shape is refused first)
    counts = np.ascontiguousarray(n_groups if n_groups else [1], dtype=np.intc)
    return h._lib.sbe_predict_set_data(h._h, N, F, S, C, K, _ptr(codes), _ptr(groups), _ptr(counts))


def test_the_library_refuses_one_past_every_limit_and_runs_at_it():
    h = predict.PredictHandle(0)
    try:
        for shape, text in [(((1 << 20) + 1, 1, 2, 1, 1, []), "n_objects=1048577"), ((1, (1 << 16) + 1, 2, 1, 1, []), "n_features=65537"),
                            ((5, 3, 33, 1, 1, []), "n_states=33"), ((5, 3, 2, 9, 1, [1] * 8), "n_components=9"),
                            ((5, 3, 2, 2, 200, [57]), "make 257 table rows"), ((5, 3, 2, 1, 257, []), "n_clusters=257"),
                            ((1 << 20, 1 << 10, 2, 2, 1, [1]), "bytes on the device")]:
            assert _raw_set_data(h, *shape) == ERR_ARG and text in h._last_error(), shape
        assert h._lib.sbe_predict_set_feature_tile(h._h, 257) == ERR_ARG and h._lib.sbe_predict_set_feature_tile(h._h, -1) == ERR_ARG
        # at the limits: 2^20 objects, 2^16 features, one sample each
        for N, F in ((1 << 20, 1), (1, 1 << 16)):
            case = orc.random_case(9, N, F, 2, 1, 1, 1, out_share=0.0)
            _set(h, case)
            rows = h.accumulate(case["clusters"], case["weights"], case["tables"], lik=True)
            pred = h.sums()[0]
            want = np.broadcast_to(case["tables"][0, 0][None], (N, F, 2))
            assert np.array_equal(pred, want)
            observed = case["codes"] != predict.NA
            x = np.where(observed, case["codes"], 0).astype(np.int64)
            assert np.array_equal(rows[0].reshape(N, F), np.where(observed, np.take_along_axis(want, x[..., None], axis=2)[..., 0], 1.0).astype(np.float32))
    finally:
        h.close()


def test_the_samples_of_one_call_are_bounded_by_what_the_call_holds_on_the_device():
    """R = 256 x F = 64 x S = 32: 4 MiB of tables per sample, 63 samples per call."""
    one = orc.random_case(88, 5, 64, 32, 2, 1, 1, group_counts=[255])
    h = predict.PredictHandle(0)
    try:
        _set(h, one)
        n_max = h.max_samples()
        assert n_max == predict.MAX_STAGE_BYTES // predict.sample_bytes(5, 64, 32, 2, 1, 256) == 63
        cl, w, tb = (np.ascontiguousarray(np.repeat(one[k], n_max, axis=0)) for k in ("clusters", "weights", "tables"))
        assert h._lib.sbe_predict_accumulate(h._h, n_max + 1, _ptr(cl), _ptr(w), _ptr(tb), None) == ERR_ARG      # refused before anything is read
        assert "at most 63 samples per call" in h._last_error() and h.sums()[2] == 0
        assert h._lib.sbe_predict_accumulate(h._h, n_max, _ptr(cl), _ptr(w), _ptr(tb), None) == 0
        pred, _resp, n, _zero = h.sums()
        sums, _lik = orc.run(one["codes"], one["groups"], one["n_groups"], cl, w, tb)
        assert n == n_max and (np.abs(pred - sums.pred) <= 2 * orc.pred_bound(sums.pred, n_max, 2)).all()
        # the handle splits a longer block itself
        h.reset()
        h.accumulate(np.concatenate([cl, cl[:2]]), np.concatenate([w, w[:2]]), np.concatenate([tb, tb[:2]]))
        assert h.sums()[2] == n_max + 2
    finally:
        h.close()
