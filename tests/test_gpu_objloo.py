"""GPU checks of the leave-one-object-out unit (include/sbe_objloo.h, sbayes_amd/objloo.py) against its checker
(tests/_objloo_oracle.py) under the bounds its docstring derives, every entry, none left out: H under the evidence unit's band, L
on the device's own H, phase 2 on the device's own columns, the second pass bit for bit on the device's own weights; bit-identical
reads for every feature tile, every split of the samples in either pass and every capacity; the refusals, each naming its
offender; the two recorded runs end to end; and one handle across shapes."""
import ctypes as ct
from functools import lru_cache

import numpy as np
import pytest

from sbayes_amd import compare, objloo
from sbayes_amd._handle import EngineError, _ptr
from tests import _contrib_oracle as co
from tests import _loopred_oracle as lo
from tests import _objloo_cases as cases
from tests import _objloo_oracle as orc
from tests import _predict_oracle as po
from tests import _psens_oracle as ps

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE, ERR_DATA = 1, 3, 4
SAMPLES = cases.SAMPLES
POINTWISE = objloo.POINTWISE


def _set(h, case, capacity=None):
    h.set_data(case["codes"], case["groups"], case["n_groups"], case["tables"].shape[3], case["clusters"].shape[1],
               capacity=capacity or case["clusters"].shape[0])


def _pass(call, case, prior, splits):
    T = case["clusters"].shape[0]
    edges = [0, *(splits or []), T]
    for a, b in zip(edges, edges[1:]):
        call(*(case[k][a:b] for k in SAMPLES), None if prior is None else (prior[a:b] if np.ndim(prior) == 3 else prior))


def _run(h, case, prior=None, add_splits=None, acc_splits=None):
    """The three phases on a handle that holds the data; dict(H [T,N,K+1], L, Cnd, w [T,N], the pointwise vectors, membership, p_loo)."""
    _pass(h.add, case, prior, add_splits)
    pointwise, membership = h.weights()
    _pass(h.accumulate, case, prior, acc_splits)
    H, L, Cnd, w = h.store()
    p, n = h.sums()
    assert n == case["clusters"].shape[0] == h.n_rows
    out = dict(H=np.ascontiguousarray(H.transpose(2, 0, 1)), L=L.T.copy(), Cnd=Cnd.T.copy(), w=w.T.copy(), membership=membership.copy(), p_loo=p)
    out.update({name: v.copy() for name, v in zip(POINTWISE, pointwise)})
    return out


def _device(case, prior=None, tile=0, capacity=None, **splits):
    h = objloo.ObjLooHandle(0)
    try:
        _set(h, case, capacity)
        h.set_feature_tile(tile)
        return _run(h, case, prior, **splits)
    finally:
        h.close()


def _same(a, b):
    return all(np.array_equal(a[key], b[key], equal_nan=True) for key in a)


def _full_prior(case, prior):
    T, K, N = case["clusters"].shape
    return orc.uniform_prior(T, N, K) if prior is None else np.broadcast_to(prior, (T, N, K + 1))


def _close(got, want, label):
    """loo, lppd, n_eff and membership at tests/_loopred_oracle.RTOL with its absolute floor."""
    got, want = np.asarray(got), np.asarray(want)
    bound = np.maximum(lo.RTOL * np.abs(want), 1e-10)
    assert got.shape == want.shape and (np.abs(got - want) <= bound).all(), (label, float((np.abs(got - want) / bound).max()))
    return float((np.abs(got - want) / bound).max())


def _check(dev, want, case, prior, label):
    """The device's result against the checker's, every entry; prints the worst error in units of its bound."""
    prior = _full_prior(case, prior)
    # H: the evidence unit's band, -inf by class
    n_terms = (case["codes"] != orc.NA).sum(axis=1)[None, :, None]
    band = co.band(n_terms, want["mag"])
    fin = np.isfinite(want["H"])
    assert np.array_equal(np.isneginf(dev["H"]), np.isneginf(want["H"])) and np.isfinite(dev["H"][fin]).all()
    eh = np.abs(np.where(fin, dev["H"] - np.where(fin, want["H"], 0.0), 0.0))
    assert (eh <= band).all(), (label, float((eh[band > 0] / band[band > 0]).max()))
    # L and Cnd on the device's own H: Cnd is a selection, L within the derived bound
    a, L, Cnd = orc.mix(dev["H"], prior, want["z"])
    lb = orc.l_bound(dev["H"], prior)
    el = np.abs(dev["L"] - L)
    assert np.array_equal(dev["Cnd"], Cnd) and (el <= lb).all(), (label, float((el / lb).max()))
    # phase 2 on the device's own columns
    two = orc.phase2(dev["L"], dev["Cnd"], a)
    worst = max(_close(dev[name], two[name], f"{label} {name}") for name in ("loo_i", "lppd_i", "n_eff", "loo_cond_i", "lppd_cond_i", "membership"))
    ek = 0.0
    for kind, column in (("k_i", dev["L"]), ("k_cond_i", dev["Cnd"])):
        for n in range(column.shape[1]):
            got, ref = dev[kind][n], two[kind][n]
            assert np.isinf(got) == np.isinf(ref) and np.isnan(got) == np.isnan(ref), (label, kind, n)
            if np.isfinite(ref):
                tol = ps.tol_k(-column[:, n])
                assert np.isfinite(tol) and abs(got - ref) <= tol, (label, kind, n, abs(got - ref), tol)
                ek = max(ek, abs(got - ref) / tol)
    ew = _close(np.log(dev["w"]), np.log(two["w"]), f"{label} log w")
    # phase 3 with the device's own weights: bit for bit, NA cells filled
    p = orc.accumulate(**case, prior=prior, w=dev["w"])
    assert np.array_equal(dev["p_loo"], p), (label, float(np.abs(dev["p_loo"] - p).max()))
    print(f"{label}: worst error / bound: H {(eh[band > 0] / band[band > 0]).max() if (band > 0).any() else 0.0:.3g}, L {(el / lb).max():.3g}, "
          f"phase 2 {worst:.3g}, k {ek:.3g}, log w {ew:.3g}; p_loo equal")


# ---- against the checker -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cases.BY_SHAPE))
def test_shapes_against_the_checker(name):
    """F = 1, 63, 64, 65, 129 (the tree's edges), K = 1 and 4, C = 1 .. 3, N = 1, 2, 9, S = 2 and 32, a seeded prior with an excluded
    hypothesis.  C = 1 has no confounder: no cell may have a code, every H is 0 and the clusters alone predict."""
    case, prior, want = cases.by_shape(name)
    dev = _device(case, prior, tile=cases.BY_SHAPE[name][7])
    _check(dev, want, case, prior, name)
    NA = case["codes"] == orc.NA
    assert NA.any() == (name != "F1") and (dev["p_loo"][NA].sum(axis=1) > 0).all()      # the cells without a code are the ones this answers for, too
    if name == "C1":                                           # "no cluster" predicts nothing, a cluster its row
        in_a_cluster = ((1 - prior[:, :, 0]) * dev["w"]).sum(axis=0)
        assert not dev["H"].any() and (np.abs(dev["L"]) < 1e-15).all() and np.allclose(dev["p_loo"].sum(axis=2), in_a_cluster[:, None], rtol=1e-12, atol=0)


@pytest.mark.parametrize("T", sorted(cases.BY_SAMPLES))
def test_sample_counts_against_the_checker(T):
    case, prior, want = cases.synthetic(T)
    dev = _device(case, prior, tile=cases.BY_SAMPLES[T][6])
    _check(dev, want, case, prior, f"T={T}")
    assert np.isinf(dev["k_i"]).all() == np.isinf(dev["k_cond_i"]).all() == (T <= 20)
    assert np.allclose(dev["membership"].sum(axis=1), 1.0, rtol=0, atol=1e-12) and np.allclose(dev["w"].sum(axis=0), 1.0, rtol=0, atol=1e-12)


def test_the_hand_case():
    case, want = cases.hand()
    dev = _device(case)
    assert np.allclose(np.exp(dev["L"]), want["expL"], rtol=1e-14, atol=0) and np.allclose(np.exp(dev["Cnd"]), want["expCnd"], rtol=1e-14, atol=0)
    for name in ("w", "n_eff", "membership", "p_loo"):
        assert np.allclose(dev[name], want[name], rtol=1e-14, atol=0), name
    for name in ("loo_i", "lppd_i", "loo_cond_i", "lppd_cond_i"):
        assert np.allclose(dev[name], want[name], rtol=1e-14, atol=1e-15), name
    assert np.isinf(dev["k_i"]).all() and np.isinf(dev["k_cond_i"]).all()


def test_duplicated_samples_tie_in_every_column_and_in_the_tail():
    case, prior, want = cases.duplicated()
    dev = _device(case)
    _check(dev, want, case, prior, "duplicated")
    assert np.array_equal(dev["L"][0::2], dev["L"][1::2]) and (dev["w"][0::2] <= dev["w"][1::2]).all()
    assert (dev["w"][0::2] < dev["w"][1::2]).any(axis=0)[:3].all()        # of two equal samples the earlier one sits lower in the tail


def test_a_column_past_the_lds_budget():
    T = objloo.lds_max_samples() + 1
    case, prior, want = cases.long_column(T)
    dev = _device(case)
    _check(dev, want, case, prior, f"T={T}")
    assert np.isfinite(dev["k_i"]).all() and np.isfinite(dev["k_cond_i"]).all()


# ---- bit-identical reads ------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _default(T):
    return _device(cases.synthetic(T)[0])


@pytest.mark.parametrize("tile", [1, 2, 3, 5, 16, 256])
def test_a_forced_feature_tile_changes_no_bit(tile):
    assert _same(_default(21), _device(cases.synthetic(21)[0], tile=tile))


def test_the_reads_do_not_depend_on_the_split_of_the_samples_or_the_capacity():
    case = cases.synthetic(64)[0]
    whole = _default(64)
    for add_splits, acc_splits in ((list(range(1, 64)), None), (None, list(range(1, 64))), ([7], [33, 40]), ([1, 2, 63], [31, 32])):
        assert _same(whole, _device(case, add_splits=add_splits, acc_splits=acc_splits)), (add_splits, acc_splits)
    prior = cases.seeded_prior(64, 64, 4, 3)                       # ... with a prior per sample, split alike
    assert _same(_device(case, prior), _device(case, prior, add_splits=[9, 10], acc_splits=[50], capacity=99))
    h = objloo.ObjLooHandle(0)
    try:                                                       # after a reset, and with room to spare in the store
        _set(h, case, capacity=100)
        first = _run(h, case, None, [5], [60])
        h.reset()
        assert h.sums()[1] == 0 and not h.sums()[0].any() and h.store(with_weights=False)[0].shape == (4, 4, 0)
        assert _same(whole, first) and _same(whole, _run(h, case))
        # weights() again starts the second pass over; a further add discards the weights
        h.weights()
        assert h.sums()[1] == 0 and not h.sums()[0].any()
        _pass(h.accumulate, case, None, [20])
        assert np.array_equal(h.sums()[0], whole["p_loo"])
        h.add(*(case[k][:3] for k in SAMPLES))
        assert h._lib.sbe_objloo_accumulate(h._h, 0, 1, *(_ptr(case[k]) for k in SAMPLES), None) == ERR_STATE and "no weights yet" in h._last_error()
    finally:
        h.close()


@pytest.mark.parametrize("name", ["F63", "F65"])
def test_a_one_hot_prior_at_the_logged_membership_gives_the_conditional_column_bit_for_bit(name):
    case, _prior, want = cases.by_shape(name)
    onehot = (np.arange(want["H"].shape[2])[None, None, :] == want["z"][..., None]).astype(np.float64)
    dev = _device(case, onehot)
    assert np.array_equal(dev["L"], dev["Cnd"]) and np.isfinite(dev["L"]).all()
    for marg, cond in (("loo_i", "loo_cond_i"), ("k_i", "k_cond_i"), ("lppd_i", "lppd_cond_i")):
        assert np.array_equal(dev[marg], dev[cond], equal_nan=True)
    member = np.zeros_like(dev["membership"])
    for t in range(want["z"].shape[0]):
        member[np.arange(member.shape[0]), want["z"][t]] += 1
    assert np.allclose(dev["membership"], member / want["z"].shape[0], rtol=1e-14, atol=0)    # the indicator frequencies


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def _raw(h, name, *args):
    return getattr(h._lib, f"sbe_objloo_{name}")(h._h, *args)


def test_the_call_sequence_is_checked():
    case = cases.synthetic(21)[0]
    cl, w, tb = (case[k] for k in SAMPLES)
    out = np.zeros(256)
    outs = [_ptr(out)] * 8
    n = ct.c_int64(0)
    h = objloo.ObjLooHandle(0)
    try:
        for rc in (_raw(h, "reset"), _raw(h, "add", 1, _ptr(cl), _ptr(w), _ptr(tb), None), _raw(h, "weights", *outs),
                   _raw(h, "accumulate", 0, 1, _ptr(cl), _ptr(w), _ptr(tb), None), _raw(h, "read", None, ct.byref(n)), _raw(h, "get_store", None, None, None, None)):
            assert rc == ERR_STATE and "sbe_objloo_set_data comes first" in h._last_error()
        _set(h, case)
        assert _raw(h, "weights", *outs) == ERR_STATE and "0 samples stored" in h._last_error()
        h.add(cl[:1], w[:1], tb[:1])
        assert _raw(h, "weights", *outs) == ERR_STATE and "1 samples stored; PSIS needs at least 2" in h._last_error()
        assert _raw(h, "weights", *outs[:7], None) == ERR_ARG and "null pointer argument: membership" in h._last_error()
        h.add(cl[1:], w[1:], tb[1:])
        assert _raw(h, "accumulate", 0, 21, _ptr(cl), _ptr(w), _ptr(tb), None) == ERR_STATE and "no weights yet" in h._last_error()
        assert _raw(h, "get_store", None, None, None, _ptr(out)) == ERR_STATE
        assert _raw(h, "add", 1, _ptr(cl), _ptr(w), _ptr(tb), None) == ERR_ARG and "store overflow: 21 samples + 1 exceed the capacity of 21" in h._last_error()
        h.weights()
        for t0, count in ((1, 1), (0, 22), (5, 3)):
            assert _raw(h, "accumulate", t0, count, _ptr(cl), _ptr(w), _ptr(tb), None) == ERR_STATE and "in order without gaps, the next sample is 0" in h._last_error()
        h.accumulate(cl[:4], w[:4], tb[:4])
        later = tuple(np.ascontiguousarray(v[6:]) for v in (cl, w, tb))
        assert _raw(h, "accumulate", 6, 2, *(_ptr(v) for v in later), None) == ERR_STATE and "the next sample is 4" in h._last_error()
        with pytest.raises(ValueError, match="4 of 21 samples accumulated: the second pass is not complete"):
            h.result()
        h.accumulate(cl[4:], w[4:], tb[4:])
        assert np.array_equal(h.sums()[0], _default(21)["p_loo"]) and np.array_equal(h.result().loo_i, _default(21)["loo_i"])
    finally:
        h.close()


def test_a_changed_sample_or_prior_in_the_second_pass_is_refused_and_named():
    case = cases.synthetic(21)[0]
    cl, w, tb = (case[k] for k in SAMPLES)
    h = objloo.ObjLooHandle(0)
    try:
        _set(h, case)
        h.add(cl, w, tb)
        h.weights()
        h.accumulate(cl[:5], w[:5], tb[:5])
        before = h.sums()
        other = tb[5:].copy()
        other[3] = tb[0]                                       # sample 8 is another draw: valid, but not the one stored
        with pytest.raises(EngineError, match="sample 8: its rows differ from the ones sbe_objloo_add stored") as err:
            h.accumulate(cl[5:], w[5:], other)
        assert err.value.code == ERR_DATA
        after = h.sums()
        assert after[1] == before[1] == 5 and np.array_equal(after[0], before[0])
        with pytest.raises(EngineError, match="sample 5: its rows differ"):        # the same samples under another prior
            h.accumulate(cl[5:], w[5:], tb[5:], prior=np.array([0.4, 0.2, 0.2, 0.2]))
        swapped = np.ascontiguousarray(cl[5:][::-1])           # the samples in another order: the first of them differs
        with pytest.raises(EngineError, match="sample 5: its rows differ"):
            h.accumulate(swapped, np.ascontiguousarray(w[5:][::-1]), np.ascontiguousarray(tb[5:][::-1]))
        h.accumulate(cl[5:], w[5:], tb[5:])                    # the handle is usable afterwards
        assert np.array_equal(h.sums()[0], _default(21)["p_loo"])
    finally:
        h.close()


@pytest.mark.parametrize("spoil,match", [
    (lambda p: p.__setitem__((3, 2, 1), -0.25), "sample 3: the prior row of object 2 has an entry that is negative or not finite"),
    (lambda p: p.__setitem__((0, 4, 0), np.nan), "sample 0: the prior row of object 4 has an entry"),
    (lambda p: p.__setitem__((6, 1), p[6, 1] * 1.001), "sample 6: the prior row of object 1 .* sums further than 1e-05 from 1")])
def test_a_bad_prior_row_is_refused_and_named_in_either_pass(spoil, match):
    case = cases.synthetic(21)[0]
    good = cases.seeded_prior(21, 21, 5, 3, zero=False)
    bad = good.copy()
    spoil(bad)
    tb = case["tables"].copy()
    tb[6, 0, 0, 0] = -1.0                                      # the prior row is the seventh kind: of one sample's offenders predict's come first
    h = objloo.ObjLooHandle(0)
    try:
        _set(h, case)
        with pytest.raises(EngineError, match=match) as err:
            h.add(*(case[k] for k in SAMPLES), prior=bad)
        assert err.value.code == ERR_DATA and h.n_rows == 0
        if "sample 6" in match:
            with pytest.raises(EngineError, match=r"sample 6: tables\[0\]\[0\]\[0\]"):
                h.add(case["clusters"], case["weights"], tb, prior=bad)
        h.add(*(case[k] for k in SAMPLES), prior=good)
        h.weights()
        with pytest.raises(EngineError, match=match):
            h.accumulate(*(case[k] for k in SAMPLES), prior=bad)
        assert h.sums()[1] == 0 and not h.sums()[0].any()
        h.accumulate(*(case[k] for k in SAMPLES), prior=good)
        assert h.sums()[1] == 21
    finally:
        h.close()


def test_a_zero_likelihood_names_the_object_and_the_sample():
    finite, (n, t) = cases.zero_likelihood("finite")
    dev = _device(finite)
    want = orc.run(**finite)
    _check(dev, want, finite, None, "-inf in H")
    assert np.isneginf(dev["H"][t, n, :2]).all() and np.isfinite(dev["H"][t, n, 2:]).all()
    h = objloo.ObjLooHandle(0)
    try:
        for kind, text in (("conditional", "under the logged membership is zero"), ("marginal", "the marginal likelihood of its observed cells is zero")):
            case, (n, t) = cases.zero_likelihood(kind)
            _set(h, case)
            with pytest.raises(EngineError, match=rf"object {n}, sample {t}: .*{text}") as err:
                h.add(*(case[k] for k in SAMPLES))
            assert err.value.code == ERR_DATA and h.n_rows == 0
            h.add(*(case[k][:t] for k in SAMPLES))             # the samples before it are fine, and the store's index names it
            with pytest.raises(EngineError, match=rf"object {n}, sample {t}: "):
                h.add(*(case[k][t:] for k in SAMPLES))
            assert h.n_rows == t
        # every hypothesis the prior leaves has no likelihood: the marginal is zero although H holds finite entries
        case, (n, t) = cases.zero_likelihood("finite")
        _set(h, case)
        only = np.array([0.5, 0.5, 0.0, 0.0])
        with pytest.raises(EngineError, match=rf"object {n}, sample {t}: .*no membership with a positive prior"):
            h.add(*(case[k] for k in SAMPLES), prior=only)
    finally:
        h.close()


def test_an_observed_cell_without_a_confounder_names_the_cell_and_the_sample():
    case = dict(cases.synthetic(21)[0])
    groups = case["groups"].copy()
    groups[:, 2] = orc.NA
    f = int(np.flatnonzero(case["codes"][2] != orc.NA)[0])
    assert orc.first_unformed(case["codes"], groups, case["n_groups"], 3, case["weights"], case["tables"]) == (0, 2, f)
    h = objloo.ObjLooHandle(0)
    try:
        _set(h, {**case, "groups": groups})
        with pytest.raises(EngineError, match=rf"cell \(object 2, feature {f}\), sample 0: no confounder applies") as err:
            h.add(*(case[k] for k in SAMPLES))
        assert err.value.code == ERR_DATA and h.n_rows == 0
        # without confounders at all every observed cell is one
        one = cases.by_shape("C1")[0]
        codes = one["codes"].copy()
        codes[1, 2] = 0
        h.set_data(codes, one["groups"], one["n_groups"], 2, 2, capacity=3)
        with pytest.raises(EngineError, match=r"cell \(object 1, feature 2\), sample 0: no confounder applies"):
            h.add(*(one[k] for k in SAMPLES))
        # the second pass recomputes the rows with the first pass's code: the same refusal there
        _set(h, case)
        h.add(*(case[k] for k in SAMPLES))
        h.weights()
        w0 = case["weights"].copy()
        w0[2, 1] = [1.0, 0.0, 0.0]                             # sample 2: feature 1 takes its weight from the clusters alone
        cell = int(np.flatnonzero(case["codes"][:, 1] != orc.NA)[0])
        with pytest.raises(EngineError, match=rf"cell \(object {cell}, feature 1\), sample 2: no confounder applies"):
            h.accumulate(case["clusters"], w0, case["tables"])
        assert h.sums()[1] == 0
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
    case = cases.synthetic(21)[0]
    bad, match = _spoil(case, name)
    assert po.first_offender(*bad) is not None
    h = objloo.ObjLooHandle(0)
    try:
        _set(h, case)
        with pytest.raises(EngineError, match=match) as err:
            h.add(*bad)
        assert err.value.code == ERR_DATA and h.n_rows == 0 and h.store(with_weights=False)[1].shape == (5, 0)
        _pass(h.add, case, None, None)
        h.weights()
        with pytest.raises(EngineError, match=match):
            h.accumulate(*bad)
        assert h.sums()[1] == 0 and not h.sums()[0].any()
        _pass(h.accumulate, case, None, [9])
        assert np.array_equal(h.sums()[0], _default(21)["p_loo"])
    finally:
        h.close()


def test_the_data_and_the_store_limit_are_checked_and_one_handle_serves_many_shapes():
    h = objloo.ObjLooHandle(0)
    try:
        first = _run_on(h, cases.synthetic(5)[0])
        codes = np.zeros((4, 3), dtype=np.uint8)
        codes[2, 1] = 2
        with pytest.raises(EngineError, match=r"codes\[2\]\[1\]=2 is neither a state below 2 nor 255") as err:
            h.set_data(codes, np.zeros((0, 4), np.uint8), [], 2, 1, capacity=5)
        assert err.value.code == ERR_DATA
        with pytest.raises(ValueError, match="no data yet"):   # the handle takes nothing until the next set_data
            h.add(*(cases.synthetic(5)[0][k] for k in SAMPLES))
        groups = np.array([[0, 1, 2, 255]], dtype=np.uint8)
        with pytest.raises(EngineError, match=r"groups\[0\]\[2\]=2 is neither a group below 2 nor 255"):
            h.set_data(np.zeros((4, 3), np.uint8), groups, [2], 2, 1, capacity=5)
        wide = np.zeros((1 << 20, 1), dtype=np.uint8)
        for capacity, text in ((0, "capacity=0"), ((1 << 20) + 1, "capacity=1048577"), (1 << 20, "take 61572651155456 bytes on the device, the limit is 17179869184")):
            assert _raw(h, "set_data", 1 << 20, 1, 2, 1, 1, _ptr(wide), None, None, capacity) == ERR_ARG and text in h._last_error(), capacity
        assert _raw(h, "set_feature_tile", 257) == ERR_ARG
        # a larger shape, a smaller one, the first again: the same bits as on fresh handles
        assert _same(_run_on(h, cases.synthetic(21)[0]), _default(21))
        assert _same(_run_on(h, cases.by_shape("F1")[0], cases.by_shape("F1")[1]), _device(*cases.by_shape("F1")[:2]))
        assert _same(_run_on(h, cases.synthetic(5)[0]), first)
    finally:
        h.close()


def _run_on(h, case, prior=None):
    _set(h, case)
    return _run(h, case, prior)


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [0, 1])
def test_object_loo_on_the_recorded_runs(r):
    full = cases.loopred_cases.recorded(r, burn=0)
    case, want = cases.recorded(r), cases.recorded_oracle(r)
    res = objloo.object_loo(full["codes"], full["groups"], full["clusters"], full["weights"], full["tables"], burnin=0.1, device=0,
                            n_groups=full["n_groups"])
    assert res.n_samples == 54 and res.p_loo.shape == (100, 36, 5) and res.membership.shape == (100, 4) and all(v > 0 for v in res.kernel_ms.values())
    # the checker's own H differs from the device's by the logs' last bits, so the comparison with its totals is at the project's
    # figure for this arithmetic; _check below compares every stage on the device's own inputs
    for name in ("loo_i", "lppd_i", "n_eff", "loo_cond_i", "lppd_cond_i", "membership"):
        _close(getattr(res, name), want[name], f"run {r} {name}")
    for kind, column in (("k_i", "L"), ("k_cond_i", "Cnd")):
        tol = np.array([ps.tol_k(-want[column][:, n]) for n in range(100)])
        assert (tol < 1.01e-10).all() and (np.abs(getattr(res, kind) - want[kind]) <= tol).all(), kind    # its floor for every column
    assert round(res.elpd, 1) == round(float(want["loo_i"].sum()), 1) and round(res.elpd_cond, 1) == round(float(want["loo_cond_i"].sum()), 1)
    assert res.n_bad_k() == int((want["k_i"] > 0.7).sum()) and res.n_bad_k(conditional=True) == int((want["k_cond_i"] > 0.7).sum())
    # p_loo: with b the bound on log w of the object's column, every weight lies within a factor exp(+-b) of the checker's; a term
    # passes at most 2 C + K + 3 roundings before the T - 1 additions (the leave-one-out predictive's bound, its rows replaced by mz)
    b = lo.log_w_bound(want["w"]).max(axis=0)[:, None, None]
    g = po.gamma(54 + 2 * 3 + 3 + 3)
    assert (np.abs(res.p_loo - want["p_loo"]) <= want["p_loo"] * (np.expm1(b) * (1 + 2 * g) + 2 * g) + 54 * 8 * po.TINY).all()
    assert np.allclose(res.p_loo.sum(axis=2), 1.0, rtol=0, atol=1e-7)
    dev = _device(case)
    assert all(np.array_equal(dev[name], getattr(res, name)) for name in POINTWISE) and np.array_equal(dev["p_loo"], res.p_loo)
    _check(dev, want, case, None, f"recorded run {r}")
    # compare takes the vectors as they are: over 100 objects the conditional score is ahead, as the issue's table has it
    cmp = compare.compare({"cond": res.loo_cond_i, "marg": res.loo_i}, device=0)
    print(f"recorded run {r}: elpd {res.elpd:.1f} (se {res.se:.1f}), conditional {res.elpd_cond:.1f}; zero-shot accuracy {res.accuracy():.4f}, "
          f"Brier {res.brier():.4f}, log score {res.log_score():.4f}; {res.n_bad_k()} objects with k > 0.7 ({res.n_bad_k(conditional=True)} conditional)")
    print(cmp.text())
    bare = objloo.object_loo(full["codes"], full["groups"], full["clusters"], full["weights"], full["tables"], burnin=0.1, predictive=False, device=0,
                             n_groups=full["n_groups"])
    assert bare.p_loo is None and np.array_equal(bare.loo_i, res.loo_i) and bare.kernel_ms["accumulate"] == 0.0
