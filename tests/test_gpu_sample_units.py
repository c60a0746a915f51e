"""GPU checks of the sample store the four units that replay logged samples share (csrc/sbe_predict_row.hip.h, sbayes_amd/_samples.py):
one handle per unit goes through a small shape, a larger one that makes every buffer grow (without confounders: null groups; F = 17
is no power of two and past the default tile of 16), a set_data the library refuses, and the small shape again, whose result
must be the first one's bit for bit although the buffers are now larger than it needs.  Every result is compared to the unit's
oracle with the comparison of the unit's own GPU test."""
from functools import lru_cache

import numpy as np
import pytest

from sbayes_amd import contribution, loopred, ppc, predict
from sbayes_amd._handle import EngineError
from tests import _contrib_oracle, _loopred_oracle, _ppc_oracle
from tests import _predict_oracle as po
from tests import test_gpu_contrib, test_gpu_loopred, test_gpu_ppc, test_gpu_predict

pytestmark = pytest.mark.gpu

T = max(12, loopred.MIN_SAMPLES)
SHAPES = {"A": (4101, 5, 3, 2, 2, 2, [2]), "B": (4102, 130, 17, 3, 1, 1, [])}     # seed, N, F, S, C, K, group counts
SAMPLES = ("clusters", "weights", "tables")
SEED = 77                                                                          # of the check's replicates


@lru_cache(maxsize=None)
def _case(name):
    """A seeded case of a shape in which every object has a component in every sample, so that every observed cell has a positive
    likelihood (the leave-one-out weights need one)."""
    seed, N, F, S, C, K, counts = SHAPES[name]
    case = po.random_case(seed, N, F, S, C, K, T, group_counts=counts)
    if C > 1:
        case["groups"][0][case["groups"][0] == po.NA] = 0
    else:
        case["clusters"][:, 0, :][~case["clusters"].any(axis=1)] = 1
    assert po.first_offender(*(case[k] for k in SAMPLES)) is None
    return case


def _sequence(h, set_data, compute, check, same):
    """The four steps on handle h.  set_data(h, case); compute(h, case) -> result; check(result, case); same(a, b)."""
    a, b = _case("A"), _case("B")
    set_data(h, a)
    first = compute(h, a)
    check(first, a)
    set_data(h, b)
    check(compute(h, b), b)
    S = SHAPES["B"][3]
    spoiled = dict(b, codes=b["codes"].copy())
    spoiled["codes"][7, 5] = S
    with pytest.raises(EngineError, match=rf"codes\[7\]\[5\]={S} ") as e:
        set_data(h, spoiled)
    assert e.value.code == 4
    with pytest.raises(ValueError, match="no data yet"):
        compute(h, b)
    set_data(h, a)
    again = compute(h, a)
    check(again, a)
    assert same(first, again)


def test_predict_reuses_its_handle_across_shapes():
    @lru_cache(maxsize=None)
    def want(name):
        return po.run(**_case(name))

    def compute(h, case):
        rows = h.accumulate(*(case[k] for k in SAMPLES), lik=True)
        return (*h.sums(), rows)

    def check(dev, case):
        name = "A" if case is _case("A") else "B"
        test_gpu_predict._check(dev, want(name), T, SHAPES[name][4])

    def same(x, y):
        return all(np.array_equal(u, v) for u, v in zip(x, y))
    h = predict.PredictHandle(0)
    try:
        _sequence(h, test_gpu_predict._set, compute, check, same)
    finally:
        h.close()


def test_ppc_reuses_its_handle_across_shapes():
    def compute(h, case):
        h.check(*(case[k] for k in SAMPLES), seed=SEED, replicates=True)
        return h.result()

    def check(res, case):
        want = _ppc_oracle.check(seed=SEED, **case)
        assert want["margin"][want["drawn"]].min() > _ppc_oracle.MARGIN       # (the case: no draw sits on a cdf step)
        test_gpu_ppc._check(res, want, f"N={case['codes'].shape[0]}")
        assert res.n_samples == T
    h = ppc.PpcHandle(0)
    try:
        _sequence(h, test_gpu_ppc._set, compute, check, test_gpu_ppc._same_bits)
    finally:
        h.close()


def test_contrib_reuses_its_handle_across_shapes():
    def check(res, case):
        test_gpu_contrib._check(res, _contrib_oracle.evaluate(**case), f"N={case['codes'].shape[0]}")
        assert res.n_samples == T
    h = contribution.ContributionHandle(0)
    try:
        _sequence(h, test_gpu_contrib._set, test_gpu_contrib._run, check, test_gpu_contrib._same_bits)
    finally:
        h.close()


def test_loopred_reuses_its_handle_across_shapes():
    def check(dev, case):
        test_gpu_loopred._check(dev, _loopred_oracle.run(**case), case, f"N={case['codes'].shape[0]}")
    h = loopred.LooPredHandle(0)
    try:
        _sequence(h, test_gpu_loopred._set, test_gpu_loopred._run, check, test_gpu_loopred._same)
    finally:
        h.close()
