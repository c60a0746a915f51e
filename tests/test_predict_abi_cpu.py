"""CPU checks of the posterior predictive's boundary (include/sbe_predict.h, sbayes_amd/predict.py): the symbols are exported
and bound by the module's own prototype table, the limits agree, and bad arguments are refused before the device is touched."""
import ctypes as ct
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from sbayes_amd import predict
from tests import _abi_header as abi

REPO = Path(__file__).resolve().parent.parent
HEADER = (REPO / "include" / "sbe_predict.h").read_text()


def test_every_symbol_of_the_header_is_exported_and_bound():
    abi.check_symbols(predict, HEADER, 11)


def test_limits_agree_with_the_header():
    assert abi.macro(HEADER, "SBE_PREDICT_MAX_STATES") == str(predict.MAX_STATES) == "32"
    assert abi.macro(HEADER, "SBE_PREDICT_MAX_COMPONENTS") == str(predict.MAX_COMPONENTS) == "8"
    assert abi.macro(HEADER, "SBE_PREDICT_MAX_ROWS") == str(predict.MAX_ROWS) == "256"
    assert abi.macro(HEADER, "SBE_PREDICT_MAX_OBJECTS") == "(1 << 20)" and predict.MAX_OBJECTS == 1 << 20
    assert abi.macro(HEADER, "SBE_PREDICT_MAX_FEATURES") == "(1 << 16)" and predict.MAX_FEATURES == 1 << 16
    assert abi.macro(HEADER, "SBE_PREDICT_MAX_ACC_BYTES") == "(1ll << 32)" and predict.MAX_ACC_BYTES == 1 << 32
    assert abi.macro(HEADER, "SBE_PREDICT_MAX_STAGE_BYTES") == "(1ll << 28)" and predict.MAX_STAGE_BYTES == 1 << 28
    assert abi.macro(HEADER, "SBE_PREDICT_MAX_TILE") == str(predict.MAX_TILE) == "256"
    assert float(abi.macro(HEADER, "SBE_PREDICT_SUM_TOL")) == predict.SUM_TOL == 1e-5
    assert abi.macro(HEADER, "SBE_PREDICT_NA") == str(predict.NA) == "255"
    # the largest table of one sample at the smallest tile still fits the LDS twice over: R = 256, S = 32, C = 8, one feature
    assert 2 * (256 * 32 + 8) * 8 <= 160 << 10


def test_the_sample_bytes_of_the_module_and_the_library_agree():
    lib = predict.load()
    for shape in [(100, 36, 5, 3, 3, 10), (1000, 200, 10, 2, 5, 15), (5, 3, 32, 1, 256, 256), (1 << 20, 1, 2, 1, 1, 1), (1, 1 << 16, 2, 8, 1, 8)]:
        for lik in (0, 1):
            assert lib.sbe_predict_sample_bytes(*shape, lik) == predict.sample_bytes(*shape, bool(lik)) > 0
    # one past every limit: 0
    for shape in [((1 << 20) + 1, 1, 2, 1, 1, 1), (1, (1 << 16) + 1, 2, 1, 1, 1), (5, 3, 33, 1, 1, 1), (5, 3, 2, 9, 1, 9), (5, 3, 2, 1, 257, 257),
                  (5, 3, 2, 2, 3, 2), (1 << 20, 1 << 10, 2, 2, 1, 2)]:
        assert lib.sbe_predict_sample_bytes(*shape, 0) == 0


def test_every_array_handed_to_the_library_is_bound_to_a_name():
    abi.check_ptr_arguments(predict)


def test_c_abi_validates_before_the_device():
    assert sorted(abi.check_null_handles(predict)) == sorted(set(predict.PROTOTYPES) - {"sbe_predict_abi_version", "sbe_predict_last_error",
                                                                                       "sbe_predict_sample_bytes"})


def test_handles_are_not_picklable():
    abi.check_not_picklable(predict.PredictHandle)


def _offline_handle():
    h = object.__new__(predict.PredictHandle)
    h._h = ct.c_void_p()

    def refuse(*a, **k):
        raise AssertionError("the device was touched")
    h._lib = SimpleNamespace(**{name: refuse for name in predict.PROTOTYPES})
    h.shape, h._codes = None, None
    return h


def _wide(shape):
    return np.broadcast_to(np.uint8(0), shape)


SHAPES = [  # (N, F, S, C, K, n_groups) at the edge ...
    ((1 << 20, 1, 2, 1, 1, []), None), ((1, 1 << 16, 2, 1, 1, []), None), ((5, 3, 32, 1, 1, []), None), ((5, 3, 2, 8, 1, [1] * 7), None),
    ((5, 3, 2, 2, 200, [56]), None), ((5, 3, 2, 1, 256, []), None),
    # ... and one past it
    (((1 << 20) + 1, 1, 2, 1, 1, []), "1048577 objects"), ((1, (1 << 16) + 1, 2, 1, 1, []), "65537 features"), ((5, 3, 33, 1, 1, []), "33 states"),
    ((5, 3, 0, 1, 1, []), "0 states"), ((5, 3, 2, 9, 1, [1] * 8), "9 components"), ((5, 3, 2, 2, 200, [57]), "make 257 table rows"),
    ((5, 3, 2, 1, 257, []), "make 257 table rows"), ((5, 3, 2, 1, 0, []), "at least one row"), ((5, 3, 2, 2, 1, [0]), "at least one row"),
    ((1 << 20, 1 << 10, 2, 2, 1, [1]), "bytes on the device"),
]


@pytest.mark.parametrize("shape,match", SHAPES)
def test_shapes_are_checked_at_and_one_past_every_limit(shape, match):
    N, F, S, C, K, n_groups = shape
    if match is None:
        assert predict._check_shape(N, F, S, C, K, n_groups) == K + sum(n_groups)
        return
    with pytest.raises(ValueError, match=match):
        predict._check_shape(N, F, S, C, K, n_groups)
    if N * F <= 1 << 26:                                      # the handle refuses the same shape before the library sees it
        with pytest.raises(ValueError, match=match):
            _offline_handle().set_data(_wide((N, F)), _wide((C - 1, N)), n_groups, S, K)


def test_a_handle_checks_its_own_arguments_before_the_library():
    h = _offline_handle()
    for call in (h.reset, h.sums, h.max_samples, lambda: h.accumulate(np.zeros((1, 1, 1)), np.zeros((1, 1, 1)), np.zeros((1, 1, 1, 1)))):
        with pytest.raises(ValueError, match="no data yet"):
            call()
    with pytest.raises(ValueError, match=r"codes must be \[N, F\]"):
        h.set_data(np.zeros(5, np.uint8), np.zeros((0, 5), np.uint8), [], 2, 1)
    with pytest.raises(ValueError, match=r"groups must be \[1, 5\]"):
        h.set_data(np.zeros((5, 3), np.uint8), np.zeros((1, 4), np.uint8), [2], 2, 1)
    h.shape = (5, 3, 2, 2, 1, 3)
    with pytest.raises(ValueError, match="2 samples take clusters"):
        h.accumulate(np.zeros((2, 1, 5), np.uint8), np.zeros((2, 3, 2)), np.zeros((2, 3, 3, 3)))
    assert h.max_samples() == (1 << 28) // (5 + 48 + 144 + 10) and h.max_samples(lik=True) == (1 << 28) // (5 + 48 + 144 + 10 + 60)
    h.shape = (1 << 12, 1 << 12, 32, 1, 256, 256)             # one sample alone exceeds what a call holds
    with pytest.raises(ValueError, match="one sample takes"):
        h.accumulate(_wide((1, 256, 1 << 12)), np.broadcast_to(0.0, (1, 1 << 12, 1)), np.broadcast_to(0.0, (1, 256, 1 << 12, 32)))
    for burnin in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError, match="burnin="):
            predict._check_burnin(burnin, 10)
    assert predict._check_burnin(0.1, 60) == 6


def test_the_forms_of_the_reference_become_indices():
    onehot = np.zeros((2, 2, 3), dtype=bool)
    onehot[0, 0, 2] = onehot[1, 1, 0] = True
    assert predict.codes_of(onehot).tolist() == [[2, 255], [255, 0]]
    assert predict.group_index(np.array([[0, 1, 0], [1, 0, 0]], dtype=bool)).tolist() == [1, 0, 255]
    with pytest.raises(ValueError, match="object 1 is in two groups"):
        predict.group_index(np.array([[0, 1], [1, 1]], dtype=bool))


def test_the_result_imputes_scores_and_prints():
    codes = np.array([[0, 255], [1, 255]], dtype=np.uint8)
    pred = np.array([[[3.0, 1.0], [2.0, 2.0]], [[1.0, 3.0], [0.5, 3.5]]])
    resp = np.array([[[1.0, 3.0], [0.0, 0.0]], [[0.0, 0.0], [0.0, 0.0]]])
    res = predict.PredictResult(codes=codes, pred_sum=pred, resp_sum=resp, n_samples=4, n_zero=4)
    assert res.probs[1, 1].tolist() == [0.125, 0.875]
    filled, p = res.impute()
    assert filled.tolist() == [[0, 0], [1, 1]] and p.tolist() == [[0.75, 0.5], [0.75, 0.875]]        # the tie goes to the lowest index
    r = res.responsibility
    assert r[0, 0].tolist() == [0.25, 0.75] and np.isnan(r[0, 1]).all() and np.isnan(r[1, 0]).all()   # NA, and no sample contributed
    truth = np.array([[0, 1], [1, 0]], dtype=np.uint8)
    assert res.log_score(truth, codes == 255) == pytest.approx(np.log(0.5) + np.log(0.125))
    with pytest.raises(ValueError, match="holds no state"):
        res.log_score(codes, codes == 255)
    header, rows = res.table(state_names=[["N", "Y"], ["A", "B"]], component_names=["areal", "universal"])
    assert header == ["object", "feature", "observed", "predicted", "probability", "resp_areal", "resp_universal"]
    assert [row[:5] for row in rows] == [[0, "F2", "", "A", 0.5], [1, "F2", "", "B", 0.875]]
    assert len(res.table(na_only=False)[1]) == 4
