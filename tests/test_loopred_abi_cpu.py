"""CPU checks of the leave-one-out predictive unit's boundary (include/sbe_loopred.h, sbayes_amd/loopred.py): the symbols are
exported and bound by the module's own prototype table, the limits agree, and bad arguments are refused before the device is
touched."""
import ctypes as ct
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from sbayes_amd import elpd, loopred, predict
from tests import _abi_header as abi

REPO = Path(__file__).resolve().parent.parent
HEADER = (REPO / "include" / "sbe_loopred.h").read_text()
OWN = ("abi_version", "last_error", "create", "destroy", "last_kernel_ms", "store_bytes", "sample_bytes", "lds_max_samples", "set_data", "reset",
       "add", "weights", "accumulate", "read", "set_feature_tile", "get_store")


def test_every_symbol_of_the_header_is_exported_and_bound():
    names = abi.check_symbols(loopred, HEADER, len(OWN))
    assert names == sorted(f"sbe_loopred_{n}" for n in OWN)
    assert not set(names) & (set(predict.PROTOTYPES) | set(elpd.PROTOTYPES))   # the other units' headers and tables are left alone


def test_limits_agree_with_the_header():
    assert abi.macro(HEADER, "SBE_LOOPRED_MAX_SAMPLES") == "SBE_ELPD_MAX_SAMPLES" and loopred.MAX_SAMPLES == elpd.MAX_SAMPLES == 1 << 20
    assert abi.macro(HEADER, "SBE_LOOPRED_MAX_STORE_BYTES") == "(1ll << 34)" and loopred.MAX_STORE_BYTES == 1 << 34
    assert abi.macro(HEADER, "SBE_LOOPRED_MAX_STAGE_BYTES") == "SBE_PREDICT_MAX_STAGE_BYTES" and loopred.MAX_STAGE_BYTES == predict.MAX_STAGE_BYTES
    assert abi.macro(HEADER, "SBE_LOOPRED_MAX_TILE") == "SBE_PREDICT_MAX_TILE" and loopred.MAX_TILE == predict.MAX_TILE == 256
    assert loopred.NA is predict.NA and loopred.MIN_SAMPLES == 2


SHAPES_OK = [(100, 36, 5, 3, 3, 10), (1000, 200, 10, 2, 5, 15), (5, 3, 32, 1, 256, 256), (1 << 20, 1, 2, 1, 1, 1), (1, 1 << 16, 2, 8, 1, 8)]
SHAPES_PAST = [((1 << 20) + 1, 1, 2, 1, 1, 1), (1, (1 << 16) + 1, 2, 1, 1, 1), (5, 3, 33, 1, 1, 1), (5, 3, 2, 9, 1, 9), (5, 3, 2, 1, 257, 257),
               (5, 3, 2, 2, 3, 2), (1 << 20, 1 << 10, 2, 2, 1, 2)]


def test_the_byte_counts_of_the_module_and_the_library_agree():
    lib = loopred.load()
    for shape in SHAPES_OK:
        assert lib.sbe_loopred_sample_bytes(*shape) == loopred.sample_bytes(*shape) == predict.sample_bytes(*shape, True)
        assert predict.load().sbe_predict_sample_bytes(*shape, 1) == predict.sample_bytes(*shape, True)
    for shape in SHAPES_PAST:                                  # one past every limit: 0
        assert lib.sbe_loopred_sample_bytes(*shape) == 0
    for M, cap in [(0, 5), (1, 1), (3508, 54), (200_000, 1000), (7, 1 << 20)]:
        assert lib.sbe_loopred_store_bytes(M, cap) == loopred.store_bytes(M, cap) == 12 * M * cap
    assert loopred.store_bytes(200_000, 1000) == 2_400_000_000 < loopred.MAX_STORE_BYTES
    assert lib.sbe_loopred_store_bytes(-1, 5) == -1 and lib.sbe_loopred_store_bytes(5, -1) == -1 and lib.sbe_loopred_store_bytes(5, (1 << 20) + 1) == -1
    # the tail's keys carry the sample index: 16 bytes per tail slot against elpd's 12, so somewhat fewer samples fit the LDS
    assert 2 < loopred.lds_max_samples() < elpd.lds_max_samples() and elpd.lds_max_samples() - loopred.lds_max_samples() == 1024


def test_every_array_handed_to_the_library_is_bound_to_a_name():
    abi.check_ptr_arguments(loopred)


def test_c_abi_validates_before_the_device():
    free = {"sbe_loopred_abi_version", "sbe_loopred_last_error", "sbe_loopred_store_bytes", "sbe_loopred_sample_bytes", "sbe_loopred_lds_max_samples"}
    assert sorted(abi.check_null_handles(loopred)) == sorted(set(loopred.PROTOTYPES) - free)


def test_handles_are_not_picklable():
    abi.check_not_picklable(loopred.LooPredHandle)


def _offline_handle():
    h = object.__new__(loopred.LooPredHandle)
    h._h = ct.c_void_p()

    def refuse(*a, **k):
        raise AssertionError("the device was touched")
    h._lib = SimpleNamespace(**{name: refuse for name in loopred.PROTOTYPES})
    h.shape = None
    h._clear()
    return h


def _wide(shape):
    return np.broadcast_to(np.uint8(0), shape)


@pytest.mark.parametrize("shape,match", [
    (((1 << 20) + 1, 1, 2, 1, 1, []), "1048577 objects"), ((1, (1 << 16) + 1, 2, 1, 1, []), "65537 features"), ((5, 3, 33, 1, 1, []), "33 states"),
    ((5, 3, 2, 9, 1, [1] * 8), "9 components"), ((5, 3, 2, 2, 200, [57]), "make 257 table rows"), ((5, 3, 2, 1, 0, []), "at least one row")])
def test_shapes_are_checked_one_past_every_limit(shape, match):
    N, F, S, C, K, n_groups = shape
    with pytest.raises(ValueError, match=match):
        _offline_handle().set_data(_wide((N, F)), _wide((C - 1, N)), n_groups, S, K, capacity=10)


def test_a_handle_checks_its_own_arguments_before_the_library():
    h = _offline_handle()
    one = (np.zeros((1, 1, 1)), np.zeros((1, 1, 1)), np.zeros((1, 1, 1, 1)))
    for call in (h.reset, h.max_samples, h.result, h.weights, h.sums, h.store, lambda: h.add(*one), lambda: h.accumulate(*one)):
        with pytest.raises(ValueError, match="no data yet"):
            call()
    with pytest.raises(ValueError, match=r"codes must be \[N, F\]"):
        h.set_data(np.zeros(5, np.uint8), np.zeros((0, 5), np.uint8), [], 2, 1, capacity=4)
    with pytest.raises(ValueError, match=r"groups must be \[1, 5\]"):
        h.set_data(np.zeros((5, 3), np.uint8), np.zeros((1, 4), np.uint8), [2], 2, 1, capacity=4)
    for capacity in (0, (1 << 20) + 1):
        with pytest.raises(ValueError, match="capacity="):
            h.set_data(np.zeros((5, 3), np.uint8), np.zeros((0, 5), np.uint8), [], 2, 1, capacity=capacity)
    # the store limit: 2^20 observed cells x 2^20 samples x 12 bytes
    with pytest.raises(ValueError, match="bytes on the device, the limit is 17179869184"):
        h.set_data(_wide((1 << 10, 1 << 10)), np.zeros((0, 1 << 10), np.uint8), [], 2, 1, capacity=1 << 20)
    h.shape, h.capacity, h.n_observed = (5, 3, 2, 2, 1, 3), 4, 15
    with pytest.raises(ValueError, match="2 samples take clusters"):
        h.add(np.zeros((2, 1, 5), np.uint8), np.zeros((2, 3, 2)), np.zeros((2, 3, 3, 3)))
    ok = (np.zeros((5, 1, 5), np.uint8), np.zeros((5, 3, 2)), np.zeros((5, 3, 3, 2)))
    with pytest.raises(ValueError, match="5 more exceed the capacity of 4"):
        h.add(*ok)
    with pytest.raises(ValueError, match="PSIS needs at least 2"):
        h.weights()
    with pytest.raises(ValueError, match="no weights yet"):
        h.accumulate(*ok)
    with pytest.raises(ValueError, match="no weights yet"):
        h.result()
    assert h.max_samples() == (1 << 28) // (5 + 48 + 144 + 10 + 60)
    h.shape = (1 << 12, 1 << 12, 32, 1, 256, 256)             # one sample alone exceeds what a call holds
    with pytest.raises(ValueError, match="one sample takes"):
        h.add(_wide((1, 256, 1 << 12)), np.broadcast_to(0.0, (1, 1 << 12, 1)), np.broadcast_to(0.0, (1, 256, 1 << 12, 32)))


def test_the_one_call_form_checks_its_arguments_before_the_device(monkeypatch):
    monkeypatch.setattr(loopred, "LooPredHandle", lambda device: (_ for _ in ()).throw(AssertionError("the device was touched")))
    with pytest.raises(ValueError, match="clusters must be"):
        loopred.loo_predictive(np.zeros((5, 3), np.uint8), [], np.zeros((2, 5)), np.zeros((2, 3, 1)), np.zeros((2, 1, 3, 2)))
    args = (np.zeros((5, 3), np.uint8), [], np.zeros((2, 1, 5)), np.zeros((2, 3, 1)), np.zeros((2, 1, 3, 2)))
    with pytest.raises(ValueError, match="burnin="):
        loopred.loo_predictive(*args, burnin=1.0)
    with pytest.raises(ValueError, match="1 samples after burn-in"):
        loopred.loo_predictive(*args, burnin=0.5)
