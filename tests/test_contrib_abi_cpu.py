"""CPU checks of the per-cluster evidence unit's boundary (include/sbe_contrib.h, sbayes_amd/contribution.py): the symbols are
exported and bound by the module's own prototype table, the limits agree, and bad arguments are refused before the device is
touched."""
import ctypes as ct
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from sbayes_amd import contribution, ppc, predict
from tests import _abi_header as abi

REPO = Path(__file__).resolve().parent.parent
HEADER = (REPO / "include" / "sbe_contrib.h").read_text()


def test_every_symbol_of_the_header_is_exported_and_bound():
    names = abi.check_symbols(contribution, HEADER, 9)
    assert names == sorted(f"sbe_contrib_{n}" for n in ("abi_version", "last_error", "create", "destroy", "last_kernel_ms", "sample_bytes", "set_data",
                                                       "evaluate", "set_feature_tile"))
    assert not set(names) & (set(predict.PROTOTYPES) | set(ppc.PROTOTYPES))   # the other units' headers and tables are left alone


def test_limits_agree_with_the_header():
    assert abi.macro(HEADER, "SBE_CONTRIB_MAX_STAGE_BYTES") == "SBE_PREDICT_MAX_STAGE_BYTES"
    assert contribution.MAX_STAGE_BYTES == predict.MAX_STAGE_BYTES == 1 << 28
    assert abi.macro(HEADER, "SBE_CONTRIB_MAX_TILE") == "SBE_PREDICT_MAX_TILE" and contribution.MAX_TILE == predict.MAX_TILE == 256
    assert contribution.NA == predict.NA == 255


SHAPES_OK = [(100, 36, 5, 3, 3, 10), (1000, 200, 10, 2, 5, 15), (5, 3, 32, 1, 256, 256), (1 << 20, 1, 2, 1, 1, 1), (1, 1 << 16, 2, 8, 1, 8)]
SHAPES_PAST = [((1 << 20) + 1, 1, 2, 1, 1, 1), (1, (1 << 16) + 1, 2, 1, 1, 1), (5, 3, 33, 1, 1, 1), (5, 3, 2, 9, 1, 9), (5, 3, 2, 1, 257, 257),
               (5, 3, 2, 2, 3, 2), (1 << 20, 1 << 10, 2, 2, 1, 2)]


def test_the_sample_bytes_of_the_module_and_the_library_agree():
    lib = contribution.load()
    for shape in SHAPES_OK:
        assert lib.sbe_contrib_sample_bytes(*shape) == contribution.sample_bytes(*shape) > 0
        N, F, _S, _C, K, _R = shape
        assert contribution.sample_bytes(*shape) == predict.sample_bytes(*shape) + 8 * K * N * F + 8 * K * (N + F)
        assert predict.load().sbe_predict_sample_bytes(*shape, 0) == predict.sample_bytes(*shape)
    N, F, S, C, K, R = SHAPES_OK[0]
    assert contribution.sample_bytes(*SHAPES_OK[0]) == K * N + 8 * F * C + 8 * R * F * S + 2 * N + 8 * K * N * F + 8 * K * (N + F)
    for shape in SHAPES_PAST:                                  # one past every limit: 0
        assert lib.sbe_contrib_sample_bytes(*shape) == 0


def test_every_array_handed_to_the_library_is_bound_to_a_name():
    abi.check_ptr_arguments(contribution)


def test_c_abi_validates_before_the_device():
    assert sorted(abi.check_null_handles(contribution)) == sorted(set(contribution.PROTOTYPES) - {"sbe_contrib_abi_version", "sbe_contrib_last_error",
                                                                                                 "sbe_contrib_sample_bytes"})


def test_handles_are_not_picklable():
    abi.check_not_picklable(contribution.ContributionHandle)


def _offline_handle():
    h = object.__new__(contribution.ContributionHandle)
    h._h = ct.c_void_p()

    def refuse(*a, **k):
        raise AssertionError("the device was touched")
    h._lib = SimpleNamespace(**{name: refuse for name in contribution.PROTOTYPES})
    h.shape = None
    h._clear()
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
        R = K + sum(n_groups)
        assert contribution.sample_bytes(N, F, S, C, K, R) > 0 and contribution.load().sbe_contrib_sample_bytes(N, F, S, C, K, R) > 0
        return
    if N * F <= 1 << 26:                                       # the handle refuses the shape before the library sees it
        with pytest.raises(ValueError, match=match):
            _offline_handle().set_data(_wide((N, F)), _wide((C - 1, N)), n_groups, S, K)


def test_a_handle_checks_its_own_arguments_before_the_library():
    h = _offline_handle()
    for call in (h.reset, h.max_samples, h.result, lambda: h.evaluate(np.zeros((1, 1, 1)), np.zeros((1, 1, 1)), np.zeros((1, 1, 1, 1)))):
        with pytest.raises(ValueError, match="no data yet"):
            call()
    with pytest.raises(ValueError, match=r"codes must be \[N, F\]"):
        h.set_data(np.zeros(5, np.uint8), np.zeros((0, 5), np.uint8), [], 2, 1)
    with pytest.raises(ValueError, match=r"groups must be \[1, 5\]"):
        h.set_data(np.zeros((5, 3), np.uint8), np.zeros((1, 4), np.uint8), [2], 2, 1)
    h.shape = (5, 3, 2, 2, 1, 3)
    with pytest.raises(ValueError, match="no sample was evaluated"):
        h.result()
    with pytest.raises(ValueError, match="2 samples take clusters"):
        h.evaluate(np.zeros((2, 1, 5), np.uint8), np.zeros((2, 3, 2)), np.zeros((2, 3, 3, 3)))
    base = 5 + 48 + 144 + 10 + 8 * 15 + 8 * 8
    assert h.max_samples() == (1 << 28) // base
    h.shape = (1 << 12, 1 << 12, 32, 1, 256, 256)             # one sample alone exceeds what a call holds
    with pytest.raises(ValueError, match="one sample takes"):
        h.evaluate(_wide((1, 256, 1 << 12)), np.broadcast_to(0.0, (1, 1 << 12, 1)), np.broadcast_to(0.0, (1, 256, 1 << 12, 32)))


def test_the_one_call_form_checks_its_arguments_before_the_device(monkeypatch):
    monkeypatch.setattr(contribution, "ContributionHandle", lambda device: (_ for _ in ()).throw(AssertionError("the device was touched")))
    with pytest.raises(ValueError, match="clusters must be"):
        contribution.cluster_contribution(np.zeros((5, 3), np.uint8), [], np.zeros((2, 5)), np.zeros((2, 3, 1)), np.zeros((2, 1, 3, 2)))
    args = (np.zeros((5, 3), np.uint8), [], np.zeros((2, 1, 5)), np.zeros((2, 3, 1)), np.zeros((2, 1, 3, 2)))
    with pytest.raises(ValueError, match="burnin="):
        contribution.cluster_contribution(*args, burnin=1.0)
