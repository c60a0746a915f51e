"""CPU checks of the leave-one-object-out unit's boundary (include/sbe_objloo.h, sbayes_amd/objloo.py): the symbols are
exported and bound by the module's own prototype table, the limits agree, and bad arguments are refused before the device is
touched."""
import ctypes as ct
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from sbayes_amd import elpd, loopred, objloo, predict, psens
from tests import _abi_header as abi

REPO = Path(__file__).resolve().parent.parent
HEADER = (REPO / "include" / "sbe_objloo.h").read_text()
OWN = ("abi_version", "last_error", "create", "destroy", "last_kernel_ms", "store_bytes", "sample_bytes", "lds_max_samples", "set_data", "reset",
       "add", "weights", "accumulate", "read", "set_feature_tile", "get_store")


def test_every_symbol_of_the_header_is_exported_and_bound():
    names = abi.check_symbols(objloo, HEADER, len(OWN))
    assert names == sorted(f"sbe_objloo_{n}" for n in OWN)
    assert not set(names) & (set(predict.PROTOTYPES) | set(elpd.PROTOTYPES) | set(loopred.PROTOTYPES))   # the other units' tables are left alone
    # the header follows sbe_loopred.h in its order
    declared = re.findall(r"\b(sbe_objloo_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S))
    assert tuple(n[len("sbe_objloo_"):] for n in declared) == OWN


def test_limits_agree_with_the_header():
    assert abi.macro(HEADER, "SBE_OBJLOO_MAX_SAMPLES") == "SBE_ELPD_MAX_SAMPLES" and objloo.MAX_SAMPLES == elpd.MAX_SAMPLES == 1 << 20
    assert abi.macro(HEADER, "SBE_OBJLOO_MAX_STORE_BYTES") == "(1ll << 34)" and objloo.MAX_STORE_BYTES == 1 << 34
    assert abi.macro(HEADER, "SBE_OBJLOO_MAX_STAGE_BYTES") == "SBE_PREDICT_MAX_STAGE_BYTES" and objloo.MAX_STAGE_BYTES == predict.MAX_STAGE_BYTES
    assert abi.macro(HEADER, "SBE_OBJLOO_MAX_TILE") == "SBE_PREDICT_MAX_TILE" and objloo.MAX_TILE == predict.MAX_TILE == 256
    assert objloo.NA is predict.NA and objloo.MIN_SAMPLES == 2 and objloo.SUM_TOL == 1e-5
    assert objloo.POINTWISE == ("loo_i", "k_i", "n_eff", "lppd_i", "loo_cond_i", "k_cond_i", "lppd_cond_i")


SHAPES_OK = [(100, 36, 5, 3, 3, 10), (1000, 200, 10, 2, 5, 15), (5, 3, 32, 1, 256, 256), (1 << 20, 1, 2, 1, 1, 1), (1, 1 << 16, 2, 8, 1, 8)]
SHAPES_PAST = [((1 << 20) + 1, 1, 2, 1, 1, 1), (1, (1 << 16) + 1, 2, 1, 1, 1), (5, 3, 33, 1, 1, 1), (5, 3, 2, 9, 1, 9), (5, 3, 2, 1, 257, 257),
               (5, 3, 2, 2, 3, 2), (1 << 20, 1 << 10, 2, 2, 1, 2)]


def test_the_byte_counts_of_the_module_and_the_library_agree():
    lib = objloo.load()
    for shape in SHAPES_OK:
        N, F, _S, _C, K, _R = shape
        assert lib.sbe_objloo_sample_bytes(*shape) == objloo.sample_bytes(*shape) == predict.sample_bytes(*shape) + 8 * (K + 1) * N * (F + 2)
    for shape in SHAPES_PAST:                                  # one past every limit: 0
        assert lib.sbe_objloo_sample_bytes(*shape) == 0
    for N, K, cap in [(0, 1, 5), (1, 1, 1), (100, 3, 54), (1000, 5, 1000), (7, 256, 1 << 20)]:
        assert lib.sbe_objloo_store_bytes(N, K, cap) == objloo.store_bytes(N, K, cap) == 8 * N * cap * (2 * K + 5)
    assert objloo.store_bytes(1000, 5, 1000) == 120_000_000 < objloo.MAX_STORE_BYTES
    for bad in ((-1, 1, 5), (5, 0, 5), (5, 1, -1), (5, 1, (1 << 20) + 1)):
        assert lib.sbe_objloo_store_bytes(*bad) == -1
    # the keys are psens's 12 bytes per sample, and the tail's exceedances share the LDS: somewhat fewer samples than psens sorts there
    T = objloo.lds_max_samples()

    def lds(t):
        return 12 * t + 8 * int(np.ceil(min(0.2 * t, 3 * np.sqrt(t)))) + 8192
    assert lds(T) <= 160 << 10 < lds(T + 1)
    assert 2 < T < psens.lds_max_draws()


def test_every_array_handed_to_the_library_is_bound_to_a_name():
    abi.check_ptr_arguments(objloo)


def test_c_abi_validates_before_the_device():
    free = {"sbe_objloo_abi_version", "sbe_objloo_last_error", "sbe_objloo_store_bytes", "sbe_objloo_sample_bytes", "sbe_objloo_lds_max_samples"}
    assert sorted(abi.check_null_handles(objloo)) == sorted(set(objloo.PROTOTYPES) - free)


def test_handles_are_not_picklable():
    abi.check_not_picklable(objloo.ObjLooHandle)


def _offline_handle():
    h = object.__new__(objloo.ObjLooHandle)
    h._h = ct.c_void_p()

    def refuse(*a, **k):
        raise AssertionError("the device was touched")
    h._lib = SimpleNamespace(**{name: refuse for name in objloo.PROTOTYPES})
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
    # the store limit: 2^20 objects x 2^20 samples x 8 (2 (K + 1) + 3) bytes
    with pytest.raises(ValueError, match="bytes on the device, the limit is 17179869184"):
        h.set_data(_wide((1 << 20, 1)), np.zeros((0, 1 << 20), np.uint8), [], 2, 1, capacity=1 << 20)
    h.shape, h.capacity = (5, 3, 2, 2, 1, 3), 4
    with pytest.raises(ValueError, match="2 samples take clusters"):
        h.add(np.zeros((2, 1, 5), np.uint8), np.zeros((2, 3, 2)), np.zeros((2, 3, 3, 3)))
    ok = (np.zeros((5, 1, 5), np.uint8), np.zeros((5, 3, 2)), np.zeros((5, 3, 3, 2)))
    with pytest.raises(ValueError, match="5 more exceed the capacity of 4"):
        h.add(*ok)
    h.capacity = 8
    for prior in (np.zeros(3), np.zeros((4, 2)), np.zeros((5, 5, 3)), np.zeros((1, 5, 5, 2))):
        with pytest.raises(ValueError, match=r"prior must be None, \[2\], \[5, 2\] or \[5, 5, 2\]"):
            h.add(*ok, prior=prior)
    with pytest.raises(ValueError, match="PSIS needs at least 2"):
        h.weights()
    with pytest.raises(ValueError, match="no weights yet"):
        h.accumulate(*ok)
    with pytest.raises(ValueError, match="no weights yet"):
        h.result()
    assert h.max_samples() == (1 << 28) // (5 + 48 + 144 + 10 + 8 * 2 * 5 * 3 + 16 * 2 * 5)
    h.shape = (1 << 12, 1 << 12, 32, 1, 256, 256)             # one sample alone exceeds what a call holds
    with pytest.raises(ValueError, match="one sample takes"):
        h.add(_wide((1, 256, 1 << 12)), np.broadcast_to(0.0, (1, 1 << 12, 1)), np.broadcast_to(0.0, (1, 256, 1 << 12, 32)))


def test_the_prior_is_broadcast_on_the_host():
    assert objloo.broadcast_prior(None, 3, 2, 1) is None
    row = np.array([0.25, 0.75])
    for prior in (row, np.stack([row, row]), np.broadcast_to(row, (3, 2, 2))):
        out = objloo.broadcast_prior(prior, 3, 2, 1)
        assert out.shape == (3, 2, 2) and out.flags["C_CONTIGUOUS"] and out.dtype == np.float64 and (out == row).all()


def test_the_one_call_form_checks_its_arguments_before_the_device(monkeypatch):
    monkeypatch.setattr(objloo, "ObjLooHandle", lambda device: (_ for _ in ()).throw(AssertionError("the device was touched")))
    with pytest.raises(ValueError, match="clusters must be"):
        objloo.object_loo(np.zeros((5, 3), np.uint8), [], np.zeros((2, 5)), np.zeros((2, 3, 1)), np.zeros((2, 1, 3, 2)))
    args = (np.zeros((5, 3), np.uint8), [], np.zeros((2, 1, 5)), np.zeros((2, 3, 1)), np.zeros((2, 1, 3, 2)))
    with pytest.raises(ValueError, match="burnin="):
        objloo.object_loo(*args, burnin=1.0)
    with pytest.raises(ValueError, match="1 samples after burn-in"):
        objloo.object_loo(*args, burnin=0.5)
    with pytest.raises(ValueError, match="prior must be None"):
        objloo.object_loo(*args, prior=np.zeros(3), burnin=0.0)
    with pytest.raises(ValueError, match="3 prior blocks for 2 samples"):
        objloo.object_loo(*args, prior=np.zeros((3, 5, 2)), burnin=0.0)
