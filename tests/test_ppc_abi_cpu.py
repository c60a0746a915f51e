"""CPU checks of the posterior predictive check's boundary (include/sbe_ppc.h, sbayes_amd/ppc.py): the symbols are exported and
bound by the module's own prototype table, the limits agree, and bad arguments are refused before the device is touched."""
import ctypes as ct
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from sbayes_amd import ppc, predict
from tests import _abi_header as abi

REPO = Path(__file__).resolve().parent.parent
HEADER = (REPO / "include" / "sbe_ppc.h").read_text()


def test_every_symbol_of_the_header_is_exported_and_bound():
    names = abi.check_symbols(ppc, HEADER, 9)
    assert names == sorted(f"sbe_ppc_{n}" for n in ("abi_version", "last_error", "create", "destroy", "last_kernel_ms", "sample_bytes", "set_data",
                                                   "check", "set_feature_tile"))
    assert not set(names) & set(predict.PROTOTYPES)           # the posterior predictive's header and table are left alone


def test_limits_agree_with_the_header():
    assert abi.macro(HEADER, "SBE_PPC_MAX_STAGE_BYTES") == "SBE_PREDICT_MAX_STAGE_BYTES" and ppc.MAX_STAGE_BYTES == predict.MAX_STAGE_BYTES == 1 << 28
    assert abi.macro(HEADER, "SBE_PPC_MAX_TILE") == "SBE_PREDICT_MAX_TILE" and ppc.MAX_TILE == predict.MAX_TILE == 256
    assert ppc.NA == predict.NA == 255


SHAPES_OK = [(100, 36, 5, 3, 3, 10), (1000, 200, 10, 2, 5, 15), (5, 3, 32, 1, 256, 256), (1 << 20, 1, 2, 1, 1, 1), (1, 1 << 16, 2, 8, 1, 8)]
SHAPES_PAST = [((1 << 20) + 1, 1, 2, 1, 1, 1), (1, (1 << 16) + 1, 2, 1, 1, 1), (5, 3, 33, 1, 1, 1), (5, 3, 2, 9, 1, 9), (5, 3, 2, 1, 257, 257),
               (5, 3, 2, 2, 3, 2), (1 << 20, 1 << 10, 2, 2, 1, 2)]


def test_the_sample_bytes_of_the_module_and_the_library_agree():
    lib = ppc.load()
    for shape in SHAPES_OK:
        for y in (0, 1):
            for u in (0, 1):
                assert lib.sbe_ppc_sample_bytes(*shape, y, u) == ppc.sample_bytes(*shape, bool(y), bool(u)) > 0
    N, F, S, C, K, R = SHAPES_OK[0]
    base = K * N + 8 * F * C + 8 * R * F * S + 2 * N + 16 * N * F + 16 * F + 16 * N + 4 * F * S
    assert ppc.sample_bytes(*SHAPES_OK[0]) == base and ppc.sample_bytes(*SHAPES_OK[0], True, True) == base + 9 * N * F
    for shape in SHAPES_PAST:                                  # one past every limit: 0
        assert lib.sbe_ppc_sample_bytes(*shape, 0, 0) == 0


def test_every_array_handed_to_the_library_is_bound_to_a_name():
    abi.check_ptr_arguments(ppc)


def test_c_abi_validates_before_the_device():
    assert sorted(abi.check_null_handles(ppc)) == sorted(set(ppc.PROTOTYPES) - {"sbe_ppc_abi_version", "sbe_ppc_last_error", "sbe_ppc_sample_bytes"})


def test_handles_are_not_picklable():
    abi.check_not_picklable(ppc.PpcHandle)


def _offline_handle():
    h = object.__new__(ppc.PpcHandle)
    h._h = ct.c_void_p()

    def refuse(*a, **k):
        raise AssertionError("the device was touched")
    h._lib = SimpleNamespace(**{name: refuse for name in ppc.PROTOTYPES})
    h.shape, h._codes = None, None
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
        assert ppc.sample_bytes(N, F, S, C, K, K + sum(n_groups)) > 0 and ppc.load().sbe_ppc_sample_bytes(N, F, S, C, K, K + sum(n_groups), 1, 1) > 0
        return
    if N * F <= 1 << 26:                                       # the handle refuses the shape before the library sees it
        with pytest.raises(ValueError, match=match):
            _offline_handle().set_data(_wide((N, F)), _wide((C - 1, N)), n_groups, S, K)


def test_a_handle_checks_its_own_arguments_before_the_library():
    h = _offline_handle()
    for call in (h.reset, h.max_samples, h.result, lambda: h.check(np.zeros((1, 1, 1)), np.zeros((1, 1, 1)), np.zeros((1, 1, 1, 1)))):
        with pytest.raises(ValueError, match="no data yet"):
            call()
    with pytest.raises(ValueError, match=r"codes must be \[N, F\]"):
        h.set_data(np.zeros(5, np.uint8), np.zeros((0, 5), np.uint8), [], 2, 1)
    with pytest.raises(ValueError, match=r"groups must be \[1, 5\]"):
        h.set_data(np.zeros((5, 3), np.uint8), np.zeros((1, 4), np.uint8), [2], 2, 1)
    h.shape = (5, 3, 2, 2, 1, 3)
    with pytest.raises(ValueError, match="no sample was checked"):
        h.result()
    good = (np.zeros((2, 1, 5), np.uint8), np.zeros((2, 3, 2)), np.zeros((2, 3, 3, 2)))
    with pytest.raises(ValueError, match="2 samples take clusters"):
        h.check(np.zeros((2, 1, 5), np.uint8), np.zeros((2, 3, 2)), np.zeros((2, 3, 3, 3)))
    for seed in (-1, 1 << 64):
        with pytest.raises(ValueError, match="seed="):
            h.check(*good, seed=seed)
    # the uniforms: dtype, shape, range
    with pytest.raises(ValueError, match="uniforms must be float64, got float32"):
        h.check(*good, uniforms=np.zeros((2, 15), np.float32))
    with pytest.raises(ValueError, match=r"uniforms must be \[2, 15\]"):
        h.check(*good, uniforms=np.zeros((2, 14)))
    with pytest.raises(ValueError, match=r"uniforms must be \[2, 15\]"):
        h.check(*good, uniforms=np.zeros((1, 15)))
    for value in (1.0, -2.0 ** -60, float("nan"), float("inf")):
        u = np.zeros((2, 5, 3))
        u[1, 2, 1] = value
        with pytest.raises(ValueError, match=r"uniforms\[1\]\[7\]=.* is outside \[0, 1\) or not finite"):
            h.check(*good, uniforms=u)
    base = 5 + 48 + 144 + 10 + 240 + 48 + 80 + 24
    assert h.max_samples() == (1 << 28) // base and h.max_samples(replicates=True) == (1 << 28) // (base + 15)
    assert h.max_samples(uniforms=True) == (1 << 28) // (base + 120) and h.max_samples(True, True) == (1 << 28) // (base + 135)
    h.shape = (1 << 12, 1 << 12, 32, 1, 256, 256)             # one sample alone exceeds what a call holds
    with pytest.raises(ValueError, match="one sample takes"):
        h.check(_wide((1, 256, 1 << 12)), np.broadcast_to(0.0, (1, 1 << 12, 1)), np.broadcast_to(0.0, (1, 256, 1 << 12, 32)))
    with pytest.raises(ValueError, match="kind="):
        ppc.PpcResult(codes=np.zeros((1, 1), np.uint8), dev_feature=np.zeros((1, 2, 1)), dev_object=np.zeros((1, 2, 1)),
                      count_rep=np.zeros((1, 1, 2), np.int32), count_obs=np.zeros((1, 2)), n_samples=1, n_skipped=0).table("cell")


def test_the_one_call_form_checks_its_arguments_before_the_device(monkeypatch):
    monkeypatch.setattr(ppc, "PpcHandle", lambda device: (_ for _ in ()).throw(AssertionError("the device was touched")))
    with pytest.raises(ValueError, match="clusters must be"):
        ppc.posterior_predictive_check(np.zeros((5, 3), np.uint8), [], np.zeros((2, 5)), np.zeros((2, 3, 1)), np.zeros((2, 1, 3, 2)))
    args = (np.zeros((5, 3), np.uint8), [], np.zeros((2, 1, 5)), np.zeros((2, 3, 1)), np.zeros((2, 1, 3, 2)))
    with pytest.raises(ValueError, match="burnin="):
        ppc.posterior_predictive_check(*args, burnin=1.0)
    with pytest.raises(ValueError, match="3 rows of uniforms for 2 samples"):
        ppc.posterior_predictive_check(*args, uniforms=np.zeros((3, 15)))
