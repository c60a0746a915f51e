"""CPU checks of the pairwise check's boundary (include/sbe_pairppc.h, sbayes_amd/pairppc.py): the symbols are exported and bound
by the module's own prototype table, the limits agree, and bad arguments are refused before the device is touched."""
import ctypes as ct
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from sbayes_amd import assoc, pairppc, predict
from tests import _abi_header as abi

REPO = Path(__file__).resolve().parent.parent
HEADER = (REPO / "include" / "sbe_pairppc.h").read_text()


def test_every_symbol_of_the_header_is_exported_and_bound():
    abi.check_symbols(pairppc, HEADER, 13)


def test_limits_agree_with_the_header():
    assert abi.macro(HEADER, "SBE_PAIRPPC_NA") == str(pairppc.NA) == "255"
    assert abi.macro(HEADER, "SBE_PAIRPPC_MAX_STAGE_BYTES") == "(256ll << 20)" and pairppc.MAX_STAGE_BYTES == predict.MAX_STAGE_BYTES == 256 << 20
    assert abi.macro(HEADER, "SBE_PAIRPPC_HELD_BYTES") == "(32ll << 20)" and pairppc.HELD_BYTES == 32 << 20
    assert {k: abi.macro(HEADER, "SBE_PAIRPPC_FORM_" + k.upper()) for k in pairppc.FORMS} == {k: str(v) for k, v in pairppc.FORMS.items()}
    lib = pairppc.load()
    for n, f in [(1, 1), (255, 17), (256, 9), (257, 33), (1000, 200), (100, 36), (1 << 24, 6), (1 << 19, 4096)]:
        for with_rep in (0, 1):
            assert lib.sbe_pairppc_replicate_bytes(n, f, with_rep) == pairppc.replicate_bytes(n, f, bool(with_rep)) > 0, (n, f)
    assert pairppc.replicate_bytes(1, 1) == 1 + 256 and pairppc.replicate_bytes(257, 3, True) == 257 * 3 + 3 * 512 + 72
    for n, f in [(0, 1), (1, 0), ((1 << 24) + 1, 1), (1, 4097), ((1 << 19) + 1, 4096), (-1, 5)]:
        assert lib.sbe_pairppc_replicate_bytes(n, f, 0) == pairppc.replicate_bytes(n, f) == 0, (n, f)
    assert (assoc.MAX_OBJECTS, assoc.MAX_FEATURES, assoc.MAX_CODES) == (1 << 24, 4096, 1 << 31)


def test_every_array_handed_to_the_library_is_bound_to_a_name():
    abi.check_ptr_arguments(pairppc)


def test_c_abi_validates_before_the_device():
    assert sorted(abi.check_null_handles(pairppc)) == sorted(set(pairppc.PROTOTYPES) - {"sbe_pairppc_abi_version", "sbe_pairppc_last_error",
                                                                                        "sbe_pairppc_replicate_bytes"})


def test_handles_are_not_picklable():
    abi.check_not_picklable(pairppc.PairHandle)


def test_a_handle_checks_its_own_arguments_before_the_library():
    h = object.__new__(pairppc.PairHandle)
    h._h = ct.c_void_p()

    def refuse(*a, **k):
        raise AssertionError("the device was touched")
    h._lib = SimpleNamespace(**{name: refuse for name in pairppc.PROTOTYPES})
    h.shape = None
    for call in (h.reset, h.result, lambda: h.add(np.zeros((1, 2, 2), dtype=np.uint8)), h.max_replicates):
        with pytest.raises(ValueError, match="no data yet"):
            call()
    with pytest.raises(TypeError, match="uint8 codes"):
        h.set_data(np.zeros((3, 2)))
    with pytest.raises(ValueError, match=r"n_states must lie in \[1, 32\]"):
        h.set_data(np.zeros((3, 2), dtype=np.uint8), [2, 33])
    with pytest.raises(ValueError, match=r"features\[1, 0\] = 2 is neither below n_states\[0\] = 2 nor 255"):
        h.set_data(np.array([[0, 0], [2, 1]], dtype=np.uint8), [2, 2])
    with pytest.raises(ValueError, match="form='fast' is none of"):
        h.set_form("fast")
    h.shape = (5, 3)
    with pytest.raises(TypeError, match="uint8 codes"):
        h.add(np.zeros((1, 5, 3)))
    with pytest.raises(ValueError, match=r"replicates must be \[n, 5, 3\], got shape \(1, 5, 4\)"):
        h.add(np.zeros((1, 5, 4), dtype=np.uint8))
    assert h.max_replicates() == (256 << 20) // (15 + 3 * 256) and h.max_replicates(True) == (256 << 20) // (15 + 3 * 256 + 72)
    h.shape = (1 << 19, 4096)                                                      # one replicate alone is beyond a call
    assert h.max_replicates() == 0
    with pytest.raises(ValueError, match="one replicate takes 4294967296 bytes on the device, a call holds 268435456"):
        h.add(np.broadcast_to(np.zeros((1, 1, 1), dtype=np.uint8), (1, 1 << 19, 4096)))


def test_bad_input_of_the_check_is_refused_before_the_device(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(pairppc.ppc.PpcHandle, "__init__", refuse)
    monkeypatch.setattr(pairppc.PairHandle, "__init__", refuse)
    codes, groups = np.zeros((4, 2), dtype=np.uint8), np.zeros((0, 4), dtype=np.uint8)
    with pytest.raises(ValueError, match=r"clusters must be \[T, K, N\] and tables \[T, R, F, S\]"):
        pairppc.pairwise_check(codes, groups, np.zeros((3, 4)), np.zeros((3, 2, 1)), np.zeros((3, 1, 2, 2)), n_groups=[])
    with pytest.raises(ValueError, match=r"must lie in \[0, 1\)"):
        pairppc.pairwise_check(codes, groups, np.zeros((3, 1, 4)), np.zeros((3, 2, 1)), np.zeros((3, 1, 2, 2)), n_groups=[], burnin=1.0)
    with pytest.raises(ValueError, match="2 rows of uniforms for 3 samples"):
        pairppc.pairwise_check(codes, groups, np.zeros((3, 1, 4)), np.zeros((3, 2, 1)), np.zeros((3, 1, 2, 2)), n_groups=[], uniforms=np.zeros((2, 8)))
