"""CPU checks of the spatial check's boundary (include/sbe_spatial.h, sbayes_amd/spatial.py): the symbols are exported and bound
by the module's own prototype table, the limits agree, and bad arguments are refused before the device is touched."""
import ctypes as ct
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from sbayes_amd import predict, spatial
from tests import _abi_header as abi
from tests import _spatial_oracle as orc

REPO = Path(__file__).resolve().parent.parent
HEADER = (REPO / "include" / "sbe_spatial.h").read_text()


def test_every_symbol_of_the_header_is_exported_and_bound():
    abi.check_symbols(spatial, HEADER, 12)


def test_limits_agree_with_the_header():
    assert abi.macro(HEADER, "SBE_SPATIAL_NA") == str(spatial.NA) == str(orc.NA) == "255"
    assert int(abi.macro(HEADER, "SBE_SPATIAL_MAX_OBJECTS")) == spatial.MAX_OBJECTS == orc.MAX_OBJECTS == 4096
    assert int(abi.macro(HEADER, "SBE_SPATIAL_MAX_FEATURES")) == spatial.MAX_FEATURES == orc.MAX_FEATURES == 4096
    # the state limit is the one of the replicates' source
    assert int(abi.macro(HEADER, "SBE_SPATIAL_MAX_STATES")) == spatial.MAX_STATES == predict.MAX_STATES == orc.MAX_STATES == 32
    assert int(abi.macro(HEADER, "SBE_SPATIAL_MAX_BANDS")) == spatial.MAX_BANDS == orc.MAX_BANDS == 8
    assert int(abi.macro(HEADER, "SBE_SPATIAL_MAX_TILE")) == spatial.MAX_TILE == 32
    assert abi.macro(HEADER, "SBE_SPATIAL_MAX_STAGE_BYTES") == "(256ll << 20)" and spatial.MAX_STAGE_BYTES == predict.MAX_STAGE_BYTES == 256 << 20


def test_max_replicates_agrees_at_the_limits_and_just_past_them():
    lib = spatial.load()
    for n, f in [(1, 1), (1, 4096), (2, 1), (2, 4096), (100, 36), (1000, 200), (4096, 1), (4096, 3), (4095, 4096), (4096, 4096)]:
        assert lib.sbe_spatial_max_replicates(n, f) == spatial.max_replicates(n, f) == orc.max_replicates(n, f) > 0, (n, f)
    for n, f in [(0, 1), (1, 0), (4097, 1), (1, 4097), (4097, 4097), (-1, 5)]:
        assert lib.sbe_spatial_max_replicates(n, f) == spatial.max_replicates(n, f) == orc.max_replicates(n, f) == 0, (n, f)
    assert spatial.max_replicates(4096, 4096) == 32784 and spatial.max_replicates(4096, 3) == 131136 and spatial.max_replicates(1, 9) == 2 ** 31 - 1
    # the derivation: the largest sum of squares after that many replicates fits int64, after one more it does not
    for n, f in [(4096, 4096), (4096, 3), (1000, 200), (100, 36)]:
        most = max(n * (n - 1) // 2, (n - 1) * f)
        cap = spatial.max_replicates(n, f)
        assert cap == 2 ** 31 - 1 or (cap * most * most <= 2 ** 63 - 1 < (cap + 1) * most * most)


def test_replicate_bytes_agree():
    lib = spatial.load()
    for n, f, s, b in [(1, 1, 1, 1), (64, 16, 32, 8), (65, 17, 2, 1), (257, 5, 32, 8), (1000, 200, 10, 8), (1025, 3, 4, 2), (4096, 4096, 32, 8)]:
        assert lib.sbe_spatial_replicate_bytes(n, f, s, b) == spatial.replicate_bytes(n, f, s, b) > 0, (n, f, s, b)
    assert [spatial.padded_words(n) for n in (1, 64, 65, 129, 257, 1000, 1024, 1025, 4096)] == [1, 1, 2, 4, 8, 16, 16, 32, 64]
    assert spatial.replicate_bytes(65, 3, 2, 1) == 65 * 3 + 128 * 3 + 8 * 2 * 3 * 3 + 8 * 68 + 8
    for n, f, s, b in [(0, 1, 2, 1), (4097, 1, 2, 1), (1, 4097, 2, 1), (5, 5, 0, 1), (5, 5, 33, 1), (5, 5, 2, 0), (5, 5, 2, 9)]:
        assert lib.sbe_spatial_replicate_bytes(n, f, s, b) == spatial.replicate_bytes(n, f, s, b) == 0, (n, f, s, b)
    assert spatial.MAX_STAGE_BYTES // spatial.replicate_bytes(4096, 4096, 32, 8) >= 1      # one replicate of the largest shape fits a call


def test_every_array_handed_to_the_library_is_bound_to_a_name():
    abi.check_ptr_arguments(spatial)


def test_c_abi_validates_before_the_device():
    assert sorted(abi.check_null_handles(spatial)) == sorted(set(spatial.PROTOTYPES) - {"sbe_spatial_abi_version", "sbe_spatial_last_error",
                                                                                        "sbe_spatial_max_replicates", "sbe_spatial_replicate_bytes"})


def test_handles_are_not_picklable():
    abi.check_not_picklable(spatial.SpatialHandle)


def test_a_handle_checks_its_own_arguments_before_the_library():
    h = object.__new__(spatial.SpatialHandle)
    h._h = ct.c_void_p()

    def refuse(*a, **k):
        raise AssertionError("the device was touched")
    h._lib = SimpleNamespace(**{name: refuse for name in spatial.PROTOTYPES})
    h.shape = None
    for call in (h.reset, h.result, lambda: h.add(np.zeros((1, 2, 2), dtype=np.uint8)), h.max_replicates, h.call_replicates):
        with pytest.raises(ValueError, match="no data yet"):
            call()
    band = np.full((3, 3), 255, dtype=np.uint8)
    with pytest.raises(TypeError, match="uint8 codes"):
        h.set_data(np.zeros((3, 2)), None, band, 1)
    with pytest.raises(ValueError, match=r"n_states must lie in \[1, 32\]"):
        h.set_data(np.zeros((3, 2), dtype=np.uint8), [2, 33], band, 1)
    with pytest.raises(ValueError, match=r"features\[1, 0\] = 2 is neither below n_states\[0\] = 2 nor 255"):
        h.set_data(np.array([[0, 0], [2, 1], [0, 0]], dtype=np.uint8), [2, 2], band, 1)
    with pytest.raises(ValueError, match="4097 objects"):
        h.set_data(np.zeros((4097, 1), dtype=np.uint8), [2], band, 1)
    with pytest.raises(TypeError, match="band must be uint8 classes"):
        h.set_data(np.zeros((3, 2), dtype=np.uint8), [2, 2], band.astype(np.int64), 1)
    with pytest.raises(ValueError, match=r"band must be \[3, 3\], got shape \(2, 3\)"):
        h.set_data(np.zeros((3, 2), dtype=np.uint8), [2, 2], band[:2], 1)
    for b in (0, 9):
        with pytest.raises(ValueError, match=rf"n_bands={b} out of range \[1, 8\]"):
            h.set_data(np.zeros((3, 2), dtype=np.uint8), [2, 2], band, b)
    h.shape, h.n_states = (5, 3, 2), np.array([2, 4, 3], dtype=np.int32)
    with pytest.raises(TypeError, match="uint8 codes"):
        h.add(np.zeros((1, 5, 3)))
    with pytest.raises(ValueError, match=r"replicates must be \[n, 5, 3\], got shape \(1, 5, 4\)"):
        h.add(np.zeros((1, 5, 4), dtype=np.uint8))
    with pytest.raises(ValueError, match="the per-replicate outputs are"):
        h.add(np.zeros((1, 5, 3), dtype=np.uint8), keep=("stat_rep",))
    assert h.max_replicates() == 2 ** 31 - 1 and h.call_replicates() == (256 << 20) // (15 + 64 * 3 + 8 * 3 * 5 + 8 * 2 * 8 + 16)


def test_bad_input_of_the_check_is_refused_before_the_device(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(spatial.ppc.PpcHandle, "__init__", refuse)
    monkeypatch.setattr(spatial.SpatialHandle, "__init__", refuse)
    codes, groups = np.zeros((4, 2), dtype=np.uint8), np.zeros((0, 4), dtype=np.uint8)
    band = np.full((4, 4), 255, dtype=np.uint8)
    with pytest.raises(ValueError, match=r"clusters must be \[T, K, N\] and tables \[T, R, F, S\]"):
        spatial.spatial_check(codes, groups, np.zeros((3, 4)), np.zeros((3, 2, 1)), np.zeros((3, 1, 2, 2)), band, n_groups=[])
    with pytest.raises(ValueError, match=r"must lie in \[0, 1\)"):
        spatial.spatial_check(codes, groups, np.zeros((3, 1, 4)), np.zeros((3, 2, 1)), np.zeros((3, 1, 2, 2)), band, n_groups=[], burnin=1.0)
    with pytest.raises(ValueError, match="2 rows of uniforms for 3 samples"):
        spatial.spatial_check(codes, groups, np.zeros((3, 1, 4)), np.zeros((3, 2, 1)), np.zeros((3, 1, 2, 2)), band, n_groups=[], uniforms=np.zeros((2, 8)))
    with pytest.raises(ValueError, match=r"band must be \[4, 4\], got shape \(3, 3\)"):
        spatial.spatial_check(codes, groups, np.zeros((3, 1, 4)), np.zeros((3, 2, 1)), np.zeros((3, 1, 2, 2)), band[:3, :3], n_groups=[])
