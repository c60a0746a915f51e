"""CPU checks of the ELPD boundary (include/sbe_elpd.h, sbayes_amd/elpd.py): the symbols are exported and bound by the
module's own prototype table, and bad arguments are refused before the device is touched."""
import ctypes as ct
from pathlib import Path

import numpy as np
import pytest

from sbayes_amd import elpd
from tests import _abi_header as abi

REPO = Path(__file__).resolve().parent.parent
HEADER = (REPO / "include" / "sbe_elpd.h").read_text()


def test_every_symbol_of_the_header_is_exported_and_bound():
    abi.check_symbols(elpd, HEADER, 12)


def test_every_array_handed_to_the_library_is_bound_to_a_name():
    abi.check_ptr_arguments(elpd)


def test_lds_threshold_is_within_the_budget():
    s = elpd.lds_max_samples()
    assert 30_000 < s < 40_960                     # 160 KiB of LDS at 4 bytes per sample, less the tail buffers


@pytest.fixture
def no_store(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(elpd, "_Store", refuse)


@pytest.mark.parametrize("lh,err", [
    (np.ones((10, 3), dtype=np.float64), TypeError),
    (np.ones(10, dtype=np.float32), ValueError),
    (np.ones((10, 0), dtype=np.float32), ValueError),
    (np.ones((1, 4), dtype=np.float32), ValueError),           # one sample: PSIS needs two
])
def test_bad_matrix_is_refused_before_the_device(no_store, lh, err):
    with pytest.raises(err):
        elpd.psis_loo(lh, burnin=0.0)


@pytest.mark.parametrize("burnin", [1.0, 1.5, -0.1, 0.95])
def test_bad_burnin_is_refused_before_the_device(no_store, burnin):
    with pytest.raises(ValueError):
        elpd.waic(np.ones((10, 3), dtype=np.float32), burnin=burnin)


def test_bad_na_mask_is_refused_before_the_device(no_store):
    lh = np.full((10, 3), 0.5, dtype=np.float32)
    with pytest.raises(ValueError, match="na_values has 2 entries"):
        elpd.psis_loo(lh, na_values=np.zeros(2, bool))
    with pytest.raises(TypeError):
        elpd.psis_loo(lh, na_values=np.zeros(3, np.int8))


def test_too_many_samples_are_refused_with_the_limit(no_store):
    with pytest.raises(ValueError, match=r"2\^20"):
        elpd.psis_loo(np.ones((elpd.MAX_SAMPLES + 1, 1), dtype=np.float32), burnin=0.0)


def test_c_abi_validates_before_the_device():
    lib = elpd.load()
    h = ct.c_void_p()
    assert lib.sbe_elpd_create(ct.byref(h), 0, 0, 10) == 1 and not h
    assert b"n_columns=0" in lib.sbe_elpd_last_error(None)
    assert lib.sbe_elpd_create(ct.byref(h), 0, 5, 0) == 1
    assert b"capacity=0" in lib.sbe_elpd_last_error(None)
    assert sorted(abi.check_null_handles(elpd, b"null store")) == sorted(set(elpd.PROTOTYPES) - {"sbe_elpd_abi_version", "sbe_elpd_last_error", "sbe_elpd_create", "sbe_elpd_lds_max_samples"})


def test_log_capacity_must_be_positive():
    with pytest.raises(ValueError):
        elpd.LikelihoodLog(object(), capacity=0)


def test_handles_are_not_picklable():
    import pickle
    with pytest.raises(TypeError):
        pickle.dumps(elpd.LikelihoodLog(object(), capacity=3))
