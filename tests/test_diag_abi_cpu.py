"""CPU checks of the diagnostics boundary (include/sbe_diag.h, sbayes_amd/diag.py): the symbols are exported and bound by
the module's own prototype table, the limits agree, and bad arguments are refused before the device is touched."""
import ctypes as ct
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from sbayes_amd import diag
from tests import _abi_header as abi

REPO = Path(__file__).resolve().parent.parent
HEADER = (REPO / "include" / "sbe_diag.h").read_text()


def test_every_symbol_of_the_header_is_exported_and_bound():
    abi.check_symbols(diag, HEADER, 12)


def test_limits_and_codes_agree_with_the_header():
    assert abi.macro(HEADER, "SBE_DIAG_MAX_CHAINS") == str(diag.MAX_CHAINS) == "64"
    assert abi.macro(HEADER, "SBE_DIAG_MIN_DRAWS") == str(diag.MIN_DRAWS) == "4"
    assert abi.macro(HEADER, "SBE_DIAG_MAX_DRAWS") == "(1 << 20)" and diag.MAX_DRAWS == 1 << 20
    assert diag.MAX_COLUMNS == 2 ** 31 - 1
    assert (abi.macro(HEADER, "SBE_DIAG_FLAG_CONSTANT"), abi.macro(HEADER, "SBE_DIAG_FLAG_NONFINITE"), abi.macro(HEADER, "SBE_DIAG_FLAG_TRUNCATED")) == \
        (str(diag.FLAG_CONSTANT), str(diag.FLAG_NONFINITE), str(diag.FLAG_TRUNCATED))
    assert {int(abi.macro(HEADER, "SBE_DIAG_PATH_LDS")): "lds", int(abi.macro(HEADER, "SBE_DIAG_PATH_GLOBAL")): "global"} == diag.PATHS
    # the staged column, the rho_t entries kept in LDS and the kernel's static LDS fit the 160 KiB of a CU
    limit = diag.lds_max_draws()
    assert 8192 <= limit and (limit + 2048) * 8 + 4096 <= 160 * 1024 < (limit + 1 + 2048) * 8 + 4096


def test_every_array_handed_to_the_library_is_bound_to_a_name():
    abi.check_ptr_arguments(diag)


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to create a handle fails the test."""
    def refuse(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(diag.DiagHandle, "__init__", refuse)


class _Flat:
    """Passes for an array of a given shape without holding its memory."""
    def __init__(self, shape):
        self.shape = shape

    def __array__(self, dtype=None, copy=None):
        return np.broadcast_to(np.zeros((), dtype=dtype or np.float64), self.shape)


@pytest.mark.parametrize("chains,kw,err,match", [
    ([], {}, ValueError, r"0 chains; the diagnostics take 1 \.\. 64"),
    ([np.zeros((10, 2))] * 65, {}, ValueError, r"65 chains; the diagnostics take 1 \.\. 64"),
    (np.zeros((65, 10, 2)), {}, ValueError, "65 chains"),
    (np.zeros((10, 2)), {}, ValueError, r"\[M, S, P\]"),
    ([np.zeros((7, 2))], dict(burnin=0.0), ValueError, "3 draws per chain after burn-in and split; at least 4"),
    ([np.zeros((3, 2))], dict(burnin=0.0, split=False), ValueError, "3 draws per chain after burn-in; at least 4"),
    ([np.zeros((20, 2)), np.zeros((8, 2))], dict(burnin=0.2), ValueError, "3 draws per chain"),
    ([np.broadcast_to(np.zeros((1, 1)), ((1 << 19) + 2, 1))] * 2, dict(burnin=0.0), ValueError, r"exceed 1048576 \(2\^20\)"),
    ([np.zeros((10, 2)), np.zeros((10, 3))], {}, ValueError, "unequal column counts"),
    ([np.zeros((10, 2))], dict(burnin=1.0), ValueError, r"must lie in \[0, 1\)"),
    ([np.zeros((10, 2))], dict(burnin=-0.1), ValueError, r"must lie in \[0, 1\)"),
    ([np.zeros((10, 2))], dict(max_lag=-1), ValueError, "max_lag"),
    ([np.zeros((10, 2))], dict(names=["a"]), ValueError, "1 names for 2 columns"),
    ([np.zeros((10, 0))], {}, ValueError, "0 columns"),
    ([np.zeros((10, 2), dtype="U1")], dict(burnin=0.0), TypeError, "numeric"),
])
def test_bad_input_is_refused_before_the_device(no_device, chains, kw, err, match):
    with pytest.raises(err, match=match):
        diag.convergence(chains, **kw)


def test_plan_follows_drop_burnin_cut_and_split():
    assert diag._plan([100], 0.1, True) == ([10], (0,), 2, 45)
    assert diag._plan([101, 90], 0.1, True) == ([10, 9], (10, 0), 4, 40)
    assert diag._plan([101, 90], 0.1, False) == ([10, 9], (10, 0), 2, 81)
    assert diag._plan([9], 0.0, True) == ([0], (0,), 2, 4)                 # the middle draw of an odd length is dropped
    assert diag._plan([1 << 20], 0.0, True)[2:] == (2, 1 << 19)


def test_c_abi_validates_before_the_device():
    assert sorted(abi.check_null_handles(diag)) == sorted(set(diag.PROTOTYPES) - {"sbe_diag_abi_version", "sbe_diag_last_error", "sbe_diag_lds_max_draws"})
    assert diag.load().sbe_diag_lds_max_draws() == diag.lds_max_draws()


def test_handles_are_not_picklable():
    abi.check_not_picklable(diag.DiagHandle)


def test_a_handle_checks_its_own_arguments_before_the_library():
    h = object.__new__(diag.DiagHandle)
    h._h = ct.c_void_p()
    h.n_chains, h.n_columns, h.capacity = 2, 3, 10

    def refuse(*a, **k):
        raise AssertionError("the device was touched")
    h._lib = SimpleNamespace(**{name: refuse for name in diag.PROTOTYPES})
    with pytest.raises(ValueError, match=r"65 chains"):
        h.reset(65, 3, 10)
    h.n_chains, h.n_columns = 2, 3
    with pytest.raises(ValueError, match="chain 2 out of range"):
        h.append(2, np.zeros((1, 3)))
    with pytest.raises(ValueError, match="rows have 4 columns, the store has 3"):
        h.append(0, np.zeros((1, 4)))
    with pytest.raises(ValueError, match="max_lag"):
        h.compute(max_lag=-3)


def test_result_summary_and_worst():
    res = diag.DiagResult(mean=np.zeros(5), sd=np.ones(5), ess=np.array([500.0, 20.0, np.nan, 150.0, 40.0]),
                          rhat=np.array([1.0, 1.2, np.nan, 1.02, np.nan]), mcse_mean=np.zeros(5), n_lags=np.zeros(5, dtype=np.int32),
                          flag=np.array([0, 0, 2, 4, 1], dtype=np.uint8), names=list("abcde"), n_chains=4, n_draws=10)
    assert [w[0] for w in res.worst(3)] == ["b", "e", "d"]
    assert [w[0] for w in res.worst(9)][-1] == "c"                          # the non-finite column comes last
    s = res.summary()
    assert (s["n_rhat_above"], s["n_ess_below"], s["n_constant"], s["n_nonfinite"], s["n_truncated"]) == (2, 2, 1, 1, 1)
    assert (s["ess_min"], s["ess_median"], s["ess_max"]) == (20.0, 150.0, 500.0)
    assert (s["rhat_threshold"], s["ess_threshold"]) == (1.01, 200.0)
    s = res.summary(rhat_threshold=1.1, ess_threshold=100)
    assert (s["n_rhat_above"], s["n_ess_below"]) == (1, 1)
