"""CPU checks of the summary boundary (include/sbe_summary.h, sbayes_amd/summary.py): the symbols are exported and bound by
the module's own prototype table, the limits agree, and bad arguments are refused before the device is touched."""
import ctypes as ct
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from sbayes_amd import diag, summary
from tests import _abi_header as abi

REPO = Path(__file__).resolve().parent.parent
HEADER = (REPO / "include" / "sbe_summary.h").read_text()


def test_every_symbol_of_the_header_is_exported_and_bound():
    names = abi.check_symbols(summary, HEADER, 12)
    assert not set(names) & set(diag.PROTOTYPES)


def test_limits_and_codes_agree_with_the_header():
    assert abi.macro(HEADER, "SBE_SUMMARY_MAX_PROBS") == str(summary.MAX_PROBS) == "8"
    assert {k: int(abi.macro(HEADER, "SBE_SUMMARY_DERIVED_" + k.upper())) for k in summary.DERIVED} == summary.DERIVED
    # the limits of the diagnostics are the summary's own
    assert (summary.MAX_CHAINS, summary.MIN_DRAWS, summary.MAX_DRAWS, summary.MAX_COLUMNS) == \
        (diag.MAX_CHAINS, diag.MIN_DRAWS, diag.MAX_DRAWS, diag.MAX_COLUMNS)
    assert summary.lds_max_draws() == diag.lds_max_draws()
    # the sort buffer of the longest staged column and the rank kernel's static LDS fit the 160 KiB of a CU
    assert summary.lds_max_draws() * 8 + 4096 <= 160 * 1024
    assert len(summary.DEFAULT_PROBS) <= summary.MAX_PROBS and 0.0 < summary.DEFAULT_HDI_PROB < 1.0


def test_every_array_handed_to_the_library_is_bound_to_a_name():
    abi.check_ptr_arguments(summary)


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to create a handle fails the test."""
    def refuse(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(summary.SummaryHandle, "__init__", refuse)


@pytest.mark.parametrize("chains,kw,err,match", [
    ([], {}, ValueError, r"0 chains; the diagnostics take 1 \.\. 64"),
    (np.zeros((65, 10, 2)), {}, ValueError, "65 chains"),
    (np.zeros((10, 2)), {}, ValueError, r"\[M, S, P\]"),
    ([np.zeros((7, 2))], dict(burnin=0.0), ValueError, "3 draws per chain after burn-in and split; at least 4"),
    ([np.broadcast_to(np.zeros((1, 1)), ((1 << 19) + 2, 1))] * 2, dict(burnin=0.0), ValueError, r"exceed 1048576 \(2\^20\)"),
    ([np.zeros((10, 2)), np.zeros((10, 3))], {}, ValueError, "unequal column counts"),
    ([np.zeros((10, 2))], dict(burnin=1.0), ValueError, r"must lie in \[0, 1\)"),
    ([np.zeros((10, 2))], dict(max_lag=-1), ValueError, "max_lag"),
    ([np.zeros((10, 2))], dict(names=["a"]), ValueError, "1 names for 2 columns"),
    ([np.zeros((10, 2), dtype="U1")], dict(burnin=0.0), TypeError, "numeric"),
    ([np.zeros((10, 2))], dict(probs=[0.1] * 9), ValueError, "9 probabilities; a call takes at most 8"),
    ([np.zeros((10, 2))], dict(probs=(0.5, 1.01)), ValueError, r"probability 1\.01 must lie in \[0, 1\]"),
    ([np.zeros((10, 2))], dict(probs=(-0.1,)), ValueError, r"must lie in \[0, 1\]"),
    ([np.zeros((10, 2))], dict(probs=(float("nan"),)), ValueError, r"must lie in \[0, 1\]"),
    ([np.zeros((10, 2))], dict(hdi_prob=0.0), ValueError, r"hdi_prob=0\.0 must lie in \(0, 1\)"),
    ([np.zeros((10, 2))], dict(hdi_prob=1.0), ValueError, r"hdi_prob=1\.0 must lie in \(0, 1\)"),
])
def test_bad_input_is_refused_before_the_device(no_device, chains, kw, err, match):
    with pytest.raises(err, match=match):
        summary.summarize(chains, **kw)


def test_c_abi_validates_before_the_device():
    assert sorted(abi.check_null_handles(summary)) == sorted(set(summary.PROTOTYPES) - {"sbe_summary_abi_version", "sbe_summary_last_error"})


def test_handles_are_not_picklable():
    abi.check_not_picklable(summary.SummaryHandle)


def test_a_handle_checks_its_own_arguments_before_the_library():
    h = object.__new__(summary.SummaryHandle)
    h._h = ct.c_void_p()
    h.n_chains, h.n_columns, h.capacity = 2, 3, 10

    def refuse(*a, **k):
        raise AssertionError("the device was touched")
    h._lib = SimpleNamespace(**{name: refuse for name in summary.PROTOTYPES})
    with pytest.raises(ValueError, match=r"65 chains"):
        h.reset(65, 3, 10)
    h.n_chains, h.n_columns = 2, 3
    with pytest.raises(ValueError, match="chain 2 out of range"):
        h.append(2, np.zeros((1, 3)))
    with pytest.raises(ValueError, match="rows have 4 columns, the store has 3"):
        h.append(0, np.zeros((1, 4)))
    with pytest.raises(ValueError, match="max_lag"):
        h.compute(max_lag=-3)
    with pytest.raises(ValueError, match="at most 8"):
        h.compute(probs=[0.5] * 9)
    with pytest.raises(ValueError, match="hdi_prob"):
        h.compute(hdi_prob=1.5)
    with pytest.raises(ValueError, match="which"):
        h.derived_column(0, "ranks")
    with pytest.raises(ValueError, match="column 3 out of range"):
        h.derived_column(3, "zb")


def test_result_table_and_header():
    p = 3
    res = summary.SummaryResult(probs=(0.05, 0.5, 0.95), hdi_prob=0.94, quantiles=np.arange(9.0).reshape(3, p), hdi_lo=np.zeros(p),
                                hdi_hi=np.ones(p), ess_bulk=np.full(p, 10.0), ess_tail=np.full(p, 9.0), rhat_rank=np.full(p, 1.01),
                                mean=np.array([0.5, 1.5, 2.5]), sd=np.ones(p), ess=np.full(p, 11.0), rhat=np.ones(p), mcse_mean=np.zeros(p),
                                n_lags=np.array([2, 4, 6], dtype=np.int32), flag=np.array([0, 4, 1], dtype=np.uint8), names=list("abc"),
                                n_chains=4, n_draws=10)
    head = res.header()
    assert head == ["column", "mean", "sd", "hdi_3%", "hdi_97%", "q5%", "q50%", "q95%", "mcse_mean", "ess", "ess_bulk", "ess_tail", "rhat",
                    "rhat_rank", "n_lags", "flag"]
    rows = res.table()
    assert rows[1] == ["b", 1.5, 1.0, 0.0, 1.0, 1.0, 4.0, 7.0, 0.0, 11.0, 10.0, 9.0, 1.0, 1.01, 4, 4]
    assert all(len(r) == len(head) for r in rows)
