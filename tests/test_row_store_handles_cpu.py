"""CPU checks of what the four row-store handles share (sbayes_amd/_handle.py, RowStoreHandle.filled): a one-shot call
gets a filled, open handle, and a handle that cannot be filled is closed before the error reaches the caller."""
import ctypes as ct
import os
from types import SimpleNamespace

import numpy as np
import pytest

from sbayes_amd import _handle, align, consensus, diag, summary

CASES = [(diag.DiagHandle, (3, 2, 4), np.zeros((4, 2))), (summary.SummaryHandle, (3, 2, 4), np.zeros((4, 2))),
         (align.AlignHandle, (3, 2, 5, 4), np.zeros((4, 2, 5), dtype=np.uint8)),
         (consensus.ConsensusHandle, (3, 2, 5, 4), np.zeros((4, 2, 5), dtype=np.uint8))]


def _fake(cls, monkeypatch, fail_at):
    """A library whose append_rows returns SBE_ERR_ARG at its call number `fail_at` (None: never), under a create that
    touches no device; returns the calls it has seen, by name."""
    calls = []

    def entry(name, code=lambda: 0):
        def fn(*args):
            calls.append(name)
            return code()
        return fn
    lib = SimpleNamespace(**{f"{cls._prefix}_{name}": entry(name) for name in ("reset", "destroy")},
                          **{f"{cls._prefix}_append_rows": entry("append_rows", lambda: int(calls.count("append_rows") == fail_at)),
                             f"{cls._prefix}_last_error": lambda h: b"refused"})

    def create_on(self, load, device):
        self._h, self._lib, self._pid, self.device = ct.c_void_p(1), lib, os.getpid(), device
    monkeypatch.setattr(cls, "_create_on", create_on)
    return calls


@pytest.mark.parametrize("cls,shape,block", CASES)
def test_a_handle_that_cannot_be_filled_is_closed_once_and_the_error_propagates(monkeypatch, cls, shape, block):
    calls = _fake(cls, monkeypatch, fail_at=2)
    with pytest.raises(_handle.EngineError, match="refused"):
        cls.filled(0, shape, [block] * 3)
    assert calls == ["reset", "append_rows", "append_rows", "destroy"]


@pytest.mark.parametrize("cls,shape,block", CASES)
def test_a_filled_handle_comes_back_open(monkeypatch, cls, shape, block):
    calls = _fake(cls, monkeypatch, fail_at=None)
    h = cls.filled(0, shape, [block] * 3)
    assert h._h and calls == ["reset"] + ["append_rows"] * 3
    h.close()
    assert not h._h and calls.count("destroy") == 1
