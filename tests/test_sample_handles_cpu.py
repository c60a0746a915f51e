"""CPU checks of what the four handles that replay logged samples share (sbayes_amd/_samples.py, SampleHandle): what set_data
hands the library, the split of a block of samples into library calls, what a failed call leaves behind, and the refusals
that are made before any library call.  A fake library, no device."""
import ctypes as ct
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from sbayes_amd import _handle, contribution, loopred, ppc, predict
from sbayes_amd._handle import _ptr

# class, its block method, the library call behind it, where that call takes the clusters, what a set_data takes behind n_clusters
CASES = [(predict.PredictHandle, "accumulate", "accumulate", 2, ()), (ppc.PpcHandle, "check", "check", 4, ()),
         (contribution.ContributionHandle, "evaluate", "evaluate", 2, ()), (loopred.LooPredHandle, "add", "add", 2, (7,))]
IDS = [c[0].__name__ for c in CASES]
N, F, S, K = 4, 3, 2, 2


def _fake(cls, monkeypatch, compute, fail_at=None):
    """A handle of `cls` on a library that records its calls as (name, args) and whose `compute` returns SBE_ERR_ARG at its
    call number `fail_at`, under a create that touches no device."""
    calls = []

    def entry(name, code=lambda: 0):
        def fn(*args):
            calls.append((name, args))
            return code()
        return fn
    names = {"set_data", "set_feature_tile", "reset", "destroy", "last_kernel_ms"}
    lib = SimpleNamespace(**{f"{cls._prefix}_{name}": entry(name) for name in names},
                          **{f"{cls._prefix}_{compute}": entry(compute, lambda: int(sum(c[0] == compute for c in calls) == fail_at)),
                             f"{cls._prefix}_last_error": lambda h: b"refused"})

    def create_on(self, load, device):
        self._h, self._lib, self._pid, self.device = ct.c_void_p(1), lib, os.getpid(), device
    monkeypatch.setattr(cls, "_create_on", create_on)
    return cls(0), calls


def _data(C):
    codes = np.zeros((N, F), dtype=np.uint8)
    groups = np.zeros((C - 1, N), dtype=np.uint8)
    return codes, groups, [2] * (C - 1)


def _samples(T, C):
    R = K + 2 * (C - 1)
    return np.zeros((T, K, N), dtype=np.uint8), np.zeros((T, F, C)), np.zeros((T, R, F, S))


@pytest.mark.parametrize("cls,method,compute,at,more", CASES, ids=IDS)
@pytest.mark.parametrize("C", [1, 2])
def test_set_data_hands_the_library_the_shape_and_null_groups_without_confounders(monkeypatch, cls, method, compute, at, more, C):
    h, calls = _fake(cls, monkeypatch, compute)
    codes, groups, n_groups = _data(C)
    h.set_data(codes, groups, n_groups, S, K, *more)
    (name, args), = calls
    assert name == "set_data" and args[1:6] == (N, F, S, C, K) and args[6] == _ptr(codes) and args[9:] == more
    if C == 1:
        assert args[7] is None and args[8] is None
    else:
        assert args[7] == _ptr(groups) and args[8] is not None
    assert h.shape == (N, F, S, C, K, K + 2 * (C - 1))


def _small_calls(cls, monkeypatch, shape, m):
    """max_samples() == m for the handle's shape."""
    unit = sys.modules[cls.__module__]
    monkeypatch.setattr(unit, "MAX_STAGE_BYTES", m * unit.sample_bytes(*shape) + 1)


@pytest.mark.parametrize("cls,method,compute,at,more", CASES, ids=IDS)
def test_a_block_goes_in_library_calls_of_at_most_max_samples_on_consecutive_slices(monkeypatch, cls, method, compute, at, more):
    h, calls = _fake(cls, monkeypatch, compute)
    h.set_data(*_data(2), S, K, *more)
    m = 3
    _small_calls(cls, monkeypatch, h.shape, m)
    assert h.max_samples() == m
    clusters, weights, tables = _samples(2 * m + 1, 2)
    getattr(h, method)(clusters, weights, tables)
    made = [args for name, args in calls if name == compute]
    assert [args[1] for args in made] == [m, m, 1]
    for t0, args in zip((0, m, 2 * m), made):
        assert args[at:at + 3] == (_ptr(clusters[t0:]), _ptr(weights[t0:]), _ptr(tables[t0:]))


@pytest.mark.parametrize("cls,method,compute,at,more", CASES, ids=IDS)
def test_a_failed_library_call_raises_and_keeps_what_the_calls_before_it_left(monkeypatch, cls, method, compute, at, more):
    h, calls = _fake(cls, monkeypatch, compute, fail_at=2)
    h.set_data(*_data(2), S, K, *more)
    m = 3
    _small_calls(cls, monkeypatch, h.shape, m)
    with pytest.raises(_handle.EngineError, match="refused"):
        getattr(h, method)(*_samples(2 * m + 1, 2))
    assert [name for name, _a in calls].count(compute) == 2 and h.shape is not None
    kept = {predict.PredictHandle: lambda: h.kernel_ms == 0.0,
            ppc.PpcHandle: lambda: h.n_samples == m and [len(v) for v in h._rows.values()] == [1, 1, 1, 1] and h._rows["count_rep"][0].shape == (m, F, S),
            contribution.ContributionHandle: lambda: h.n_samples == m and h.n_calls == 1 and h._rows["member"][0].shape == (m, K, N),
            loopred.LooPredHandle: lambda: h.n_rows == m}
    assert kept[cls]()


@pytest.mark.parametrize("cls,method,compute,at,more", CASES, ids=IDS)
def test_the_refusals_before_any_library_call_read_the_same_for_every_class(monkeypatch, cls, method, compute, at, more):
    h, calls = _fake(cls, monkeypatch, compute)
    block = getattr(h, method)
    with pytest.raises(ValueError) as e:
        block(*_samples(2, 2))
    assert str(e.value) == "no data yet (set_data)"
    codes, groups, n_groups = _data(2)
    with pytest.raises(ValueError) as e:
        h.set_data(codes[0], groups, n_groups, S, K, *more)
    assert str(e.value) == f"codes must be [N, F], got shape ({F},)"
    with pytest.raises(ValueError) as e:
        h.set_data(codes, np.zeros((1, N + 1), dtype=np.uint8), n_groups, S, K, *more)
    assert str(e.value) == f"groups must be [1, {N}], got shape (1, {N + 1})"
    assert calls == [] and h.shape is None
    h.set_data(codes, groups, n_groups, S, K, *more)
    clusters, weights, tables = _samples(2, 2)
    with pytest.raises(ValueError) as e:
        block(clusters, weights[:, :, :1], tables)
    assert str(e.value) == (f"2 samples take clusters (2, {K}, {N}), weights (2, {F}, 2) and tables (2, {K + 2}, {F}, {S}); got (2, {K}, {N}), "
                            f"(2, {F}, 1), (2, {K + 2}, {F}, {S})")
    assert [name for name, _a in calls] == ["set_data"]
