"""CPU checks of the boundary of the Gibbs weights step (include/sbe_wgibbs.h, sbayes_amd/wgibbs.py): the symbols are
exported and bound by the module's own prototype table, and bad arguments are refused before the device is touched."""
import ctypes as ct
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from sbayes_amd import _lib, wgibbs
from tests import _abi_header as abi

REPO = Path(__file__).resolve().parent.parent
HEADER = (REPO / "include" / "sbe_wgibbs.h").read_text()


def test_every_symbol_of_the_header_is_exported_and_bound():
    names = abi.check_symbols(wgibbs, HEADER, 3)
    assert names == ["sbe_wgibbs_abi_version", "sbe_wgibbs_pair_counts", "sbe_wgibbs_step"]
    lib = wgibbs.load()
    for name in names:
        fn = getattr(lib, name)
        assert fn.restype is wgibbs.PROTOTYPES[name][0] and list(fn.argtypes) == wgibbs.PROTOTYPES[name][1]
    assert lib.sbe_abi_version() == _lib.ABI_VERSION      # the engine's ABI version is not touched


def test_constants_agree_with_the_header():
    assert abi.macro(HEADER, "SBE_WGIBBS_ABI_VERSION") == str(wgibbs.ABI_VERSION)
    assert abi.macro(HEADER, "SBE_WGIBBS_FEATURE_TILE") == str(wgibbs.FEATURE_TILE)
    # the step kernel's tile at the engine's limits (64 patterns, 8 components): the float64 table of log differences and
    # the lane sums fit a workgroup's LDS
    assert wgibbs.FEATURE_TILE * 64 * 8 * 8 + 64 * wgibbs.FEATURE_TILE * 8 <= 160 * 1024


def test_the_argument_counts_of_the_prototypes_match_the_header():
    text = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    for name, (_res, args) in wgibbs.PROTOTYPES.items():
        params = re.search(rf"\b{name}\s*\((.*?)\)\s*;", text, flags=re.S).group(1).strip()
        n = 0 if params == "void" else len(params.split(","))
        assert n == len(args), name


class _NoDevice:
    """An engine as far as the host-side checks know; any library call fails the test."""
    n_slots, n_features, n_components = 2, 6, 3
    _h = ct.c_void_p()

    def _check(self, rc):
        raise AssertionError("the device was touched")

    _i = _o = _check


F, C = _NoDevice.n_features, _NoDevice.n_components
GOOD = dict(a2=np.full(F, 0.5), u=np.full(F, 0.5, dtype=np.float32), alpha=np.ones((F, C)), beta_ab=np.full((F, 2), 2.0),
            prior_temperature=1.0)


def _step(slot=0, i1=0, i2=1, **kw):
    return wgibbs.step(_NoDevice(), slot, i1, i2, **{**GOOD, **kw})


@pytest.mark.parametrize("call,match", [
    (lambda: wgibbs.pair_counts(_NoDevice(), 2, 0, 1), "slot 2 out of range"),
    (lambda: wgibbs.pair_counts(_NoDevice(), 0, 1, 1), "two different indices"),
    (lambda: wgibbs.pair_counts(_NoDevice(), 0, -1, 1), "two different indices"),
    (lambda: wgibbs.pair_counts(_NoDevice(), 0, 0, 3), "two different indices"),
    (lambda: _step(slot=-1), "slot -1 out of range"),
    (lambda: _step(i1=3), "two different indices"),
    (lambda: _step(prior_temperature=0.0), "positive and finite"),
    (lambda: _step(prior_temperature=-1.0), "positive and finite"),
    (lambda: _step(prior_temperature=float("inf")), "positive and finite"),
    (lambda: _step(prior_temperature=float("nan")), "positive and finite"),
    (lambda: _step(a2=np.zeros(F + 1)), "a2 must have shape"),
    (lambda: _step(u=np.zeros(F - 1, dtype=np.float32)), "u must have shape"),
    (lambda: _step(alpha=np.ones((F, C + 1))), "alpha must have shape"),
    (lambda: _step(beta_ab=np.ones((F, 3))), "beta_ab must have shape"),
])
def test_bad_input_is_refused_before_the_device(call, match):
    with pytest.raises(ValueError, match=match):
        call()


def test_c_abi_refuses_a_null_engine_before_the_device():
    lib = wgibbs.load()
    out = np.zeros((4, 2), dtype=np.int32)
    assert lib.sbe_wgibbs_pair_counts(None, 0, 0, 1, out.ctypes.data) == 1
    assert b"null engine handle" in lib.sbe_last_error(None)
    assert lib.sbe_wgibbs_step(None, 0, 0, 1, None, None, None, None, 1.0, None, None, None) == 1
    assert b"null engine handle" in lib.sbe_last_error(None)


def test_covered_says_which_proposals_the_device_form_takes():
    def op(kind):
        return SimpleNamespace(model=SimpleNamespace(prior=SimpleNamespace(prior_weights=SimpleNamespace(prior_type=SimpleNamespace(value=kind)))))
    sample = SimpleNamespace(n_components=3)
    for kind in ("uniform", "jeffreys", "BBS", "symmetric_dirichlet"):
        assert wgibbs.covered(op(kind), sample)
    assert not wgibbs.covered(op("dirichlet"), sample) and not wgibbs.covered(op("universal"), sample)
    assert not wgibbs.covered(op("uniform"), SimpleNamespace(n_components=1))
    assert not wgibbs.covered(SimpleNamespace(model=SimpleNamespace()), sample)
