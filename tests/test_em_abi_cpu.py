"""CPU checks of the EM initializer's boundary (include/sbe_em.h, sbayes_amd/em.py): the symbols are exported and bound
by the module's own prototype table, and bad shapes, limits and data are refused before the device is touched."""
import ctypes as ct
from pathlib import Path

import numpy as np
import pytest

from sbayes_amd import em
from tests import _abi_header as abi

REPO = Path(__file__).resolve().parent.parent
HEADER = (REPO / "include" / "sbe_em.h").read_text()


def _header_define(name):
    return eval(abi.macro(HEADER, name).replace("(int64_t)", ""))


def test_every_symbol_of_the_header_is_exported_and_bound():
    abi.check_symbols(em, HEADER, 7)


def test_python_limits_are_the_header_limits():
    assert em.MAX_STATES == _header_define("SBE_EM_MAX_STATES") == 254
    assert em.MAX_GROUPS == _header_define("SBE_EM_MAX_GROUPS")
    assert em.MAX_OBJECTS == _header_define("SBE_EM_MAX_OBJECTS")
    assert em.MAX_FEATURES == _header_define("SBE_EM_MAX_FEATURES")
    assert em.MAX_COST_BYTES == _header_define("SBE_EM_MAX_COST_BYTES")


def test_every_array_handed_to_the_library_is_bound_to_a_name():
    abi.check_ptr_arguments(em)


def _data(n=6, f=3, s=4, g=3, k=2):
    x = (np.arange(n * f).reshape(n, f) % max(s, 1)).astype(np.uint8)
    app = np.ones((f, s), dtype=np.uint8)
    avail = np.ones((g, n), dtype=np.uint8)
    return x, app, avail


def _create(n=6, f=3, s=4, g=3, k=2, x=None, app=None, avail=None, device=0):
    x0, a0, v0 = _data(n, f, s, g, k)
    x = x0 if x is None else x
    app = a0 if app is None else app
    avail = v0 if avail is None else avail
    lib = em.load()
    h = ct.c_void_p()
    rc = lib.sbe_em_create(ct.byref(h), device, n, f, s, x.ctypes.data, app.ctypes.data, g, k, avail.ctypes.data)
    return rc, h, lib.sbe_em_last_error(None).decode()


@pytest.mark.parametrize("kw,needle", [
    (dict(n=0), "n_objects=0"), (dict(n=(1 << 20) + 1), "n_objects="),
    (dict(f=0), "n_features=0"), (dict(f=(1 << 16) + 1), "n_features="),
    (dict(s=0), "n_states=0"), (dict(s=255), "n_states=255"),
    (dict(g=0, k=0), "n_groups=0"), (dict(g=1025), "n_groups=1025"),
    (dict(k=0), "n_clusters=0"), (dict(k=4), "n_clusters=4"),
    (dict(device=-1), "device -1"),
])
def test_c_abi_refuses_bad_shapes_before_the_device(kw, needle):
    n, f, s, g = kw.get("n", 6), kw.get("f", 3), kw.get("s", 4), kw.get("g", 3)
    x = np.zeros((max(n, 1), max(f, 1)), dtype=np.uint8)
    app = np.ones((max(f, 1), max(s, 1)), dtype=np.uint8)
    avail = np.ones((max(g, 1), max(n, 1)), dtype=np.uint8)
    rc, h, msg = _create(x=x, app=app, avail=avail, **kw)
    assert rc == 1 and not h and needle in msg, (rc, msg)


def test_c_abi_refuses_bad_data_before_the_device():
    x, app, avail = _data()
    x[2, 1] = 5                                          # > S = 4 (S itself is NA)
    rc, h, msg = _create(x=x)
    assert rc == 4 and "exceeds n_states" in msg
    x, app, avail = _data()
    app[1] = 0
    rc, h, msg = _create(app=app)
    assert rc == 4 and "feature 1 has no applicable state" in msg
    x, app, avail = _data()
    avail[:, 4] = 0
    rc, h, msg = _create(avail=avail)
    assert rc == 4 and "object 4 has no available group" in msg
    rc, h, msg = _create(x=np.full((6, 3), 4, dtype=np.uint8))      # all NA is valid data: only the device is missing here
    assert rc in (0, 5), msg
    if rc == 0:
        em.load().sbe_em_destroy(h)


def test_c_abi_null_handles_and_pointers():
    lib = em.load()
    assert lib.sbe_em_create(None, 0, 1, 1, 1, None, None, 1, 1, None) == 1
    assert b"null pointer argument: out" in lib.sbe_em_last_error(None)
    h = ct.c_void_p()
    assert lib.sbe_em_create(ct.byref(h), 0, 4, 2, 2, None, None, 1, 1, None) == 1
    assert b"null pointer argument: data" in lib.sbe_em_last_error(None)
    assert sorted(abi.check_null_handles(em, b"null EM handle")) == ["sbe_em_destroy", "sbe_em_last_kernel_ms", "sbe_em_run", "sbe_em_set_geo_cost"]


@pytest.fixture
def no_device(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(em, "load", refuse)


@pytest.mark.parametrize("bad,err", [
    (dict(x=np.zeros((4, 2), dtype=np.int32)), TypeError),
    (dict(app=np.ones((3, 2), dtype=bool)), ValueError),                 # F mismatch
    (dict(app=np.ones((2, 255), dtype=bool)), ValueError),               # S > 254
    (dict(avail=np.ones((1025, 4), dtype=bool)), ValueError),            # G > 1024
    (dict(avail=np.ones((3, 5), dtype=bool)), ValueError),               # N mismatch
    (dict(k=4), ValueError), (dict(k=0), ValueError),
])
def test_python_refuses_bad_shapes_before_the_device(no_device, bad, err):
    x = bad.get("x", np.zeros((4, 2), dtype=np.uint8))
    app = bad.get("app", np.ones((2, 3), dtype=bool))
    avail = bad.get("avail", np.ones((3, 4), dtype=bool))
    with pytest.raises(err):
        em.EmHandle(x, app, avail, bad.get("k", 2), device=0)


def test_state_index_refuses_rows_that_are_not_one_hot():
    f = np.zeros((3, 2, 4), dtype=bool)
    f[:, :, 1] = True
    f[1, 1] = False                                      # missing
    x = em.state_index(f)
    assert x.tolist() == [[1, 1], [1, 4], [1, 1]] and x.dtype == np.uint8
    f[0, 0, 2] = True
    with pytest.raises(ValueError, match="one-hot"):
        em.state_index(f)
    with pytest.raises(TypeError):
        em.state_index(f.astype(np.float32))


def test_cost_limits_are_refused_before_the_device():
    with pytest.raises(ValueError, match="cost must be"):
        em._check_cost(np.zeros((3, 4)), 1.0, 3)
    with pytest.raises(ValueError, match="scale"):
        em._check_cost(np.zeros((3, 3)), 0.0, 3)
    huge = np.lib.stride_tricks.as_strided(np.zeros(1), shape=(32769, 32769), strides=(0, 0))
    with pytest.raises(ValueError, match="32768"):
        em._check_cost(huge, 1.0, 32769)


def test_temperatures_are_the_reference_doubles():
    t = em.temperatures(50)
    assert t[0] == (50 / 1) ** 3 and t[49] == 1.0 and t[6] == (50 / 7) ** 3
    assert em.temperatures(0).size == 0


def test_handles_are_not_picklable():
    import pickle
    h = em.EmHandle.__new__(em.EmHandle)
    with pytest.raises(TypeError):
        pickle.dumps(h)
