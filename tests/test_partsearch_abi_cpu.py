"""CPU checks of the partition-search boundary (include/sbe_partsearch.h, sbayes_amd/partsearch.py): the symbols are
exported and bound by the module's own prototype table, the limits agree, and bad arguments are refused before the device is
touched."""
import ctypes as ct
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from sbayes_amd import _clusters, partdist, partsearch
from tests import _abi_header as abi

REPO = Path(__file__).resolve().parent.parent
HEADER = (REPO / "include" / "sbe_partsearch.h").read_text()


def test_every_symbol_of_the_header_is_exported_and_bound():
    names = abi.check_symbols(partsearch, HEADER, 11)
    assert {n[len("sbe_partsearch_"):] for n in names} == {"abi_version", "last_error", "create", "destroy", "reset", "append_rows", "rows", "scratch_bytes",
                                                            "search", "evaluate", "last_kernel_ms"}


def test_limits_agree_with_the_header():
    assert abi.macro(HEADER, "SBE_PARTSEARCH_MAX_CLUSTERS") == str(partsearch.MAX_CLUSTERS) == str(partdist.MAX_CLUSTERS)
    assert abi.macro(HEADER, "SBE_PARTSEARCH_MAX_OBJECTS") == str(partsearch.MAX_OBJECTS) == str(partdist.MAX_OBJECTS)
    assert abi.macro(HEADER, "SBE_PARTSEARCH_MAX_ROWS") == "(1 << 16)" and partsearch.MAX_ROWS == partdist.MAX_SUM_ROWS == 1 << 16
    assert abi.macro(HEADER, "SBE_PARTSEARCH_MAX_SWEEPS") == str(partsearch.MAX_SWEEPS) == "1024"
    assert abi.macro(HEADER, "SBE_PARTSEARCH_THREADS") == str(partsearch.THREADS) == "256"
    assert abi.macro(HEADER, "SBE_PARTSEARCH_MAX_SCRATCH_BYTES") == "(1ll << 30)" and partsearch.MAX_SCRATCH_BYTES == 1 << 30
    assert abi.macro(HEADER, "SBE_PARTSEARCH_LOSS_VI") == str(partsearch.LOSSES.index("vi")) == "0"
    assert abi.macro(HEADER, "SBE_PARTSEARCH_LOSS_BINDER") == str(partsearch.LOSSES.index("binder")) == "1"
    assert partsearch.MAX_OBJECTS < 1 << 16                                                     # a count in a uint16
    assert partsearch.MAX_ROWS * 2 * partsearch.MAX_OBJECTS ** 2 < 2 ** 53                     # a Binder sum, exact in the trace's float64 too
    assert partsearch.MAX_ROWS * (2 * partsearch.MAX_OBJECTS + 1) * 2 < 2 ** 63                # a Binder score
    lib = partsearch.load()
    for shape in [(1, 1, 1), (2, 255, 3), (5, 256, 1), (5, 257, 65), (8, 1 << 16, 101), (5, 10000, 64), (3, 1000, (1 << 24) - 1)]:
        assert lib.sbe_partsearch_scratch_bytes(*shape) == partsearch.scratch_bytes(*shape) > 0, shape
    assert partsearch.scratch_bytes(1, 1, 1) == 4 * 256 * 2 and partsearch.scratch_bytes(5, 257, 3) == 3 * 36 * 512 * 2
    # the speed tool's largest call fits; 102 starts of the largest shape do not
    assert partsearch.scratch_bytes(5, 10000, 64) < partsearch.MAX_SCRATCH_BYTES < partsearch.scratch_bytes(8, 1 << 16, 102)
    for shape in [(0, 1, 1), (9, 1, 1), (1, 0, 1), (1, (1 << 16) + 1, 1), (1, 1, 0), (1, 1, 1 << 24)]:
        assert lib.sbe_partsearch_scratch_bytes(*shape) == 0, shape
    for shape in [(0, 1, 1), (9, 1, 1), (1, 0, 1), (1, 16385, 1), (1, 1, 0), (1, 1, (1 << 16) + 1)]:
        with pytest.raises(ValueError):
            partsearch.LIMITS.check_shape(*shape)


def test_every_array_handed_to_the_library_is_bound_to_a_name():
    abi.check_ptr_arguments(partsearch)


def test_c_abi_validates_before_the_device():
    assert sorted(abi.check_null_handles(partsearch)) == sorted(set(partsearch.PROTOTYPES) - {"sbe_partsearch_abi_version", "sbe_partsearch_last_error",
                                                                                               "sbe_partsearch_scratch_bytes"})


def test_handles_are_not_picklable():
    abi.check_not_picklable(partsearch.SearchHandle)


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to create a handle fails the test."""
    def refuse(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(partsearch.SearchHandle, "__init__", refuse)
    monkeypatch.setattr(partdist.PartitionHandle, "__init__", refuse)


def _z(*shape):
    return np.zeros(shape, dtype=np.uint8)


def _overlap():
    c = _z(3, 2, 5)
    c[1, 0, 4] = c[1, 1, 4] = 1
    return c


BAD_RUNS = [
    ([], {}, ValueError, r"0 runs; the partition store takes 1 \.\. 64"),
    ([_z(3, 9, 5)], {}, ValueError, r"9 clusters; the partition store takes 1 \.\. 8"),
    ([_z(2, 1, 16385)], {}, ValueError, r"16385 objects; the partition store takes 1 \.\. 16384"),
    ([_z(3, 2, 5), _z(3, 2, 6)], {}, ValueError, "differ in clusters or objects"),
    ([np.full((3, 2, 5), 2)], {}, ValueError, "0 and 1 only"),
    ([np.zeros((3, 2, 5), dtype=np.float64)], {}, TypeError, "boolean or integer"),
    ([_z(3, 2, 5)], dict(burnin=1.0), ValueError, r"must lie in \[0, 1\)"),
    ([_z(0, 2, 5)], {}, ValueError, "hold no samples"),
    ([_z(3, 2, 5), _overlap()], {}, ValueError, r"sample 1: object 4 is in 2 areas \(the areas of a sample must be disjoint\)"),
]


@pytest.mark.parametrize("runs,kw,err,match", BAD_RUNS)
def test_bad_runs_are_refused_with_the_partition_distances_messages_before_the_device(no_device, runs, kw, err, match):
    with pytest.raises(err, match=match):
        partsearch.search(runs, **kw)
    with pytest.raises(err, match=match):
        partsearch.evaluate(runs, _z(2, 5), **kw)
    with pytest.raises(err, match=match):
        partsearch.credible_ball(runs, _z(2, 5), **kw)


def test_bad_options_are_refused_before_the_device(no_device, monkeypatch):
    runs = [_z(3, 2, 5)]
    with pytest.raises(ValueError, match="neither 'vi' nor 'binder'"):
        partsearch.search(runs, loss="rand")
    with pytest.raises(ValueError, match="neither 'vi' nor 'binder'"):
        partsearch.credible_ball(runs, _z(2, 5), loss="ari")
    for starts in (0, -1, (1 << 16) + 1):
        with pytest.raises(ValueError, match=r"starts=-?\d+ out of range \[1, 65536\]"):
            partsearch.search(runs, starts=starts)
    for sweeps in (0, 1025):
        with pytest.raises(ValueError, match=r"max_sweeps=\d+ out of range \[1, 1024\]"):
            partsearch.search(runs, max_sweeps=sweeps)
    for mass in (0.0, 1.5):
        with pytest.raises(ValueError, match=r"must lie in \(0, 1\]"):
            partsearch.credible_ball(runs, _z(2, 5), mass=mass)
    with pytest.raises(ValueError, match="samples are 2 clusters x 6 objects, the store holds 2 x 5"):
        partsearch.evaluate(runs, _z(2, 6))
    with pytest.raises(ValueError, match="object 4 is in 2 areas"):
        partsearch.evaluate(runs, _overlap()[1])
    with pytest.raises(ValueError, match=r"the estimate must be one sample \[2, 5\], got 3"):
        partsearch.credible_ball(runs, _z(3, 2, 5))
    monkeypatch.setattr(_clusters, "check_samples", lambda r, shape=None: r)    # (no copy of the large shape below)
    monkeypatch.setattr(_clusters, "check_disjoint", lambda b: None)
    wide = np.broadcast_to(_z(1, 1, 1), ((1 << 16) + 1, 1, 2))
    for call in (lambda: partsearch.search([wide]), lambda: partsearch.evaluate([wide], _z(1, 2))):
        with pytest.raises(ValueError, match=r"the selection holds 65537 samples, the limit for the sums is 65536"):
            call()


def test_a_handle_checks_its_own_arguments_before_the_library():
    h = object.__new__(partsearch.SearchHandle)
    h._h = ct.c_void_p()

    def refuse(*a, **k):
        raise AssertionError("the device was touched")
    h._lib = SimpleNamespace(**{name: refuse for name in partsearch.PROTOTYPES})
    h._unshape()
    for call in (lambda: h.append(_z(1, 2, 10)), lambda: h.search("vi", _z(1, 10), np.arange(10)[None]), lambda: h.evaluate(_z(1, 10))):
        with pytest.raises(ValueError, match="no shape yet"):
            call()
    for args, match in [((0, 10, 4), "0 clusters"), ((9, 10, 4), "9 clusters"), ((8, 16385, 4), "16385 objects"), ((3, 10, 0), "capacity=0"),
                        ((3, 10, (1 << 16) + 1), "capacity=65537")]:
        with pytest.raises(ValueError, match=match):
            h.reset(*args)
    h.n_clusters, h.n_objects, h.capacity, h._stored = 2, 10, 1 << 16, 0
    for call in (lambda: h.search("vi", _z(1, 10), np.arange(10)[None]), lambda: h.evaluate(_z(1, 10))):
        with pytest.raises(ValueError, match="holds no samples"):
            call()
    h._stored = (1 << 16) - 1
    with pytest.raises(ValueError, match="samples are 2 clusters x 11 objects, the store holds 2 x 10"):
        h.append(_z(1, 2, 11))
    with pytest.raises(ValueError, match="0 and 1 only"):
        h.append(np.full((1, 2, 10), 2, dtype=np.uint8))
    both = _z(1, 2, 10)
    both[0, :, 3] = 1
    with pytest.raises(ValueError, match="sample 0: object 3 is in 2 areas"):
        h.append(both)
    with pytest.raises(ValueError, match="store overflow: the store holds 65535 samples, 2 more exceed the capacity of 65536"):
        h.append(_z(2, 2, 10))
    identity = np.arange(10)[None]
    with pytest.raises(ValueError, match="neither 'vi' nor 'binder'"):
        h.search("rand", _z(1, 10), identity)
    with pytest.raises(ValueError, match=r"max_sweeps=0 out of range \[1, 1024\]"):
        h.search("vi", _z(1, 10), identity, max_sweeps=0)
    with pytest.raises(ValueError, match=r"init must be \[n, 10\] label rows"):
        h.search("vi", _z(1, 11), identity)
    with pytest.raises(TypeError, match="integer labels"):
        h.search("vi", np.zeros((1, 10)), identity)
    high = _z(2, 10)
    high[1, 3] = 3
    with pytest.raises(ValueError, match=r"init\[1\]\[3\]=3 is not a label in \[0, 2\]"):
        h.search("vi", high, np.repeat(identity, 2, axis=0))
    with pytest.raises(ValueError, match=r"labels\[1\]\[3\]=3 is not a label in \[0, 2\]"):
        h.evaluate(high)
    with pytest.raises(ValueError, match=r"order must be \[2, 10\]"):
        h.search("vi", _z(2, 10), identity)
    twice = np.repeat(identity, 2, axis=0)
    twice[1, 4] = 0
    with pytest.raises(ValueError, match=r"order\[1\] is not a permutation of 0 \.\. 9"):
        h.search("vi", _z(2, 10), twice)
    # the starts of one call stay within the scratch limit: the handle splits a longer list
    h.n_clusters, h._stored = 8, 1 << 16
    assert h.per_call() == 101 and partsearch.scratch_bytes(8, 1 << 16, 101) <= partsearch.MAX_SCRATCH_BYTES


def test_the_starts_and_the_renaming_of_blocks():
    y = np.array([[1, 1, 2, 2, 0, 0], [1, 1, 2, 2, 2, 0], [1, 1, 1, 2, 0, 0]], dtype=np.uint8)
    init, order, kinds = partsearch.make_starts(y, 1, 2, 7, seed=3)
    assert kinds == ["medoid", "sample", "sample", "sample", "zero", "random", "random"]
    assert np.array_equal(init[0], y[1]) and np.array_equal(order[0], np.arange(6)) and not init[4].any()
    assert all(any(np.array_equal(init[s], row) for row in y) for s in (1, 2, 3)) and init.max() <= 2
    assert all(sorted(order[s]) == list(range(6)) for s in range(7)) and order.dtype == np.int32 and init.dtype == np.uint8
    again = partsearch.make_starts(y, 1, 2, 7, seed=3)
    assert np.array_equal(again[0], init) and np.array_equal(again[1], order)
    # the samples' partition under other names comes back under theirs; Binder's loss keeps block 0 where it is
    other = np.array([2, 2, 0, 0, 1, 1], dtype=np.uint8)
    assert partsearch.rename_blocks(other, y, 2, "vi").tolist() == [1, 1, 2, 2, 0, 0]
    assert partsearch.rename_blocks(other, y, 2, "binder").tolist() == [1, 1, 0, 0, 2, 2]
    assert partsearch.rename_blocks(np.zeros(6, dtype=np.uint8), y, 2, "binder").tolist() == [0] * 6
    assert partsearch.labels_of(partsearch.rows_of(y, 2)).tolist() == y.tolist()
