"""CPU checks of the partition-distance boundary (include/sbe_partdist.h, sbayes_amd/partdist.py): the symbols are exported
and bound by the module's own prototype table, the limits agree, and bad arguments are refused before the device is touched."""
import ctypes as ct
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from sbayes_amd import _clusters, partdist
from tests import _abi_header as abi

REPO = Path(__file__).resolve().parent.parent
HEADER = (REPO / "include" / "sbe_partdist.h").read_text()


def test_every_symbol_of_the_header_is_exported_and_bound():
    abi.check_symbols(partdist, HEADER, 14)


def test_limits_agree_with_the_header():
    assert abi.macro(HEADER, "SBE_PARTDIST_MAX_CLUSTERS") == str(partdist.MAX_CLUSTERS) == "8"
    assert abi.macro(HEADER, "SBE_PARTDIST_MAX_OBJECTS") == str(partdist.MAX_OBJECTS) == "16384"
    assert abi.macro(HEADER, "SBE_PARTDIST_MAX_RUNS") == str(partdist.MAX_RUNS) == "64"
    assert abi.macro(HEADER, "SBE_PARTDIST_MAX_ROWS") == "(1 << 20)" and partdist.MAX_ROWS == 1 << 20
    assert abi.macro(HEADER, "SBE_PARTDIST_ROUND") == str(partdist.ROUND) == "256"
    assert abi.macro(HEADER, "SBE_PARTDIST_MAX_IMAGE_BYTES") == "(1ll << 34)" and partdist.MAX_IMAGE_BYTES == 1 << 34
    assert abi.macro(HEADER, "SBE_PARTDIST_MAX_BLOCK") == "(1 << 28)" and partdist.MAX_BLOCK == 1 << 28
    assert abi.macro(HEADER, "SBE_PARTDIST_MAX_SUM_ROWS") == "(1 << 16)" and partdist.MAX_SUM_ROWS == 1 << 16
    assert abi.macro(HEADER, "SBE_PARTDIST_MAX_PAIRS") == "(1 << 24)" and partdist.MAX_PAIRS == 1 << 24
    assert 2 * partdist.MAX_OBJECTS ** 2 == 1 << 29 < 2 ** 31                                  # sum a^2 + sum b^2 in an int32
    assert partdist.MAX_SUM_ROWS * 2 * partdist.MAX_OBJECTS ** 2 < 2 ** 63                    # a binder sum
    assert [partdist.padded_clusters(k) for k in range(1, 9)] == [1, 2, 4, 4, 8, 8, 8, 8]
    lib = partdist.load()
    for shape in [(1, 1, 1, 1), (2, 3, 33, 85), (3, 8, 257, 33), (2, 8, 2, 1 << 20), (64, 5, 1000, 10000), (1, 8, 16384, 1 << 20), (1, 5, 1000, 10000)]:
        assert lib.sbe_partdist_image_bytes(*shape) == partdist.image_bytes(*shape) > 0, shape
    # one sample of one area of one object: a tile of 32 rows of 128 bytes, and one word of bits
    assert partdist.image_bytes(1, 1, 1, 1) == 32 * 128 + 4
    # the speed tool's largest shape fits; the largest shape of the limits does not
    assert partdist.image_bytes(1, 5, 1000, 10000) < partdist.MAX_IMAGE_BYTES < partdist.image_bytes(1, 8, 16384, 1 << 20)
    for shape in [(0, 1, 1, 1), (65, 1, 1, 1), (1, 0, 1, 1), (1, 9, 1, 1), (1, 1, 0, 1), (1, 1, 16385, 1), (1, 1, 1, 0), (1, 1, 1, (1 << 20) + 1)]:
        assert lib.sbe_partdist_image_bytes(*shape) == 0, shape
        with pytest.raises(ValueError):
            partdist.LIMITS.check_shape(*shape)


def test_every_array_handed_to_the_library_is_bound_to_a_name():
    abi.check_ptr_arguments(partdist)


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to create a handle fails the test."""
    def refuse(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(partdist.PartitionHandle, "__init__", refuse)


def _z(*shape):
    return np.zeros(shape, dtype=np.uint8)


def _wide(*shape):
    """Zeros of a large shape that take no memory (the checks look at shapes before they copy anything)."""
    return np.broadcast_to(_z(1, 1, 1), shape)


def _overlap():
    c = _z(3, 2, 5)
    c[1, 0, 4] = c[1, 1, 4] = 1
    return c


BAD_RUNS = [
    ([], {}, ValueError, r"0 runs; the partition store takes 1 \.\. 64"),
    ([_z(3, 2, 5)] * 65, {}, ValueError, r"65 runs; the partition store takes 1 \.\. 64"),
    ([_z(3, 0, 5)], {}, ValueError, r"0 clusters; the partition store takes 1 \.\. 8"),
    ([_z(3, 9, 5)], {}, ValueError, r"9 clusters; the partition store takes 1 \.\. 8"),
    ([_z(3, 2, 0)], {}, ValueError, "0 objects"),
    ([_z(2, 1, 16385)], {}, ValueError, r"16385 objects; the partition store takes 1 \.\. 16384"),
    ([_z(3, 2, 5), _z(3, 2, 6)], {}, ValueError, "differ in clusters or objects"),
    ([_z(3, 5)], {}, ValueError, r"\[n_samples, n_clusters, n_objects\]"),
    ([np.full((3, 2, 5), 2)], {}, ValueError, "0 and 1 only"),
    ([np.zeros((3, 2, 5), dtype=np.float64)], {}, TypeError, "boolean or integer"),
    ([_z(3, 2, 5)], dict(burnin=1.0), ValueError, r"must lie in \[0, 1\)"),
    ([_z(0, 2, 5)], {}, ValueError, "hold no samples"),
    ([_z(3, 2, 5), _overlap()], {}, ValueError, r"sample 1: object 4 is in 2 areas \(the areas of a sample must be disjoint\)"),
]


@pytest.mark.parametrize("runs,kw,err,match", BAD_RUNS)
def test_bad_input_is_refused_before_the_device(no_device, runs, kw, err, match):
    for fn in (partdist.distances, partdist.medoid, partdist.run_distances, partdist.credible_ball):
        with pytest.raises(err, match=match):
            fn(runs, **kw)


def test_bad_options_are_refused_before_the_device(no_device):
    runs = [_z(3, 2, 5)]
    with pytest.raises(ValueError, match="neither 'vi' nor 'binder'"):
        partdist.medoid(runs, loss="rand")
    with pytest.raises(ValueError, match="neither 'vi' nor 'binder'"):
        partdist.credible_ball(runs, loss="ari")
    for mass in (0.0, 1.5, -1):
        with pytest.raises(ValueError, match=r"must lie in \(0, 1\]"):
            partdist.credible_ball(runs, mass=mass)
    with pytest.raises(ValueError, match="samples are 2 clusters x 6 objects, the store holds 2 x 5"):
        partdist.credible_ball(runs, estimate=_z(2, 6))
    with pytest.raises(ValueError, match="object 4 is in 2 areas"):
        partdist.credible_ball(runs, estimate=_overlap()[1])
    with pytest.raises(ValueError, match=r"64 runs; the partition store takes 1 \.\. 63"):      # the estimate takes a run of its own
        partdist.credible_ball([_z(1, 2, 5)] * 64, estimate=_z(2, 5))


def test_shapes_beyond_the_limits_are_refused_before_the_device(no_device, monkeypatch):
    monkeypatch.setattr(_clusters, "check_samples", lambda r, shape=None: r)    # (no copy of the large shapes below)
    monkeypatch.setattr(_clusters, "check_disjoint", lambda b: None)
    with pytest.raises(ValueError, match="capacity=1048577 out of range"):
        partdist.distances([_wide((1 << 20) + 1, 1, 1)])
    with pytest.raises(ValueError, match=r"takes \d+ bytes on the device, the limit is 17179869184"):
        partdist.distances([_wide(1 << 20, 8, 16384)])
    with pytest.raises(ValueError, match=r"16385 samples make 268468225 pairs, the limit is 268435456"):
        partdist.distances([_wide(16384, 1, 2), _wide(1, 1, 2)])
    for fn in (partdist.medoid, partdist.run_distances, partdist.credible_ball):
        with pytest.raises(ValueError, match=r"the selection holds 65537 samples, the limit for the sums is 65536"):
            fn([_wide(1 << 16, 1, 2), _wide(1, 1, 2)])


def test_c_abi_validates_before_the_device():
    assert sorted(abi.check_null_handles(partdist)) == sorted(set(partdist.PROTOTYPES) - {"sbe_partdist_abi_version", "sbe_partdist_last_error", "sbe_partdist_image_bytes"})


def test_handles_are_not_picklable():
    abi.check_not_picklable(partdist.PartitionHandle)


def test_a_handle_checks_its_own_arguments_before_the_library():
    h = object.__new__(partdist.PartitionHandle)
    h._h = ct.c_void_p()

    def refuse(*a, **k):
        raise AssertionError("the device was touched")
    h._lib = SimpleNamespace(**{name: refuse for name in partdist.PROTOTYPES})
    shape = (3, 2, 10, 1 << 20)
    h.n_runs, h.n_clusters, h.n_objects, h.capacity = shape
    for args, match in [((65, 3, 10, 4), "65 runs"), ((2, 0, 10, 4), "0 clusters"), ((2, 9, 10, 4), "9 clusters"),
                        ((2, 8, 16385, 4), "16385 objects"), ((2, 3, 10, 0), "capacity=0"), ((2, 3, 10, (1 << 20) + 1), "capacity="),
                        ((64, 8, 16384, 1 << 20), "bytes on the device")]:
        with pytest.raises(ValueError, match=match):
            h.reset(*args)
        h.n_runs, h.n_clusters, h.n_objects, h.capacity = shape
    h._stored = [1 << 20, 1 << 16, 1]
    with pytest.raises(ValueError, match=r"run 3 out of range \[0, 3\)"):
        h.append(3, _z(1, 2, 10))
    with pytest.raises(ValueError, match="samples are 2 clusters x 11 objects, the store holds 2 x 10"):
        h.append(0, _z(1, 2, 11))
    with pytest.raises(ValueError, match="0 and 1 only"):
        h.append(2, np.full((1, 2, 10), 2, dtype=np.uint8))
    both = _z(1, 2, 10)
    both[0, :, 3] = 1
    with pytest.raises(ValueError, match="sample 0: object 3 is in 2 areas"):                # an overlap
        h.append(2, both)
    with pytest.raises(ValueError, match="store overflow: run 0 holds 1048576 samples, 2 more exceed the capacity of 1048576"):
        h.append(0, _z(2, 2, 10))
    with pytest.raises(ValueError, match=r"rows \[0, 0 \+ 2\) are not within the 1 samples of run 2"):
        h.block(2, 0, 2)
    with pytest.raises(ValueError, match=r"cols \[1, 1 \+ 0\) are not within the 1 samples of run 2"):
        h.block(0, 0, 1, col_run=2, col_first=1)
    with pytest.raises(ValueError, match=r"rows \[-1, -1 \+ 1\)"):
        h.block(0, -1, 1)
    with pytest.raises(ValueError, match="run 7 out of range"):
        h.block(0, 0, 1, col_run=7)
    with pytest.raises(ValueError, match=r"a block of 1048576 x 65536 = 68719476736 entries, the limit is 268435456"):
        h.block(0, col_run=1)
    with pytest.raises(ValueError, match="at least one of binder, vi and sumsq"):
        h.block(2, binder=False, vi=False, sumsq=False)
    with pytest.raises(ValueError, match="the selection holds 1114113 samples, the limit for the sums is 65536"):
        h.sums()
    with pytest.raises(ValueError, match="hold no samples"):                                 # an empty selection
        h.sums(runs=[])
    with pytest.raises(ValueError, match="run 5 out of range"):
        h.sums(runs=[0, 5])
    with pytest.raises(ValueError, match="run 5 out of range"):
        h.sizes(5)
    with pytest.raises(ValueError, match=r"pairs must be \[n_pairs, 4\]"):
        h.tables(np.zeros((2, 3), dtype=np.int64))
    with pytest.raises(ValueError, match=r"pairs must be \[n_pairs, 4\]"):
        h.tables(np.zeros((0, 4), dtype=np.int64))
    with pytest.raises(ValueError, match=r"pairs\[1\]: \(run 2, sample 1\) is not a stored sample"):
        h.tables([[0, 0, 1, 0], [0, 5, 2, 1]])
    with pytest.raises(ValueError, match=r"pairs\[0\]: \(run 3, sample 0\) is not a stored sample"):
        h.tables([[3, 0, 1, 0]])
    h.n_runs = 0
    for call in (h.sums, lambda: h.block(0), lambda: h.sizes(0), lambda: h.tables([[0, 0, 0, 0]])):
        with pytest.raises(ValueError, match="no shape yet"):
            call()


def test_the_trace_file_reads_back_as_a_column(tmp_path):
    from sbayes_amd import diag
    d = np.random.default_rng(8).random(17) * 3.0
    partdist.write_trace(tmp_path / "partition_trace_K3_0.txt", d, "vi")
    names, rows = diag.read_stats(tmp_path / "partition_trace_K3_0.txt")
    assert names == ["vi_to_estimate"] and rows.shape == (17, 1) and np.array_equal(rows[:, 0], d)
