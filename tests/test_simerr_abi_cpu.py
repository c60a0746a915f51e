"""CPU checks of the similarity-error boundary (include/sbe_simerr.h, sbayes_amd/simerr.py): the symbols are exported and
bound by the module's own prototype table, the limits agree, and bad arguments are refused before the device is touched."""
import ctypes as ct
import math
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from sbayes_amd import _clusters, simerr
from tests import _abi_header as abi
from tests import _simerr_oracle as orc

REPO = Path(__file__).resolve().parent.parent
HEADER = (REPO / "include" / "sbe_simerr.h").read_text()


def test_every_symbol_of_the_header_is_exported_and_bound():
    abi.check_symbols(simerr, HEADER, 12)


def test_limits_agree_with_the_header():
    assert abi.macro(HEADER, "SBE_SIMERR_MAX_CLUSTERS") == str(simerr.MAX_CLUSTERS) == "8"
    assert abi.macro(HEADER, "SBE_SIMERR_MAX_OBJECTS") == str(simerr.MAX_OBJECTS) == "8192"
    assert abi.macro(HEADER, "SBE_SIMERR_MAX_RUNS") == str(simerr.MAX_RUNS) == "64"
    assert abi.macro(HEADER, "SBE_SIMERR_MAX_ROWS") == "(1 << 20)" and simerr.MAX_ROWS == 1 << 20
    assert abi.macro(HEADER, "SBE_SIMERR_MAX_ELEMENTS") == "(1 << 24)" and simerr.MAX_ELEMENTS == 1 << 24
    assert abi.macro(HEADER, "SBE_SIMERR_STEP") == str(simerr.STEP) == "64"
    assert abi.macro(HEADER, "SBE_SIMERR_MAX_THRESHOLDS") == str(simerr.MAX_THRESHOLDS) == "4"
    assert abi.macro(HEADER, "SBE_SIMERR_MAX_IMAGE_BYTES") == "(1ll << 34)" and simerr.MAX_IMAGE_BYTES == 1 << 34
    assert simerr.MAX_OBJECTS ** 2 * 12 == 768 << 20                                   # one side: int32 S1 and int64 S2
    assert simerr.MAX_ELEMENTS ** 2 == 1 << 48 and (1 << 48) < 1 << 53                    # nB S2, S1^2, D and nB^2 are exact in a double
    lib = simerr.load()
    for shape in [(1, 1, 1, 1, 1), (2, 3, 33, 85, 7), (3, 8, 257, 33, 33), (2, 8, 2, 1 << 20, 1 << 10), (4, 5, 1000, 10000, 100),
                  (4, 5, 1000, 10000, 10), (1, 1, 8192, 1 << 20, 1)]:
        assert lib.sbe_simerr_image_bytes(*shape) == simerr.image_bytes(*shape) > 0, shape
    assert simerr.image_bytes(2, 3, 33, 85, 7) == 64 * 2 * 13 * 1 * 32                   # 13 batches (the last incomplete) of one step
    assert simerr.image_bytes(1, 5, 1, 26, 13) == 32 * 2 * 2 * 32                        # b K = 65: two steps a batch
    # the store of the limit test (two runs of 2^20 samples of 8 x 2 in batches of 2^10) fits, as do the speed tool's; one sample per
    # batch at the largest shape does not
    assert simerr.image_bytes(3, 8, 2, 1 << 20, 1 << 10) == 384 << 20 < simerr.MAX_IMAGE_BYTES
    assert simerr.image_bytes(4, 5, 1000, 10000, 10) < simerr.MAX_IMAGE_BYTES < simerr.image_bytes(1, 1, 8192, 1 << 20, 1)
    for shape in [(0, 1, 1, 1, 1), (65, 1, 1, 1, 1), (1, 0, 1, 1, 1), (1, 9, 1, 1, 1), (1, 1, 0, 1, 1), (1, 1, 8193, 1, 1), (1, 1, 1, 0, 1),
                  (1, 1, 1, (1 << 20) + 1, 1), (1, 1, 1, 4, 0), (1, 1, 1, 4, 5)]:
        assert lib.sbe_simerr_image_bytes(*shape) == 0, shape
        with pytest.raises(ValueError):
            simerr._check_shape(*shape)


def test_every_array_handed_to_the_library_is_bound_to_a_name():
    abi.check_ptr_arguments(simerr)


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to create a handle fails the test."""
    def refuse(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(simerr.SimErrHandle, "__init__", refuse)


def _z(*shape):
    return np.zeros(shape, dtype=np.uint8)


def _wide(*shape):
    """Zeros of a large shape that take no memory (the checks look at shapes before they copy anything)."""
    return np.broadcast_to(_z(1, 1, 1), shape)


BAD_RUNS = [
    ([], {}, ValueError, r"0 runs; the similarity-error store takes 1 \.\. 64"),
    ([_z(9, 2, 5)] * 65, {}, ValueError, r"65 runs; the similarity-error store takes 1 \.\. 64"),
    ([_z(9, 0, 5)], {}, ValueError, r"0 clusters; the similarity-error store takes 1 \.\. 8"),
    ([_z(9, 9, 5)], {}, ValueError, r"9 clusters; the similarity-error store takes 1 \.\. 8"),
    ([_z(9, 2, 0)], {}, ValueError, "0 objects"),
    ([_z(9, 1, 8193)], {}, ValueError, r"8193 objects; the similarity-error store takes 1 \.\. 8192"),
    ([_z(9, 2, 5), _z(9, 2, 6)], {}, ValueError, "differ in clusters or objects"),
    ([_z(9, 5)], {}, ValueError, r"\[n_samples, n_clusters, n_objects\]"),
    ([np.full((9, 2, 5), 2)], {}, ValueError, "0 and 1 only"),
    ([np.zeros((9, 2, 5), dtype=np.float64)], {}, TypeError, "boolean or integer"),
    ([_z(9, 2, 5)], dict(burnin=1.0), ValueError, r"must lie in \[0, 1\)"),
    ([_z(9, 2, 5)], dict(batch_rows=0), ValueError, r"batch_rows=0 out of range \[1, 9\]"),
    ([_z(9, 2, 5)], dict(batch_rows=10), ValueError, r"batch_rows=10 out of range \[1, 9\]"),
    ([_z(9, 2, 5)], dict(batch_rows=2.5), ValueError, "not a whole number"),
    ([_z(9, 2, 5)], dict(batch_rows=5), ValueError, r"hold 1 complete batches of 5 samples \(5 samples in all\); a side takes at least 2"),
    ([_z(0, 2, 5)], {}, ValueError, r"hold 0 complete batches of 1 samples \(0 samples in all\)"),
    ([_z(1, 2, 5)], {}, ValueError, r"hold 1 complete batches of 1 samples"),
]


@pytest.mark.parametrize("runs,kw,err,match", BAD_RUNS)
def test_bad_input_is_refused_before_the_device(no_device, runs, kw, err, match):
    for fn in (simerr.similarity_error, simerr.run_agreement):
        with pytest.raises(err, match=match):
            fn(runs, **kw)


def test_run_agreement_asks_two_batches_of_every_run_and_checks_its_thresholds(no_device):
    with pytest.raises(ValueError, match=r"hold 1 complete batches of 4 samples \(4 samples in all\)"):
        simerr.run_agreement([_z(12, 2, 5), _z(7, 2, 5)], batch_rows=4)
    with pytest.raises(ValueError, match=r"5 thresholds; a comparison takes 0 \.\. 4"):
        simerr.run_agreement([_z(12, 2, 5)] * 2, thresholds=(1, 2, 3, 4, 5))
    with pytest.raises(ValueError, match="not a number"):
        simerr.run_agreement([_z(12, 2, 5)] * 2, thresholds=(1.0, math.nan))


def test_shapes_beyond_the_limits_are_refused_before_the_device(no_device, monkeypatch):
    monkeypatch.setattr(_clusters, "check_samples", lambda r, shape=None: r)    # (no copy of the large shapes below)
    with pytest.raises(ValueError, match="capacity=1048577 out of range"):
        simerr.similarity_error([_wide((1 << 20) + 1, 1, 1)])
    # T K = 2^24 + K: three runs of 2^20, 2^20 and 1 samples of K = 8 in batches of one sample
    with pytest.raises(ValueError, match=r"2097153 samples x 8 clusters = 16777224 elements, the limit is 16777216"):
        simerr.similarity_error([_wide(1 << 20, 8, 2), _wide(1 << 20, 8, 2), _wide(1, 8, 2)], batch_rows=1)
    with pytest.raises(ValueError, match=r"takes \d+ bytes on the device, the limit is 17179869184"):
        simerr.similarity_error([_wide(1 << 20, 1, 8192)], batch_rows=1)


def test_c_abi_validates_before_the_device():
    assert sorted(abi.check_null_handles(simerr)) == sorted(set(simerr.PROTOTYPES) - {"sbe_simerr_abi_version", "sbe_simerr_last_error", "sbe_simerr_image_bytes"})


def test_handles_are_not_picklable():
    abi.check_not_picklable(simerr.SimErrHandle)


def test_a_handle_checks_its_own_arguments_before_the_library():
    h = object.__new__(simerr.SimErrHandle)
    h._h = ct.c_void_p()

    def refuse(*a, **k):
        raise AssertionError("the device was touched")
    h._lib = SimpleNamespace(**{name: refuse for name in simerr.PROTOTYPES})
    shape = (3, 8, 10, 1 << 20, 1)

    def shaped():
        h.n_runs, h.n_clusters, h.n_objects, h.capacity, h.batch_rows = shape
        h.side_batches = [0, 0]
    shaped()
    for args, match in [((65, 3, 10, 4, 2), "65 runs"), ((2, 0, 10, 4, 2), "0 clusters"), ((2, 9, 10, 4, 2), "9 clusters"),
                        ((2, 8, 8193, 4, 2), "8193 objects"), ((2, 3, 10, 0, 1), "capacity=0"), ((2, 3, 10, (1 << 20) + 1, 2), "capacity="),
                        ((2, 3, 10, 4, 0), r"batch_rows=0 out of range \[1, 4\]"), ((2, 3, 10, 4, 5), r"batch_rows=5 out of range \[1, 4\]"),
                        ((64, 1, 8192, 1 << 20, 1), "bytes on the device")]:
        with pytest.raises(ValueError, match=match):
            h.reset(*args)
        shaped()
    h._stored = [1 << 20, 1 << 20, 1]
    with pytest.raises(ValueError, match=r"run 3 out of range \[0, 3\)"):
        h.append(3, _z(1, 8, 10))
    with pytest.raises(ValueError, match="samples are 8 clusters x 11 objects, the store holds 8 x 10"):
        h.append(0, _z(1, 8, 11))
    with pytest.raises(ValueError, match="0 and 1 only"):
        h.append(2, np.full((1, 8, 10), 2, dtype=np.uint8))
    with pytest.raises(ValueError, match="store overflow: run 0 holds 1048576 samples, 2 more exceed the capacity of 1048576"):
        h.append(0, _z(2, 8, 10))
    with pytest.raises(ValueError, match="16777224 elements, the limit is 16777216"):        # T K = 2^24 + K
        h.moments()
    with pytest.raises(ValueError, match=r"hold 0 complete batches of 1 samples \(0 samples in all\)"):   # an empty selection
        h.moments(runs=[])
    with pytest.raises(ValueError, match=r"hold 1 complete batches of 1 samples \(1 samples in all\)"):   # a side with one batch
        h.moments(runs=[2])
    h.batch_rows, h._stored = 1 << 19, [(1 << 20) - 1, 1 << 19, 0]
    with pytest.raises(ValueError, match=r"hold 1 complete batches of 524288 samples \(1048575 samples in all\)"):
        h.moments(runs=[0])
    for side in (2, -1, True, 0.5):
        with pytest.raises(ValueError, match="neither 0 nor 1"):
            h.moments([0, 1], side=side)
    with pytest.raises(ValueError, match="run 7 out of range"):
        h.moments(runs=[0, 7])
    with pytest.raises(ValueError, match=r"5 thresholds; a comparison takes 0 \.\. 4"):
        h.compare(thresholds=(1, 2, 3, 4, 5))
    with pytest.raises(ValueError, match="not a number"):
        h.compare(thresholds=(math.nan,))
    h.n_runs = 0
    with pytest.raises(ValueError, match="no shape yet"):
        h.moments()
    with pytest.raises(ValueError, match="no shape yet"):
        h.compare()


def test_what_the_host_forms_from_the_integers():
    rng = np.random.default_rng(7500)
    runs = [(rng.random((s, 3, 11)) < 0.4).astype(np.uint8) for s in (24, 30)]
    s1, s2, nb = orc.moments(runs, 6)
    err = simerr.SimilarityError(s1.astype(np.int32), orc.variance(s1, s2, nb), nb, 6)
    assert err.n_samples == 54 and np.array_equal(err.probability, orc.probability(s1, nb, 6))
    assert np.array_equal(err.se, np.sqrt(orc.se_squared(s1, s2, nb, 6))) and err.se.dtype == np.float64
    p = err.probability
    positive = err.se > 0
    assert positive.any() and np.array_equal(err.ess[positive], (p * (1 - p))[positive] / (err.se * err.se)[positive])
    still = simerr.SimilarityError(np.full((2, 2), 8, dtype=np.int32), np.zeros((2, 2), dtype=np.int64), 4, 2)
    assert not still.se.any() and np.isinf(still.ess).all() and still.probability.tolist() == [[1.0, 1.0], [1.0, 1.0]]
    sides = [orc.moments([r], 6) for r in runs]
    got = simerr.z_squared(sides[0][0], orc.variance(*sides[0]), sides[0][2], sides[1][0], orc.variance(*sides[1]), sides[1][2])
    assert np.array_equal(got, orc.z2(*sides))
    assert simerr.z_squared([3, 3], [0, 0], 2, [3, 0], [0, 0], 2).tolist() == [0.0, math.inf]
    assert simerr.Moments(s1.astype(np.int32), s2, nb).variance.tolist() == orc.variance(s1, s2, nb).tolist()
    assert simerr.default_batch_rows([37, 50]) == 6 and simerr.default_batch_rows([0]) == 1 and simerr.default_batch_rows([10 ** 6]) == 1000


def test_the_agreement_file(tmp_path):
    agreement = simerr.RunAgreement(np.array([[0.0, 2.5], [2.5, 0.0]]), np.array([[[0, 0], [1, 4]], [[1, 4], [0, 0]]], dtype=np.int32),
                                    np.zeros((2, 2, 2)), np.array([[0.0, 0.1], [0.1, 0.0]]),
                                    np.zeros((2, 2, 5)), (3.84, 6.63), (6, 9), 5)
    agreement.share[0, 1] = [0.25, 0.125]
    simerr.write_agreement(tmp_path / "agreement_K3.tsv", ["a.txt", "b.txt"], agreement)
    lines = (tmp_path / "agreement_K3.tsv").read_text().splitlines()
    assert lines[0].split("\t") == ["run_a", "run_b", "batches_a", "batches_b", "batch_rows", "max_z2", "object_i", "object_j", "max_abs",
                                    "share_above_3.84", "share_above_6.63"]
    assert lines[1:] == ["a.txt\tb.txt\t6\t9\t5\t2.5\t1\t4\t0.1\t0.25\t0.125"]
