"""CPU checks of the consensus boundary (include/sbe_consensus.h, sbayes_amd/consensus.py): the symbols are exported and
bound by the module's own prototype table, the limits agree, and bad arguments are refused before the device is touched."""
import ctypes as ct
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from sbayes_amd import _clusters, align, consensus
from tests import _abi_header as abi

REPO = Path(__file__).resolve().parent.parent
HEADER = (REPO / "include" / "sbe_consensus.h").read_text()


def test_every_symbol_of_the_header_is_exported_and_bound():
    abi.check_symbols(consensus, HEADER, 13)


def test_limits_agree_with_the_header():
    assert abi.macro(HEADER, "SBE_CONSENSUS_MAX_CLUSTERS") == str(consensus.MAX_CLUSTERS) == "8"
    assert abi.macro(HEADER, "SBE_CONSENSUS_MAX_OBJECTS") == str(consensus.MAX_OBJECTS) == "16384"
    assert abi.macro(HEADER, "SBE_CONSENSUS_MAX_RUNS") == str(consensus.MAX_RUNS) == "64"
    assert abi.macro(HEADER, "SBE_CONSENSUS_MAX_ROWS") == "(1 << 20)" and consensus.MAX_ROWS == 1 << 20
    assert abi.macro(HEADER, "SBE_CONSENSUS_MAX_ELEMENTS") == "(1 << 24)" and consensus.MAX_ELEMENTS == 1 << 24
    assert abi.macro(HEADER, "SBE_CONSENSUS_ROUND") == str(consensus.ROUND) == "256"
    assert abi.macro(HEADER, "SBE_CONSENSUS_MAX_IMAGE_BYTES") == "(1ll << 34)" and consensus.MAX_IMAGE_BYTES == 1 << 34
    assert consensus.MAX_OBJECTS ** 2 * 4 == 1 << 30 and consensus.MAX_OBJECTS <= 1 << 16      # one matrix; a member index in 16 bits
    assert consensus.MAX_OBJECTS * consensus.MAX_ELEMENTS ** 2 < 2 ** 63                        # a row sum of the comparison
    assert consensus.MAX_ELEMENTS * consensus.MAX_OBJECTS ** 2 < 2 ** 63                        # K T m^2 of a score
    lib = consensus.load()
    for shape in [(1, 1, 1, 1), (2, 3, 33, 85), (3, 8, 257, 33), (2, 8, 2, 1 << 20), (64, 5, 1000, 10000), (1, 8, 16384, 1 << 20)]:
        assert lib.sbe_consensus_image_bytes(*shape) == consensus.image_bytes(*shape) > 0, shape
    # the store of the limit test (two runs of 2^20 samples of 8 x 2) and the speed tool's largest fit; the largest shape does not
    assert consensus.image_bytes(2, 8, 2, 1 << 20) == (256 + 64) << 20 < consensus.MAX_IMAGE_BYTES
    assert consensus.image_bytes(1, 8, 5000, 10000) < consensus.MAX_IMAGE_BYTES < consensus.image_bytes(1, 8, 16384, 1 << 20)
    for shape in [(0, 1, 1, 1), (65, 1, 1, 1), (1, 0, 1, 1), (1, 9, 1, 1), (1, 1, 0, 1), (1, 1, 16385, 1), (1, 1, 1, 0), (1, 1, 1, (1 << 20) + 1)]:
        assert lib.sbe_consensus_image_bytes(*shape) == 0, shape
        with pytest.raises(ValueError):
            consensus.LIMITS.check_shape(*shape)


def test_every_array_handed_to_the_library_is_bound_to_a_name():
    abi.check_ptr_arguments(consensus)


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to create a handle fails the test."""
    def refuse(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(consensus.ConsensusHandle, "__init__", refuse)


def _z(*shape):
    return np.zeros(shape, dtype=np.uint8)


def _wide(*shape):
    """Zeros of a large shape that take no memory (the checks look at shapes before they copy anything)."""
    return np.broadcast_to(_z(1, 1, 1), shape)


BAD_RUNS = [
    ([], {}, ValueError, r"0 runs; the consensus store takes 1 \.\. 64"),
    ([_z(3, 2, 5)] * 65, {}, ValueError, r"65 runs; the consensus store takes 1 \.\. 64"),
    ([_z(3, 0, 5)], {}, ValueError, r"0 clusters; the consensus store takes 1 \.\. 8"),
    ([_z(3, 9, 5)], {}, ValueError, r"9 clusters; the consensus store takes 1 \.\. 8"),
    ([_z(3, 2, 0)], {}, ValueError, "0 objects"),
    ([_z(2, 1, 16385)], {}, ValueError, r"16385 objects; the consensus store takes 1 \.\. 16384"),
    ([_z(3, 2, 5), _z(3, 2, 6)], {}, ValueError, "differ in clusters or objects"),
    ([_z(3, 5)], {}, ValueError, r"\[n_samples, n_clusters, n_objects\]"),
    ([np.full((3, 2, 5), 2)], {}, ValueError, "0 and 1 only"),
    ([np.zeros((3, 2, 5), dtype=np.float64)], {}, TypeError, "boolean or integer"),
    ([_z(3, 2, 5)], dict(burnin=1.0), ValueError, r"must lie in \[0, 1\)"),
    ([_z(0, 2, 5)], {}, ValueError, "hold no samples"),
]


@pytest.mark.parametrize("runs,kw,err,match", BAD_RUNS)
def test_bad_input_is_refused_before_the_device(no_device, runs, kw, err, match):
    for fn in (consensus.similarity, consensus.point_estimate, consensus.compare_runs):
        with pytest.raises(err, match=match):
            fn(runs, **kw)


def test_shapes_beyond_the_limits_are_refused_before_the_device(no_device, monkeypatch):
    monkeypatch.setattr(_clusters, "check_samples", lambda r, shape=None: r)    # (no copy of the large shapes below)
    with pytest.raises(ValueError, match="capacity=1048577 out of range"):
        consensus.similarity([_wide((1 << 20) + 1, 1, 1)])
    # T K = 2^24 + K: three runs of 2^20, 2^20 and 1 samples of K = 8
    with pytest.raises(ValueError, match=r"2097153 samples x 8 clusters = 16777224 elements, the limit is 16777216"):
        consensus.similarity([_wide(1 << 20, 8, 2), _wide(1 << 20, 8, 2), _wide(1, 8, 2)])
    with pytest.raises(ValueError, match="16777224 elements"):
        consensus.point_estimate([_wide(1 << 20, 8, 2), _wide(1 << 20, 8, 2), _wide(1, 8, 2)])
    with pytest.raises(ValueError, match=r"takes \d+ bytes on the device, the limit is 17179869184"):
        consensus.similarity([_wide(1 << 20, 8, 16384)])


def test_c_abi_validates_before_the_device():
    assert sorted(abi.check_null_handles(consensus)) == sorted(set(consensus.PROTOTYPES) - {"sbe_consensus_abi_version", "sbe_consensus_last_error", "sbe_consensus_image_bytes"})


def test_handles_are_not_picklable():
    abi.check_not_picklable(consensus.ConsensusHandle)


def test_a_handle_checks_its_own_arguments_before_the_library():
    h = object.__new__(consensus.ConsensusHandle)
    h._h = ct.c_void_p()

    def refuse(*a, **k):
        raise AssertionError("the device was touched")
    h._lib = SimpleNamespace(**{name: refuse for name in consensus.PROTOTYPES})
    shape = (3, 8, 10, 1 << 20)
    h.n_runs, h.n_clusters, h.n_objects, h.capacity = shape
    for args, match in [((65, 3, 10, 4), "65 runs"), ((2, 0, 10, 4), "0 clusters"), ((2, 9, 10, 4), "9 clusters"),
                        ((2, 8, 16385, 4), "16385 objects"), ((2, 3, 10, 0), "capacity=0"), ((2, 3, 10, (1 << 20) + 1), "capacity="),
                        ((64, 8, 16384, 1 << 20), "bytes on the device")]:
        with pytest.raises(ValueError, match=match):
            h.reset(*args)
        h.n_runs, h.n_clusters, h.n_objects, h.capacity = shape
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
        h.similarity()
    with pytest.raises(ValueError, match="hold no samples"):                                 # an empty selection
        h.similarity(runs=[])
    for slot in (2, -1, True, 0.5):
        with pytest.raises(ValueError, match="neither 0 nor 1"):
            h.similarity([2], slot=slot)
        with pytest.raises(ValueError, match="neither 0 nor 1"):
            h.scores(2, slot=slot)
    with pytest.raises(ValueError, match="run 7 out of range"):
        h.similarity(runs=[0, 7])
    with pytest.raises(ValueError, match="run 5 out of range"):
        h.scores(5)
    h.n_runs = 0
    with pytest.raises(ValueError, match="no shape yet"):
        h.similarity()
    with pytest.raises(ValueError, match="no shape yet"):
        h.compare()


def test_the_consensus_is_the_smallest_score_run_sample():
    assert consensus.argmin_score([np.array([5, 3, 3]), np.array([3, 9])]) == (0, 1)
    assert consensus.argmin_score([np.array([5, 4]), np.array([3, 3])]) == (1, 0)
    assert consensus.argmin_score([np.array([], dtype=np.int64), np.array([7])]) == (1, 0)
    with pytest.raises(ValueError, match="no sample"):
        consensus.argmin_score([np.array([], dtype=np.int64)])
    big = 1 << 62                                                           # (Python integers: no float on the way)
    assert consensus.difference(np.array([big, 3]), np.array([big, big]), 1 << 24, 1 << 24) == (16384.0, 8192.0)    # (the sum of the rows, 2^63, is beyond int64)


def test_the_cluster_and_similarity_files_round_trip(tmp_path):
    rng = np.random.default_rng(6)
    c = (rng.random((1, 3, 37)) < 0.4).astype(np.uint8)
    path = tmp_path / "consensus_K3.txt"
    align.write_clusters(path, c)
    lines = path.read_text().splitlines()
    assert len(lines) == 1 and [len(s) for s in lines[0].split("\t")] == [37, 37, 37]
    assert np.array_equal(align.read_clusters(path), c)
    p = rng.integers(0, 1000, (37, 37)) / 997.0
    consensus.write_similarity(tmp_path / "similarity_K3.txt", p)
    assert len((tmp_path / "similarity_K3.txt").read_text().splitlines()) == 37
    assert np.array_equal(consensus.read_similarity(tmp_path / "similarity_K3.txt"), p)
