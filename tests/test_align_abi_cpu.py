"""CPU checks of the alignment boundary (include/sbe_align.h, sbayes_amd/align.py): the symbols are exported and bound by
the module's own prototype table, the limits agree, and bad arguments are refused before the device is touched."""
import ctypes as ct
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from sbayes_amd import align
from tests import _abi_header as abi

REPO = Path(__file__).resolve().parent.parent
HEADER = (REPO / "include" / "sbe_align.h").read_text()


def test_every_symbol_of_the_header_is_exported_and_bound():
    abi.check_symbols(align, HEADER, 12)
    assert align.ABI_VERSION == 1


def test_limits_agree_with_the_header():
    assert abi.macro(HEADER, "SBE_ALIGN_MAX_CLUSTERS") == str(align.MAX_CLUSTERS) == "8"
    assert abi.macro(HEADER, "SBE_ALIGN_MAX_RUNS") == str(align.MAX_RUNS) == "64"
    assert abi.macro(HEADER, "SBE_ALIGN_MAX_ROWS") == "(1 << 20)" and align.MAX_ROWS == 1 << 20
    assert abi.macro(HEADER, "SBE_ALIGN_MAX_SEED_ROWS") == str(align.MAX_SEED_ROWS) == "1024"
    assert abi.macro(HEADER, "SBE_ALIGN_LDS_BYTES") == "(160 * 1024)" and align.LDS_BYTES == 160 * 1024
    assert abi.macro(HEADER, "SBE_ALIGN_STATIC_LDS") == str(align.STATIC_LDS)
    assert max(align.MAX_SEED_ROWS, 1) * align.MAX_ROWS + align.MAX_SEED_ROWS < 2 ** 31      # the int32 running sums
    lib = align.load()
    for k in range(1, 9):
        limit = align.max_objects(k)
        assert lib.sbe_align_max_objects(k) == limit
        # the running sums and the kernel's own LDS fit the 160 KiB of a CU, and one more object does not
        assert k * limit * 4 + align.STATIC_LDS <= 160 * 1024 < k * (limit + 1) * 4 + align.STATIC_LDS
        # the kernel pads the sums of every cluster to whole words of 32 objects and keeps 4 x 64 int64 partial
        # agreements and the permutation: both inside the static part
        assert k * 31 * 4 + 4 * 64 * 8 + 16 <= align.STATIC_LDS
    assert align.max_objects(8) == 4992 and align.max_objects(2) > 8192
    assert lib.sbe_align_max_objects(0) == 0 and lib.sbe_align_max_objects(9) == 0
    for k in (0, 9):
        with pytest.raises(ValueError, match=r"clusters; the alignment takes 1 \.\. 8"):
            align.max_objects(k)


def test_every_array_handed_to_the_library_is_bound_to_a_name():
    abi.check_ptr_arguments(align)


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to create a handle fails the test."""
    def refuse(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(align.AlignHandle, "__init__", refuse)


def _z(*shape):
    return np.zeros(shape, dtype=np.uint8)


@pytest.mark.parametrize("runs,kw,err,match", [
    ([], {}, ValueError, r"0 runs; the alignment takes 1 \.\. 64"),
    ([_z(3, 2, 5)] * 65, {}, ValueError, r"65 runs; the alignment takes 1 \.\. 64"),
    ([_z(3, 0, 5)], {}, ValueError, r"0 clusters; the alignment takes 1 \.\. 8"),
    ([_z(3, 9, 5)], {}, ValueError, r"9 clusters; the alignment takes 1 \.\. 8"),
    ([_z(3, 2, 0)], {}, ValueError, "0 objects"),
    ([np.broadcast_to(_z(1, 1, 1), (2, 8, 4993))], {}, ValueError, r"4993 objects; with 8 clusters the alignment takes 1 \.\. 4992"),
    ([np.broadcast_to(_z(1, 1, 1), ((1 << 20) + 1, 1, 1))], {}, ValueError, "capacity=1048577 out of range"),
    ([_z(3, 2, 5), _z(3, 2, 6)], {}, ValueError, "differ in clusters or objects"),
    ([_z(3, 5)], {}, ValueError, r"\[n_samples, n_clusters, n_objects\]"),
    ([np.full((3, 2, 5), 2)], {}, ValueError, "0 and 1 only"),
    ([np.zeros((3, 2, 5), dtype=np.float64)], {}, TypeError, "boolean or integer"),
    ([_z(3, 2, 5)], dict(pivot=1), ValueError, "pivot 1 out of range"),
    ([_z(3, 2, 5)], dict(within=1025), ValueError, r"seed=1025 must lie in \[0, 1024\]"),
    ([_z(3, 2, 5)], dict(within=-1), ValueError, "seed=-1"),
    ([_z(3, 2, 5)], dict(burnin=1.0), ValueError, r"must lie in \[0, 1\)"),
])
def test_bad_input_is_refused_before_the_device(no_device, runs, kw, err, match):
    with pytest.raises(err, match=match):
        align.align_runs(runs, **kw)


def test_the_one_run_forms_refuse_before_the_device(no_device):
    with pytest.raises(ValueError, match="seed=2000"):
        align.realign_within_run(_z(3, 2, 5), seed=2000)
    with pytest.raises(ValueError, match="9 clusters"):
        align.match_online(_z(3, 9, 5))


def test_c_abi_validates_before_the_device():
    assert sorted(abi.check_null_handles(align)) == sorted(set(align.PROTOTYPES) - {"sbe_align_abi_version", "sbe_align_last_error", "sbe_align_max_objects"})


def test_handles_are_not_picklable():
    abi.check_not_picklable(align.AlignHandle)


def test_a_handle_checks_its_own_arguments_before_the_library():
    h = object.__new__(align.AlignHandle)
    h._h = ct.c_void_p()

    def refuse(*a, **k):
        raise AssertionError("the device was touched")
    h._lib = SimpleNamespace(**{name: refuse for name in align.PROTOTYPES})
    h.n_runs, h.n_clusters, h.n_objects, h.capacity = 2, 3, 10, 4
    for args, match in [((65, 3, 10, 4), "65 runs"), ((2, 0, 10, 4), "0 clusters"), ((2, 9, 10, 4), "9 clusters"),
                        ((2, 8, 4993, 4), "4993 objects"), ((2, 3, 10, 0), "capacity=0"), ((2, 3, 10, (1 << 20) + 1), "capacity=")]:
        with pytest.raises(ValueError, match=match):
            h.reset(*args)
        h.n_runs, h.n_clusters, h.n_objects, h.capacity = 2, 3, 10, 4
    with pytest.raises(ValueError, match=r"run 2 out of range \[0, 2\)"):
        h.append(2, _z(1, 3, 10))
    with pytest.raises(ValueError, match="samples are 3 clusters x 11 objects, the store holds 3 x 10"):
        h.append(0, _z(1, 3, 11))
    h._stored = [3, 0]
    with pytest.raises(ValueError, match="store overflow: run 0 holds 3 samples, 2 more exceed the capacity of 4"):
        h.append(0, _z(2, 3, 10))
    with pytest.raises(ValueError, match="seed=1025"):
        h.within(1025)
    with pytest.raises(ValueError, match="one value per run"):
        h.counts(burn_rows=[0, 0, 0])
    with pytest.raises(ValueError, match="run 5 out of range"):
        h.runs(pivot=5)
    h.n_runs = 0
    with pytest.raises(ValueError, match="no shape yet"):
        h.within(0)


def test_apply_and_permute_stats_are_true_permutations():
    c = np.arange(2 * 3 * 4).reshape(2, 3, 4)
    perms = np.array([[2, 0, 1], [1, 0, 2]])
    out = align.apply(c, perms)
    assert np.array_equal(out[0], c[0][[2, 0, 1]]) and np.array_equal(out[1], c[1][[1, 0, 2]])
    assert np.array_equal(align.apply(c, [2, 0, 1])[1], c[1][[2, 0, 1]])
    with pytest.raises(ValueError, match="not a permutation"):
        align.apply(c, [[0, 0, 1], [0, 1, 2]])
    names = ["Sample", "size_a0", "size_a1", "size_a2", "w_areal_f", "areal_a0_f_x", "areal_a1_f_x", "areal_a2_f_x",
             "post_a0", "post_a1", "post_a2", "prior", "cluster_size_prior"]
    rows = np.array([[0, 10, 11, 12, .5, 20, 21, 22, 30, 31, 32, 7, 8],
                     [1, 40, 41, 42, .6, 50, 51, 52, 60, 61, 62, 7, 8]], dtype=np.float64)
    same, moved = align.permute_stats(names, rows, perms)
    assert same == names
    assert moved[0].tolist() == [0, 12, 10, 11, .5, 22, 20, 21, 32, 30, 31, 7, 8]
    assert moved[1].tolist() == [1, 41, 40, 42, .6, 51, 50, 52, 61, 60, 62, 7, 8]
    assert rows[0, 1] == 10                                                 # the input is not written
    with pytest.raises(ValueError, match="do not cover the labels"):
        align.permute_stats(names[:3] + names[4:], np.delete(rows, 3, axis=1), perms)


def test_cluster_files_round_trip(tmp_path):
    c = (np.random.default_rng(5).random((6, 3, 37)) < 0.4).astype(np.uint8)
    path = tmp_path / "clusters_K3_0.txt"
    align.write_clusters(path, c)
    lines = path.read_text().splitlines()
    assert len(lines) == 6 and [len(s) for s in lines[0].split("\t")] == [37, 37, 37]
    assert np.array_equal(align.read_clusters(path), c)
