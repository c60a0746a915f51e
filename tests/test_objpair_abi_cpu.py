"""CPU checks of the object-pair check's boundary (include/sbe_objpair.h, sbayes_amd/objpair.py): the symbols are exported and bound
by the module's own prototype table, the limits agree, and bad arguments are refused before the device is touched."""
import ctypes as ct
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from sbayes_amd import objpair, predict, spatial
from tests import _abi_header as abi
from tests import _objpair_oracle as orc

REPO = Path(__file__).resolve().parent.parent
HEADER = (REPO / "include" / "sbe_objpair.h").read_text()


def test_every_symbol_of_the_header_is_exported_and_bound():
    abi.check_symbols(objpair, HEADER, 13)


def test_the_unit_is_in_both_build_lists():
    assert "sbe_objpair" in (REPO / "build.sh").read_text().split('units="')[1].split('"')[0].split()
    import __graft_entry__ as entry
    assert entry.CSRC / "sbe_objpair.hip" in entry.SOURCES


def test_limits_agree_with_the_header():
    assert abi.macro(HEADER, "SBE_OBJPAIR_NA") == str(objpair.NA) == str(orc.NA) == "255"
    # the shape limits are the spatial check's
    assert int(abi.macro(HEADER, "SBE_OBJPAIR_MAX_OBJECTS")) == objpair.MAX_OBJECTS == orc.MAX_OBJECTS == spatial.MAX_OBJECTS == 4096
    assert int(abi.macro(HEADER, "SBE_OBJPAIR_MAX_FEATURES")) == objpair.MAX_FEATURES == orc.MAX_FEATURES == spatial.MAX_FEATURES == 4096
    # the state limit is the one of the replicates' source
    assert int(abi.macro(HEADER, "SBE_OBJPAIR_MAX_STATES")) == objpair.MAX_STATES == predict.MAX_STATES == orc.MAX_STATES == 32
    assert int(abi.macro(HEADER, "SBE_OBJPAIR_ROUND")) == objpair.ROUND == orc.ROUND == 256 and objpair.TILE == orc.TILE == 32
    assert abi.macro(HEADER, "SBE_OBJPAIR_MAX_STAGE_BYTES") == "(256ll << 20)"
    assert objpair.MAX_STAGE_BYTES == predict.MAX_STAGE_BYTES == orc.MAX_STAGE_BYTES == 256 << 20
    # the exactness argument of the header: the longest contraction axis and the largest count stay far below 2^24
    assert objpair.MAX_STATES * objpair.MAX_FEATURES == 131072 < 2 ** 24 and objpair.MAX_FEATURES ** 2 == 2 ** 24


def test_max_replicates_agrees_at_the_limits_and_just_past_them():
    lib = objpair.load()
    for n, f in [(1, 1), (1, 4096), (2, 1), (100, 36), (1000, 200), (4096, 1), (4095, 4096), (4096, 4096)]:
        assert lib.sbe_objpair_max_replicates(n, f) == objpair.max_replicates(n, f) == orc.max_replicates(n, f) == 2 ** 31 - 1, (n, f)
    for n, f in [(0, 1), (1, 0), (4097, 1), (1, 4097), (4097, 4097), (-1, 5)]:
        assert lib.sbe_objpair_max_replicates(n, f) == objpair.max_replicates(n, f) == orc.max_replicates(n, f) == 0, (n, f)
    # the derivation: after 2^31 - 1 replicates of the largest count the sum of squares is far from the int64's end
    assert (2 ** 31 - 1) * 4096 ** 2 < 2 ** 63 - 1


def test_replicate_bytes_agree():
    lib = objpair.load()
    for n, f, e, rep in [(1, 1, 1, 0), (1, 1, 32, 1), (31, 17, 255, 0), (32, 17, 256, 1), (33, 17, 257, 1), (97, 17, 513, 0), (100, 36, 180, 0),
                         (1000, 200, 2000, 0), (1000, 200, 2000, 1), (33, 4096, 131072, 0), (4096, 4096, 4096, 1), (4096, 4096, 131072, 1)]:
        assert lib.sbe_objpair_replicate_bytes(n, f, e, rep) == objpair.replicate_bytes(n, f, e, rep) == orc.replicate_bytes(n, f, e, rep) > 0, (n, f, e, rep)
    assert objpair.replicate_bytes(33, 17, 257, True) == 33 * 17 + 64 * 256 + 4 * 33 * 33
    assert objpair.replicate_bytes(1000, 200, 2000) == 200000 + (1 << 20)
    for n, f, e in [(0, 1, 1), (4097, 1, 1), (1, 4097, 4097), (5, 5, 4), (5, 5, 161), (5, 0, 0), (-1, 5, 5)]:
        assert lib.sbe_objpair_replicate_bytes(n, f, e, 0) == objpair.replicate_bytes(n, f, e) == orc.replicate_bytes(n, f, e) == 0, (n, f, e)
    # one replicate of the largest shape is more than a call's limit by itself: a call always takes one
    assert objpair.replicate_bytes(4096, 4096, 131072) > objpair.MAX_STAGE_BYTES


def test_every_array_handed_to_the_library_is_bound_to_a_name():
    abi.check_ptr_arguments(objpair)


def test_c_abi_validates_before_the_device():
    assert sorted(abi.check_null_handles(objpair)) == sorted(set(objpair.PROTOTYPES) - {"sbe_objpair_abi_version", "sbe_objpair_last_error",
                                                                                        "sbe_objpair_max_replicates", "sbe_objpair_replicate_bytes"})


def test_handles_are_not_picklable():
    abi.check_not_picklable(objpair.ObjPairHandle)


def test_a_handle_checks_its_own_arguments_before_the_library():
    h = object.__new__(objpair.ObjPairHandle)
    h._h = ct.c_void_p()

    def refuse(*a, **k):
        raise AssertionError("the device was touched")
    h._lib = SimpleNamespace(**{name: refuse for name in objpair.PROTOTYPES})
    h.shape = None
    for call in (h.reset, h.result, lambda: h.add(np.zeros((1, 2, 2), dtype=np.uint8)), h.max_replicates):
        with pytest.raises(ValueError, match="no data yet"):
            call()
    with pytest.raises(TypeError, match="uint8 codes"):
        h.set_data(np.zeros((3, 2)), None)
    with pytest.raises(ValueError, match=r"n_states must lie in \[1, 32\]"):
        h.set_data(np.zeros((3, 2), dtype=np.uint8), [2, 33])
    with pytest.raises(ValueError, match=r"features\[1, 0\] = 2 is neither below n_states\[0\] = 2 nor 255"):
        h.set_data(np.array([[0, 0], [2, 1], [0, 0]], dtype=np.uint8), [2, 2])
    with pytest.raises(ValueError, match="4097 objects"):
        h.set_data(np.zeros((4097, 1), dtype=np.uint8), [2])
    with pytest.raises(ValueError, match="4097 features"):
        h.set_data(np.zeros((1, 4097), dtype=np.uint8), None)
    h.shape, h.n_states = (5, 3, 9), np.array([2, 4, 3], dtype=np.int32)
    with pytest.raises(TypeError, match="uint8 codes"):
        h.add(np.zeros((1, 5, 3)))
    with pytest.raises(ValueError, match=r"replicates must be \[n, 5, 3\], got shape \(1, 5, 4\)"):
        h.add(np.zeros((1, 5, 4), dtype=np.uint8))
    assert h.max_replicates() == (256 << 20) // (15 + 32 * 128) and h.max_replicates(True) == (256 << 20) // (15 + 32 * 128 + 100)
    h.shape = (4096, 4096, 131072)
    assert h.max_replicates() == 1


def test_bad_input_of_the_check_is_refused_before_the_device(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(objpair.ppc.PpcHandle, "__init__", refuse)
    monkeypatch.setattr(objpair.ObjPairHandle, "__init__", refuse)
    codes, groups = np.zeros((4, 2), dtype=np.uint8), np.zeros((0, 4), dtype=np.uint8)
    with pytest.raises(ValueError, match=r"clusters must be \[T, K, N\] and tables \[T, R, F, S\]"):
        objpair.object_pair_check(codes, groups, np.zeros((3, 4)), np.zeros((3, 2, 1)), np.zeros((3, 1, 2, 2)), n_groups=[])
    with pytest.raises(ValueError, match=r"must lie in \[0, 1\)"):
        objpair.object_pair_check(codes, groups, np.zeros((3, 1, 4)), np.zeros((3, 2, 1)), np.zeros((3, 1, 2, 2)), n_groups=[], burnin=1.0)
    with pytest.raises(ValueError, match="2 rows of uniforms for 3 samples"):
        objpair.object_pair_check(codes, groups, np.zeros((3, 1, 4)), np.zeros((3, 2, 1)), np.zeros((3, 1, 2, 2)), n_groups=[], uniforms=np.zeros((2, 8)))
    with pytest.raises(AssertionError, match="the device was touched"):      # (good arguments do reach the handles)
        objpair.object_pair_check(codes, groups, np.zeros((3, 1, 4)), np.zeros((3, 2, 1)), np.zeros((3, 1, 2, 2)), n_groups=[])


def test_the_result_of_the_hand_case():
    """The host side of a result, on the checker's arrays of the hand case (no device)."""
    from tests import _objpair_cases as cases
    x, ns, y = cases.hand()
    want = orc.check(x, ns, y)
    res = objpair.ObjPairResult(want["agree_obs"], want["comparable_obs"], want["n_greater"], want["n_equal"], want["n_less"], want["sum"], want["sumsq"], 3)
    p = res.p_value()
    assert np.isnan(np.diag(p)).all() and p[0, 1] == 1 / 3 and p[0, 2] == 2 / 3 and p[1, 2] == 2.5 / 3 and np.array_equal(p[np.triu_indices(3, 1)], p.T[np.triu_indices(3, 1)])
    assert res.mean()[0, 2] == 7 / 3 and res.excess()[0, 2] == 2 - 7 / 3 and abs(res.sd()[0, 2] - np.sqrt(3 * 17 - 49) / 3) < 1e-15
    assert abs(res.z()[1, 2] - (1 - 5 / 3) / (np.sqrt(3 * 9 - 25) / 3)) < 1e-12 and np.isnan(res.z()[0, 0])
    assert res.flagged(0.5) == [(1 / 3, 0, 1)] and res.flagged(0.9) == [(1 / 3, 0, 1), (2 / 3, 0, 2), (2.5 / 3, 1, 2)] and res.flagged(0.1) == []
    worst = res.worst(2, ["a", "b", "c"])
    assert [r[:4] for r in worst] == [["a", "b", 2, 2], ["a", "c", 2, 3]] and worst[0][4] == 1.0 and len(res.worst(10)) == 3 and res.worst(0) == []
    header, rows = res.object_table(["a", "b", "c"], p_threshold=0.7)
    assert header == ["object", "n_flagged", "max_excess", "max_excess_partner", "sum_excess"]
    assert [r[:2] for r in rows] == [["a", 2], ["b", 1], ["c", 1]] and rows[0][3] == "b" and abs(rows[0][4] - (2 - 5 / 3 + 2 - 7 / 3)) < 1e-12
    assert res.pair_table(top=1)[1][0][:2] == ["O1", "O2"] and len(res.pair_table(p_threshold=0.7)[1]) == 2
    with pytest.raises(ValueError, match="2 names for 3 objects"):
        res.worst(1, ["a", "b"])


def test_write_tables(tmp_path):
    from tests import _objpair_cases as cases
    x, ns, y = cases.hand()
    want = orc.check(x, ns, y)
    res = objpair.ObjPairResult(want["agree_obs"], want["comparable_obs"], want["n_greater"], want["n_equal"], want["n_less"], want["sum"], want["sumsq"], 3)
    res.write_tables(tmp_path / "pairs.tsv", tmp_path / "objects.tsv", ["a", "b", "c"], p_threshold=0.5)
    pairs = (tmp_path / "pairs.tsv").read_text().splitlines()
    assert pairs[0].split("\t") == objpair.ObjPairResult.HEADER and len(pairs) == 2 and pairs[1].split("\t")[:4] == ["a", "b", "2", "2"]
    assert len((tmp_path / "objects.tsv").read_text().splitlines()) == 4
    res.write_tables(tmp_path / "top.tsv", None, None, top=2)
    assert len((tmp_path / "top.tsv").read_text().splitlines()) == 3
