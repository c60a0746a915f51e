"""CPU checks of the feature-screening boundary (include/sbe_assoc.h, sbayes_amd/assoc.py): the symbols are exported and
bound by the module's own prototype table, and bad arguments are refused before the device is touched."""
from pathlib import Path

import numpy as np
import pytest

from sbayes_amd import assoc
from tests import _abi_header as abi

REPO = Path(__file__).resolve().parent.parent
HEADER = (REPO / "include" / "sbe_assoc.h").read_text()


def test_every_symbol_of_the_header_is_exported_and_bound():
    abi.check_symbols(assoc, HEADER, 9)


def test_limits_agree_with_the_header():
    assert abi.macro(HEADER, "SBE_ASSOC_NA") == str(assoc.NA)
    assert abi.macro(HEADER, "SBE_ASSOC_MAX_OBJECTS") == "(1 << 24)" and assoc.MAX_OBJECTS == 1 << 24
    assert abi.macro(HEADER, "SBE_ASSOC_MAX_STATES") == str(assoc.MAX_STATES)
    assert abi.macro(HEADER, "SBE_ASSOC_MAX_FEATURES") == str(assoc.MAX_FEATURES)
    assert abi.macro(HEADER, "SBE_ASSOC_MAX_CODES") == "((int64_t)1 << 31)" and assoc.MAX_CODES == 1 << 31


def test_every_array_handed_to_the_library_is_bound_to_a_name():
    abi.check_ptr_arguments(assoc)


@pytest.fixture
def no_handle(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(assoc, "AssocHandle", refuse)
    monkeypatch.setattr(assoc, "_HANDLES", {})


@pytest.mark.parametrize("features,n_states,err,match", [
    (np.zeros((4, 3), dtype=np.int64), None, TypeError, "uint8"),
    (np.zeros(4, dtype=np.uint8), None, ValueError, "n_objects, n_features"),
    (np.zeros((0, 3), dtype=np.uint8), None, ValueError, "both positive"),
    (np.zeros((4, 3), dtype=np.uint8), [2, 2], ValueError, "n_states must be 3 integers"),
    (np.zeros((4, 3), dtype=np.uint8), [2, 33, 2], ValueError, r"\[1, 32\]"),
    (np.full((4, 3), 40, dtype=np.uint8), None, ValueError, r"\[1, 32\]"),
    (np.array([[0, 2], [1, 255]], dtype=np.uint8), [2, 2], ValueError, r"features\[0, 1\] = 2 is neither below n_states\[1\] = 2"),
    (np.zeros((4, 3, 33), dtype=bool), None, ValueError, "at most 32"),
    (np.ones((4, 3, 2), dtype=bool), None, ValueError, "more than one state"),
    (np.zeros((2, assoc.MAX_FEATURES + 1), dtype=np.uint8), None, ValueError, "4096 features"),
])
def test_bad_input_is_refused_before_the_device(no_handle, features, n_states, err, match):
    with pytest.raises(err, match=match):
        assoc.feature_association(features, n_states)


def test_too_many_objects_are_refused_with_the_limit(no_handle):
    x = np.broadcast_to(np.zeros((1, 1), dtype=np.uint8), (assoc.MAX_OBJECTS + 1, 1))      # (no memory behind it)
    with pytest.raises(ValueError, match=r"2\^24"):
        assoc.feature_association(x)


def test_one_hot_features_become_codes():
    onehot = np.zeros((3, 2, 4), dtype=bool)
    onehot[0, 0, 2] = onehot[1, 0, 0] = onehot[2, 1, 3] = True
    assert np.array_equal(assoc.state_codes(onehot), np.array([[2, 255], [0, 255], [255, 3]], dtype=np.uint8))
    x, ns = assoc._check_inputs(onehot, None)
    assert x.dtype == np.uint8 and np.array_equal(ns, [4, 4])
    x, ns = assoc._check_inputs(np.array([[0, 255], [3, 255]], dtype=np.uint8), None)
    assert np.array_equal(ns, [4, 1])                      # one more than the largest code; a feature never observed: 1


def test_c_abi_validates_before_the_device():
    assert sorted(abi.check_null_handles(assoc)) == sorted(set(assoc.PROTOTYPES) - {"sbe_assoc_abi_version", "sbe_assoc_last_error"})


def test_frame_codes_number_states_in_sorted_order():
    pd = pytest.importorskip("pandas")
    frame = pd.DataFrame({"F1": ["Y", "N", None, "Y"], "F2": ["B", "A", "C", None], "F3": [None] * 4}, dtype=object)
    codes, n_states, names, states = assoc.frame_codes(frame)
    assert names == ["F1", "F2", "F3"] and states == [["N", "Y"], ["A", "B", "C"], []]
    assert np.array_equal(n_states, [2, 3, 1])
    assert np.array_equal(codes, np.array([[1, 1, 255], [0, 0, 255], [255, 2, 255], [1, 255, 255]], dtype=np.uint8))


def test_csv_needs_the_metadata_columns(tmp_path):
    pytest.importorskip("pandas")
    path = tmp_path / "features.csv"
    path.write_text("id,name,family,x,y,F1,F2\na,A,,0,0, Y ,\nb,B,fam,1,1,N,Q\n")
    frame = assoc.read_features_csv(path)
    assert list(frame.columns) == ["F1", "F2"]
    assert frame["F1"].tolist() == ["Y", "N"] and frame["F2"].isna().tolist() == [True, False]
    path.write_text("id,name,x,y,F1\na,A,0,0,Y\n")
    with pytest.raises(ValueError, match="Required column 'family' missing"):
        assoc.read_features_csv(path)


def test_handles_are_not_picklable_and_results_sort_like_the_tool():
    abi.check_not_picklable(assoc.AssocHandle)
    p = np.array([[np.nan, 1e-9, 0.5], [1e-9, np.nan, 1e-12], [0.5, 1e-12, np.nan]])
    valid = ~np.isnan(p)
    res = assoc.AssociationResult(np.zeros((3, 3)), p, np.ones((3, 3), np.int32), np.ones((3, 3), np.int32), valid,
                                  np.array([2, 2, 2], np.int32))
    assert res.correlated() == [(1e-12, 1, 2), (1e-9, 0, 1)]
    assert res.correlated(1e-10) == [(1e-12, 1, 2)]
