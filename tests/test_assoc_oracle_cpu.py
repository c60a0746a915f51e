"""tests/_assoc_oracle.py (the NumPy restatement of the feature screening's contract) against what pandas and SciPy
themselves returned, recorded in tests/golden/assoc.npz; its incomplete-gamma routine against scipy.special.chdtrc; the
fixture's own make-up; and the fixture regenerates bit for bit from the committed script."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests import _assoc_oracle as ao

REPO = Path(__file__).resolve().parent.parent
GOLDEN = REPO / "tests" / "golden"
CASES = ["south_america", "ragged", "binary", "duplicated", "edge_s32", "edge_one_object", "edge_ragged_n", "edge_two_features"]


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN / "assoc.npz", allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def _case(golden, name):
    return {k[len(name) + 1:]: v for k, v in golden.items() if k.startswith(name + "_")}


def test_fixture_holds_the_cases(golden):
    assert sorted({k.rsplit("_", 1)[0] for k in golden if k.endswith("_x")}) == sorted(CASES)
    assert (GOLDEN / "assoc.npz").stat().st_size < 240_000
    sa = _case(golden, "south_america")
    assert sa["x"].shape == (100, 36) and len(sa["pvalue"]) == 630 and not sa["skipped"].any()
    assert int((sa["dof"] == 1).sum()) == 435 and int((sa["pvalue"] < 1e-4).sum()) == 40
    assert 9.1e-12 < sa["pvalue"].min() < 9.3e-12
    rg = _case(golden, "ragged")
    assert rg["skipped"].any() and not rg["skipped"].all()                 # conditional features: skipped pairs occur
    assert rg["n_states"].min() == 2 and rg["n_states"].max() == 10 and 0.05 < np.mean(rg["x"] == ao.NA)
    bn = _case(golden, "binary")
    assert bn["x"].shape == (1000, 64) and np.all(bn["n_states"] == 2) and np.all(bn["dof"] == 1)
    du = _case(golden, "duplicated")
    assert du["x"].shape[0] == 5000 and np.all(du["n_states"] == 10) and du["pvalue"].min() == 0.0
    assert _case(golden, "edge_s32")["n_states"].max() == 32
    assert _case(golden, "edge_one_object")["x"].shape[0] == 1 and _case(golden, "edge_one_object")["skipped"].all()
    er = _case(golden, "edge_ragged_n")
    assert er["x"].shape[0] % 64 != 0 and np.any(np.all(er["x"] == ao.NA, axis=0))
    assert _case(golden, "edge_two_features")["x"].shape[1] == 2


def test_only_the_duplicated_feature_underflows(golden):
    """P-values below the smallest normal double are compared as "both below it": only case (d) has such pairs."""
    for name in CASES:
        c = _case(golden, name)
        tiny = c["pvalue"][~c["skipped"]] < ao.DBL_MIN
        assert bool(tiny.any()) == (name == "duplicated"), name


@pytest.mark.parametrize("name", CASES)
def test_oracle_matches_pandas_and_scipy(golden, name):
    c = _case(golden, name)
    r = ao.feature_association(c["x"], c["n_states"])
    keep = ~c["skipped"]
    assert np.array_equal(ao.upper(r["valid"]), keep)
    assert np.array_equal(ao.upper(r["dof"]), c["dof"])
    assert np.array_equal(ao.upper(r["n"]), c["n"])
    for key in ("statistic", "dof", "n", "valid"):
        assert np.array_equal(r[key], r[key].T), key
    assert not r["valid"].diagonal().any() and np.all(np.isnan(r["pvalue"][~r["valid"]])) and np.all(r["statistic"][~r["valid"]] == 0)
    stat, want = ao.upper(r["statistic"])[keep], c["statistic"][keep]
    bound = ao.statistic_bound(ao.upper(r["R"]), ao.upper(r["C"]))[keep]
    rel = np.abs(stat - want) / np.maximum(want, ao.DBL_MIN)
    print(f"{name}: statistic, largest relative difference {rel.max() if rel.size else 0:.3g}")
    assert np.all(np.abs(stat - want) <= bound * want)
    pv, want_p = ao.upper(r["pvalue"])[keep], c["pvalue"][keep]
    tiny = want_p < ao.DBL_MIN
    assert np.all(pv[tiny] < ao.DBL_MIN)
    pb = ao.pvalue_bound_end_to_end(c["statistic"], ao.upper(r["R"]), ao.upper(r["C"]))[keep]
    assert np.all(np.abs(pv - want_p)[~tiny] <= (pb * want_p)[~tiny])


def test_single_table_form_agrees_with_the_vectorized_one(golden):
    c = _case(golden, "ragged")
    r = ao.feature_association(c["x"], c["n_states"])
    for i, j in [(0, 1), (1, 3), (3, 10), (5, 6), (38, 39)]:
        valid, dof, n, stat, R, C = ao.table_statistic(r["tables"][i, j])
        assert (valid, dof, n, R, C) == (r["valid"][i, j], r["dof"][i, j], r["n"][i, j], r["R"][i, j], r["C"][i, j])
        assert stat == r["statistic"][i, j]                                # the same operations in the same order


def test_gamma_q_against_chdtrc_over_the_fixture(golden):
    """The measured figure DESIGN.md section 13 quotes and the GPU tests' bound is four times of."""
    special = pytest.importorskip("scipy.special")
    worst = 0.0
    for name in CASES:
        c = _case(golden, name)
        keep = ~c["skipped"]
        if not keep.any():
            continue
        dof, stat = c["dof"][keep], c["statistic"][keep]
        want = special.chdtrc(dof, stat)
        got = ao.chi2_sf(dof, stat)
        normal = want >= ao.DBL_MIN
        assert np.all(got[~normal] < ao.DBL_MIN)
        rel = float(np.max(np.abs(got - want)[normal] / want[normal]))
        print(f"{name}: gamma_q against chdtrc, largest relative error {rel:.3g} (dof up to {dof.max()})")
        worst = max(worst, rel)
    assert 0.5 * ao.GAMMA_Q_MEASURED < worst <= ao.GAMMA_Q_MEASURED        # the recorded figure is the measured one


def test_gamma_q_known_values():
    """Q(1, x) = exp(-x), Q(1/2, x) = erfc(sqrt(x)), Q(a, 0) = 1.  The exponent a log x - x - lgamma(a) is rounded at the
    size of x, so the relative error grows with x: (x + 16) 2^-52 bounds it with room for the series."""
    import math
    x = np.array([0.0, 0.3, 1.0, 2.5, 40.0, 700.0])
    tol = (x + 16.0) * 2.0 ** -52
    want = np.exp(-x)
    assert np.all(np.abs(ao.gamma_q(np.ones_like(x), x) - want) <= tol * want)
    want = np.array([math.erfc(math.sqrt(v)) for v in x])
    assert np.all(np.abs(ao.gamma_q(np.full_like(x, 0.5), x) - want) <= tol * want)
    assert ao.gamma_q(np.array([480.5]), np.array([1e5]))[0] == 0.0


@pytest.mark.skipif(not os.path.isfile("/root/reference/experiments/south_america/data/features.csv"),
                    reason="the reference's south_america features.csv is not present")
def test_fixture_regenerates_bit_for_bit(golden, tmp_path):
    pytest.importorskip("pandas")
    pytest.importorskip("scipy")
    env = dict(os.environ, SBAYES_AMD_GOLDEN_OUT=str(tmp_path), PYTHONHASHSEED="0")
    subprocess.run([sys.executable, str(GOLDEN / "make_golden_assoc.py")], check=True, env=env, cwd=str(REPO),
                   stdout=subprocess.DEVNULL, timeout=600)
    with np.load(tmp_path / "assoc.npz", allow_pickle=False) as z:
        assert sorted(z.files) == sorted(golden)
        for k in z.files:
            assert z[k].dtype == golden[k].dtype and z[k].shape == golden[k].shape, k
            assert z[k].tobytes() == golden[k].tobytes(), f"assoc.npz:{k} differs from the regenerated fixture"
