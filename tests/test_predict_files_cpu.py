"""CPU checks of the posterior predictive's file readers (sbayes_amd/predict.py) on the two recorded reference runs of
tests/golden/diag_runs.npz with the data of tests/golden/south_america.npz: the logger's header rule reproduces the file's
names, every row passes the validation, and the reference's output alone gives a stable answer."""
import numpy as np
import pytest

from sbayes_amd import predict
from tests import _predict_cases as cases
from tests import _predict_oracle as orc


def test_the_fixture_has_the_stated_shape():
    d, s = cases.data(), cases.run(0)
    assert len(s["names"]) == 970 and s["rows"].shape == (60, 970)
    assert d["codes"].shape == (100, 36) and d["states_per_feature"].shape == (36, 5) and int(d["states_per_feature"].sum()) == 85
    assert s["clusters"].shape == (60, 3, 100) and s["weights"].shape == (60, 36, 3) and s["tables"].shape == (60, 10, 36, 5)
    assert int((d["codes"] == predict.NA).sum()) == 92 and int((d["groups"][1] == predict.NA).sum()) == 44 and not (d["groups"][0] == predict.NA).any()
    assert d["n_groups"] == [1, 6]


def test_the_header_rule_reproduces_the_files_names_exactly():
    d, s = cases.data(), cases.run(0)
    want = predict.expected_header(d["feature_names"], d["state_names"], d["confounders"], cases.K)
    at = s["names"].index("w_areal_F1")
    assert at == 7 and len(want) == 36 * 3 + 10 * 85 and s["names"][at:at + len(want)] == want
    assert s["names"][:at] == ["Sample", "posterior", "likelihood", "prior", "size_a0", "size_a1", "size_a2"]
    assert s["names"][at + len(want):] == ["cluster_size_prior", "geo_prior", "source_prior", "weights_prior", "sample_id"]


@pytest.mark.parametrize("r", [0, 1])
def test_every_row_of_the_recorded_runs_passes_the_validation(r):
    d, s = cases.data(), cases.run(r)
    assert orc.first_offender(s["clusters"], s["weights"], s["tables"]) is None
    # inapplicable states are zero, the recorded deviation of a row sum from 1 is that of %.8g prints of float32 values
    assert not s["tables"][:, :, ~d["states_per_feature"]].any()
    assert np.abs(s["tables"].sum(axis=3) - 1).max() <= 2e-7 and np.abs(s["weights"].sum(axis=2) - 1).max() <= 2e-7
    sizes = s["rows"][:, [s["names"].index(f"size_a{k}") for k in range(cases.K)]]
    assert np.array_equal(sizes, s["clusters"].sum(axis=2))


def test_a_header_with_two_columns_swapped_is_refused():
    d, s = cases.data(), cases.run(0)
    names = list(s["names"])
    i, j = names.index("areal_a1_F7_N"), names.index("areal_a1_F7_Y")
    names[i], names[j] = names[j], names[i]
    with pytest.raises(ValueError, match=rf"column {i} of the stats file is 'areal_a1_F7_Y', the logger's rule gives 'areal_a1_F7_N'"):
        predict.parameters_from_columns(names, s["rows"], d["feature_names"], d["state_names"], d["confounders"])
    with pytest.raises(ValueError, match="the stats file ends after column 'family_Tupian_F36_N'"):
        predict.parameters_from_columns(s["names"][:-6], s["rows"][:, :-6], d["feature_names"], d["state_names"], d["confounders"])
    with pytest.raises(ValueError, match="no size_a"):
        predict.parameters_from_columns([n for n in s["names"] if not n.startswith("size_a")], s["rows"], d["feature_names"], d["state_names"],
                                        d["confounders"])


def test_the_readers_take_the_reference_files(tmp_path):
    d, s = cases.data(), cases.run(1)
    stats, clusters = tmp_path / "stats_K3_0.txt", tmp_path / "clusters_K3_0.txt"
    with open(stats, "w") as f:
        f.write("\t".join(s["names"]) + "\n")
        for row in s["rows"][:4]:
            f.write("\t".join("%.8g" % v for v in row) + "\n")
    with open(clusters, "w") as f:
        for sample in s["clusters"][:4]:
            f.write("\t".join("".join(str(b) for b in row) for row in sample) + "\n")
    weights, tables = predict.read_parameters(stats, d["feature_names"], d["state_names"], d["confounders"])
    assert np.array_equal(weights, s["weights"][:4]) and np.array_equal(tables, s["tables"][:4])
    assert np.array_equal(predict.read_cluster_samples(clusters), s["clusters"][:4])


def test_read_data_numbers_the_states_in_the_feature_states_files_order(tmp_path):
    pytest.importorskip("pandas")
    (tmp_path / "features.csv").write_text("id,name,family,x,y,F1,F2\na,A,Tupian,0,0,Y,B\nb,B,,1,1,N,\nc,C,Arawak,2,2,,A\n")
    (tmp_path / "feature_states.csv").write_text("F1,F2\nN,B\nY,A\n,C\n")
    d = predict.read_data(tmp_path / "features.csv", tmp_path / "feature_states.csv", ["universal", "family"])
    assert d["feature_names"] == ["F1", "F2"] and d["state_names"] == [["N", "Y"], ["B", "A", "C"]]
    assert d["codes"].tolist() == [[1, 0], [0, 255], [255, 1]]
    assert d["confounders"] == {"universal": ["<ALL>"], "family": ["Arawak", "Tupian"]} and d["groups"].tolist() == [[0, 0, 0], [1, 255, 0]]


def test_the_reference_output_alone_gives_a_stable_answer():
    """What the oracle makes of the recorded runs: no observed cell of probability 0, and an arg-max that rounding cannot move."""
    for r in (0, 1):
        sums, lik = orc.run(**cases.case(r))
        observed = (cases.data()["codes"] != predict.NA).ravel()
        assert sums.n_zero == 0 and sums.n_samples == 60 and lik[:, observed].min() >= 6e-3 and (lik[:, ~observed] == 1).all()
        probs = np.sort(sums.pred[cases.data()["codes"] == predict.NA] / 60, axis=1)
        assert (probs[:, -1] - probs[:, -2]).min() >= 5e-4
        assert np.abs(sums.pred.sum(axis=2) - 60).max() < 1e-4 and np.abs(sums.resp.sum(axis=2)[cases.data()["codes"] != predict.NA] - 60).max() < 1e-9
