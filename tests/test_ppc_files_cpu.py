"""CPU checks of the posterior predictive check's command line and tables (sbayes_amd/ppc.py) on the recorded reference runs of
tests/golden/diag_runs.npz: the files are read through the posterior predictive's readers, the device call is replaced by the
oracle (tests/_ppc_oracle.py), and the tables and the printed lines say what the result holds."""
import numpy as np
import pytest

from sbayes_amd import ppc, predict
from tests import _ppc_cases as cases
from tests import _ppc_oracle as orc
from tests import _predict_cases as recorded


def _result(r, burn=0):
    case, got = cases.recorded(r), cases.recorded_oracle(r)
    return ppc.PpcResult(codes=case["codes"], dev_feature=got["dev_feature"][burn:], dev_object=got["dev_object"][burn:],
                         count_rep=got["count_rep"][burn:], count_obs=ppc.count_observed(case["codes"], 5), n_samples=60 - burn,
                         n_skipped=got["n_skipped"], y_rep=got["y_rep"][burn:])


def test_the_module_reuses_the_readers_of_the_posterior_predictive():
    for name in ("_check_shape", "group_index", "codes_of", "read_data", "read_parameters", "read_cluster_samples", "_check_burnin"):
        assert not hasattr(ppc, name) or getattr(ppc, name) is getattr(predict, name)
    assert ppc.NA is predict.NA


@pytest.mark.parametrize("r", [0, 1])
def test_the_tables_of_the_recorded_runs(r, tmp_path):
    res, d = _result(r), recorded.data()
    assert res.p_feature.shape == (36,) and res.p_object.shape == (100,) and res.p_count.shape == (36, 5) and 0 <= res.p_total <= 1
    assert np.array_equal(res.p_feature, orc.p_value(res.dev_feature[:, 1], res.dev_feature[:, 0]))
    assert res.n_cells_feature.sum() == res.n_cells_object.sum() == 3600 - 92
    assert np.array_equal(res.count_obs.sum(axis=1), res.n_cells_feature) and (res.count_rep.sum(axis=2) == res.n_cells_feature).all()
    # the replicate has the data's missingness, and the counts are the replicate's
    assert np.array_equal(res.y_rep == ppc.NA, np.broadcast_to(res.codes == ppc.NA, res.y_rep.shape))
    assert np.array_equal(res.count_rep[7], ppc.count_observed(res.y_rep[7], 5))
    # inapplicable states are never drawn
    assert not res.count_rep[:, ~d["states_per_feature"]].any()
    header, rows = res.table("feature", d["feature_names"])
    assert header == ["feature", "n_cells", "deviance_observed", "deviance_replicated", "p", "flag"] and len(rows) == 36
    assert [row[0] for row in rows] == d["feature_names"] and [row[4] for row in rows] == res.p_feature.tolist()
    assert all(row[5] == ("p < 0.05" if row[4] < 0.05 else "") for row in rows)
    worst = res.worst("object", k=5)
    assert len(worst) == 5 and [row[4] for row in worst] == sorted(res.p_object.tolist())[:5]
    with pytest.raises(ValueError, match="35 names for 36 features"):
        res.table("feature", d["feature_names"][:-1])
    res.write_table(tmp_path / "objects.tsv", "object")
    lines = (tmp_path / "objects.tsv").read_text().splitlines()
    assert lines[0].split("\t") == ["object", "n_cells", "deviance_observed", "deviance_replicated", "p", "flag"] and len(lines) == 101
    first = lines[1].split("\t")
    assert first[0] == "0" and int(first[1]) == int(res.n_cells_object[0]) and float(first[4]) == pytest.approx(res.p_object[0], rel=1e-9)


def test_the_command_line_reads_the_run_and_prints_the_worst(tmp_path, monkeypatch, capsys):
    pytest.importorskip("pandas")
    d, s = recorded.data(), recorded.run(1)
    # the run's files, as the reference writes them: the features with their family column, the states top down, stats, clusters
    families = ["" if g == ppc.NA else d["confounders"]["family"][g] for g in d["groups"][1]]
    with open(tmp_path / "features.csv", "w") as f:
        f.write("id,name,family,x,y," + ",".join(d["feature_names"]) + "\n")
        for n in range(100):
            cells = ["" if c == ppc.NA else d["state_names"][k][c] for k, c in enumerate(d["codes"][n])]
            f.write(f"o{n},O{n},{families[n]},{n},{n}," + ",".join(cells) + "\n")
    depth = max(len(names) for names in d["state_names"])
    with open(tmp_path / "feature_states.csv", "w") as f:
        f.write(",".join(d["feature_names"]) + "\n")
        for i in range(depth):
            f.write(",".join(names[i] if i < len(names) else "" for names in d["state_names"]) + "\n")
    with open(tmp_path / "stats_K3_0.txt", "w") as f:
        f.write("\t".join(s["names"]) + "\n")
        for row in s["rows"]:
            f.write("\t".join("%.8g" % v for v in row) + "\n")
    with open(tmp_path / "clusters_K3_0.txt", "w") as f:
        for sample in s["clusters"]:
            f.write("\t".join("".join(str(b) for b in row) for row in sample) + "\n")
    seen = {}

    def stub(codes, groups, clusters, weights, tables, burnin=0.1, seed=0, n_groups=None, replicates=False, uniforms=None, device=None):
        seen.update(codes=codes, groups=groups, clusters=clusters, weights=weights, tables=tables, burnin=burnin, seed=seed, n_groups=n_groups,
                    device=device)
        return _result(1, burn=predict._check_burnin(burnin, clusters.shape[0]))
    monkeypatch.setattr(ppc, "posterior_predictive_check", stub)
    out_f, out_o = tmp_path / "f.tsv", tmp_path / "o.tsv"
    argv = [str(tmp_path / n) for n in ("features.csv", "feature_states.csv", "stats_K3_0.txt", "clusters_K3_0.txt")]
    assert ppc.main(argv + ["--confounders", "universal", "family", "--seed", str(cases.SEED), "--out-features", str(out_f), "--out-objects",
                            str(out_o), "--device", "0"]) == 0
    case = cases.recorded(1)
    assert np.array_equal(seen["codes"], case["codes"]) and np.array_equal(seen["groups"], case["groups"]) and seen["n_groups"] == [1, 6]
    assert np.array_equal(seen["clusters"], case["clusters"]) and np.array_equal(seen["weights"], case["weights"])
    assert np.array_equal(seen["tables"], case["tables"]) and (seen["burnin"], seen["seed"], seen["device"]) == (0.1, cases.SEED, 0)
    res = _result(1, burn=6)
    lines = capsys.readouterr().out.splitlines()
    assert lines[0] == f"54 samples, p_total {res.p_total:.4f} (conservative: given the logged effect draws), 0 cells skipped"
    assert lines[1] == "the five features with the smallest p:" and lines[7] == "the five objects with the smallest p:" and len(lines) == 13
    assert [line.split("\t")[0].strip() for line in lines[2:7]] == [row[0] for row in res.worst("feature", d["feature_names"])]
    assert [line.split("\t")[0].strip() for line in lines[8:13]] == [row[0] for row in res.worst("object")]
    assert out_f.read_text().splitlines()[1].split("\t")[0] == "F1" and len(out_o.read_text().splitlines()) == 101
    # the samples and the rows must agree in number
    with open(tmp_path / "clusters_short.txt", "w") as f:
        f.write("\n".join((tmp_path / "clusters_K3_0.txt").read_text().splitlines()[:-1]) + "\n")
    with pytest.raises(SystemExit, match="60 stats rows, 59 cluster samples"):
        ppc.main(argv[:3] + [str(tmp_path / "clusters_short.txt"), "--confounders", "universal", "family"])
