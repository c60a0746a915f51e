"""CPU checks of the per-cluster evidence unit's command line and tables (sbayes_amd/contribution.py) on the recorded reference
runs of tests/golden/diag_runs.npz: the files are read through the posterior predictive's readers, the device call is replaced by
the oracle (tests/_contrib_oracle.py), and the tables and the printed lines say what the result holds."""
import numpy as np
import pytest

from sbayes_amd import contribution, predict
from tests import _contrib_cases as cases
from tests import _contrib_oracle as orc
from tests import _predict_cases as recorded


def _result(r, burn=0):
    got = cases.recorded_oracle(r)
    return contribution.ContributionResult(affinity=got["affinity"][burn:], gain_feature=got["gain_feature"][burn:], member=got["member"][burn:],
                                           n_samples=60 - burn, n_skipped=got["n_skipped"])


def test_the_module_reuses_the_readers_of_the_posterior_predictive():
    for name in ("_check_shape", "group_index", "codes_of", "read_data", "read_parameters", "read_cluster_samples", "_check_burnin"):
        assert not hasattr(contribution, name) or getattr(contribution, name) is getattr(predict, name)
    assert contribution.NA is predict.NA
    for caveat in ("aligned first", "OPTIMISTIC"):
        assert caveat in contribution.__doc__


@pytest.mark.parametrize("r", [0, 1])
def test_the_tables_of_the_recorded_runs(r, tmp_path):
    res, d, got = _result(r), recorded.data(), cases.recorded_oracle(r)
    assert res.affinity.shape == (60, 3, 100) and res.gain_feature.shape == (60, 3, 36) and res.member.shape == (60, 3, 100)
    assert res.gain.shape == (60, 3) and res.n_skipped == 0 and np.isfinite(res.affinity).all()
    assert np.array_equal(res.member, cases.recorded(r)["clusters"] != 0)
    assert sorted(res.rank()) == [0, 1, 2] and res.rank() == orc.rank(got["gain_feature"])
    # a cluster's gain is its members' affinities added up the other way round (two orders of one sum of the same d values)
    by_object = np.where(res.member, res.affinity, 0.0).sum(axis=2)
    assert np.allclose(by_object, res.gain, rtol=1e-9, atol=1e-9)
    for k in range(3):
        header, rows = res.feature_table(k, d["feature_names"])
        assert header == ["feature", "gain_mean", "gain_sd", "share_positive"] and sorted(row[0] for row in rows) == sorted(d["feature_names"])
        assert [row[1] for row in rows] == sorted((row[1] for row in rows), reverse=True)
        assert res.top_features(k, 10, d["feature_names"]) == rows[:10]
    paths = res.write_tables(tmp_path, d["feature_names"])
    assert len(paths) == 5 and all(p.exists() for p in paths)
    lines = (tmp_path / "membership.tsv").read_text().splitlines()
    assert lines[0].split("\t") == ["cluster", "object", "member_share", "affinity_mean", "share_affinity_positive"] and len(lines) == 301
    first = lines[1].split("\t")
    assert first[:2] == ["0", "0"] and float(first[2]) == pytest.approx(res.member[:, 0, 0].mean()) and float(first[3]) == pytest.approx(res.affinity[:, 0, 0].mean(), rel=1e-9)
    lines = (tmp_path / "clusters.tsv").read_text().splitlines()
    assert [int(line.split("\t")[0]) for line in lines[1:]] == res.rank()


def _write_run(tmp_path, d, s):
    """The run's files, as the reference writes them: the features with their family column, the states top down, stats, clusters."""
    families = ["" if g == contribution.NA else d["confounders"]["family"][g] for g in d["groups"][1]]
    with open(tmp_path / "features.csv", "w") as f:
        f.write("id,name,family,x,y," + ",".join(d["feature_names"]) + "\n")
        for n in range(100):
            cells = ["" if c == contribution.NA else d["state_names"][k][c] for k, c in enumerate(d["codes"][n])]
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
    return [str(tmp_path / n) for n in ("features.csv", "feature_states.csv", "stats_K3_0.txt", "clusters_K3_0.txt")]


def test_the_command_line_reads_the_run_prints_the_clusters_and_writes_the_tables(tmp_path, monkeypatch, capsys):
    pytest.importorskip("pandas")
    d, s = recorded.data(), recorded.run(1)
    argv = _write_run(tmp_path, d, s)
    seen = {}

    def stub(codes, groups, clusters, weights, tables, burnin=0.1, n_groups=None, device=None):
        seen.update(codes=codes, groups=groups, clusters=clusters, weights=weights, tables=tables, burnin=burnin, n_groups=n_groups, device=device)
        return _result(1, burn=predict._check_burnin(burnin, clusters.shape[0]))
    monkeypatch.setattr(contribution, "cluster_contribution", stub)
    out = tmp_path / "tables"
    assert contribution.main(argv + ["--confounders", "universal", "family", "--out", str(out), "--device", "0"]) == 0
    case = cases.recorded(1)
    assert np.array_equal(seen["codes"], case["codes"]) and np.array_equal(seen["groups"], case["groups"]) and seen["n_groups"] == [1, 6]
    assert np.array_equal(seen["clusters"], case["clusters"]) and np.array_equal(seen["weights"], case["weights"])
    assert np.array_equal(seen["tables"], case["tables"]) and (seen["burnin"], seen["device"]) == (0.1, 0)
    res = _result(1, burn=6)
    lines = capsys.readouterr().out.splitlines()
    assert lines[0] == "54 samples, 3 clusters (labels as logged), 0 entries skipped" and len(lines) == 4
    assert [line.split("\t")[0].strip() for line in lines[1:]] == [f"a{k}" for k in res.rank()]
    top = res.top_features(res.rank()[0], 3, d["feature_names"])
    assert lines[1].split("\t")[3] == "top features: " + ", ".join(f"{row[0]} {row[1]:.3f}" for row in top)
    assert sorted(p.name for p in out.iterdir()) == ["clusters.tsv", "features_a0.tsv", "features_a1.tsv", "features_a2.tsv", "membership.tsv"]
    rows = (out / "features_a2.tsv").read_text().splitlines()
    assert len(rows) == 37 and rows[1].split("\t")[0] == res.feature_table(2, d["feature_names"])[1][0][0]
    # burn-in is passed on
    assert contribution.main(argv + ["--confounders", "universal", "family", "--burnin", "0.5"]) == 0 and seen["burnin"] == 0.5
    assert capsys.readouterr().out.splitlines()[0].startswith("30 samples")


def test_the_readers_error_paths(tmp_path, monkeypatch):
    pytest.importorskip("pandas")
    d, s = recorded.data(), recorded.run(1)
    argv = _write_run(tmp_path, d, s)
    monkeypatch.setattr(contribution, "cluster_contribution", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the device was touched")))
    conf = ["--confounders", "universal", "family"]
    # the samples and the rows must agree in number
    with open(tmp_path / "clusters_short.txt", "w") as f:
        f.write("\n".join((tmp_path / "clusters_K3_0.txt").read_text().splitlines()[:-1]) + "\n")
    with pytest.raises(SystemExit, match="60 stats rows, 59 cluster samples"):
        contribution.main(argv[:3] + [str(tmp_path / "clusters_short.txt")] + conf)
    # the confounders must be the model's: without the family the header rule gives other columns
    with pytest.raises(ValueError, match="the logger's rule gives"):
        contribution.main(argv + ["--confounders", "universal"])
    # a state the states file does not know
    text = (tmp_path / "features.csv").read_text().splitlines()
    cells = text[1].split(",")
    cells[5] = "no-such-state"
    (tmp_path / "features_bad.csv").write_text("\n".join([text[0], ",".join(cells), *text[2:]]) + "\n")
    with pytest.raises(ValueError, match="'no-such-state' is no state of feature 'F1'"):
        contribution.main([str(tmp_path / "features_bad.csv")] + argv[1:] + conf)
    # a stats file without parameter columns
    (tmp_path / "stats_bare.txt").write_text("Sample\tposterior\tsize_a0\n0\t-1.0\t3\n")
    with pytest.raises(ValueError, match="no column 'w_areal_F1'"):
        contribution.main(argv[:2] + [str(tmp_path / "stats_bare.txt"), argv[3]] + conf)
