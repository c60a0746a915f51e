"""CPU checks of the leave-one-out predictive's command line, summaries and tables (sbayes_amd/loopred.py) on the recorded
reference runs of tests/golden/diag_runs.npz: the files are read through the posterior predictive's readers, the device handle is
replaced by the oracle (tests/_loopred_oracle.py), and the tables and the printed lines say what the result holds."""
import numpy as np
import pytest

from sbayes_amd import loopred, predict
from tests import _loopred_cases as cases
from tests import _predict_cases as recorded
from tests import _predict_oracle as po
from tests.test_contrib_files_cpu import _write_run


def _result(r=1):
    case, got = cases.recorded(r), cases.recorded_oracle(r)
    return loopred.result_from(case["codes"], got["p_loo"], got["loo_i"], got["k"], got["n_eff"], n_samples=got["lik"].shape[0])


def test_the_module_reuses_the_readers_of_the_posterior_predictive():
    for name in ("_check_shape", "group_index", "_check_burnin", "NA"):
        assert getattr(loopred, name) is getattr(predict, name)
    for name in ("read_data", "read_parameters", "read_cluster_samples", "codes_of"):
        assert not hasattr(loopred, name)
    for caveat in ("CONDITIONAL ON THE LOGGED EFFECT DRAWS", "not on a draw already made", "not the LikelihoodLogger's collapsed form"):
        assert caveat in loopred.__doc__


def test_the_summaries_of_a_recorded_run():
    res, case, got = _result(), cases.recorded(1), cases.recorded_oracle(1)
    obs = case["codes"] != predict.NA
    assert res.probs.shape == (100, 36, 5) and res.n_samples == 54 and int(obs.sum()) == 3508
    assert np.isnan(res.probs[~obs]).all() and np.isnan(res.loo_i[~obs]).all() and np.isnan(res.k[~obs]).all() and np.isnan(res.n_eff[~obs]).all()
    assert np.array_equal(res.loo_i[obs], got["loo_i"]) and np.array_equal(res.k[obs], got["k"])
    assert np.allclose(res.probs[obs].sum(axis=1), 1.0, rtol=0, atol=1e-6)              # (the stats files print 8 digits)
    assert np.allclose(res.p_obs[obs], np.exp(got["loo_i"]), rtol=2.0 ** -22, atol=0) and np.isnan(res.p_obs[~obs]).all()
    best = res.predicted
    assert (best[~obs] == -1).all() and np.array_equal(best[obs], got["p_loo"][obs].argmax(axis=1))
    hit = (best == case["codes"]) & obs
    assert res.accuracy() == hit.sum() / 3508 and 0.3 < res.accuracy() < 1.0
    assert np.array_equal(res.accuracy("feature"), hit.sum(axis=0) / obs.sum(axis=0)) and res.accuracy("object").shape == (100,)
    onehot = np.arange(5)[None, None, :] == case["codes"][..., None]
    brier = ((got["p_loo"] - onehot) ** 2).sum(axis=2)
    assert res.brier() == pytest.approx(brier[obs].mean(), rel=1e-12) and res.brier("feature").shape == (36,)
    assert res.log_score() == pytest.approx(got["loo_i"].mean(), rel=1e-12)
    assert res.log_score("object")[0] == pytest.approx(res.loo_i[0][obs[0]].mean(), rel=1e-12)
    with pytest.raises(ValueError, match="by='cell'"):
        res.accuracy(by="cell")
    assert res.n_bad_k() == int((got["k"] > 0.7).sum()) > 0 and res.n_bad_k(10.0) == 0
    # the calibration table counts every (observed cell, state) pair once; a tie in the arg-max goes to the lowest state
    count, mean, freq = res.calibration(bins=10)
    assert count.sum() == 3508 * 5 and count.shape == mean.shape == freq.shape == (10,)
    full = count > 0
    assert ((mean[full] >= np.arange(10)[full] / 10) & (mean[full] <= (np.arange(10)[full] + 1) / 10)).all()
    assert (count * np.nan_to_num(freq)).sum() == pytest.approx(3508) and (count * np.nan_to_num(mean)).sum() == pytest.approx(res.probs[obs].sum())
    tie = loopred.result_from(np.array([[1]], np.uint8), np.array([[[0.25, 0.375, 0.375]]]), [0.0], [0.0], [1.0], 2)
    assert tie.predicted.tolist() == [[1]] and tie.accuracy() == 1.0 and tie.calibration(4)[0].tolist() == [0, 3, 0, 0]


def test_the_optimism_against_the_posterior_predictive():
    res, case = _result(), cases.recorded(1)
    sums, _lik = po.run(**case)
    inside = predict.PredictResult(codes=case["codes"], pred_sum=sums.pred, resp_sum=sums.resp, n_samples=54, n_zero=0)
    opt = res.optimism(inside)
    obs = case["codes"] != predict.NA
    x = np.where(obs, case["codes"], 0).astype(np.int64)[..., None]
    log_in = np.log(np.take_along_axis(inside.probs, x, axis=2)[..., 0][obs]).mean()
    assert opt["log_score"] == pytest.approx(log_in - res.log_score(), rel=1e-12) and opt["log_score"] > 0     # the in-sample fit is optimistic
    assert opt["accuracy"] == pytest.approx(((inside.probs.argmax(axis=2) == case["codes"]) & obs).sum() / 3508 - res.accuracy(), abs=1e-15)
    with pytest.raises(ValueError, match="holds 60 samples"):
        res.optimism(predict.PredictResult(codes=case["codes"], pred_sum=sums.pred, resp_sum=sums.resp, n_samples=60, n_zero=0))
    with pytest.raises(ValueError, match="other data"):
        res.optimism(predict.PredictResult(codes=case["codes"][:50], pred_sum=sums.pred[:50], resp_sum=sums.resp[:50], n_samples=54, n_zero=0))


def test_the_tables_of_a_recorded_run(tmp_path):
    res, d = _result(), recorded.data()
    header, rows = res.table(d["feature_names"], d["state_names"])
    assert header == ["object", "feature", "observed", "predicted", "p_obs", "loo_i", "k"] and len(rows) == 3508
    n, f = np.argwhere(res.observed)[17]
    row = rows[17]
    assert row[:2] == [n, d["feature_names"][f]] and row[2] == d["state_names"][f][res.codes[n, f]] and row[3] == d["state_names"][f][res.predicted[n, f]]
    assert row[4:] == [res.p_obs[n, f], res.loo_i[n, f], res.k[n, f]]
    header, rows = res.feature_table(d["feature_names"])
    assert header == ["feature", "n_observed", "accuracy", "brier", "log_score", "n_bad_k"] and [r[0] for r in rows] == d["feature_names"]
    assert sum(r[1] for r in rows) == 3508 and sum(r[5] for r in rows) == res.n_bad_k()
    paths = res.write_tables(tmp_path / "out", d["feature_names"], d["state_names"])
    assert [p.name for p in paths] == ["loo_predictive.tsv", "loo_features.tsv"]
    lines = paths[0].read_text().splitlines()
    assert len(lines) == 3509 and lines[0].split("\t")[4:] == ["p_obs", "loo_i", "k"] and float(lines[1].split("\t")[5]) == pytest.approx(res.loo_i[res.observed][0], rel=1e-9)
    assert len(paths[1].read_text().splitlines()) == 37


def test_the_command_line_reads_the_run_prints_the_summary_and_writes_the_tables(tmp_path, monkeypatch, capsys):
    pytest.importorskip("pandas")
    d, s = recorded.data(), recorded.run(1)
    argv = _write_run(tmp_path, d, s)
    seen = {}

    def stub(codes, groups, clusters, weights, tables, burnin=0.1, device=None, n_groups=None):
        seen.update(codes=codes, groups=groups, clusters=clusters, weights=weights, tables=tables, burnin=burnin, n_groups=n_groups, device=device)
        assert predict._check_burnin(burnin, clusters.shape[0]) == cases.BURN
        return _result()
    monkeypatch.setattr(loopred, "loo_predictive", stub)
    out = tmp_path / "tables"
    assert loopred.main(argv + ["--confounders", "universal", "family", "--out", str(out), "--device", "0"]) == 0
    case = recorded.case(1)
    assert np.array_equal(seen["codes"], case["codes"]) and np.array_equal(seen["groups"], case["groups"]) and seen["n_groups"] == [1, 6]
    assert np.array_equal(seen["clusters"], case["clusters"]) and np.array_equal(seen["weights"], case["weights"])
    assert np.array_equal(seen["tables"], case["tables"]) and (seen["burnin"], seen["device"]) == (0.1, 0)
    res = _result()
    lines = capsys.readouterr().out.splitlines()
    assert lines[0] == (f"54 samples, 3508 observed cells (given the logged effect draws): leave-one-out accuracy {res.accuracy():.4f}, "
                        f"Brier {res.brier():.4f}, log score {res.log_score():.4f}")
    assert lines[1] == f"warning: {res.n_bad_k()} cells with Pareto k > 0.7: their leave-one-out weights are unreliable" and len(lines) == 2
    assert sorted(p.name for p in out.iterdir()) == ["loo_features.tsv", "loo_predictive.tsv"]
    # the samples and the rows must agree in number
    with open(tmp_path / "clusters_short.txt", "w") as f:
        f.write("\n".join((tmp_path / "clusters_K3_0.txt").read_text().splitlines()[:-1]) + "\n")
    with pytest.raises(SystemExit, match="60 stats rows, 59 cluster samples"):
        loopred.main(argv[:3] + [str(tmp_path / "clusters_short.txt"), "--confounders", "universal", "family"])
