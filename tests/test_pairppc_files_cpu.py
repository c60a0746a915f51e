"""CPU checks of the pairwise check's command line and table (sbayes_amd/pairppc.py) on the recorded reference runs of
tests/golden/diag_runs.npz: the files are read through the posterior predictive's readers, the device calls are replaced by the
oracles (tests/_pairppc_oracle.py over the replicates of tests/_ppc_oracle.py, tests/_assoc_oracle.py for the raw screen), and
the table and the printed lines say what the result holds."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from sbayes_amd import pairppc, predict
from tests import _assoc_oracle as ao
from tests import _pairppc_oracle as orc
from tests import _ppc_cases as ppc_cases
from tests import _predict_cases as recorded

FIELDS = ("stat_obs", "dof_obs", "n_obs", "valid_obs") + orc.INT_FIELDS + ("sum", "sumsq")


def _n_states():
    return np.array([max(1, len(s)) for s in recorded.data()["state_names"]], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def _oracle(r, burn):
    case = ppc_cases.recorded(r)
    return orc.check(case["codes"], _n_states(), ppc_cases.recorded_oracle(r)["y_rep"][burn:])


def _result(r, burn=0):
    want = _oracle(r, burn)
    return pairppc.PairResult(*(want[k] for k in FIELDS), want["n_replicates"], _n_states())


def test_the_module_reuses_the_readers_and_the_limits():
    assert pairppc.NA is pairppc.assoc.NA and pairppc.MAX_STAGE_BYTES is predict.MAX_STAGE_BYTES
    for name in ("read_data", "read_parameters", "read_cluster_samples", "_check_burnin", "group_index"):
        assert not hasattr(pairppc, name)


def test_the_table_of_a_recorded_run(tmp_path):
    res, d = _result(0), recorded.data()
    names = d["feature_names"]
    header, rows = res.table(names)
    assert header == ["feature_1", "feature_2", "n", "dof", "statistic", "p_raw", "p_predictive", "mean_replicated", "sd_replicated", "z"]
    live = np.triu(res.valid_obs, 1)
    assert len(rows) == int(live.sum()) > 100 and res.n_replicates == 60
    p = res.p_value()
    assert ((p[res.valid_obs] >= 0) & (p[res.valid_obs] <= 1)).all() and np.isnan(p[~res.valid_obs]).all()
    keys = [(r[6], -r[9] if r[9] == r[9] else np.inf) for r in rows]
    assert keys == sorted(keys)
    at = {n: i for i, n in enumerate(names)}
    for row in rows[:5] + rows[-5:]:
        i, j = at[row[0]], at[row[1]]
        assert i < j and live[i, j] and row[2:5] == [int(res.n_obs[i, j]), int(res.dof_obs[i, j]), float(res.stat_obs[i, j])]
        assert row[6] == p[i, j] and row[7] == res.sum[i, j] / 60 and row[5] != row[5]          # (no raw screen: NaN)
    assert [r[:5] + r[6:] for r in res.worst(3, names)] == [r[:5] + r[6:] for r in rows[:3]]          # (NaN is not equal to itself)
    with pytest.raises(ValueError, match="35 names for 36 features"):
        res.table(names[:-1])
    res.write_table(tmp_path / "pairs.tsv", names)
    lines = (tmp_path / "pairs.tsv").read_text().splitlines()
    assert lines[0].split("\t") == header and len(lines) == len(rows) + 1
    first = lines[1].split("\t")
    assert first[:2] == rows[0][:2] and int(first[3]) == rows[0][3] and float(first[6]) == pytest.approx(rows[0][6], rel=1e-9)


def test_the_command_line_reads_the_run_and_writes_both_p_values(tmp_path, monkeypatch, capsys):
    pytest.importorskip("pandas")
    d, s = recorded.data(), recorded.run(1)
    families = ["" if g == pairppc.NA else d["confounders"]["family"][g] for g in d["groups"][1]]
    with open(tmp_path / "features.csv", "w") as f:
        f.write("id,name,family,x,y," + ",".join(d["feature_names"]) + "\n")
        for n in range(100):
            cells = ["" if c == pairppc.NA else d["state_names"][k][c] for k, c in enumerate(d["codes"][n])]
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

    def stub(codes, groups, clusters, weights, tables, n_states=None, burnin=0.1, seed=0, n_groups=None, uniforms=None, device=None):
        seen.update(codes=codes, groups=groups, clusters=clusters, weights=weights, tables=tables, n_states=n_states, burnin=burnin, seed=seed,
                    n_groups=n_groups, device=device)
        return _result(1, burn=predict._check_burnin(burnin, clusters.shape[0]))

    def raw(codes, n_states, device=0):
        seen["raw"] = (codes, n_states, device)
        return SimpleNamespace(pvalue=ao.feature_association(codes, n_states)["pvalue"])
    monkeypatch.setattr(pairppc, "pairwise_check", stub)
    monkeypatch.setattr(pairppc.assoc, "feature_association", raw)
    out = tmp_path / "pairs.tsv"
    argv = [str(tmp_path / n) for n in ("features.csv", "feature_states.csv", "stats_K3_0.txt", "clusters_K3_0.txt")]
    assert pairppc.main(argv + ["--confounders", "universal", "family", "--seed", str(ppc_cases.SEED), "--out", str(out), "--device", "0"]) == 0
    case = ppc_cases.recorded(1)
    assert np.array_equal(seen["codes"], case["codes"]) and np.array_equal(seen["groups"], case["groups"]) and seen["n_groups"] == [1, 6]
    assert np.array_equal(seen["clusters"], case["clusters"]) and np.array_equal(seen["weights"], case["weights"])
    assert np.array_equal(seen["tables"], case["tables"]) and (seen["burnin"], seen["seed"], seen["device"]) == (0.1, ppc_cases.SEED, 0)
    assert np.array_equal(seen["n_states"], _n_states()) and np.array_equal(seen["raw"][0], case["codes"]) and seen["raw"][2] == 0
    res = _result(1, burn=6)
    res.raw_pvalue = ao.feature_association(case["codes"], _n_states())["pvalue"]
    header, rows = res.table(d["feature_names"])
    lines = capsys.readouterr().out.splitlines()
    pairs = int(np.triu(res.valid_obs, 1).sum())
    assert lines[0] == (f"54 replicates, {pairs} pairs valid on the data, {len(res.flagged(0.05))} with predictive p < 0.05 "
                        f"(conservative: given the logged effect draws; {pairs} comparisons, uncorrected)")
    assert lines[1] == "the five pairs with the smallest predictive p:" and len(lines) == 7
    assert [line.split("\t")[:2] for line in lines[2:]] == [["  " + r[0], r[1]] for r in rows[:5]]
    written = [line.split("\t") for line in out.read_text().splitlines()]
    assert written[0] == header and len(written) == pairs + 1
    assert [w[:2] for w in written[1:]] == [r[:2] for r in rows]
    assert all(float(w[5]) == pytest.approx(r[5], rel=1e-9) and float(w[6]) == pytest.approx(r[6], rel=1e-9) for w, r in zip(written[1:], rows))
    with open(tmp_path / "clusters_short.txt", "w") as f:
        f.write("\n".join((tmp_path / "clusters_K3_0.txt").read_text().splitlines()[:-1]) + "\n")
    with pytest.raises(SystemExit, match="60 stats rows, 59 cluster samples"):
        pairppc.main(argv[:3] + [str(tmp_path / "clusters_short.txt"), "--confounders", "universal", "family"])
