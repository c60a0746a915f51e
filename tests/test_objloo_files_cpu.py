"""CPU checks of the leave-one-object-out unit's host side (sbayes_amd/objloo.py) without a device: the handle against a fake
library (what each call hands it, the split of a block with its prior, what a failed call leaves), the result's totals, scores
and tables on a recorded run with the checker (tests/_objloo_oracle.py) in the device's place, and the command line."""
import ctypes as ct
import os
from types import SimpleNamespace

import numpy as np
import pytest

from sbayes_amd import _handle, compare, loopred, objloo, predict
from sbayes_amd._handle import _ptr
from tests import _objloo_cases as cases
from tests import _predict_cases as recorded

N, F, S, K = 4, 3, 2, 2


def _result(r=1, predictive=True):
    case, got = cases.recorded(r), cases.recorded_oracle(r)
    return objloo.result_from(case["codes"], [got[name] for name in objloo.POINTWISE], got["membership"], got["p_loo"] if predictive else None,
                              n_samples=got["L"].shape[0])


# ---- the handle against a fake library ---------------------------------------------------------------------------------------------
def _fake(monkeypatch, fail=None):
    """An ObjLooHandle on a library that records its calls as (name, args); `fail`: (name, call number) that returns SBE_ERR_ARG."""
    calls = []

    def entry(name):
        def fn(*args):
            calls.append((name, args))
            if name == "read":
                args[2]._obj.value = sum(a[2] for n, a in calls if n == "accumulate")
            return int(fail == (name, sum(c[0] == name for c in calls)))
        return fn
    names = ("set_data", "set_feature_tile", "reset", "destroy", "last_kernel_ms", "add", "weights", "accumulate", "read", "get_store")
    lib = SimpleNamespace(**{f"sbe_objloo_{name}": entry(name) for name in names}, sbe_objloo_last_error=lambda h: b"refused")

    def create_on(self, load, device):
        self._h, self._lib, self._pid, self.device = ct.c_void_p(1), lib, os.getpid(), device
    monkeypatch.setattr(objloo.ObjLooHandle, "_create_on", create_on)
    return objloo.ObjLooHandle(0), calls


def _samples(T, C=2):
    R = K + 2 * (C - 1)
    return np.zeros((T, K, N), dtype=np.uint8), np.zeros((T, F, C)), np.zeros((T, R, F, S))


def _with_data(h, capacity=7):
    h.set_data(np.zeros((N, F), np.uint8), np.zeros((1, N), np.uint8), [2], S, K, capacity=capacity)


def test_set_data_hands_the_library_the_shape_and_the_capacity(monkeypatch):
    h, calls = _fake(monkeypatch)
    _with_data(h)
    (name, args), = calls
    assert name == "set_data" and args[1:6] == (N, F, S, 2, K) and args[9:] == (7,) and h.shape == (N, F, S, 2, K, K + 2) and h.capacity == 7


def test_a_block_goes_in_calls_of_at_most_max_samples_with_its_slice_of_the_prior(monkeypatch):
    h, calls = _fake(monkeypatch)
    _with_data(h)
    m = 3
    monkeypatch.setattr(objloo, "MAX_STAGE_BYTES", m * objloo.sample_bytes(*h.shape) + 1)
    assert h.max_samples() == m
    clusters, weights, tables = _samples(2 * m + 1)
    h.add(clusters, weights, tables)                             # no prior: a null pointer
    made = [a for n, a in calls if n == "add"]
    assert [a[1] for a in made] == [m, m, 1] and all(a[5] is None for a in made) and h.n_rows == 7
    for t0, a in zip((0, m, 2 * m), made):
        assert a[2:5] == (_ptr(clusters[t0:]), _ptr(weights[t0:]), _ptr(tables[t0:]))
    h.weights()
    (args,) = [a for n, a in calls if n == "weights"]
    assert len(args) == 9 and all(isinstance(a, int) for a in args[1:])
    row = np.array([0.5, 0.25, 0.25])
    h.accumulate(clusters, weights, tables, prior=row)           # one row for everyone: broadcast to [T, N, K+1] and sliced
    made = [a for n, a in calls if n == "accumulate"]
    assert [a[1:3] for a in made] == [(0, m), (m, m), (2 * m, 1)] and all(isinstance(a[6], int) for a in made)
    step = N * (K + 1) * 8
    assert made[1][6] - made[0][6] == m * step and made[2][6] - made[1][6] == m * step
    assert h.next_t == 7 and h.sums()[1] == 7
    res = h.result()
    assert res.n_samples == 7 and res.p_loo.shape == (N, F, S) and res.membership.shape == (N, K + 1) and set(res.kernel_ms) == {"add", "weights", "accumulate"}
    assert h.result(predictive=False).p_loo is None


def test_a_failed_call_raises_and_keeps_what_the_calls_before_it_left(monkeypatch):
    h, calls = _fake(monkeypatch, fail=("add", 2))
    _with_data(h)
    monkeypatch.setattr(objloo, "MAX_STAGE_BYTES", 3 * objloo.sample_bytes(*h.shape) + 1)
    with pytest.raises(_handle.EngineError, match="refused"):
        h.add(*_samples(7))
    assert h.n_rows == 3 and [n for n, _a in calls].count("add") == 2
    with pytest.raises(ValueError, match="no weights yet"):
        h.accumulate(*_samples(3))
    h.weights()
    with pytest.raises(ValueError, match="0 of 3 samples accumulated, 4 more are too many"):
        h.accumulate(*_samples(4))
    h.accumulate(*_samples(2))
    with pytest.raises(ValueError, match="2 of 3 samples accumulated: the second pass is not complete"):
        h.result()
    h.add(*_samples(1))                                          # a further add discards the weights
    with pytest.raises(ValueError, match="no weights yet"):
        h.result()
    h.reset()
    assert (h.n_rows, h.next_t) == (0, 0) and calls[-1][0] == "reset"


# ---- the result --------------------------------------------------------------------------------------------------------------------
def test_the_module_states_its_caveats_and_reuses_the_shared_helpers():
    assert objloo._group is loopred._group and objloo.NA is predict.NA
    for name in ("read_data", "read_parameters", "read_cluster_samples", "codes_of"):
        assert not hasattr(objloo, name)
    for caveat in ("CONDITIONAL ON THE LOGGED EFFECT DRAWS", "THE PRIOR MUST BE THE MODEL'S CONDITIONAL PRIOR OF THE MEMBERSHIP", "uniform_area",
                   "geo.costs_per_object", "LABELS MUST BE ALIGNED", "PARETO K HAS TO BE READ"):
        assert caveat in objloo.__doc__, caveat


def test_the_totals_and_scores_of_a_recorded_run():
    res, case, got = _result(), cases.recorded(1), cases.recorded_oracle(1)
    obs = case["codes"] != predict.NA
    assert res.loo_i.dtype == np.float64 and res.loo_i.shape == (100,) and res.n_samples == 54 and res.membership.shape == (100, 4)
    assert res.elpd == float(np.sum(got["loo_i"])) and round(res.elpd, 1) == -2067.6 and round(res.elpd_cond, 1) == -2034.8
    assert res.se == pytest.approx((100 * np.var(got["loo_i"])) ** 0.5, rel=1e-15)
    cell = cases.loopred_cases.recorded_oracle(1)["loo_i"]      # the spread over N objects, not over N F cells taken as independent
    assert res.se > (cell.size * np.var(cell)) ** 0.5
    assert res.p_eff == pytest.approx(got["lppd_i"].sum() - got["loo_i"].sum(), rel=1e-15) and res.p_eff > 0
    assert res.n_bad_k() == 12 and res.n_bad_k(conditional=True) == 20 and res.n_bad_k(10.0) == 0
    nan_k = objloo.result_from(case["codes"], [np.full(100, np.nan)] * 7, got["membership"], None, 54)
    assert nan_k.n_bad_k() == 100
    # the zero-shot scores: every cell is predicted without the object's own data
    best = res.predicted
    assert best.shape == (100, 36) and np.array_equal(best, got["p_loo"].argmax(axis=2))
    hit = (best == case["codes"]) & obs
    assert res.accuracy() == hit.sum() / obs.sum() and 0.2 < res.accuracy() < 1.0
    assert np.array_equal(res.accuracy("object"), hit.sum(axis=1) / obs.sum(axis=1)) and res.accuracy("feature").shape == (36,)
    onehot = np.arange(5)[None, None, :] == case["codes"][..., None]
    assert res.brier() == pytest.approx(((got["p_loo"] - onehot) ** 2).sum(axis=2)[obs].mean(), rel=1e-12)
    x = np.where(obs, case["codes"], 0).astype(np.int64)[..., None]
    p_obs = np.take_along_axis(got["p_loo"], x, axis=2)[..., 0]
    assert res.log_score() == pytest.approx(np.log(p_obs[obs]).mean(), rel=1e-12) and np.isnan(res.p_obs[~obs]).all()
    with pytest.raises(ValueError, match="by='cell'"):
        res.accuracy(by="cell")
    # predicting an undocumented object is harder than predicting one of its cells from the others
    by_cell = loopred.result_from(case["codes"], *(cases.loopred_cases.recorded_oracle(1)[k] for k in ("p_loo", "loo_i", "k", "n_eff")), n_samples=54)
    assert res.log_score() < by_cell.log_score() and res.brier() > by_cell.brier()
    bare = _result(predictive=False)
    assert bare.p_loo is None and bare.elpd == res.elpd
    with pytest.raises(ValueError, match="no predictive"):
        bare.accuracy()


def test_compare_takes_the_pointwise_vectors_as_they_are():
    res = _result()
    names, vectors, kind, _p, _warn = compare._check_models({"cond": res.loo_cond_i, "marg": res.loo_i})
    assert names == ["cond", "marg"] and kind == "elpd" and vectors[1] is res.loo_i and vectors[0].size == 100


def test_the_tables_of_a_recorded_run(tmp_path):
    res = _result()
    header, rows = res.table()
    assert header == ["object", "n_observed", "loo_i", "k", "n_eff", "lppd_i", "loo_cond_i", "k_cond", "lppd_cond_i", "membership", "p_membership",
                      "accuracy", "log_score"] and len(rows) == 100
    n = 17
    assert rows[n][:4] == [n, int(res.observed[n].sum()), res.loo_i[n], res.k_i[n]] and rows[n][9] == int(res.membership[n].argmax())
    assert rows[n][10] == res.membership[n].max() and rows[n][11] == res.accuracy("object")[n]
    assert len(_result(predictive=False).table(object_names=[f"L{i}" for i in range(100)])[0]) == 11
    header, rows = res.summary_table()
    assert header == ["column", "n_objects", "n_samples", "elpd", "se", "p_eff", "n_bad_k"]
    assert rows[0] == ["marginal", 100, 54, res.elpd, res.se, res.p_eff, 12] and rows[1][:4] == ["conditional", 100, 54, res.elpd_cond] and rows[1][6] == 20
    paths = res.write_tables(tmp_path / "out")
    assert [p.name for p in paths] == ["object_loo.tsv", "object_loo_summary.tsv"]
    lines = paths[0].read_text().splitlines()
    assert len(lines) == 101 and lines[0].split("\t")[:3] == ["object", "n_observed", "loo_i"] and float(lines[1].split("\t")[2]) == pytest.approx(res.loo_i[0], rel=1e-9)
    assert len(paths[1].read_text().splitlines()) == 3


def test_the_command_line_reads_the_run_prints_the_summary_and_writes_the_tables(tmp_path, monkeypatch, capsys):
    pytest.importorskip("pandas")
    from tests.test_contrib_files_cpu import _write_run
    d, s = recorded.data(), recorded.run(1)
    argv = _write_run(tmp_path, d, s)
    seen = {}

    def stub(codes, groups, clusters, weights, tables, prior=None, burnin=0.1, predictive=True, device=None, n_groups=None):
        seen.update(codes=codes, groups=groups, clusters=clusters, weights=weights, tables=tables, prior=prior, burnin=burnin, n_groups=n_groups,
                    device=device, predictive=predictive)
        return _result()
    monkeypatch.setattr(objloo, "object_loo", stub)
    row = np.array([0.4, 0.2, 0.2, 0.2])
    np.save(tmp_path / "prior.npy", row)
    out = tmp_path / "tables"
    assert objloo.main(argv + ["--confounders", "universal", "family", "--out", str(out), "--device", "0", "--prior", str(tmp_path / "prior.npy")]) == 0
    case = recorded.case(1)
    assert np.array_equal(seen["codes"], case["codes"]) and np.array_equal(seen["groups"], case["groups"]) and seen["n_groups"] == [1, 6]
    assert np.array_equal(seen["clusters"], case["clusters"]) and np.array_equal(seen["weights"], case["weights"])
    assert np.array_equal(seen["tables"], case["tables"]) and (seen["burnin"], seen["device"], seen["predictive"]) == (0.1, 0, True)
    assert np.array_equal(seen["prior"], row)
    res = _result()
    lines = capsys.readouterr().out.splitlines()
    assert lines[0] == (f"54 samples, 100 objects (given the logged effect draws, membership integrated out): elpd {res.elpd:.2f} (se {res.se:.2f}), "
                        f"p_eff {res.p_eff:.2f}; conditional on the logged membership: elpd {res.elpd_cond:.2f}")
    assert lines[1] == f"zero-shot accuracy {res.accuracy():.4f}, Brier {res.brier():.4f}, log score {res.log_score():.4f}"
    assert lines[2] == "warning: 12 objects with Pareto k > 0.7: their leave-one-out weights are unreliable" and len(lines) == 3
    assert sorted(p.name for p in out.iterdir()) == ["object_loo.tsv", "object_loo_summary.tsv"]
    assert objloo.main(argv + ["--confounders", "universal", "family"]) == 0 and seen["prior"] is None
