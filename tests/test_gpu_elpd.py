"""PSIS-LOO and WAIC on the device (sbayes_amd.elpd) against the NumPy restatement tests/_elpd_oracle.py, and the
LikelihoodLog fed from engine slots along the recorded reference traces."""
import numpy as np
import pytest

from oracle import sbayes_oracle as orc
from sbayes_amd import elpd
from sbayes_amd.engine import EngineError
from sbayes_amd.registry import release_all
from tests import _elpd_oracle as eo

pytestmark = pytest.mark.gpu

RTOL = 1e-10


@pytest.fixture(autouse=True)
def _fresh_engines():
    yield
    release_all()


def make_lh(s, m, seed):
    """float32 [s, m]: smooth columns, quantised (tied) columns, constant columns and heavy tails (k > 0.7)."""
    rng = np.random.default_rng(seed)
    kind = np.arange(m) % 5
    lh = np.exp(rng.normal(-1.5, 0.8, (s, m)))                       # smooth
    q = kind == 1
    lh[:, q] = np.round(rng.uniform(0.05, 1, (s, q.sum())), 1)       # ten distinct values: heavy ties
    lh[:, kind == 2] = 0.37                                          # constant
    h = kind == 3
    lh[:, h] = rng.uniform(1e-5, 1, (s, h.sum()))                    # importance ratios with tail index 1
    t = kind == 4
    lh[:, t] = np.exp(-rng.standard_exponential((s, t.sum())) * 3)  # lighter tail
    return lh.astype(np.float32)


def close(got, want, rtol=RTOL, atol=1e-10):
    got, want = np.asarray(got, float), np.asarray(want, float)
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = np.isnan(want) | (np.abs(got - want) <= np.maximum(rtol * np.abs(want), atol))
    assert ok.all(), (np.flatnonzero(~ok)[:5], got[~ok][:5], want[~ok][:5])


def check_k(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert np.array_equal(np.isinf(got), np.isinf(want)) and np.array_equal(np.isnan(got), np.isnan(want))
    fin = np.isfinite(want)
    assert np.all(np.abs(got[fin] - want[fin]) <= 1e-9), np.max(np.abs(got[fin] - want[fin]))


def compare(lh, na, burnin, columns=None):
    """Device against the oracle; `columns` (indices into the kept columns) limits the per-column oracle."""
    res = elpd.psis_loo(lh, na_values=na, burnin=burnin)
    w = elpd.waic(lh, na_values=na, burnin=burnin)
    keep = eo.kept_columns(lh, na)
    b = eo.burnin_rows(lh.shape[0], burnin)
    x = lh[b:, keep]
    s = x.shape[0]
    assert res.n_samples == w.n_samples == s and res.n_data_points == w.n_data_points == x.shape[1]
    idx = np.arange(x.shape[1]) if columns is None else columns
    want = np.array([eo.column_stats(x[:, j]) for j in idx]).reshape(-1, 4)
    close(res.loo_i[idx], want[:, 0])
    check_k(res.pareto_k[idx], want[:, 1])
    close(w.waic_i[idx], want[:, 2] - want[:, 3])
    if columns is None:
        t = eo.totals(want[:, 0], want[:, 1], want[:, 2], want[:, 3], s)
        for got, key in [(res.elpd_loo, "elpd_loo"), (res.se, "se"), (res.p_loo, "p_loo"), (res.lppd, "lppd"),
                         (w.elpd_waic, "elpd_waic"), (w.se, "waic_se"), (w.p_waic, "p_waic")]:
            close([got], [t[key]])
        assert res.good_k == t["good_k"] and res.warning == t["warning"] and w.warning == t["waic_warning"]
        assert res.n_data_points == t["n_data_points"]
    return res, w


@pytest.mark.parametrize("s", [5, 64, 1000, 4000])
def test_sample_counts_against_the_oracle(s):
    lh = make_lh(s, 25, seed=s)
    res, _w = compare(lh, np.zeros(25, bool), 0.0)
    assert np.isinf(res.pareto_k[2])                                 # the constant column
    if s >= 1000:
        assert res.pareto_k[3] > 0.7 and res.warning


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_the_lds_threshold_and_the_global_form(delta):
    s = elpd.lds_max_samples() + delta
    lh = make_lh(s, 10, seed=100 + delta)
    compare(lh, np.zeros(10, bool), 0.0)


def test_global_and_staged_forms_agree_bit_for_bit():
    """One column cut to S = threshold and threshold + 1 elements differs by one sample; the same S reached by
    burn-in from a longer store takes the same kernel path: the results are identical."""
    s = elpd.lds_max_samples() + 1
    lh = make_lh(s + 7, 5, seed=5)
    a = elpd.psis_loo(lh[7:], na_values=np.zeros(5, bool), burnin=0.0)
    b = elpd.psis_loo(lh, na_values=np.zeros(5, bool), burnin=7 / (s + 7) + 1e-12)
    assert b.n_samples == s
    assert np.array_equal(a.loo_i, b.loo_i) and np.array_equal(a.pareto_k, b.pareto_k, equal_nan=True)


@pytest.mark.parametrize("na_kind", ["mask", "isclose"])
@pytest.mark.parametrize("burnin", [0.0, 0.1, 0.5])
def test_na_and_burnin_combinations(na_kind, burnin):
    lh = make_lh(200, 60, seed=7)
    lh[:, 5] = 1.0
    lh[:, 11] = np.float32(1 + 4e-6)
    lh[:, 17] = 1.0
    lh[0, 17] = 0.5                          # not NA by the isclose rule: a burn-in row differs
    na = np.zeros(60, bool)
    na[[5, 11, 40]] = True
    compare(lh, na if na_kind == "mask" else None, burnin)


def test_3600_observations():
    compare(make_lh(1000, 3600, seed=36), np.zeros(3600, bool), 0.1)


def test_headline_width():
    """M = 200 000 (the headline N * F): every column computed, a sample of them checked column by column."""
    lh = make_lh(64, 200_000, seed=2)
    na = np.zeros(200_000, bool)
    na[::13] = True
    res, w = compare(lh, na, 0.1, columns=np.arange(0, 200_000 - 200_000 // 13 - 1, 97))
    assert res.n_data_points == 200_000 - len(range(0, 200_000, 13))
    assert np.isfinite(res.loo_i).all() and np.isfinite(w.waic_i).all()


def test_store_overflow_and_bad_values():
    st = elpd._Store(0, 3, 2)
    try:
        st.append_rows(np.full((2, 3), 0.5, dtype=np.float32))
        with pytest.raises(EngineError, match="store overflow") as info:
            st.append_rows(np.full((1, 3), 0.5, dtype=np.float32))
        assert info.value.code == 1 and st.n_rows == 2
        with pytest.raises(EngineError, match="burn_rows"):
            st.compute(2, None, False)
    finally:
        st.close()
    lh = np.full((10, 4), 0.5, dtype=np.float32)
    lh[3, 2] = -0.5
    with pytest.raises(EngineError, match="not positive and finite") as info:
        elpd.psis_loo(lh, na_values=np.zeros(4, bool), burnin=0.0)
    assert info.value.code == 4


def test_rows_round_trip_through_the_store():
    lh = make_lh(70, 33, seed=70)
    st = elpd._Store(0, 33, 100)
    try:
        st.append_rows(lh[:30])
        st.append_rows(lh[30:])
        assert np.array_equal(st.rows(), lh)
        st.reset()
        assert st.n_rows == 0
    finally:
        st.close()


# ---- end to end: the LikelihoodLog along the recorded reference traces ------------------------------------------
def _replay(name):
    from sbayes_amd import model as sbm
    from sbayes_amd.counts import recalculate_feature_counts, update_feature_counts
    from tests.test_gpu_dropin import build, load_case
    fx, tr = load_case(name)
    model, sample = build(fx)
    feats = model.data.features.values
    recalculate_feature_counts(feats, sample)
    yield model, sample, fx
    for i in range(tr.n_steps):
        cand = sample.copy()
        new_clusters, new_source, new_weights = tr.clusters(i), tr.source(i), tr.weights[i]
        moved = np.flatnonzero((new_clusters != sample.clusters.value).any(axis=0) |
                               (new_source != sample.source.value).any(axis=(1, 2)))
        for k in np.flatnonzero((new_clusters != sample.clusters.value).any(axis=1)):
            with cand.clusters.edit_cluster(int(k)) as row:
                row[:] = new_clusters[k]
        if (new_source != sample.source.value).any():
            with cand.source.edit() as src:
                src[moved] = new_source[moved]
        if not np.array_equal(new_weights, sample.weights.value):
            cand.weights.set_value(new_weights.copy())
        if moved.size:
            update_feature_counts(sample, cand, feats, moved)
        yield model, cand, fx
        sample = cand
    del sbm


@pytest.mark.parametrize("name", ["cfg1", "south_america"])
def test_likelihood_log_along_a_recorded_trace(name):
    from sbayes_amd.likelihood import update_weights
    log = None
    want_rows = []
    for i, (model, sample, fx) in enumerate(_replay(name)):
        if log is None:
            log = elpd.LikelihoodLog(model, capacity=500)
        log.append(sample)
        if i % 20 == 0 or i < 3:
            groups = [sample.clusters.value] + [np.asarray(g) for g in fx.groups[1:]]
            counts = orc.recalculate_feature_counts(fx.features, groups, sample.source.value)
            lh_exact = orc.likelihood_per_component_exact(fx.features, model.data.features.na_values, groups, counts,
                                                          fx.conc, sample.source.value)
            row = orc.logger_row(np.asarray(update_weights(sample)), lh_exact).astype(np.float32)
            want_rows.append((i, row))
    rows = log.rows()
    assert len(log) == rows.shape[0] > 300
    for i, row in want_rows:
        assert np.array_equal(rows[i], row), f"state {i}"
    na = log.na_values()
    dev = log.psis_loo(burnin=0.1)
    host = elpd.psis_loo(rows, na_values=na, burnin=0.1)
    assert np.array_equal(dev.loo_i, host.loo_i) and np.array_equal(dev.pareto_k, host.pareto_k, equal_nan=True)
    assert dev.elpd_loo == host.elpd_loo and dev.se == host.se and dev.p_loo == host.p_loo
    wd, wh = log.waic(burnin=0.1), elpd.waic(rows, na_values=na, burnin=0.1)
    assert np.array_equal(wd.waic_i, wh.waic_i) and wd.elpd_waic == wh.elpd_waic
    compare(rows, na, 0.1)
    log.close()


def test_sbayes_psis_loo_reads_a_likelihood_file(tmp_path):
    lh = make_lh(300, 40, seed=300)
    na = np.zeros(40, bool)
    na[3] = True
    np.savez(tmp_path / "likelihood.npz", likelihood=lh, na_values=na)
    got = elpd.sbayes_psis_loo(tmp_path / "likelihood.npz", burnin=0.2)
    assert got == elpd.psis_loo(lh, na_values=na, burnin=0.2).elpd_loo
