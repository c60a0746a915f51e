"""PSIS-LOO and WAIC on the device across the range DESIGN section 11 promises: long columns at every tail-buffer step
(Tp = 1024 / 2048 / 4096, up to S = 2^20), a statistical known answer at 2^20 samples, short columns and the tail
thresholds, extreme float32 values and the data check, host <-> store staging in several pieces, more than 2^24
columns, the LikelihoodLog over a wide engine, and a fixed-seed slice of the randomised generator
(tools/fuzz_gpu.py --elpd).  Every result is checked against the NumPy restatement tests/_elpd_oracle.py."""
import math

import numpy as np
import pytest

from sbayes_amd import elpd
from sbayes_amd.engine import EngineError
from sbayes_amd.registry import release_all
from tests import _elpd_oracle as eo
from tests.test_gpu_elpd import check_k, close, compare, make_lh

pytestmark = pytest.mark.gpu

FLT_MAX = float(np.finfo(np.float32).max)
FLT_TRUE_MIN = float(np.float32(2.0 ** -149))          # the smallest positive subnormal, 1.4e-45


@pytest.fixture(autouse=True)
def _fresh_engines():
    yield
    release_all()


def tail_count(s):
    return int(math.ceil(min(0.2 * s, 3 * math.sqrt(s))))


def harmonic(col):
    return -math.log(np.mean(1 / np.asarray(col, dtype=np.float64)))


# ---- 1. long columns: the global-memory form at each tail-buffer size -------------------------------------------
@pytest.mark.parametrize("s, tp", [(116_508, 1024), (116_509, 2048), (466_033, 2048), (466_034, 4096), (1 << 20, 4096)])
def test_long_columns_at_each_tail_buffer_size(s, tp):
    """Tp (the power of two >= T) steps at S = 116 509 and 466 034: the bitonic network then holds 8 and 16 keys per
    thread, the radix select runs over up to 2^20 global values and _gpdfit over up to 85 candidates.  S = 2^20 is
    reached by burn-in from a longer store (S_total > 2^20 is accepted)."""
    assert 1 << (tail_count(s) - 1).bit_length() == tp and s > elpd.lds_max_samples()
    extra = 1000 if s == 1 << 20 else 0
    lh = make_lh(s + extra, 8, seed=s)
    lh[:, 7] = np.random.default_rng(s + 1).uniform(0.5, 1.0, s + extra)   # bounded ratios: a fitted k < 0
    burnin = extra / (s + extra) + 1e-12 if extra else 0.0
    res, _w = compare(lh, np.zeros(8, bool), burnin)
    assert res.n_samples == s
    assert res.pareto_k[7] < 0 and np.isinf(res.pareto_k[2]) and res.pareto_k[3] > 0.7


# ---- 2. a statistical known answer at 2^20 samples ---------------------------------------------------------------
def beta_bernoulli(s, seed, n=20, ones=14, a=1.0, b=1.0):
    """lh [s, n] of a Beta-Bernoulli model under s exact posterior draws, and the exact log p(y_i | y_-i)."""
    y = np.zeros(n, bool)
    y[:ones] = True
    theta = np.random.default_rng(seed).beta(a + ones, b + n - ones, s)
    lh = np.where(y[None, :], theta[:, None], 1 - theta[:, None]).astype(np.float32)
    p1 = (a + ones - 1) / (a + b + n - 1)
    exact = np.where(y, math.log(p1), math.log(1 - (a + ones) / (a + b + n - 1)))
    return lh, exact


def test_beta_bernoulli_exact_leave_one_out_at_2_20_samples():
    """The longest global-form column (Tp = 4096): the device equals the restatement to 1e-10 and both recover the
    closed-form leave-one-out predictive to 2e-3 (tests/test_elpd_oracle_cpu.py has the measured spread)."""
    lh, exact = beta_bernoulli(1 << 20, seed=0)
    res, _w = compare(lh, np.zeros(20, bool), 0.0)
    assert np.all(np.abs(res.loo_i - exact) <= 2e-3), res.loo_i - exact
    assert np.all((res.pareto_k > 0) & (res.pareto_k < 0.5))


# ---- 3. short columns and the tail thresholds --------------------------------------------------------------------
@pytest.mark.parametrize("s", [2, 3, 4, 20])
def test_short_columns_are_unsmoothed(s):
    """T <= 4 up to S = 20: k = inf and loo_i is the harmonic-mean estimate."""
    rng = np.random.default_rng(s)
    lh = rng.uniform(0.01, 1.0, (s, 12)).astype(np.float32)
    lh[:, 1] = 0.25
    lh[:, 2] = np.round(lh[:, 2], 1)
    res, w = compare(lh, np.zeros(12, bool), 0.0)
    assert np.isinf(res.pareto_k).all()
    close(res.loo_i, [harmonic(lh[:, j]) for j in range(12)], rtol=1e-12)
    ll = np.log(lh.astype(np.float64))
    close(w.waic_i, np.log(np.mean(lh, axis=0, dtype=np.float64)) - np.var(ll, axis=0), rtol=1e-12)


def _sorted_with_ties(rng, s, lo, hi):
    """A column of s distinct values whose ascending ranks lo .. hi (inclusive) all hold the value of rank lo."""
    v = np.sort(rng.choice(np.arange(1, 100 * s + 1), s, replace=False).astype(np.float64) / (100 * s + 1))
    v[lo:hi + 1] = v[lo]
    return rng.permutation(v).astype(np.float32)


def test_the_first_fitted_tail_and_ties_at_the_cutoff():
    """S = 21 (T = 5): five distinct values below the cutoff are fitted; a tie at the cutoff leaving four is not.
    S = 20 (T = 4) is never fitted."""
    rng = np.random.default_rng(21)
    lh = np.stack([_sorted_with_ties(rng, 21, 0, 0), _sorted_with_ties(rng, 21, 4, 5), _sorted_with_ties(rng, 21, 3, 9),
                   _sorted_with_ties(rng, 21, 5, 7), _sorted_with_ties(rng, 21, 0, 0)], axis=1)
    res, _w = compare(lh, np.zeros(5, bool), 0.0)
    assert np.isfinite(res.pareto_k[[0, 3, 4]]).all() and np.isinf(res.pareto_k[[1, 2]]).all()
    close(res.loo_i[1:3], [harmonic(lh[:, 1]), harmonic(lh[:, 2])], rtol=1e-12)
    res20, _w = compare(lh[1:], np.zeros(5, bool), 0.0)
    assert np.isinf(res20.pareto_k).all()


@pytest.mark.parametrize("s", [224, 225, 226])
def test_where_the_two_tail_rules_meet(s):
    """S = 225: 0.2 S = 3 sqrt(S) = 45."""
    compare(make_lh(s, 10, seed=s), np.zeros(10, bool), 0.0)


@pytest.mark.parametrize("s", [100, 1000, 50_000])
def test_ties_on_both_sides_of_the_cutoff_rank(s):
    """The (T+1)-th smallest value tied several times below and above its rank (shortening the tail to T - 3, to
    exactly 5 and to exactly 4), and a tail made of one repeated value.  S = 50 000 takes the global form."""
    t = tail_count(s)
    rng = np.random.default_rng(s)
    cols = [_sorted_with_ties(rng, s, t - 3, t + 3), _sorted_with_ties(rng, s, 5, t + 2), _sorted_with_ties(rng, s, 4, t),
            _sorted_with_ties(rng, s, t, t + 5)]
    rep = np.concatenate([np.full(t, 0.01), rng.uniform(0.2, 1.0, s - t)])
    cols.append(rng.permutation(rep).astype(np.float32))
    rep2 = np.concatenate([np.full(t // 2, 0.01), np.full(t - t // 2, 0.02), rng.uniform(0.2, 1.0, s - t)])
    cols.append(rng.permutation(rep2).astype(np.float32))
    lh = np.stack(cols, axis=1)
    res, _w = compare(lh, np.zeros(len(cols), bool), 0.0)
    assert np.isfinite(res.pareto_k[[0, 1, 3, 4, 5]]).all() and np.isinf(res.pareto_k[2])
    close([res.loo_i[2]], [harmonic(lh[:, 2])], rtol=1e-12)


# ---- 4. extreme float32 values and the data check ----------------------------------------------------------------
def extreme_columns(rng, s):
    sub = np.exp(rng.uniform(math.log(FLT_TRUE_MIN), math.log(1.1e-38), s)).astype(np.float32)
    sub = np.maximum(sub, np.float32(FLT_TRUE_MIN))
    sub[0] = FLT_TRUE_MIN
    big = (rng.uniform(0.01, 1.0, s) * FLT_MAX).astype(np.float32)
    big[1] = FLT_MAX
    both = np.where(rng.random(s) < 0.5, sub, big)
    both[:2] = [FLT_TRUE_MIN, FLT_MAX]                  # x spans log(FLT_MAX / 2^-149) = 192.1
    out1 = rng.uniform(0.49, 0.51, s).astype(np.float32)
    out1[s // 2] = 1e-40
    out2 = rng.uniform(0.49, 0.51, s).astype(np.float32)
    out2[s // 3] = FLT_MAX
    return np.stack([sub, big, both, out1, out2], axis=1)


@pytest.mark.parametrize("s", [1000, 40_000])
def test_subnormals_and_values_near_flt_max(s):
    lh = extreme_columns(np.random.default_rng(s), s)
    assert (lh[:, 0] < np.finfo(np.float32).tiny).all() and lh[:, 2].min() == FLT_TRUE_MIN and lh[:, 2].max() == FLT_MAX
    res, w = compare(lh, np.zeros(5, bool), 0.0)
    assert np.isfinite(res.loo_i).all() and np.isfinite(w.waic_i).all()


@pytest.mark.parametrize("bad", [0.0, -0.0, -FLT_TRUE_MIN, np.inf, np.nan], ids=["zero", "neg_zero", "neg_subnormal", "inf", "nan"])
def test_bad_values_are_refused_after_the_burnin_and_ignored_inside_it(bad):
    lh = make_lh(60, 5, seed=60)
    after = lh.copy()
    after[40, 3] = bad                                  # burn-in 0.1: rows 0 .. 5 are dropped
    with pytest.raises(EngineError, match="not positive and finite") as info:
        elpd.psis_loo(after, na_values=np.zeros(5, bool), burnin=0.1)
    assert info.value.code == 4
    inside = lh.copy()
    inside[3, 3] = bad
    compare(inside, np.zeros(5, bool), 0.1)
    compare(inside, None, 0.1)                          # (the isclose rule reads every row, burn-in included)


# ---- 5. host <-> store staging in several 64 MiB pieces ----------------------------------------------------------
def wide_rows(s, m, seed):
    """float32 [s, m]: make_lh's families over 1009 columns, tiled and scaled per column so that no two columns agree."""
    base = make_lh(s, 1009, seed)
    lh = np.ascontiguousarray(np.tile(base, (1, -(-m // 1009)))[:, :m])
    scale = (1.0 - 0.5 * ((np.arange(m) * 0.6180339887) % 1.0)).astype(np.float32)
    lh *= scale
    return lh


def test_staging_in_pieces():
    """M = 200 003: the staging buffer holds 83 rows, so 300 rows move in pieces of 83 + 83 + 83 + 51.  Batches of 1,
    82, 83, 84 and 50 rows straddle pieces at non-zero offsets; rows read back bit for bit, also a sub-range through
    the C ABI; results do not depend on how the store was filled nor on its capacity."""
    m, s = 200_003, 300
    lh = wide_rows(s, m, seed=203)
    assert (64 << 20) // (4 * m) == 83
    stores = [elpd._Store(0, m, 300), elpd._Store(0, m, 300), elpd._Store(0, m, 1000)]
    try:
        stores[0].append_rows(lh)
        r = 0
        for k in (1, 82, 83, 84, 50):
            stores[1].append_rows(np.ascontiguousarray(lh[r:r + k]))
            r += k
        assert r == s
        stores[2].append_rows(lh)
        for st in stores:
            assert st.n_rows == s
            got = st.rows()
            assert np.array_equal(got.view(np.uint32), lh.view(np.uint32))
            del got
        sub = np.empty((170, m), dtype=np.float32)
        st = stores[1]
        st._check(st._lib.sbe_elpd_get_rows(st._h, 81, 170, elpd._ptr(sub)))
        assert np.array_equal(sub.view(np.uint32), lh[81:251].view(np.uint32))
        del sub
        na = np.zeros(m, bool)
        na[::17] = True
        outs = [st.compute(30, na, False) for st in stores]
        for o in outs[1:]:
            for a, b in zip(outs[0], o):
                assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    finally:
        for st in stores:
            st.close()
    loo_i, k_i, lppd_i, v_i = outs[0]
    kept = np.flatnonzero(~na)
    idx = np.arange(0, len(kept), 389)
    want = np.array([eo.column_stats(lh[30:, kept[j]]) for j in idx])
    close(loo_i[idx], want[:, 0])
    check_k(k_i[idx], want[:, 1])
    close(lppd_i[idx] - v_i[idx], want[:, 2] - want[:, 3])
    assert np.isfinite(loo_i).all()


# ---- 6. more than 2^24 columns -----------------------------------------------------------------------------------
def test_more_than_2_24_columns():
    """M = 2^24 + 3 columns at S = 2 (one staging row per piece): one 256-thread workgroup per kept column passes 2^32
    work-items from 2^24 columns on, so the column kernel is launched in chunks.  1009 distinct column pairs are tiled
    and three columns are all ones; every kept column must equal its pattern's result, under a mask (2^24 + 1 kept)
    and under the isclose NA rule (2^24 kept)."""
    m, p = (1 << 24) + 3, 1009
    rng = np.random.default_rng(24)
    pat = rng.uniform(0.05, 1.0, (2, p)).astype(np.float32)
    pat[:, 11] = [1e-40, FLT_MAX]
    want = np.array([eo.column_stats(pat[:, j]) for j in range(p)])
    ones = eo.column_stats(np.ones(2, np.float32))
    assert np.isinf(want[:, 1]).all()
    close(want[:, 0], -np.log(np.mean(1 / pat.astype(np.float64), axis=0)), rtol=1e-13)
    special = np.array([3, m // 2, m - 1])
    lh = np.empty((2, m), dtype=np.float32)
    lh[0] = np.resize(pat[0], m)
    lh[1] = np.resize(pat[1], m)
    lh[:, special] = 1.0
    st = elpd._Store(0, m, 2)
    try:
        st.append_rows(lh)
        del lh
        cols = np.arange(m, dtype=np.int64)
        na = np.zeros(m, bool)
        na[[10, m - 2]] = True
        for mask, isclose in ((na, False), (None, True)):
            loo_i, k_i, lppd_i, v_i = st.compute(0, mask, isclose)
            drop = na if mask is not None else np.isin(cols, special)
            kept = cols[~drop]
            assert len(loo_i) == len(kept) and len(kept) >= 1 << 24
            j = kept % p
            at = np.searchsorted(kept, special)
            at = at[(at < len(kept)) & (kept[np.minimum(at, len(kept) - 1)] == special)]
            del kept, drop
            assert np.isinf(k_i).all()
            del k_i
            for got, col in ((loo_i, 0), (lppd_i, 2), (v_i, 3)):
                w = want[:, col][j]
                w[at] = ones[col]
                assert (np.abs(got - w) <= np.maximum(1e-10 * np.abs(w), 1e-10)).all(), (col, np.flatnonzero(np.abs(got - w) > 1e-10)[:5])
                del w
            del loo_i, lppd_i, v_i, j
    finally:
        st.close()


# ---- 7. the LikelihoodLog over a wide engine ---------------------------------------------------------------------
def test_likelihood_log_at_a_wide_shape():
    """N * F = 39 000 (not a multiple of 256), C = 4: 120 rows from two slots whose weights and sources change between
    appends equal the restated LikelihoodLogger row bit for bit; device results equal the host-matrix path."""
    from oracle import sbayes_oracle as orc
    from sbayes_amd import model as sbm
    from sbayes_amd.counts import recalculate_feature_counts
    from sbayes_amd.likelihood import update_weights
    from sbayes_amd.synthetic import make_workload
    from tests.test_gpu_delta_forms import _SHAPES
    wl = make_workload("wide", shape=_SHAPES["wide"])
    n, f, _ = wl.features.shape
    assert (n * f) % 256 != 0
    names = ["clusters", "universal"] + [f"conf{i}" for i in range(1, len(wl.groups) - 1)]
    model, sample = sbm.build(wl.features, wl.states_per_feature, names, wl.groups, wl.concentration, wl.weights, wl.source)
    feats = model.data.features.values
    na_feat = model.data.features.na_values
    hc = orc.has_components(wl.groups)
    rng = np.random.default_rng(39)
    log = elpd.LikelihoodLog(model, capacity=150)
    want = []
    try:
        for i in range(120):
            cand = sample.copy()
            src_idx = np.argmax(rng.random((n, f, len(wl.groups))) * hc[:, None, :], axis=-1)
            src = np.eye(len(wl.groups), dtype=bool)[src_idx]
            src[~feats.any(-1)] = False
            with cand.source.edit() as s_:
                s_[...] = src
            cand.weights.set_value(rng.dirichlet(np.ones(len(wl.groups)), size=f).astype(np.float32))
            recalculate_feature_counts(feats, cand)
            log.append(cand, slot=i % 2)
            if i % 7 == 0 or i > 115:
                counts = orc.recalculate_feature_counts(wl.features, wl.groups, cand.source.value)
                lh_exact = orc.likelihood_per_component_exact(wl.features, na_feat, wl.groups, counts, wl.concentration,
                                                              cand.source.value)
                want.append((i, orc.logger_row(np.asarray(update_weights(cand)), lh_exact).astype(np.float32)))
        rows = log.rows()
        assert rows.shape == (120, n * f)
        for i, row in want:
            assert np.array_equal(rows[i].view(np.uint32), row.view(np.uint32)), f"row {i}"
        na = log.na_values()
        dev, host = log.psis_loo(burnin=0.1), elpd.psis_loo(rows, na_values=na, burnin=0.1)
        assert np.array_equal(dev.loo_i, host.loo_i) and np.array_equal(dev.pareto_k, host.pareto_k, equal_nan=True)
        assert dev.elpd_loo == host.elpd_loo and dev.se == host.se
        wd, wh = log.waic(burnin=0.1), elpd.waic(rows, na_values=na, burnin=0.1)
        assert np.array_equal(wd.waic_i, wh.waic_i) and wd.elpd_waic == wh.elpd_waic
        kept = np.flatnonzero(~na)
        compare(rows, na, 0.1, columns=np.arange(0, len(kept), 211))
    finally:
        log.close()


# ---- 8. the randomised generator of tools/fuzz_gpu.py --elpd ------------------------------------------------------
FAMILIES = ("smooth", "tied", "constant", "heavy", "light", "bounded", "subnormal", "near_max", "both_extremes",
            "outlier", "repeated_tail", "one")


def random_column(rng, kind, s):
    if kind == "smooth":
        x = np.exp(rng.normal(rng.uniform(-6, 0), rng.uniform(0.05, 3), s))
    elif kind == "tied":
        x = np.round(rng.uniform(0.05, 1, s), int(rng.integers(1, 3)))
    elif kind == "constant":
        x = np.full(s, rng.uniform(1e-3, 2))
    elif kind == "heavy":
        x = rng.uniform(1e-5, 1, s)
    elif kind == "light":
        x = np.exp(-rng.standard_exponential(s) * rng.uniform(0.5, 4))
    elif kind == "bounded":
        x = rng.uniform(0.5, 1, s)
    elif kind == "subnormal":
        x = np.exp(rng.uniform(math.log(FLT_TRUE_MIN), math.log(1.1e-38), s))
    elif kind == "near_max":
        x = rng.uniform(0.01, 1, s) * FLT_MAX
    elif kind == "both_extremes":
        x = np.where(rng.random(s) < 0.5, np.exp(rng.uniform(math.log(FLT_TRUE_MIN), math.log(1e-38), s)),
                     rng.uniform(0.01, 1, s) * FLT_MAX)
    elif kind == "outlier":
        x = rng.uniform(0.4, 0.6, s)
        x[rng.integers(0, s)] = rng.choice([FLT_TRUE_MIN, 1e-40, FLT_MAX])
    elif kind == "repeated_tail":
        # at most half the tail: when 3/4 of it is one value, _gpdfit's candidate b = -1/ary[q] + 1/ary[-1] can cancel
        # to exactly 0 (m_est = 40, 56, ...) and arviz returns NaN; whether it cancels follows the last bit of exp,
        # which the device does not share with NumPy (test_ties_on_both_sides_of_the_cutoff_rank keeps whole tails)
        t = int(rng.integers(1, tail_count(s) // 2 + 2))
        x = rng.permutation(np.concatenate([np.full(max(t, 0), 0.01), rng.uniform(0.2, 1, s - max(t, 0))]))
    else:                                               # "one": NA under the isclose rule
        x = np.ones(s)
    return np.maximum(x.astype(np.float32), np.float32(FLT_TRUE_MIN))


BAD_VALUES = (0.0, -0.0, -FLT_TRUE_MIN, np.inf, np.nan)


def random_elpd_case(rng, s_max=1 << 20):
    """(lh, na_values, burnin): S log-uniform in [2, s_max] weighted toward short columns, random families, NA rule,
    burn-in, and now and then a bad value inside the burn-in rows (which must be ignored)."""
    s = int(round(2.0 ** (1 + (math.log2(s_max) - 1) * rng.random() ** 2)))
    s = min(max(s, 2), s_max)
    burnin = 0.0 if rng.random() < 0.4 else float(rng.uniform(0, 0.6))
    s_total = int(math.ceil(s / (1 - burnin)))
    if not 2 <= s_total - int(burnin * s_total) <= s_max:
        burnin, s_total = 0.0, s
    m = int(rng.integers(1, max(2, min(40, 3_000_000 // s_total)) + 1))
    kinds = rng.choice(len(FAMILIES), m)
    lh = np.stack([random_column(rng, FAMILIES[k], s_total) for k in kinds], axis=1)
    r = rng.random()
    if r < 0.35:
        na = None                                       # the isclose rule ("one" columns are dropped)
    elif r < 0.7:
        na = rng.random(m) < 0.2
        na[0] = False
    else:
        na = np.zeros(m, bool)
    burn = int(burnin * s_total)
    if burn and rng.random() < 0.3:
        lh[rng.integers(0, burn), rng.integers(0, m)] = rng.choice(BAD_VALUES)
    return lh, na, burnin


def run_elpd_case(lh, na, burnin):
    if eo.kept_columns(lh, na).any():                  # (a case whose every column is NA has nothing to compare)
        compare(lh, na, burnin)


@pytest.mark.parametrize("block", range(4))
def test_fixed_seed_random_cases(block):
    """40 cases of the fuzz generator (10 per block), S <= 2^17: bounded by case count, so deterministic."""
    for i in range(10):
        seed = 5000 + 10 * block + i
        lh, na, burnin = random_elpd_case(np.random.default_rng(seed), s_max=1 << 17)
        try:
            run_elpd_case(lh, na, burnin)
        except AssertionError as exc:
            raise AssertionError(f"fuzz case seed {seed}: {exc}") from exc
