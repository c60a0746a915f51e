"""Device against checker for the posterior summary (sbayes_amd.summary, include/sbe_summary.h): every fixed case of
tests/_summary_cases.py -- quantiles, HDI, n_lags and flag equal bit for bit, the five outputs shared with the diagnostics
bit-equal to DiagHandle.compute on the same rows, ess_bulk, ess_tail and rhat_rank within the bounds tests/_summary_oracle.py
derives; the derived columns themselves (ranks and indicators exact, z against mpmath); the bits independent of the launch
size, the store's capacity and the way rows were appended; the recorded two-run reference output and the command line."""
import math
from pathlib import Path

import mpmath
import numpy as np
import pytest

from tests import _summary_cases as cases
from tests import _summary_oracle as sorc
from sbayes_amd import diag, summary

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "diag_runs.npz"
DIAG_EQUAL = ("mean", "sd", "ess", "rhat", "mcse_mean", "n_lags")
EXACT = ("quantiles", "hdi_lo", "hdi_hi")
OUTPUTS = EXACT + sorc.BOUNDED + DIAG_EQUAL + ("flag",)


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _check(res, want, label):
    """Bit-equal: quantiles, HDI, n_lags, flag.  Within the derived bound: ess_bulk, ess_tail, rhat_rank (the largest
    error / bound is printed)."""
    assert (res.n_chains, res.n_draws) == (want["n_chains"], want["n_draws"])
    assert np.array_equal(res.flag, want["flag"]), (label, res.flag, want["flag"])
    assert np.array_equal(res.n_lags, want["n_lags"]), (label, res.n_lags, want["n_lags"])
    for k in EXACT:
        assert _bits(getattr(res, k)) == _bits(want[k]), (label, k, getattr(res, k), want[k])
    frac = sorc.fractions(res, want)
    print(f"[summary-bound] {label}: " + " ".join(f"{k}={v:.3g}" for k, v in frac.items()))
    assert max(frac.values()) <= 1.0, (label, frac)
    return frac


def _same_bits(a, b):
    return all(_bits(getattr(a, k)) == _bits(getattr(b, k)) for k in OUTPUTS)


def _diag_equal(res, x, kw):
    ref = diag.convergence(list(x), **{k: v for k, v in kw.items() if k in ("burnin", "split", "max_lag")})
    for k in DIAG_EQUAL:
        assert _bits(getattr(res, k)) == _bits(getattr(ref, k)), k
    assert np.array_equal(res.flag & 3, ref.flag & 3) and np.all((res.flag & 4) >= (ref.flag & 4))
    assert res.path == ref.path


@pytest.mark.parametrize("name", list(cases.CASES))
def test_device_matches_the_checker_and_the_diagnostics(name):
    x, kw, want = cases.case(name)
    assert want["margin_ok"].all() and want["margin"].min() >= cases.MIN_MARGIN
    res = summary.summarize(list(x), **kw)
    _check(res, want, name)
    _diag_equal(res, x, kw)
    assert res.rank_ms > 0.0 and res.column_ms > 0.0


def test_the_cases_cover_what_they_are_there_for():
    limit = summary.lds_max_draws()
    for name, n_total, path in (("lds_edge", limit, "lds"), ("lds_edge_plus_1", limit + 1, "global"), ("global_2x40000", 72000, "global")):
        x, kw, want = cases.case(name)
        assert want["n_chains"] * want["n_draws"] == n_total
        assert summary.summarize(list(x), **kw).path == path
    for name, total in (("n64", 64), ("n65", 65), ("n255", 255), ("n256", 256), ("n257", 257), ("split_1x8", 8), ("split_3x14", 42)):
        want = cases.case(name)[2]
        assert want["n_chains"] * want["n_draws"] == total
    assert (cases.case("split_1x8")[2]["n_chains"], cases.case("split_3x14")[2]["n_chains"]) == (2, 6)
    want = cases.case("special")[2]
    assert want["flag"].tolist() == [0, 1, 2, 0, 2, 0, 0, 0, 0, 0, 0, 0]
    assert np.isnan(want["quantiles"][:, 2]).all() and want["quantiles"][:, 1].tolist() == [0.25] * 3 and want["ess_bulk"][1] == 216.0
    assert np.all(cases.case("max_lag_hit")[2]["flag"] == 4)
    n = 10
    assert cases.case("hdi_widest")[2]["n_chains"] * cases.case("hdi_widest")[2]["n_draws"] == n == cases.case("hdi_clips_low")[2]["n_chains"] * cases.case("hdi_clips_low")[2]["n_draws"]
    assert cases.case("hdi_widest")[1]["hdi_prob"] < 1.0 and sorc.hdi_span(cases.case("hdi_widest")[1]["hdi_prob"], n) == n - 1
    assert math.floor(cases.case("hdi_clips_low")[1]["hdi_prob"] * n) == 0 and sorc.hdi_span(cases.case("hdi_clips_low")[1]["hdi_prob"], n) == 1
    assert cases.case("wide_257")[0].shape[2] == 257 and cases.case("one_column")[0].shape[2] == 1
    # rho_t past the 2048 entries kept in LDS, in the store's own pass and in a derived one
    for name, path in (("spill_2x2051", "lds"), ("spill_2x2400", "lds"), ("spill_global_8x2300", "global")):
        x, kw, want = cases.case(name)
        assert want["n_draws"] > 2048 and want["n_lags"].max() > 2048
        assert max(p["col"]["n_lags"] for c in want["columns"] for p in c["parts"].values()) > 2048
        assert summary.summarize(list(x), **kw).path == path
    assert (cases.case("spill_global_8x2300")[2]["n_chains"] * 2300 > limit) and cases.case("spill_2x2400")[0].shape[2] == 3


def _mp_ndtri(p):
    return mpmath.sqrt(2) * mpmath.erfinv(2 * mpmath.mpf(float(p)) - 1)


@pytest.mark.parametrize("name,columns", [("special", (0, 5, 6, 8, 10, 11)), ("n257", (0,)), ("ar09_4x1000", (1,)), ("lds_edge_plus_1", (1,))])
def test_derived_columns_ranks_and_indicators_exact_z_against_mpmath(name, columns):
    """sbe_summary_derived_column: the average ranks and the two indicators equal the checker's, bit for bit; zb and zf are
    within C_NDTRI u max(1, |z|) of ndtri at 40 digits of the same rank probability (every value of a short column, 300
    spread over a long one, both ends included)."""
    x, kw, want = cases.case(name)
    mpmath.mp.dps = 40
    worst = 0.0
    h = summary.SummaryHandle()
    try:
        h.reset(x.shape[0], x.shape[2], x.shape[1])
        for c in range(x.shape[0]):
            h.append(c, x[c])
        h.compute(**kw)
        for j in columns:
            d = want["columns"][j]["derived"]
            N = d["rank"].size
            for which in ("rank", "i05", "i95"):
                assert _bits(h.derived_column(j, which)) == _bits(d[which]), (name, j, which)
            xs = np.ascontiguousarray(sorc.orc.prepare(list(x), kw.get("burnin", 0.1), kw.get("split", True))[0][:, :, j]) + 0.0
            for which, values in (("zb", xs), ("zf", np.abs(xs - d["q50"]))):
                z = h.derived_column(j, which).ravel()
                p = sorc.rank_probability(sorc.ranks(values), N).ravel()
                order = np.argsort(p, kind="stable")
                pick = order if N <= 600 else order[np.unique(np.concatenate([np.arange(8), np.linspace(0, N - 1, 300).astype(int), np.arange(N - 8, N)]))]
                for i in pick:
                    exact = _mp_ndtri(p[i])
                    err = abs(mpmath.mpf(float(z[i])) - exact) / (sorc.U * max(1.0, abs(float(exact))))
                    worst = max(worst, float(err))
        with pytest.raises(ValueError, match="which"):
            h.derived_column(0, "nope")
        h.reset(1, 2, 8)
        with pytest.raises(_handle_error(), match="no compute call"):
            h.derived_column(0, "zb")
    finally:
        h.close()
    print(f"[summary-bound] {name}: ndtri worst {worst:.3g} u max(1, |z|) of {sorc.C_NDTRI}")
    assert worst <= sorc.C_NDTRI


def test_a_column_constant_within_every_chain_holds_doubled_ranks_and_gives_an_infinite_rank_rhat():
    """W = 0: zb and zf are 2 r (exact integers) on both sides, so rhat_rank is +inf and ess_bulk that of rho = 1, exactly."""
    x, kw, want = cases.case("chain_constant")
    h = summary.SummaryHandle()
    try:
        h.reset(x.shape[0], x.shape[2], x.shape[1])
        for c in range(x.shape[0]):
            h.append(c, x[c])
        res = h.compute(**kw)
        assert np.isinf(res.rhat_rank[:2]).all() and np.isfinite(res.rhat_rank[2])
        assert _bits(res.ess_bulk[:2]) == _bits(want["ess_bulk"][:2]) == _bits(res.ess[:2])
        for j in (0, 1):
            d = want["columns"][j]["derived"]
            assert d["flat"]
            for which in ("zb", "zf", "rank", "i05", "i95"):
                assert _bits(h.derived_column(j, which)) == _bits(d[which]), (j, which)
        assert not np.array_equal(h.derived_column(2, "zb"), 2.0 * h.derived_column(2, "rank"))
    finally:
        h.close()


def _table():
    """[2][S][P]: the special columns, a wide block and repeats of columns 0 and 3 at the end (column position)."""
    x = np.concatenate([cases.case("special")[0], cases.orc.ar1(np.random.default_rng(71), 0.8, 2, 120, 9, loc=0.5)], axis=2)
    return np.concatenate([x, x[:, :, :1], x[:, :, 3:4]], axis=2)


def test_bits_do_not_depend_on_launch_size_capacity_appends_or_position():
    x = _table()
    m, s, p = x.shape
    ref = summary.summarize(list(x))
    assert _bits(ref.ess_bulk) != _bits(np.zeros_like(ref.ess_bulk))
    for k in OUTPUTS:
        v = getattr(ref, k)
        assert _bits(v[..., [0, 3]]) == _bits(v[..., [p - 2, p - 1]]), k
    h = summary.SummaryHandle()
    try:
        for launch, capacity, by_row in ((1, s, False), (7, s + 37, False), (0, 4 * s, True), (5, s, True)):
            h.set_launch_columns(launch)
            h.reset(m, p, capacity)
            for c in range(m):
                if by_row:
                    for r in range(s):
                        h.append(c, x[c, r])
                else:
                    h.append(c, x[c])
            res = h.compute()
            assert _same_bits(res, ref), (launch, capacity, by_row)
            assert (res.launches, res.launch_columns) == ((math.ceil(p / launch), launch) if launch else (1, p))
        h.set_launch_columns(0)
        h.reset(1, 3, 50)
        h.append(0, x[0, :50, :3])
        h.compute(burnin=0.0)
        h.reset(m, p, s)
        for c in range(m):
            h.append(c, x[c])
        assert _same_bits(h.compute(), ref)
    finally:
        h.close()


def test_spilled_bits_do_not_depend_on_the_launch_size():
    """2 x 2400 x 3, rho_t past entry 2048 in the store's pass and in the derived ones.  With C = 1, 2 or 3 columns per launch of
    the rank kernel the derived store is laid out [M][4 C][n] anew, the derived pass needs 4 C scratch slices and the store's own
    pass C of the same scratch."""
    x, kw, want = cases.case("spill_2x2400")
    m, s, p = x.shape
    ref = summary.summarize(list(x), **kw)
    _check(ref, want, "spill_2x2400 (reference of the launch sizes)")
    h = summary.SummaryHandle()
    try:
        for launch, shape in ((1, (3, 1)), (2, (2, 2)), (0, (1, 3))):
            h.set_launch_columns(launch)
            h.reset(m, p, s)
            for c in range(m):
                h.append(c, x[c])
            res = h.compute(**kw)
            assert _same_bits(res, ref), launch
            assert (res.launches, res.launch_columns) == shape
    finally:
        h.close()


def test_rows_appended_in_pieces_to_two_chains_of_unequal_length(monkeypatch):
    rng = np.random.default_rng(72)
    a, b = cases.orc.ar1(rng, 0.7, 1, 230, 5)[0], cases.orc.ar1(rng, 0.7, 1, 200, 5)[0]
    want = sorc.summarize([a, b], burnin=0.1)
    assert want["cut"] == (27, 0) and want["margin_ok"].all()
    h = summary.SummaryHandle()
    try:
        h.reset(2, 5, 256)
        for lo in range(0, 230, 33):
            h.append(0, a[lo:lo + 33])
            h.append(1, b[lo:lo + 33][:max(0, 200 - lo)])
        assert (h.rows(0), h.rows(1)) == (230, 200)
        monkeypatch.setattr(diag, "_warned_cut", False)
        with pytest.warns(UserWarning, match="cut from the end"):
            res = h.compute(burnin=0.1, names=list("abcde"))
        assert res.cut == (27, 0) and res.names == list("abcde")
        _check(res, want, "pieces")
        assert h.last_kernel_ms() == pytest.approx(res.rank_ms + res.column_ms)
        rows = res.table()
        assert len(rows) == 5 and len(rows[0]) == len(res.header()) and rows[2][0] == "c" and rows[2][1] == res.mean[2]
        assert res.header()[3:8] == ["hdi_3%", "hdi_97%", "q5%", "q50%", "q95%"]
    finally:
        h.close()


def test_bad_calls_on_a_live_handle_are_refused_with_the_limit_named():
    h = summary.SummaryHandle()
    try:
        with pytest.raises(ValueError, match="no shape"):
            h.compute()
        h.reset(1, 2, 8)
        h.append(0, np.zeros((7, 2)))
        with pytest.raises(ValueError, match="at least 4"):
            h.compute(burnin=0.0)
        with pytest.raises(ValueError, match="at most 8"):
            h.compute(burnin=0.0, split=False, probs=[0.5] * 9)
        with pytest.raises(_handle_error(), match="store overflow"):
            h.append(0, np.zeros((2, 2)))
        lib, probs, out = h._lib, np.array([0.5, 1.5]), np.zeros(8)
        burn = np.zeros(1, dtype=np.int64)
        args = [summary._ptr(out)] * 13
        assert lib.sbe_summary_compute(h._h, summary._ptr(burn), 0, 0, 2, summary._ptr(probs), 0.94, *args) == 1
        assert "probs[1]=1.5 out of range [0, 1]" in h._last_error()
        assert lib.sbe_summary_compute(h._h, summary._ptr(burn), 0, 0, 9, summary._ptr(probs), 0.94, *args) == 1
        assert "n_probs=9 out of range [0, 8]" in h._last_error()
        assert lib.sbe_summary_compute(h._h, summary._ptr(burn), 0, 0, 1, summary._ptr(probs), 1.0, *args) == 1
        assert "hdi_prob=1 out of range (0, 1)" in h._last_error()
        res = h.compute(burnin=0.0, split=False)
        assert res.flag.tolist() == [1, 1] and res.ess_bulk.tolist() == [7.0, 7.0] and np.isnan(res.rhat_rank).all()
        assert res.quantiles.tolist() == [[0.0, 0.0]] * 3 and res.hdi_lo.tolist() == [0.0, 0.0]
    finally:
        h.close()


def _handle_error():
    from sbayes_amd._handle import EngineError
    return EngineError


def _recorded():
    with np.load(GOLDEN, allow_pickle=False) as z:
        names = [str(v) for v in z["names"]]
        cnames = [str(v) for v in z["cluster_names"]]
        stats = [z[f"stats_{r}"] for r in range(2)]
        clusters = [np.unpackbits(z[f"clusters_{r}"], axis=1, count=int(z["n_cluster_columns"])) for r in range(2)]
    return names, cnames, stats, clusters


def test_recorded_reference_runs():
    """Two short south_america runs of the reference (tests/golden/diag_runs.npz): the numeric columns of their stats files
    and their cluster lines, device against checker on every column."""
    names, cnames, stats, clusters = _recorded()
    runs = [np.concatenate([s, c.astype(np.float64)], axis=1) for s, c in zip(stats, clusters)]
    want = sorc.summarize(runs, burnin=0.1)
    assert want["margin_ok"].all()
    res = summary.summarize(runs, burnin=0.1, names=names + cnames)
    _check(res, want, "recorded runs")
    _diag_equal(res, np.stack(runs), dict(burnin=0.1))
    assert (res.flag & 1).any() and (res.flag == 0).any()
    assert np.isinf(res.rhat_rank).any()                         # indicators that differ between halves but not within one


def test_command_line_on_the_recorded_runs_written_back_as_text(tmp_path, capsys):
    names, cnames, stats, clusters = _recorded()
    k = len({n.split("_")[0] for n in cnames})
    paths = []
    for r in range(2):
        sp, cp = tmp_path / f"stats_K{k}_{r}.txt", tmp_path / f"clusters_K{k}_{r}.txt"
        with open(sp, "w") as f:
            f.write("\t".join(names) + "\n")
            for row in stats[r]:
                f.write("\t".join("%.8g" % v for v in row) + "\n")
        with open(cp, "w") as f:
            for row in clusters[r]:
                f.write("\t".join("".join(map(str, part)) for part in row.reshape(k, -1)) + "\n")
        paths.append((sp, cp))
    out = tmp_path / "summary.tsv"
    assert summary.main([str(paths[0][0]), str(paths[1][0]), "--clusters", str(paths[0][1]), str(paths[1][1]), "--top", "5",
                         "--out", str(out)]) == 0
    text = capsys.readouterr().out
    p = len(names) - 2 + len(cnames)                               # without Sample and sample_id
    assert f"{p} columns, 2 runs -> 4 chains x 27 draws" in text and "rank kernel" in text and "ess_bulk" in text
    table = out.read_text().splitlines()
    assert len(table) == p + 1 and table[0].split("\t")[:5] == ["column", "mean", "sd", "hdi_3%", "hdi_97%"]
    keep = [j for j, n in enumerate(names) if n not in diag.INDEX_COLUMNS]
    runs = [np.loadtxt(sp, delimiter="\t", skiprows=1, ndmin=2)[:, keep] for sp, _cp in paths]
    runs = [np.concatenate([s, c.astype(np.float64)], axis=1) for s, c in zip(runs, clusters)]
    res = summary.summarize(runs, burnin=0.1)
    col = table[0].split("\t").index("ess_bulk")
    assert [float(line.split("\t")[col]) for line in table[1:]] == pytest.approx(res.ess_bulk.tolist(), rel=1e-9, nan_ok=True)
    q50 = table[0].split("\t").index("q50%")
    assert [float(line.split("\t")[q50]) for line in table[1:]] == pytest.approx(res.quantiles[1].tolist(), rel=1e-9, nan_ok=True)
