"""Device against checker for the convergence diagnostics (sbayes_amd.diag, include/sbe_diag.h): every fixed case of
tests/_diag_cases.py at the bounds tests/_diag_oracle.py derives, n_lags and flag equal; the bits independent of the
launch chunking, the store's capacity, the way rows were appended and the column's position; the path taken at the
LDS limit; the recorded two-run reference output."""
import math
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from tests import _diag_cases as cases
from tests import _diag_oracle as orc
from sbayes_amd import diag

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "diag_runs.npz"
OUTPUTS = orc.FIELDS + ("n_lags", "flag")


def _check(res, want, label):
    """n_lags and flag equal; every float output within its derived bound.  Prints the largest error / bound."""
    assert (res.n_chains, res.n_draws) == (want["n_chains"], want["n_draws"])
    assert np.array_equal(res.flag, want["flag"]), (label, res.flag, want["flag"])
    assert np.array_equal(res.n_lags, want["n_lags"]), (label, res.n_lags, want["n_lags"])
    frac = orc.fractions(res, want)
    print(f"[diag-bound] {label}: " + " ".join(f"{k}={v:.3g}" for k, v in frac.items()))
    assert max(frac.values()) <= 1.0, (label, frac)
    return frac


def _same_bits(a, b):
    return all(getattr(a, k).tobytes() == getattr(b, k).tobytes() for k in OUTPUTS)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_device_matches_the_checker_within_the_derived_bounds(name):
    x, kw, want = cases.case(name)
    assert want["margin"].min() >= cases.MIN_MARGIN
    res = diag.convergence(list(x), **kw)
    _check(res, want, name)


def test_the_cases_cover_what_they_are_there_for():
    flags = cases.case("mixed")[2]["flag"]
    assert flags.tolist() == [0, 1, 2, 0, 2, 0, 0, 0]
    assert cases.case("shifted_2x400")[2]["n_lags"][0] == 397                 # the n - 3 bound of the first loop
    n = 1000
    assert cases.case("neg05_2x500")[2]["ess"][0] == n / (1.0 / math.log10(n))  # the floor
    assert np.all(cases.case("max_lag_hit")[2]["flag"] == 4) and np.all(cases.case("max_lag_not_hit")[2]["flag"] == 0)
    assert cases.case("max_lag_hit")[2]["n_lags"].max() <= 10


def test_the_path_changes_at_the_lds_limit():
    limit = diag.lds_max_draws()
    for name, path in (("lds_edge", "lds"), ("lds_edge_plus_1", "global"), ("global_2x40000", "global"), ("ar09_4x1000", "lds")):
        x, kw, want = cases.case(name)
        res = diag.convergence(list(x), **kw)
        assert res.path == path and (res.n_chains * res.n_draws <= limit) == (path == "lds")
    # the same data on both sides of the limit: the two paths do the same arithmetic, so the first column's outputs, all
    # smooth in one more draw, stay close; each is checked against the checker above
    a, b = cases.case("lds_edge")[2], cases.case("lds_edge_plus_1")[2]
    assert abs(a["mean"][0] - b["mean"][0]) < 1e-3


def _table():
    """[2][S][P]: the mixed columns, a wide block and a repeat of column 0 at the end (column position)."""
    x = np.concatenate([cases.case("mixed")[0], orc.ar1(np.random.default_rng(31), 0.8, 2, 120, 14, loc=0.5)], axis=2)
    return np.concatenate([x, x[:, :, :1], x[:, :, 3:4]], axis=2)


def test_bits_do_not_depend_on_launches_capacity_appends_or_position():
    x = _table()
    m, s, p = x.shape
    ref = diag.convergence(list(x))
    assert ref.ess.tobytes() != np.zeros_like(ref.ess).tobytes()
    # column position: columns 0 and 3 again at the end of the table
    for k in OUTPUTS:
        assert getattr(ref, k)[[0, 3]].tobytes() == getattr(ref, k)[[p - 2, p - 1]].tobytes(), k
    h = diag.DiagHandle()
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
            assert res.launches == (math.ceil(p / launch) if launch else 1)
        # a store that is reset to another shape and filled again gives the same bits once more
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


def test_rows_appended_in_pieces_to_two_chains_of_unequal_length(monkeypatch):
    """The LikelihoodLog-style use: rows arrive in pieces, the runs differ in length, the cut is reported."""
    rng = np.random.default_rng(32)
    a, b = orc.ar1(rng, 0.7, 1, 230, 5)[0], orc.ar1(rng, 0.7, 1, 200, 5)[0]
    want = orc.diagnose([a, b], burnin=0.1)
    assert want["cut"] == (27, 0) and want["margin"].min() >= cases.MIN_MARGIN
    h = diag.DiagHandle()
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
        assert h.last_kernel_ms() > 0.0
        worst = res.worst(2)
        assert [w[0] for w in worst] == [res.names[i] for i in np.argsort(res.ess, kind="stable")[:2]]
        s = res.summary()
        assert s["n_columns"] == 5 and s["ess_min"] == res.ess.min() and s["n_ess_below"] == int((res.ess < 200).sum())
    finally:
        h.close()


def test_wide_rows_go_through_the_staging_buffer_in_pieces_at_any_offset():
    """A row of P = 200 003 float64 columns leaves the 64 MiB staging buffer 41 rows: 100 rows appended in one call go in
    pieces of 41 + 41 + 18, and batches of 1, 40, 41, 18 straddle the pieces at row offsets that are not 0.  Both stores
    give the same bits, and those meet the checker on 64 columns spread over the width, the last one included (P is no
    multiple of 32: the transpose's edge tile)."""
    p, s = 200_003, 100
    assert (64 << 20) // (8 * p) == 41
    x = orc.ar1(np.random.default_rng(33), 0.6, 1, s, p)[0]
    results = []
    for batches in ((s,), (1, 40, 41, 18)):
        h = diag.DiagHandle()
        try:
            h.reset(1, p, s)
            lo = 0
            for n in batches:
                h.append(0, x[lo:lo + n])
                lo += n
            assert h.rows(0) == s
            results.append(h.compute())
        finally:
            h.close()
    one, many = results
    assert _same_bits(one, many)
    cols = np.linspace(0, p - 1, 64).astype(np.int64)
    want = orc.diagnose([x[:, cols]])
    assert cols[-1] == p - 1 and want["margin"].min() >= cases.MIN_MARGIN
    part = SimpleNamespace(n_chains=one.n_chains, n_draws=one.n_draws, **{k: getattr(one, k)[cols] for k in OUTPUTS})
    _check(part, want, "wide rows")


def test_bad_calls_on_a_live_handle_are_refused_with_the_limit_named():
    h = diag.DiagHandle()
    try:
        with pytest.raises(ValueError, match="no shape"):
            h.compute()
        h.reset(1, 2, 8)
        h.append(0, np.zeros((7, 2)))
        with pytest.raises(ValueError, match="at least 4"):
            h.compute(burnin=0.0)                                   # 7 rows split: halves of 3
        with pytest.raises(_handle_error(), match="store overflow"):
            h.append(0, np.zeros((2, 2)))
        res = h.compute(burnin=0.0, split=False)
        assert res.flag.tolist() == [1, 1] and res.ess.tolist() == [7.0, 7.0]
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
    """Two short south_america runs of the reference (tests/golden/make_golden_diag.py): the numeric columns of their stats
    files and their cluster lines, device against checker on every column."""
    names, cnames, stats, clusters = _recorded()
    runs = [np.concatenate([s, c.astype(np.float64)], axis=1) for s, c in zip(stats, clusters)]
    want = orc.diagnose(runs, burnin=0.1)
    assert want["margin"].min() >= cases.MIN_MARGIN
    res = diag.convergence(runs, burnin=0.1, names=names + cnames)
    _check(res, want, "recorded runs")
    assert (res.flag & 1).any() and (res.flag == 0).any()       # cluster indicators that never change, parameters that do
    assert np.isinf(res.rhat).any()                             # ... and indicators that differ between halves but not within one


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
    out = tmp_path / "diag.tsv"
    assert diag.main([str(paths[0][0]), str(paths[1][0]), "--clusters", str(paths[0][1]), str(paths[1][1]), "--top", "5",
                      "--out", str(out)]) == 0
    text = capsys.readouterr().out
    p = len(names) - 2 + len(cnames)                               # without Sample and sample_id
    assert f"{p} columns, 2 runs -> 4 chains x 27 draws" in text and "ess min" in text and "rhat > 1.01" in text
    table = out.read_text().splitlines()
    assert len(table) == p + 1 and table[0].split("\t")[:4] == ["column", "mean", "sd", "ess"]
    # the table holds what the library call gives for the same columns
    keep = [j for j, n in enumerate(names) if n not in diag.INDEX_COLUMNS]
    runs = [np.concatenate([s[:, keep], c.astype(np.float64)], axis=1) for s, c in zip(stats, clusters)]
    res = diag.convergence(runs, burnin=0.1)
    assert [float(line.split("\t")[3]) for line in table[1:]] == pytest.approx(res.ess.tolist(), rel=1e-9, nan_ok=True)
